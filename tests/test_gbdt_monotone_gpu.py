"""monotone_constraints on the GPU: the bounded split kernels (dense and CSR)
against their references, the three growers against each other, the deferred
tree path, and the app against its CPU run."""
import functools
import math
import os
import re

import pytest
import torch

import _gbdt_monotone_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
INF = math.inf


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _bsp():
    from wormhole_amd.parallel.bsp import BSP
    return BSP(CPU)


# ------------------------------------------------------------ split kernels
def _bounds_around(p, totals, g, width):
    """[S, 2]: slot 0 unbounded, the others an interval of random reach
    (< width on either side) around the slot's own unclamped weight."""
    S = totals.shape[0]
    w0 = torch.tensor([p.calc_weight(float(t[0]), float(t[1])) for t in totals],
                      dtype=torch.float64)
    r = torch.rand(S, 2, generator=g, dtype=torch.float64) * width
    b = torch.stack([w0 - r[:, 0], w0 + r[:, 1]], 1)
    b[0, 0], b[0, 1] = -INF, INF
    return b


def dense_case(S, F, nbin, alpha, mcw):
    """The inputs of test_gbdt_split_kernel (tests/test_kernels_gpu.py) with
    signs and bounds; the gap between each slot's best and second-best gain
    is checked by the caller."""
    G = _G()
    g = torch.Generator().manual_seed(S * F + nbin)
    hist = torch.zeros(S, F, nbin, 2, dtype=torch.float64)
    hist[..., 0] = torch.randn(S, F, nbin, generator=g, dtype=torch.float64)
    hist[..., 1] = torch.rand(S, F, nbin, generator=g, dtype=torch.float64) * 2
    present = hist.sum(2)  # [S, F, 2]
    totals = present.max(1).values + torch.rand(S, 2, generator=g, dtype=torch.float64)
    totals[:, 0] = present[:, :, 0].mean(1)  # rows missing a feature move the totals
    valid = torch.rand(F, nbin, generator=g) < 0.8
    valid[0] = False
    p = G.GBDTParam()
    p.alpha, p.min_child_weight = alpha, mcw
    if S > 2:
        hist[2].zero_()  # no candidate passes min_child_weight on either side
        totals[2] = 0.0
    mono = torch.randint(-1, 2, (F,), generator=g).to(torch.int8)
    # child weights scatter ~ sqrt(nbin) / (nbin + lambda) around the node's
    bounds = _bounds_around(p, totals, g, 0.5 / math.sqrt(nbin))
    return p, hist, totals, valid, mono, bounds


def top_two_gap(gain):
    """Per slot (best - second best) / max(1, |best|) over all candidates of
    gain [S, ...] (inf where fewer than two are finite)."""
    flat = gain.reshape(gain.shape[0], -1)
    top = flat.topk(2, dim=1).values
    gap = (top[:, 0] - top[:, 1]) / top[:, 0].abs().clamp_min(1.0)
    return torch.where(torch.isfinite(top[:, 1]), gap, torch.full_like(gap, INF))


DENSE_SHAPES = [(5, 7, 33, 0.0, 1.0), (3, 28, 256, 0.5, 0.1), (2, 4, 1000, 0.0, 5.0)]


@pytest.mark.parametrize("S,F,nbin,alpha,mcw", DENSE_SHAPES)
def test_split_kernel_with_bounds(S, F, nbin, alpha, mcw):
    """k_split_feat<true, false> / k_split_node against find_splits_ref: the same
    feature / bin / direction (the reference's best beats its runner-up by
    more than the tolerance, so the index is well defined), gains and left
    sums to fp64 rounding (rtol = atol = 1e-9, both sides fp64)."""
    G = _G()
    p, hist, totals, valid, mono, bounds = dense_case(S, F, nbin, alpha, mcw)
    gains, _ = G.split_gains(p, hist, totals, valid, mono, bounds)
    gap = top_two_gap(gains)
    ref = G.split_fields(G.find_splits_ref(p, hist, totals, valid, mono, bounds))
    ok = torch.isfinite(ref[0])
    assert bool((gap[ok] > 1e-9).all()), gap
    free = G.split_fields(G.find_splits_ref(p, hist, totals, valid))
    assert not torch.equal(free[0][ok], ref[0][ok])  # the bounds and signs bite
    got = G.split_fields(G.find_splits(p, hist.to(DEV), totals.to(DEV), valid, mono, bounds))
    print("gain", got[0].tolist(), ref[0].tolist())
    assert torch.equal(torch.isfinite(got[0]), ok)
    for k in (1, 2, 3):
        assert torch.equal(got[k][ok], ref[k][ok]), k
    assert torch.allclose(got[0][ok], ref[0][ok], rtol=1e-9, atol=1e-9)
    assert torch.allclose(got[4][ok], ref[4][ok], rtol=1e-9, atol=1e-9)
    # no signs, no bounds: the bounded instantiation gives the plain kernel's table
    inf = torch.tensor([[-INF, INF]] * S, dtype=torch.float64)
    zero = G.find_splits(p, hist.to(DEV), totals.to(DEV), valid, torch.zeros_like(mono), inf)
    assert torch.equal(zero, G.find_splits(p, hist.to(DEV), totals.to(DEV), valid))


CSR_BINS = [5, 0, 33, 1, 17, 64, 9]  # a feature's bin count (F = 7)


def csr_case(S, alpha, mcw, seed):
    G = _G()
    g = torch.Generator().manual_seed(seed)
    off = [0]
    for c in CSR_BINS:
        off.append(off[-1] + c)
    F, tb, nbin = len(CSR_BINS), off[-1], max(CSR_BINS)
    hist = torch.zeros(S, tb, 2, dtype=torch.float64)
    hist[..., 0] = torch.randn(S, tb, generator=g, dtype=torch.float64)
    hist[..., 1] = torch.rand(S, tb, generator=g, dtype=torch.float64) * 2
    dense = torch.zeros(S, F, nbin, 2, dtype=torch.float64)  # the same bins, padded
    valid = torch.zeros(F, nbin, dtype=torch.bool)
    for f in range(F):
        dense[:, f, :CSR_BINS[f]] = hist[:, off[f]:off[f + 1]]
        valid[f, :CSR_BINS[f]] = True
    present = dense.sum(2)
    totals = present.max(1).values + torch.rand(S, 2, generator=g, dtype=torch.float64)
    totals[:, 0] = present[:, :, 0].mean(1)
    fvalid = torch.ones(F, dtype=torch.uint8)
    fvalid[0] = 0
    valid[0] = False
    p = G.GBDTParam()
    p.alpha, p.min_child_weight = alpha, mcw
    mono = torch.tensor([1, -1, 1, 0, -1, 1, 0], dtype=torch.int8)
    bounds = _bounds_around(p, totals, g, 0.1)
    return p, hist, off, fvalid, totals, mono, bounds, dense, valid


@pytest.mark.parametrize("S,alpha,mcw,seed", [(5, 0.0, 1.0, 1), (3, 0.5, 0.1, 2)])
def test_split_csr_kernel_with_bounds(S, alpha, mcw, seed):
    """k_split_csr_feat<true, false> / k_split_csr_node against the CSR builder's
    Python search, on compact bins of uneven counts (one feature has none,
    one a single bin, feature 0 is not a candidate)."""
    G = _G()
    from wormhole_amd import _native
    p, hist, off, fvalid, totals, mono, bounds, dense, valid = csr_case(S, alpha, mcw, seed)
    ref = G.split_fields(G.find_splits_csr_ref(p, hist, totals, off, fvalid, mono, bounds))
    # (the padded dense search is the same search: its candidates give the gap)
    dref = G.split_fields(G.find_splits_ref(p, dense, totals, valid, mono, bounds))
    for k in (1, 2, 3):
        assert torch.equal(ref[k], dref[k])
    gap = top_two_gap(G.split_gains(p, dense, totals, valid, mono, bounds)[0])
    ok = torch.isfinite(ref[0])
    assert bool(ok.all()) and bool((gap > 1e-9).all()), gap
    free = G.split_fields(G.find_splits_csr_ref(p, hist, totals, off, fvalid))
    assert not torch.allclose(free[0], ref[0], rtol=1e-6, atol=1e-6)
    cut_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    hip = _native.hip()
    args = (hist.to(DEV), totals.to(DEV), cut_off, fvalid.to(DEV), float(p.alpha),
            float(p.reg_lambda), float(p.min_child_weight))
    got = G.split_fields(hip.gbdt_split_csr(*args, mono=mono.to(DEV),
                                            bounds=bounds.to(DEV)).cpu())
    print("gain", got[0].tolist(), ref[0].tolist())
    assert torch.equal(torch.isfinite(got[0]), ok)
    for k in (1, 2, 3):
        assert torch.equal(got[k], ref[k]), k
    assert torch.allclose(got[0], ref[0], rtol=1e-9, atol=1e-9)
    assert torch.allclose(got[4], ref[4], rtol=1e-9, atol=1e-9)
    inf = torch.tensor([[-INF, INF]] * S, dtype=torch.float64, device=DEV)
    zero = hip.gbdt_split_csr(*args, mono=torch.zeros_like(mono).to(DEV), bounds=inf)
    assert torch.equal(zero, hip.gbdt_split_csr(*args))


# ------------------------------------------------------------- the growers
GN, GF, GDEPTH, GTREES = 20000, 12, 6, 3
GMONO = C.cycled(GF)


@functools.lru_cache(maxsize=None)
def _gpu_inputs():
    G = _G()
    X, y = C.data(GN, GF)
    dm = G.DMatrix.from_dense(X, y, DEV)
    cuts = G.Cuts.build(dm, 64, _bsp())
    return dm, cuts, cuts.bin(dm)


def _grow(monkeypatch, grower, gamma, colsample, mono=GMONO, defer=True):
    """(trees, margins) of GTREES trees by the device level loop ("dev"), the
    per-level host grower ("host") or the Python level loop ("py")."""
    G = _G()
    dm, cuts, B = _gpu_inputs()
    monkeypatch.setattr(G, "HOST_GROWER", grower == "host")
    monkeypatch.setattr(G, "DEFER_TREES", defer)
    p = C.param(G, mono, max_depth=GDEPTH, gamma=gamma, colsample_bytree=colsample)
    obj = G.Objective(p.objective)
    tb = G.TreeBuilder(p, _bsp(), dm, cuts, B)
    margin = torch.full((dm.n,), 0.5, device=DEV)
    gen = torch.Generator().manual_seed(5)
    trees = []
    for _ in range(GTREES):
        tb.sample_features(gen)
        gp = obj.gpair(margin, dm.label, None)
        trees.append(tb._build_py(gp, margin) if grower == "py" else tb._build_native(gp, margin))
    for t in trees:
        t.feat  # (a deferred device tree builds its lists)
    return trees, margin.cpu()


def _same_structure(a, b):
    assert a.feat == b.feat and a.cond == b.cond and a.defl == b.defl
    assert a.left == b.left and a.right == b.right


@pytest.mark.parametrize("gamma,colsample", [(0.0, 1.0), (2.0, 0.6)])
def test_growers_agree_under_constraints(gamma, colsample, monkeypatch):
    dev, mdev = _grow(monkeypatch, "dev", gamma, colsample)
    host, mhost = _grow(monkeypatch, "host", gamma, colsample)
    py, mpy = _grow(monkeypatch, "py", gamma, colsample)
    assert sum(len(t.feat) for t in dev) > 3 * 7  # real trees, not stumps
    for a, b in zip(dev, host):
        _same_structure(a, b)
        assert all(abs(x - z) < 1e-9 for x, z in zip(a.leaf, b.leaf))
        assert all(abs(x - z) < 1e-6 * max(1.0, abs(z)) for x, z in zip(a.gain, b.gain))
    assert torch.equal(mdev, mhost)
    for a, b in zip(host, py):
        _same_structure(a, b)
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))
    assert torch.allclose(mhost, mpy, atol=1e-6)
    for trees in (dev, host, py):
        s = C.structure(trees, GMONO)
        assert all(bad == 0 for _, bad in s.values()), s
        assert sum(n for n, _ in s.values()) > 0
    # the control: the same growers break the guarantee when left alone
    free, _ = _grow(monkeypatch, "dev", gamma, colsample, mono=None)
    assert sum(bad for _, bad in C.structure(free, GMONO).values()) > 0
    # an all-zero vector takes the bounded kernels and grows the unconstrained trees
    zero, mzero = _grow(monkeypatch, "dev", gamma, colsample, mono=(0,) * GF)
    assert [t.dump(None, True) for t in zero] == [t.dump(None, True) for t in free]


def test_deferred_trees_under_constraints(monkeypatch):
    """gamma = 0 with DEFER_TREES: the margins come from the heap walk of the
    device node table (clamped leaf values), the host lists one tree later."""
    G = _G()
    dm, _, _ = _gpu_inputs()
    calls = []
    from wormhole_amd import _native
    hip = _native.hip()
    monkeypatch.setattr(hip, "gbdt_walk_heap",
                        lambda *a, _f=hip.gbdt_walk_heap, **k: (calls.append(1), _f(*a, **k))[1])
    deferred, md = _grow(monkeypatch, "dev", 0.0, 1.0, defer=True)
    assert len(calls) == GTREES  # the deferred path ran
    direct, mn = _grow(monkeypatch, "dev", 0.0, 1.0, defer=False)
    assert len(calls) == GTREES
    b = G.Booster(C.param(G, GMONO), GF)
    b.trees = list(deferred)
    assert torch.allclose(md, b.predict_margin(dm).cpu(), atol=1e-6)
    for a, c in zip(deferred, direct):
        _same_structure(a, c)
        assert a.leaf == c.leaf and a.gain == c.gain and a.cover == c.cover
    assert torch.equal(md, mn)
    assert C.holds(deferred, GMONO)


# ---------------------------------------------------------------- the app
@pytest.fixture()
def work(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    X, y = C.data()
    C.write_libsvm(tmp_path / "train.libsvm", X, y)
    return tmp_path


def test_app_gpu_matches_cpu(work, capsys, monkeypatch):
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    args = ["data=train.libsvm", "objective=reg:linear", "max_depth=5", "eta=0.5", "max_bin=64",
            "num_round=3", "eval_train=1"]
    mono = ["monotone_constraints=(1,-1,0,0)"]

    def run(device, extra, model):
        monkeypatch.setenv("WH_DEVICE", device)
        assert main(args + extra + ["model_out=" + model]) == 0
        out = capsys.readouterr().out
        assert "unknown parameter" not in out
        return ([l for l in out.splitlines() if re.match(r"^\[\d+\]\t", l)],
                G.Booster.load(model, G.GBDTParam()))

    gl, gb = run("auto", mono, "g.model")
    cl, cb = run("cpu", mono, "c.model")
    assert gl == cl and len(gl) == 3
    sl, sb = run("auto", mono + ["dsparse=1"], "s.model")
    for a, b in zip(gb.trees, sb.trees):
        assert a.feat == b.feat and a.cond == b.cond and a.defl == b.defl
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))
    assert len(gb.trees) == len(sb.trees) == 3
    for b in (gb, sb):
        s = C.structure(b.trees, C.MONO)
        assert s[0][0] > 0 and s[1][0] > 0 and s[0][1] == 0 and s[1][1] == 0, s
    _, free = run("auto", [], "f.model")
    s = C.structure(free.trees, C.MONO)
    assert s[0][1] > 0 and s[1][1] > 0, s
    with pytest.raises(SystemExit, match="monotone_constraints"):
        main(args + ["monotone_constraints=(1,1,1,1,1)", "model_out=x.model"])
