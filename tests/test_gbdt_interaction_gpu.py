"""interaction_constraints on the GPU: the admitting split kernels (dense and
CSR, alone and with the bounded search) against their references, the growers
against each other, a level of more than 256 slots, the feature-sharded device
grower, and the app against its CPU run."""
import functools
import json
import math
import os
import re
import socket

import pytest
import torch
import torch.multiprocessing as mp

import _gbdt_interaction_cases as C
import _gbdt_monotone_cases as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
INF = math.inf
BIT63 = -(1 << 63)


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _bsp(device=CPU):
    from wormhole_amd.parallel.bsp import BSP
    os.environ.pop("RANK", None)
    return BSP(device)


def top_two_gap(gain):
    """Per slot (best - second best) / max(1, |best|) over all candidates of
    gain [S, ...] (inf where fewer than two are finite)."""
    flat = gain.reshape(gain.shape[0], -1)
    top = flat.topk(2, dim=1).values
    gap = (top[:, 0] - top[:, 1]) / top[:, 0].abs().clamp_min(1.0)
    return torch.where(torch.isfinite(top[:, 1]), gap, torch.full_like(gap, INF))


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


def _masks(S, F, g):
    """Random group sets over 3 groups: fmask [F] (every seventh feature in no
    group), state [S] with slot 0 all ones and slot 1 admitting nothing."""
    fmask = torch.randint(1, 8, (F,), generator=g)
    fmask[torch.arange(F) % 7 == 6] = BIT63
    state = torch.randint(1, 8, (S,), generator=g)
    state[0] = -1
    state[1] = 0
    return fmask, state


# ------------------------------------------------------------ split kernels
def dense_case(S, F, nbin, alpha, mcw):
    """Random histograms with missing mass in every feature, a candidate mask
    with holes, signs, bounds, feature masks and slot states."""
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
    mono = torch.randint(-1, 2, (F,), generator=g).to(torch.int8)
    bounds = _bounds_around(p, totals, g, 0.5 / math.sqrt(nbin))
    fmask, state = _masks(S, F, g)
    return p, hist, totals, valid, mono, bounds, fmask, state


DENSE_SHAPES = [(5, 7, 33, 0.0, 1.0), (3, 28, 256, 0.5, 0.1), (2, 4, 1000, 0.0, 5.0)]


@pytest.mark.parametrize("with_mono", [False, True])
@pytest.mark.parametrize("S,F,nbin,alpha,mcw", DENSE_SHAPES)
def test_split_kernel_with_admission(S, F, nbin, alpha, mcw, with_mono):
    """k_split_feat<false, true> / <true, true> with k_split_node against
    find_splits_ref: the same feature / bin / direction (the reference's best
    beats its runner-up by more than the tolerance, so the index is well
    defined), gains and left sums to fp64 rounding (rtol = atol = 1e-9, both
    sides fp64)."""
    G = _G()
    p, hist, totals, valid, mono, bounds, fmask, state = dense_case(S, F, nbin, alpha, mcw)
    mb = (mono, bounds) if with_mono else (None, None)
    gains, _ = G.split_gains(p, hist, totals, valid, *mb, fmask, state)
    gap = top_two_gap(gains)
    ref_t = G.find_splits_ref(p, hist, totals, valid, *mb, fmask, state)
    ref = G.split_fields(ref_t)
    ok = torch.isfinite(ref[0])
    assert bool(ok[0]) and not bool(ok[1])  # all ones admits, no bit admits nothing
    assert bool((gap[ok] > 1e-9).all()), gap
    free_t = G.find_splits_ref(p, hist, totals, valid, *mb)
    assert not torch.equal(free_t, ref_t)  # the masks bite
    assert torch.equal(free_t[0], ref_t[0])  # ... but not the all-ones slot
    hd, td = hist.to(DEV), totals.to(DEV)
    got_t = G.find_splits(p, hd, td, valid, *mb, fmask, state)
    got = G.split_fields(got_t)
    print("gain", got[0].tolist(), ref[0].tolist())
    assert torch.equal(torch.isfinite(got[0]), ok)
    assert bool((got[0][~ok] == -INF).all())
    for k in (1, 2, 3):
        assert torch.equal(got[k][ok], ref[k][ok]), k
    assert torch.allclose(got[0][ok], ref[0][ok], rtol=1e-9, atol=1e-9)
    assert torch.allclose(got[4][ok], ref[4][ok], rtol=1e-9, atol=1e-9)
    # admitted features only
    adm = G.admitted(fmask, state)
    assert all(bool(adm[s, int(got[1][s])]) for s in range(S) if bool(ok[s]))
    plain = G.find_splits(p, hd, td, valid, *mb)
    assert not torch.equal(plain, got_t)  # the constrained table differs from the free one
    # one group of every feature, every slot a root: bit-equal to the kernel without the flag
    one = G.find_splits(p, hd, td, valid, *mb, torch.ones(F, dtype=torch.int64),
                        torch.full((S,), -1, dtype=torch.int64))
    assert torch.equal(one, plain)


CSR_BINS = [5, 0, 33, 1, 17, 64, 9]  # a feature's bin count (F = 7)


def csr_case(bins, S, alpha, mcw, seed, fmask, state, mono=None):
    """Compact histograms over ``bins`` (a feature's bin count) and the same
    bins padded to a dense table, whose search is the fp64 reference."""
    G = _G()
    g = torch.Generator().manual_seed(seed)
    off = [0]
    for c in bins:
        off.append(off[-1] + c)
    F, tb, nbin = len(bins), off[-1], max(bins)
    hist = torch.zeros(S, tb, 2, dtype=torch.float64)
    hist[..., 0] = torch.randn(S, tb, generator=g, dtype=torch.float64)
    hist[..., 1] = torch.rand(S, tb, generator=g, dtype=torch.float64) * 2
    dense = torch.zeros(S, F, nbin, 2, dtype=torch.float64)
    valid = torch.zeros(F, nbin, dtype=torch.bool)
    for f in range(F):
        dense[:, f, :bins[f]] = hist[:, off[f]:off[f + 1]]
        valid[f, :bins[f]] = True
    present = dense.sum(2)
    totals = present.max(1).values + torch.rand(S, 2, generator=g, dtype=torch.float64)
    totals[:, 0] = present[:, :, 0].mean(1)
    fvalid = torch.ones(F, dtype=torch.uint8)
    fvalid[0] = 0
    valid[0] = False
    p = G.GBDTParam()
    p.alpha, p.min_child_weight = alpha, mcw
    if mono is None:
        mono = torch.randint(-1, 2, (F,), generator=g).to(torch.int8)
    bounds = _bounds_around(p, totals, g, 0.1)
    return p, hist, off, fvalid, totals, mono, bounds, dense, valid


def _check_csr(case, fmask, state, with_mono):
    """-> the kernel's split fields, checked against the padded dense search
    (fp64) and, for the picked indexes, the CSR builder's Python search."""
    G = _G()
    from wormhole_amd import _native
    p, hist, off, fvalid, totals, mono, bounds, dense, valid = case
    S = hist.shape[0]
    mb = (mono, bounds) if with_mono else (None, None)
    ref = G.split_fields(G.find_splits_ref(p, dense, totals, valid, *mb, fmask, state))
    pyref = G.split_fields(G.find_splits_csr_ref(p, hist, totals, off, fvalid, *mb, fmask, state))
    ok = torch.isfinite(ref[0])
    assert torch.equal(torch.isfinite(pyref[0]), ok)
    for k in (1, 2, 3):
        assert torch.equal(ref[k][ok], pyref[k][ok])
    gap = top_two_gap(G.split_gains(p, dense, totals, valid, *mb, fmask, state)[0])
    assert bool((gap[ok] > 1e-9).all()), gap
    hip = _native.hip()
    cut_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    args = (hist.to(DEV), totals.to(DEV), cut_off, fvalid.to(DEV), float(p.alpha),
            float(p.reg_lambda), float(p.min_child_weight))
    kw = dict(mono=mono.to(DEV), bounds=bounds.to(DEV)) if with_mono else {}
    got_t = hip.gbdt_split_csr(*args, **kw, fmask=fmask.to(DEV), state=state.to(DEV)).cpu()
    got = G.split_fields(got_t)
    print("gain", got[0].tolist(), ref[0].tolist())
    assert torch.equal(torch.isfinite(got[0]), ok)
    for k in (1, 2, 3):
        assert torch.equal(got[k][ok], ref[k][ok]), k
    assert torch.allclose(got[0][ok], ref[0][ok], rtol=1e-9, atol=1e-9)
    assert torch.allclose(got[4][ok], ref[4][ok], rtol=1e-9, atol=1e-9)
    plain = hip.gbdt_split_csr(*args, **kw).cpu()
    assert not torch.equal(plain, got_t)
    F = len(off) - 1
    one = hip.gbdt_split_csr(*args, **kw, fmask=torch.ones(F, dtype=torch.int64, device=DEV),
                             state=torch.full((S,), -1, dtype=torch.int64, device=DEV)).cpu()
    assert torch.equal(one, plain)
    return got, ok


@pytest.mark.parametrize("with_mono", [False, True])
@pytest.mark.parametrize("S,alpha,mcw,seed", [(5, 0.0, 1.0, 1), (3, 0.5, 0.1, 2)])
def test_split_csr_kernel_with_admission(S, alpha, mcw, seed, with_mono):
    """k_split_csr_feat<false, true> / <true, true> on compact bins of uneven counts
    (one feature has none, one a single bin, feature 0 is not a candidate)."""
    fmask = torch.tensor([1, 1, 3, 2, 6, 4, BIT63], dtype=torch.int64)
    state = torch.tensor([-1, 0, 1, 2, 4][:S], dtype=torch.int64)
    mono = torch.tensor([1, -1, 1, 0, -1, 1, 0], dtype=torch.int8)
    case = csr_case(CSR_BINS, S, alpha, mcw, seed, fmask, state, mono)
    got, ok = _check_csr(case, fmask, state, with_mono)
    assert ok.tolist() == [True, False, True, True, True][:S]
    adm = _G().admitted(fmask, state)
    assert all(bool(adm[s, int(got[1][s])]) for s in range(S) if bool(ok[s]))


@pytest.mark.parametrize("with_mono", [False, True])
def test_split_csr_kernel_two_blocks(with_mono):
    """F = 300, 0..3 bins per feature: two blocks of the 256-wide grid, with
    admitted features on both sides of the boundary."""
    F = 300
    g = torch.Generator().manual_seed(9)
    bins = torch.randint(0, 4, (F,), generator=g).tolist()
    bins[255], bins[256] = 3, 3
    # group 0: the even features below 256; group 1: features from 256 on;
    # group 2: every third feature; the others in none
    fmask = torch.zeros(F, dtype=torch.int64)
    idx = torch.arange(F)
    fmask[(idx < 256) & (idx % 2 == 0)] |= 1
    fmask[idx >= 256] |= 2
    fmask[idx % 3 == 0] |= 4
    fmask[fmask == 0] = BIT63
    state = torch.tensor([-1, 0, 1, 2, 4, 3], dtype=torch.int64)
    case = csr_case(bins, 6, 0.0, 0.5, 4, fmask, state)
    got, ok = _check_csr(case, fmask, state, with_mono)
    assert ok.tolist() == [True, False, True, True, True, True]
    f = got[1].tolist()
    assert f[2] < 256 and f[2] % 2 == 0 and f[3] >= 256 and f[4] % 3 == 0
    adm = _G().admitted(fmask, state)
    assert all(bool(adm[s, f[s]]) for s in range(6) if bool(ok[s]))


# ------------------------------------------------------------- the growers
GN, GF, GDEPTH, GTREES = 20000, 12, 6, 3
GGROUPS = ((0, 2, 4, 6, 8), (1, 3, 5, 7, 9), (4, 5, 10))  # feature 11 in none
GMONO = M.cycled(GF)


@functools.lru_cache(maxsize=None)
def _gpu_inputs():
    G = _G()
    X, y = M.data(GN, GF)
    dm = G.DMatrix.from_dense(X, y, DEV)
    cuts = G.Cuts.build(dm, 64, _bsp())
    return dm, cuts, cuts.bin(dm)


def _grow(monkeypatch, grower, gamma, colsample, groups=GGROUPS, mono=None, defer=True):
    """(trees, margins) of GTREES trees by the device level loop ("dev"), the
    per-level host grower ("host") or the Python level loop ("py")."""
    G = _G()
    dm, cuts, B = _gpu_inputs()
    monkeypatch.setattr(G, "HOST_GROWER", grower == "host")
    monkeypatch.setattr(G, "DEFER_TREES", defer)
    p = C.param(G, groups, mono, max_depth=GDEPTH, max_bin=64, gamma=gamma,
                colsample_bytree=colsample)
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


@pytest.mark.parametrize("with_mono", [False, True])
@pytest.mark.parametrize("gamma,colsample", [(0.0, 1.0), (2.0, 0.6)])
def test_growers_agree_under_constraints(gamma, colsample, with_mono, monkeypatch):
    """gamma = 0 takes the deferred path of the device loop (DEFER_TREES)."""
    mono = GMONO if with_mono else None
    dev, mdev = _grow(monkeypatch, "dev", gamma, colsample, mono=mono)
    host, mhost = _grow(monkeypatch, "host", gamma, colsample, mono=mono)
    py, mpy = _grow(monkeypatch, "py", gamma, colsample, mono=mono)
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
        bad, total = C.broken(trees, GGROUPS)
        assert bad == 0 and total > 3 * 4, (bad, total)
        if with_mono:
            assert M.holds(trees, GMONO)
    # the control: the same growers break the rule when left alone
    free, _ = _grow(monkeypatch, "dev", gamma, colsample, groups=None, mono=mono)
    assert C.broken(free, GGROUPS)[0] > 0
    # one group of every feature takes the admitting kernels and grows the free trees
    one, _ = _grow(monkeypatch, "dev", gamma, colsample, groups=(tuple(range(GF)),), mono=mono)
    assert [t.dump(None, True) for t in one] == [t.dump(None, True) for t in free]


def test_deferred_trees_under_constraints(monkeypatch):
    """gamma = 0 with DEFER_TREES: the device node table is walked on the
    device; the same trees and margins as the direct path."""
    calls = []
    from wormhole_amd import _native
    hip = _native.hip()
    monkeypatch.setattr(hip, "gbdt_walk_heap",
                        lambda *a, _f=hip.gbdt_walk_heap, **k: (calls.append(1), _f(*a, **k))[1])
    deferred, md = _grow(monkeypatch, "dev", 0.0, 1.0, defer=True)
    assert len(calls) == GTREES  # the deferred path ran
    direct, mn = _grow(monkeypatch, "dev", 0.0, 1.0, defer=False)
    assert len(calls) == GTREES
    for a, c in zip(deferred, direct):
        _same_structure(a, c)
        assert a.leaf == c.leaf and a.gain == c.gain and a.cover == c.cover
    assert torch.equal(md, mn)
    assert C.broken(deferred, GGROUPS)[0] == 0


def test_device_loop_level_of_more_than_256_slots(monkeypatch):
    """max_depth = 10, min_child_weight = 0, n = 4000: the device loop's
    level 9 holds 512 slots, so k_gd_apply's stride loop carries the states;
    the tree of the Python level loop, and the path rule. The margin starts
    at the labels' mean (2.0), so the gradients are centred and lambda stops
    few splits: 165 of the constrained tree's splits are at level 9, 96 of
    them in slots from 256 on (counted on the CPU path)."""
    G = _G()
    X, y = C.data(n=4000)
    dm = G.DMatrix.from_dense(X, y, DEV)
    p = C.param(G, C.GROUPS, max_depth=10, min_child_weight=0.0)
    cuts = G.Cuts.build(dm, p.max_bin, _bsp())
    monkeypatch.setattr(G, "HOST_GROWER", False)
    monkeypatch.setattr(G, "DEFER_TREES", False)
    tb = G.TreeBuilder(p, _bsp(), dm, cuts, cuts.bin(dm))
    base = 2.0
    gp = G.Objective(p.objective).gpair(torch.full((dm.n,), base, device=DEV), dm.label, None)
    m_dev, m_py = torch.full((dm.n,), base, device=DEV), torch.full((dm.n,), base, device=DEV)
    dev = tb._build_native(gp, m_dev)
    py = tb._build_py(gp, m_py)

    def high_splits(t, i=0, d=0, pos=0):
        """splits at level 9 in slots from 256 on (heap position in the level)"""
        if t.feat[i] < 0:
            return 0
        return (int(d == 9 and pos >= 256) + high_splits(t, t.left[i], d + 1, 2 * pos)
                + high_splits(t, t.right[i], d + 1, 2 * pos + 1))

    assert high_splits(dev) > 32
    _same_structure(dev, py)
    assert all(abs(x - z) < 1e-6 for x, z in zip(dev.leaf, py.leaf))
    assert torch.allclose(m_dev.cpu(), m_py.cpu(), atol=1e-6)
    bad, total = C.broken([dev])
    assert bad == 0 and total > 256
    # the control
    free = G.TreeBuilder(C.param(G, None, max_depth=10, min_child_weight=0.0), _bsp(), dm, cuts,
                         cuts.bin(dm))._build_native(gp, torch.full((dm.n,), base, device=DEV))
    assert C.broken([free])[0] > 0


# ----------------------------------------------- feature-sharded device loop
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _xtrain(bsp, device):
    G = _G()
    X, y = C.data()
    rows = torch.arange(X.shape[0])[bsp.rank::bsp.world]
    dm = G.DMatrix.from_dense(X[rows], y[rows], device)
    p = C.param(G, C.GROUPS)
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    tb = G.TreeBuilder(p, bsp, dm, cuts, cuts.bin(dm))
    obj = G.Objective(p.objective)
    margin = torch.full((dm.n,), 0.5, device=device)
    trees = [tb.build(obj.gpair(margin, dm.label, None), margin) for _ in range(C.ROUNDS)]
    return [t.dump(with_stats=True) for t in trees], trees, tb.xchg is not None


def _gpu_main(rank, world, port, out, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), WH_GBDT_XCHG=mode, WH_COMM_BACKEND="gloo")
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    from wormhole_amd.parallel.bsp import BSP
    dev = torch.device("cuda", 0)
    bsp = BSP(dev)  # ranks share the GPU: gloo-staged collectives
    dumps, _, sharded = _xtrain(bsp, dev)
    if rank == 0:
        json.dump({"dumps": dumps, "sharded": sharded}, open(out, "w"))
    bsp.finalize()


@pytest.mark.parametrize("world,mode", [(2, "rs"), (3, "rs"), (2, "allreduce")])
def test_device_grower_feature_sharded(world, mode, tmp_path):
    """gbdt_grow_dev with the feature reduce-scatter: the split search reads
    this rank's slice of the masks, the apply kernel the picked, global
    feature -- identical trees to one rank."""
    one, trees, _ = _xtrain(_bsp(DEV), DEV)
    bad, total = C.broken(trees)
    assert bad == 0 and total > 2 * C.ROUNDS
    out = str(tmp_path / "g.json")
    mp.spawn(_gpu_main, args=(world, _free_port(), out, mode), nprocs=world, join=True)
    r = json.load(open(out))
    assert r["sharded"] == (mode == "rs")
    assert r["dumps"] == one


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
    """The app on the GPU against its CPU run: the same model dump with the
    64-bit fixed-point histograms, whose sums are exact far below the dump's
    six digits. The default 32-bit histogram passes round every row's
    gradient to a multiple of 2^-16 .. 2^-17 of the largest
    (models/gbdt.py _hist_scale), and a small node's sum, taken by
    subtraction, inherits the rounding of its whole parent: there the trees
    agree in structure and the evaluation lines in all their digits, and the
    dense and the CSR kernels, which sum the same rounded rows, in the leaves."""
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    args = ["data=train.libsvm", "objective=reg:linear", "max_depth=4", "eta=0.5", "max_bin=16",
            "num_round=3", "eval_train=1"]
    inter = ["interaction_constraints=" + C.spell(C.GROUPS)]

    def run(device, extra, model):
        monkeypatch.setenv("WH_DEVICE", device)
        assert main(args + extra + ["model_out=" + model]) == 0
        out = capsys.readouterr().out
        assert "unknown parameter" not in out
        return ([l for l in out.splitlines() if re.match(r"^\[\d+\]\t", l)],
                G.Booster.load(model, G.GBDTParam()))

    cl, cb = run("cpu", inter, "c.model")
    monkeypatch.setattr(G, "HIST32", False)
    xl, xb = run("auto", inter, "x.model")
    assert xb.dump() == cb.dump() and "yes=" in cb.dump()
    assert xl == cl and len(cl) == 3
    monkeypatch.setattr(G, "HIST32", True)
    gl, gb = run("auto", inter, "g.model")
    assert gl == cl
    sl, sb = run("auto", inter + ["dsparse=1"], "s.model")
    for other in (gb, sb):
        for a, b in zip(cb.trees, other.trees):
            assert a.feat == b.feat and a.cond == b.cond and a.defl == b.defl
    for a, b in zip(gb.trees, sb.trees):
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))
    assert len(gb.trees) == len(sb.trees) == len(cb.trees) == 3
    for b in (gb, sb, cb):
        bad, total = C.broken(b.trees)
        assert bad == 0 and total > 6
    _, free = run("auto", [], "f.model")
    assert C.broken(free.trees)[0] > 0
    with pytest.raises(SystemExit, match="interaction_constraints"):
        main(args + ["interaction_constraints=[[0,7]]", "model_out=x2.model"])
    assert not os.path.exists("x2.model")
