"""monotone_constraints on the CPU path (the Python level loop, which is also
the native growers' reference): parsing, the bounded split search against a
brute-force loop, the guarantee on every tree (with an unconstrained control
that breaks it), dense = CSR, multi-class, the command line, several ranks."""
import functools
import json
import math
import os
import re
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

import _gbdt_monotone_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKER = os.path.join(ROOT, "tracker", "dmlc_local.py")
XGB = os.path.join(ROOT, "bin", "xgboost.dmlc")
CPU = torch.device("cpu")


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _bsp():
    from wormhole_amd.parallel.bsp import BSP
    os.environ.pop("RANK", None)
    return BSP(CPU)


# ------------------------------------------------------------------ parsing
def test_parsing():
    G = _G()
    for text in ("(1,-1)", "1,-1", "( 1, -1 )", "'(1,-1)'", '"1, -1"'):
        p = G.GBDTParam()
        assert p.set("monotone_constraints", text) is True
        assert p.monotone == [1, -1], text
    p = G.GBDTParam()
    assert p.set("monotone_constraints", '"( 1, 0 ,-1 )"') and p.monotone == [1, 0, -1]
    assert p.monotone_vector(5).tolist() == [1, 0, -1, 0, 0]  # padded with zeros
    assert p.monotone_vector(5).dtype == torch.int8
    assert p.monotone_vector(3).tolist() == [1, 0, -1]
    assert G.GBDTParam().monotone_vector(4) is None  # not set
    for bad in ("(1,2)", "1,a", "(1,,0)", "0.5", ""):
        with pytest.raises(SystemExit, match="monotone_constraints"):
            G.GBDTParam().set("monotone_constraints", bad)
    with pytest.raises(SystemExit, match="monotone_constraints"):
        p.monotone_vector(2)  # more entries than features


def test_quoted_value_survives_the_conf_parser(tmp_path):
    from wormhole_amd.apps.xgboost_app import parse_args
    conf = tmp_path / "m.conf"
    conf.write_text('max_depth = 3\nmonotone_constraints = "( 1, 0 ,-1 )"\n')
    items = dict(parse_args([str(conf)]))
    assert items["monotone_constraints"] == "( 1, 0 ,-1 )"
    p = _G().GBDTParam()
    assert p.set("monotone_constraints", items["monotone_constraints"]) and p.monotone == [1, 0, -1]
    # the command line, with and without quotes
    for arg in ("monotone_constraints=(1,-1)", 'monotone_constraints="(1,-1)"'):
        (k, v), = parse_args([arg])
        p = _G().GBDTParam()
        assert p.set(k, v) and p.monotone == [1, -1]


# ------------------------------------------- bounded search vs brute force
def _side(G_, H_, lo, hi, alpha, lam, mcw):
    """(gain, weight) of one side, from the issue's formulas."""
    T = G_ - alpha if G_ > alpha else (G_ + alpha if G_ < -alpha else 0.0)
    w0 = 0.0 if H_ < mcw else -T / (H_ + lam)
    w = min(max(w0, lo), hi)
    if w == w0:
        return (0.0 if H_ < mcw else T * T / (H_ + lam)), w
    return -(2 * T * w + (H_ + lam) * w * w), w


def _brute(hist, totals, valid, mono, bounds, alpha, lam, mcw):
    S, F, nbin = hist.shape[:3]
    out = []
    rejected = [[0] * F for _ in range(S)]  # candidates dropped by the order check
    for s in range(S):
        TG, TH = float(totals[s, 0]), float(totals[s, 1])
        lo, hi = float(bounds[s, 0]), float(bounds[s, 1])
        parent = _side(TG, TH, lo, hi, alpha, lam, mcw)[0]
        best = (-math.inf, 0, 0, 0, 0.0, 0.0)
        for f in range(F):
            pg = float(hist[s, f, :, 0].sum())
            ph = float(hist[s, f, :, 1].sum())
            for b in range(nbin):
                if not bool(valid[f, b]):
                    continue
                cg = float(hist[s, f, :b + 1, 0].sum())
                ch = float(hist[s, f, :b + 1, 1].sum())
                for d in (0, 1):
                    GL = cg + ((TG - pg) if d else 0.0)
                    HL = ch + ((TH - ph) if d else 0.0)
                    GR, HR = TG - GL, TH - HL
                    if not (HL >= mcw and HR >= mcw):
                        continue
                    gl, wl = _side(GL, HL, lo, hi, alpha, lam, mcw)
                    gr, wr = _side(GR, HR, lo, hi, alpha, lam, mcw)
                    c = int(mono[f])
                    if (c > 0 and wl > wr) or (c < 0 and wl < wr):
                        rejected[s][f] += 1
                        continue
                    g = gl + gr - parent
                    if g > best[0]:
                        best = (g, f, b, d, GL, HL)
        out.append(best)
    return out, rejected


@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_bounded_search_matches_brute_force(alpha):
    G = _G()
    S, F, nbin = 4, 4, 9
    g = torch.Generator().manual_seed(5)
    mono = torch.tensor([1, -1, 0, 0], dtype=torch.int8)
    hist = torch.zeros(S, F, nbin, 2, dtype=torch.float64)
    hist[..., 0] = torch.randn(S, F, nbin, generator=g, dtype=torch.float64) * 3
    hist[..., 1] = torch.rand(S, F, nbin, generator=g, dtype=torch.float64) * 4 + 0.5
    # slot 2: feature 0 (+1) has g ascending around 0, so every left weight is
    # above its right one, feature 1 (-1) the mirror image: all their
    # candidates are rejected; features 2 and 3 hold the same bins shuffled
    ramp = torch.linspace(-4, 4, nbin, dtype=torch.float64)
    hist[2, :, :, 1] = 2.0
    hist[2, 0, :, 0] = ramp
    hist[2, 1, :, 0] = ramp.flip(0)
    hist[2, 2, :, 0] = ramp[torch.randperm(nbin, generator=g)]
    hist[2, 3, :, 0] = ramp[torch.randperm(nbin, generator=g)]
    # slot 3: too little hessian for any pair of children
    hist[3, :, :, 1] = 0.01
    # node totals: slots 0 and 1 carry missing mass in every feature (>= 1.5 of
    # hessian), slots 2 and 3 none in h
    totals = hist[:, 0].sum(1)
    totals[:2, 0] += 0.7
    totals[:2, 1] = hist[:2, :, :, 1].sum(2).max(1).values + 1.5
    p = G.GBDTParam()
    p.alpha, p.reg_lambda, p.min_child_weight = alpha, 1.0, 1.0
    w0 = [p.calc_weight(float(t[0]), float(t[1])) for t in totals]
    inf = math.inf
    bounds = torch.tensor([[-inf, inf], [w0[1] - 0.02, w0[1] + 0.02], [-inf, inf], [-inf, inf]],
                          dtype=torch.float64)
    valid = torch.ones(F, nbin, dtype=torch.bool)
    valid[3, 7:] = False
    valid[0, 0] = False
    got = G.find_splits_ref(p, hist, totals, valid, mono, bounds)
    want, rejected = _brute(hist, totals, valid, mono, bounds, alpha, p.reg_lambda,
                            p.min_child_weight)
    # the cases are what they claim to be
    assert want[0][0] > 0 and want[1][0] > -inf
    lo1, hi1 = bounds[1].tolist()
    wl = _side(want[1][4], want[1][5], lo1, hi1, alpha, 1.0, 1.0)[1]
    wr = _side(float(totals[1, 0]) - want[1][4], float(totals[1, 1]) - want[1][5], lo1, hi1,
               alpha, 1.0, 1.0)[1]
    assert {wl, wr} <= {lo1, hi1}, "slot 1: both children clamp"
    assert rejected[2][0] == 2 * (nbin - 2) and rejected[2][1] == 2 * (nbin - 1)
    assert want[2][1] in (2, 3) and want[2][0] > 0
    assert want[3][0] == -inf
    for s in range(S):
        gain, f, b, d, GL, HL = want[s]
        assert math.isfinite(float(got[s, 0])) == math.isfinite(gain), s
        if not math.isfinite(gain):
            assert float(got[s, 0]) == -inf
            continue
        assert (int(got[s, 1]), int(got[s, 2]), int(got[s, 3])) == (f, b, d), s
        assert float(got[s, 0]) == pytest.approx(gain, rel=1e-12, abs=1e-12)
        assert float(got[s, 4]) == pytest.approx(GL, rel=1e-12, abs=1e-12)
        assert float(got[s, 5]) == pytest.approx(HL, rel=1e-12, abs=1e-12)
    # without bounds and signs the bounded form is the plain search
    free = G.find_splits_ref(p, hist, totals, valid, torch.zeros(F, dtype=torch.int8),
                             torch.tensor([[-inf, inf]] * S, dtype=torch.float64))
    assert torch.equal(free, G.find_splits_ref(p, hist, totals, valid))


# ------------------------------------------------------------ the guarantee
@functools.lru_cache(maxsize=None)
def _model(sparse, gamma, mono):
    G = _G()
    X, y = C.data()
    dm = C.dmatrix(G, X, y, CPU, sparse)
    return C.train(G, _bsp(), dm, C.param(G, mono, gamma=float(gamma)))[0]


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("gamma", [0, 1])
def test_guarantee_on_every_tree(sparse, gamma):
    G = _G()
    X, _ = C.data()
    b = _model(sparse, gamma, C.MONO)
    s = C.structure(b.trees, C.MONO)
    assert s[0][0] > 0 and s[1][0] > 0, s  # the constrained features are split on
    assert s[0][1] == 0 and s[1][1] == 0, s
    up, down = C.sweep(G, b, X, 0, CPU), C.sweep(G, b, X, 1, CPU)
    assert bool((up[:, 1:] >= up[:, :-1]).all())
    assert bool((down[:, 1:] <= down[:, :-1]).all())
    assert bool((up[:, -1] > up[:, 0]).all()) and bool((down[:, -1] < down[:, 0]).all())
    # the control: the same data need the constraint
    c = C.structure(_model(sparse, gamma, None).trees, C.MONO)
    assert c[0][1] > 0 and c[1][1] > 0, c
    free = _model(sparse, gamma, None)
    up = C.sweep(G, free, X, 0, CPU)
    assert not bool((up[:, 1:] >= up[:, :-1]).all())


def test_all_zero_vector_changes_nothing():
    zero, none = _model(False, 0, (0, 0, 0, 0)), _model(False, 0, None)
    assert zero.dump(None, True) == none.dump(None, True)
    assert len(none.trees) == C.ROUNDS and "yes=" in none.dump()
    zero, none = _model(False, 1, (0, 0, 0, 0)), _model(False, 1, None)
    assert zero.dump(None, True) == none.dump(None, True)
    # the CSR builder's Python search takes unconstrained gains in fp32 (its
    # torch scalars) and bounded ones in fp64: the trees agree, the printed
    # gains to fp32 precision
    zero, none = _model(True, 0, (0, 0, 0, 0)), _model(True, 0, None)
    assert zero.dump() == none.dump()


@pytest.mark.parametrize("gamma", [0, 1])
def test_csr_builder_grows_the_dense_trees(gamma):
    dense, csr = _model(False, gamma, C.MONO), _model(True, gamma, C.MONO)
    assert len(dense.trees) == len(csr.trees) == C.ROUNDS
    for a, b in zip(dense.trees, csr.trees):
        assert a.feat == b.feat and a.cond == b.cond and a.defl == b.defl
        assert all(abs(x - z) < 1e-9 for x, z in zip(a.leaf, b.leaf))


def test_multiclass_trees_are_constrained():
    G = _G()
    X, y = C.data()
    q = torch.quantile(y, torch.tensor([1 / 3, 2 / 3]))
    lab = (y > q[0]).float() + (y > q[1]).float()
    res = {}
    for mono in (C.MONO, None):
        p = C.param(G, mono, objective="multi:softprob", num_class=3)
        b, _ = C.train(G, _bsp(), C.dmatrix(G, X, lab, CPU), p, rounds=3)
        assert len(b.trees) == 9
        res[mono] = [C.structure(b.trees[k::3], C.MONO) for k in range(3)]
    for k in range(3):
        s = res[C.MONO][k]
        assert s[0][1] == 0 and s[1][1] == 0, (k, s)
        assert s[0][0] + s[1][0] > 0
    assert sum(s[0][1] + s[1][1] for s in res[None]) > 0  # the control


# ------------------------------------------------------------ command line
def _cli(args, cwd, n=1):
    env = dict(os.environ, WH_DEVICE="cpu")
    return subprocess.run([sys.executable, TRACKER, "-n", str(n), XGB] + args, cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=300)


def _rounds(out):
    return [l for l in out.splitlines() if re.match(r"^\[\d+\]\t", l)]


def test_cli(tmp_path):
    G = _G()
    X, y = C.data()
    C.write_libsvm(tmp_path / "train.libsvm", X, y)
    conf = tmp_path / "m.conf"
    conf.write_text('objective = "reg:linear"\nmax_depth = 5\neta = 0.5\nmax_bin = 64\n'
                    'num_round = 4\neval_train = 1\ndata = "train.libsvm"\n'
                    'monotone_constraints = "(1,-1,0,0)"\n')
    r1 = _cli(["m.conf", "model_out=a.model"], tmp_path, 1)
    r3 = _cli(["m.conf", "model_out=b.model"], tmp_path, 3)
    assert r1.returncode == 0 and r3.returncode == 0, (r1.stderr[-2000:], r3.stderr[-2000:])
    assert "unknown parameter" not in r1.stdout + r1.stderr
    a = G.Booster.load(str(tmp_path / "a.model"), G.GBDTParam())
    b = G.Booster.load(str(tmp_path / "b.model"), G.GBDTParam())
    assert a.dump() == b.dump()
    assert _rounds(r1.stdout) == _rounds(r3.stdout) and len(_rounds(r1.stdout)) == 4
    assert len(a.trees) == 4 and C.holds(a.trees, C.MONO)
    s = C.structure(a.trees, C.MONO)
    assert s[0][0] > 0 and s[1][0] > 0
    # the command line overrides the conf; five entries on four features
    bad = _cli(["m.conf", "monotone_constraints=(1,1,1,1,1)", "model_out=c.model"], tmp_path, 1)
    assert bad.returncode != 0
    assert "monotone_constraints" in bad.stdout + bad.stderr
    assert not (tmp_path / "c.model").exists()


# ------------------------------------------------ feature-sharded exchange
XROUNDS = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _xtrain(bsp):
    G = _G()
    X, y = C.data()
    rows = torch.arange(X.shape[0])[bsp.rank::bsp.world]
    dm = G.DMatrix.from_dense(X[rows], y[rows], CPU)
    b, _ = C.train(G, bsp, dm, C.param(G, C.MONO), rounds=XROUNDS)
    return [t.dump(with_stats=True) for t in b.trees], b


def _xmain(rank, world, port, out, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), WH_GBDT_XCHG=mode)
    torch.set_num_threads(1)
    from wormhole_amd.parallel.bsp import BSP
    bsp = BSP(CPU)
    dumps, _ = _xtrain(bsp)
    if rank == 0:
        json.dump(dumps, open(out, "w"))
    bsp.finalize()


@pytest.fixture(scope="module")
def single():
    dumps, b = _xtrain(_bsp())
    assert C.holds(b.trees, C.MONO)
    return dumps


@pytest.mark.parametrize("world,mode", [(2, "rs"), (4, "rs"), (2, "allreduce"), (4, "allreduce")])
def test_feature_sharded_trees_equal_single_rank(single, world, mode, tmp_path):
    out = str(tmp_path / "x.json")
    mp.spawn(_xmain, args=(world, _free_port(), out, mode), nprocs=world, join=True)
    assert json.load(open(out)) == single
    assert any("yes=" in d for d in single)
