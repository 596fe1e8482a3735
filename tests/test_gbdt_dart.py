"""booster=dart on the CPU path: the walk plan and the tree table, the draw,
the closed forms of the weights, equivalence with gbtree, the kept margins
against predict_margin, the model file and state, the model's consumers, and
the app."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import _gbdt_dart_cases as D
import _gbdt_forest_cases as fc
import _gbdt_monotone_cases as M
import _gbdt_objective_cases as C

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _hip():
    from wormhole_amd import _native
    return _native.hip()


def _bsp():
    from wormhole_amd.parallel.bsp import BSP
    os.environ.pop("RANK", None)
    return BSP(CPU)


# ------------------------------------------------------- 1. plan and pack
def test_plan():
    hip = _hip()
    assert hip.gbdt_dart_lds_nodes() >= 511 * 4
    assert hip.gbdt_dart_plan(tree_sizes=[3, 5], sel=[], lds_nodes=16) == []
    assert hip.gbdt_dart_plan(tree_sizes=[1], sel=[0], lds_nodes=16) == [(0, 1, 1, True, [0])]
    # three chunks, the last one partial, over a selection with gaps
    sel = [0, 2, 3, 5, 6, 8, 9]
    got = hip.gbdt_dart_plan(tree_sizes=[7] * 10, sel=sel, lds_nodes=21)
    assert got == [(0, 3, 21, True, [0, 7, 14]), (3, 3, 21, True, [0, 7, 14]),
                   (6, 1, 7, True, [0])]
    # an over-budget tree in the middle is not staged; neither is one outside the table
    got = hip.gbdt_dart_plan(tree_sizes=[7, 7, 40, 7, 0, 7], sel=[0, 1, 2, 3, 4, 5], lds_nodes=21)
    assert got == [(0, 2, 14, True, [0, 7]), (2, 1, 40, False, []), (3, 1, 7, True, [0]),
                   (4, 1, 0, False, []), (5, 1, 7, True, [0])]
    # the tree cap of a chunk
    cap = hip.gbdt_dart_max_trees()
    got = hip.gbdt_dart_plan(tree_sizes=[1] * (cap + 1), sel=list(range(cap + 1)),
                             lds_nodes=hip.gbdt_dart_lds_nodes())
    assert [c[1] for c in got] == [cap, 1]
    with pytest.raises(ValueError):
        hip.gbdt_dart_plan(tree_sizes=[3], sel=[1], lds_nodes=16)


def _stump_tree(G, feat, cond, bin_):
    t = G.RegTree()
    r = t.add(-1)
    t.feat[r], t.cond[r], t.bin[r], t.defl[r] = feat, cond, bin_, 1
    t.left[r], t.right[r] = t.add(r), t.add(r)
    t.leaf[1], t.leaf[2] = 0.5, -1.25
    return t


def test_pack_and_admission():
    G, hip = _G(), _hip()
    vals, off = D.grid_cuts(3)

    def pack(t, known=True, cv=vals, co=off):
        return hip.gbdt_dart_pack(feat=t.feat, bin=t.bin if known else None, cond=t.cond,
                                  left=t.left, right=t.right, defl=t.defl, leaf=t.leaf,
                                  cut_vals=cv, cut_off=co)

    nodes = pack(_stump_tree(G, 2, 0.25, 7))
    assert nodes.dtype == torch.int32 and nodes.tolist()[0] == [2 | 7 << 16 | 1 << 24, 1 | 2 << 16]
    assert nodes[1:, 0].tolist() == [0xffff, 0xffff]
    assert nodes[1:, 1].contiguous().view(torch.float32).tolist() == [0.5, -1.25]
    leaf = G.RegTree()
    leaf.add(-1)
    leaf.leaf[0] = 3.0
    assert pack(leaf).view(torch.float32)[0, 1].item() == 3.0  # a single leaf
    # bins recovered from the cuts: an exact hit, and a cond that is no cut
    hit = pack(_stump_tree(G, 1, fc.GRID[4], 0), known=False)
    assert (hit[0, 0].item() >> 16) & 255 == 4
    assert pack(_stump_tree(G, 1, fc.GRID[4] + 0.01, 0), known=False) is None
    # the limits
    assert pack(_stump_tree(G, 2, 0.25, 254)) is not None
    assert pack(_stump_tree(G, 2, 0.25, 255)) is None
    assert pack(_stump_tree(G, 3, 0.25, 1)) is None  # a feature the cuts do not have
    wide = [0] * 65537
    assert pack(_stump_tree(G, 65534, 0.25, 1), cv=[], co=wide) is not None
    assert pack(_stump_tree(G, 65535, 0.25, 1), cv=[], co=wide) is None
    big = fc.random_tree(__import__("random").Random(1), 3, 15, 1.0)  # 65535 nodes
    big.bin = [1] * len(big.feat)
    assert len(big.feat) == 65535 and pack(big) is not None
    big.add(-1)  # (an unreachable 65536th node)
    assert pack(big) is None


def test_table_grows_and_keeps_its_trees():
    G = _G()
    rng = __import__("random").Random(3)
    table = G.DartForest(CPU, D.grid_cuts(4))
    trees = [fc.random_tree(rng, 4, 9, 0.97) for _ in range(40)]
    for t in trees:
        assert table.append(t, False)
    assert table.used == sum(len(t.feat) for t in trees) > 4096  # the capacity doubled
    assert not table.append(_stump_tree(G, 1, 0.26, 0), False) and table.size[-1] == 0
    for t, o, s in zip(trees, table.off, table.size):
        w1 = table.table[o:o + s, 1]
        leaves = [i for i in range(s) if t.feat[i] < 0]
        assert s == len(t.feat)
        assert w1[leaves].view(torch.float32).tolist() == [float(F32(t.leaf[i])) for i in leaves]


def test_plan_test_binary():
    exe = os.path.join(ROOT, "bin", "native", "gbdt_dart_plan_test")
    assert os.path.exists(exe), "native tools not built (python build_native.py)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_plan_test_binary_sanitized():
    b = subprocess.run([sys.executable, os.path.join(ROOT, "build_native.py"),
                        "--sanitize-dart-plan"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    exe = b.stdout.strip().splitlines()[-1]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ------------------------------------------------------------ 2. the draw
def test_draw():
    G = _G()
    p = D.param(G, rate_drop=0.5)
    w = [1.0] * 12
    sets = [G.dart_draw(7, r, w, p) for r in range(8)]
    assert sets == [G.dart_draw(7, r, w, p) for r in range(8)]  # a function of (seed, r)
    assert len({tuple(s) for s in sets}) > 1  # another round, another set
    assert sets != [G.dart_draw(8, r, w, p) for r in range(8)]
    assert all(s == sorted(set(s)) and all(0 <= j < 12 for j in s) for s in sets)
    assert G.dart_draw(7, 3, w, D.param(G, rate_drop=1.0)) == list(range(12))
    for r in range(20):
        one = G.dart_draw(7, r, w, D.param(G, rate_drop=0, one_drop=1))
        assert len(one) == 1 and 0 <= one[0] < 12
        assert G.dart_draw(7, r, w, D.param(G, rate_drop=1.0, skip_drop=1.0)) == []
        assert G.dart_draw(7, r, [], D.param(G, rate_drop=1.0, one_drop=1)) == []  # R = 0
        assert G.dart_draw(7, r, w, D.param(G, rate_drop=0.0)) == []
    assert len({G.dart_draw(7, r, w, D.param(G, rate_drop=0, one_drop=1))[0]
                for r in range(40)}) > 3
    # weighted: a round of weight 0 is never dropped by rate; the heavy one mostly
    ww = [1.0, 0.0, 1.0, 5.0]
    pw = D.param(G, rate_drop=0.5, sample_type="weighted")
    drawn = [G.dart_draw(7, r, ww, pw) for r in range(200)]
    assert not any(1 in s for s in drawn)
    assert sum(3 in s for s in drawn) > 150 > 130 > sum(0 in s for s in drawn)
    # ... nor by one_drop, which draws in proportion to w
    p1 = D.param(G, rate_drop=0, one_drop=1, sample_type="weighted")
    ones = [G.dart_draw(7, r, ww, p1)[0] for r in range(200)]
    assert 1 not in ones and ones.count(3) > ones.count(0) + ones.count(2)


def test_draw_uses_neither_generator():
    """rate_drop = 0 consumes nothing that gbtree consumes: the round's
    generators are where a gbtree round leaves them."""
    G, bsp = _G(), _bsp()
    p = D.param(G, rate_drop=0.9, one_drop=1, subsample=0.8, colsample_bytree=0.75)
    dm, b, tb = D.setup(G, bsp, p, 300, 1, CPU)
    gen, fgen = D.gens(p)
    tr = G.DartTrainer(b, tb, dm)
    margin = b.predict_margin(dm)
    for r in range(3):
        tr.round(r, margin, gen, fgen)
    q = M.param(G, max_depth=3, subsample=0.8, colsample_bytree=0.75)
    dm2, b2, tb2 = D.setup(G, bsp, q, 300, 1, CPU)
    gen2, fgen2 = D.gens(q)
    m2 = b2.predict_margin(dm2)
    for r in range(3):
        b2.trees += G.boost_round(b2.obj, tb2, dm2, m2, gen2, fgen2)
    assert torch.equal(gen.get_state(), gen2.get_state())
    assert torch.equal(fgen.get_state(), fgen2.get_state())
    assert [k for _, k in tr.history][1:] != [[], []]  # (rounds were dropped)


# ------------------------------------------------------ 3. closed forms
@pytest.mark.parametrize("norm", ["tree", "forest"])
def test_closed_forms(norm):
    """eta = 1, rate_drop = 1: every round drops all earlier ones, so it fits
    the residual at the base margin again: the same tree every round."""
    G, bsp = _G(), _bsp()
    p = D.param(G, eta=1.0, rate_drop=1.0, normalize_type=norm)
    seen = []
    b, tr, _, _ = D.train_dart(G, bsp, p, 600, 1, CPU, 4,
                               each=lambda b, tr: seen.append(list(b.tree_w)))
    want, hist = [], []
    for r in range(4):  # the fp32 recurrence
        k = r
        if k == 0:
            f, new = F32(1.0), F32(1.0)
        elif norm == "tree":
            f, new = F32(k / (k + 1.0)), F32(1.0 / (k + 1.0))
        else:
            f, new = F32(0.5), F32(0.5)
        want = [float(F32(w) * f) for w in want] + [float(new)]
        hist.append(list(want))
    assert seen == hist
    assert b.weights() == ([0.25] * 4 if norm == "tree" else [0.125, 0.125, 0.25, 0.5])
    assert [d for _, d in tr.history] == [[], [0], [0, 1], [0, 1, 2]]
    assert len(b.trees[0].feat) >= 7
    for t in b.trees[1:]:
        C.same_structure(b.trees[0], t)
        assert all(abs(x - z) < 1e-6 for x, z in zip(b.trees[0].leaf, t.leaf))


# ------------------------------------------- 4. equivalence with gbtree
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("how", [dict(rate_drop=0), dict(rate_drop=0.5, skip_drop=1, one_drop=1)])
def test_no_drop_is_gbtree(how, K, sparse, tmp_path):
    G, bsp = _G(), _bsp()
    kw = dict(subsample=0.7, colsample_bytree=0.75)
    p = D.param(G, K, **kw, **how)
    b, tr, _, _ = D.train_dart(G, bsp, p, 400, K, CPU, 3, sparse)
    q = D.param(G, K, **kw)
    q.booster = "gbtree"
    ref = D.train_gbtree(G, bsp, q, 400, K, CPU, 3, sparse)
    got, want = D.model_bytes(b, tmp_path / "d.model"), D.model_bytes(ref, tmp_path / "g.model")
    assert got == want and len(b.trees) == 3 * K and sum(len(t.feat) for t in b.trees) > 3 * K


def test_booster_dart_runs_in_the_app(tmp_path, monkeypatch, capsys):
    """(fails on a tree without the feature at the app's SystemExit)"""
    from wormhole_amd.apps.xgboost_app import main
    _work(tmp_path, monkeypatch)
    X, y = D.labels(200, 1)
    C.write_libsvm(tmp_path / "t.libsvm", X, y)
    base = ["data=t.libsvm", "objective=reg:linear", "max_depth=3", "num_round=3", "max_bin=64"]
    assert main(base + ["booster=dart", "model_out=d.model"]) == 0
    assert main(base + ["model_out=g.model"]) == 0
    assert open("d.model", "rb").read() == open("g.model", "rb").read()


# ------------------------------------------------------- 5. consistency
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("K", [1, 3])
def test_kept_margins_agree_with_predict(K, sparse):
    G, bsp = _G(), _bsp()
    p = D.param(G, K, rate_drop=0.5, one_drop=1)
    mags = []
    b, tr, margin, ev = D.train_dart(G, bsp, p, 500, K, CPU, 8, sparse, evals=120,
                                     each=lambda b, tr: mags.append(D.magnitude(b)))
    assert sum(len(d) for _, d in tr.history) >= 8 and b.weighted()
    S = 2.0 * max(mags)
    tol = D.rounding_bound(D.fp32_ops(tr.history, len(b.trees) // K), S)
    assert tol < 1e-3
    dm = tr.dm
    err = float((margin - b.predict_margin(dm)).abs().max())
    err_eval = float((ev[0][1] - b.predict_margin(ev[0][0])).abs().max())
    print("kept vs predicted margins: train %.3g eval %.3g bound %.3g" % (err, err_eval, tol))
    assert err <= tol and err_eval <= tol
    assert float((b.predict_margin(dm) - b.base_margin).abs().max()) > 100 * tol  # (a real model)


# ------------------------------------------------------ 6. files and state
def _state_roundtrip(G, b):
    from wormhole_amd.apps.xgboost_app import _booster_from_state, _booster_state
    s = _booster_state(b)
    q = G.GBDTParam()
    for k, v in b.param.__dict__.items():
        setattr(q, k, v)
    return _booster_from_state(G, s, q), s


def test_model_file_trailer(tmp_path):
    G, bsp = _G(), _bsp()
    p = D.param(G, rate_drop=0.5, one_drop=1)
    b, _, _, _ = D.train_dart(G, bsp, p, 300, 1, CPU, 4)
    raw = D.model_bytes(b, tmp_path / "d.model")
    w = b.weights()
    assert any(x != 1.0 for x in w)
    tail = 8 + 4 * len(w)
    assert raw[-tail:-tail + 4] == b"DART"
    assert struct.unpack("<I", raw[-tail + 4:-tail + 8])[0] == len(w)
    assert np.frombuffer(raw[-4 * len(w):], dtype="<f4").tolist() == w
    back = G.Booster.load(str(tmp_path / "d.model"), G.GBDTParam())
    assert back.weights() == w and len(back.trees) == 4
    assert D.model_bytes(back, tmp_path / "e.model") == raw
    dm = M.dmatrix(G, *D.labels(300, 1), CPU)
    assert torch.equal(back.predict_margin(dm), b.predict_margin(dm))
    # a gbtree model: header and trees, no trailer
    q = M.param(G, max_depth=3)
    g = D.train_gbtree(G, bsp, q, 300, 1, CPU, 2)
    graw = D.model_bytes(g, tmp_path / "g.model")
    hdr = 4 + 4 + struct.unpack("<I", graw[4:8])[0]
    assert len(graw) == hdr + sum(4 + 32 * len(t.feat) for t in g.trees) and b"DART" not in graw
    assert G.Booster.load(str(tmp_path / "g.model"), G.GBDTParam()).weights() == [1.0, 1.0]


def test_state_roundtrip():
    G, bsp = _G(), _bsp()
    p = D.param(G, 3, rate_drop=0.5, one_drop=1)
    b, _, _, _ = D.train_dart(G, bsp, p, 300, 3, CPU, 3)
    b2, s = _state_roundtrip(G, b)
    assert b2.weights() == b.weights() and b.weighted()
    s2 = _state_roundtrip(G, b2)[1]
    assert s.keys() == s2.keys() and torch.equal(s["tree_w"], s2["tree_w"])
    assert all(torch.equal(x[k], z[k]) for x, z in zip(s["trees"], s2["trees"]) for k in x)
    g = D.train_gbtree(G, bsp, M.param(G, max_depth=3), 300, 1, CPU, 2)
    assert "tree_w" not in _state_roundtrip(G, g)[1]  # (gbtree states are what they were)


@pytest.mark.parametrize("K", [1, 3])
def test_restart_goes_on_bit_for_bit(K, tmp_path):
    """6 rounds straight = 3 rounds, the state saved and restored, 3 rounds."""
    G, bsp = _G(), _bsp()
    p = D.param(G, K, rate_drop=0.5, one_drop=1, subsample=0.8)
    straight, _, m6, _ = D.train_dart(G, bsp, p, 400, K, CPU, 6)
    half, _, m3, _ = D.train_dart(G, bsp, p, 400, K, CPU, 3)
    b2, _ = _state_roundtrip(G, half)
    dm, _, tb = D.setup(G, bsp, p, 400, K, CPU)
    tr = G.DartTrainer(b2, tb, dm)
    margin = tr.start_margin()
    assert torch.equal(margin, m3)  # the kept margins, replayed
    gen, fgen = D.gens(p)
    for _ in range(3 * K):  # (the generators where three rounds leave them)
        torch.rand(dm.n, generator=gen)
    for r in range(3, 6):
        tr.round(r, margin, gen, fgen)
    assert torch.equal(margin, m6)
    assert D.model_bytes(b2, tmp_path / "a.model") == D.model_bytes(straight, tmp_path / "b.model")
    # a model these parameters did not train starts from predict_margin
    p2 = D.param(G, K, rate_drop=0.5, one_drop=1, seed=5)
    b3, _ = _state_roundtrip(G, half)
    b3.param = p2
    assert torch.equal(G.DartTrainer(b3, tb, dm).start_margin(), b3.predict_margin(dm))


def test_continuation_both_ways(tmp_path):
    G, bsp = _G(), _bsp()
    dm0 = M.dmatrix(G, *D.labels(300, 1), CPU)
    # gbtree -> dart
    g = D.train_gbtree(G, bsp, M.param(G, max_depth=3), 300, 1, CPU, 2)
    g.save(str(tmp_path / "g.model"))
    p = D.param(G, rate_drop=1.0)
    b = G.Booster.load(str(tmp_path / "g.model"), p)
    dm, _, tb = D.setup(G, bsp, p, 300, 1, CPU)
    tr = G.DartTrainer(b, tb, dm)
    margin = tr.start_margin()
    assert torch.equal(margin, b.predict_margin(dm))
    tr.round(2, margin, *D.gens(p))
    assert len(b.trees) == 3 and tr.history == [(2, [0, 1])] and b.weights()[0] < 1.0
    assert float((margin - b.predict_margin(dm0)).abs().max()) < 1e-5
    b.save(str(tmp_path / "d.model"))
    # dart -> gbtree: the loaded weights stay, the new tree weighs 1
    q = M.param(G, max_depth=3)
    c = G.Booster.load(str(tmp_path / "d.model"), q)
    dm, _, tb = D.setup(G, bsp, q, 300, 1, CPU)
    margin = c.predict_margin(dm)
    c.trees += G.boost_round(c.obj, tb, dm, margin, *D.gens(q))
    assert c.weights() == b.weights() + [1.0]
    assert torch.equal(margin, c.predict_margin(dm0))
    c.save(str(tmp_path / "c.model"))
    assert G.Booster.load(str(tmp_path / "c.model"), G.GBDTParam()).weights() == c.weights()


# --------------------------------------------- 7. consumers on a dart model
@pytest.fixture(scope="module")
def dart_model():
    G, bsp = _G(), _bsp()
    out = {}
    for K in (1, 3):
        p = D.param(G, K, rate_drop=0.5, one_drop=1)
        b, _, _, _ = D.train_dart(G, bsp, p, 300, K, CPU, 4)
        assert b.weighted()
        out[K] = (b, M.dmatrix(G, *[t[:60] for t in D.labels(300, K)], CPU))
    return out


@pytest.mark.parametrize("K", [1, 3])
def test_consumers(dart_model, K):
    G = _G()
    b, dm = dart_model[K]
    margin = b.predict_margin(dm).double()
    tol = 1e-5  # (float64 attributions against fp32 margins of magnitude ~1)
    phi = b.predict_contribs(dm)
    assert float((phi.sum(-1) - margin).abs().max()) < tol
    assert float((b.predict_contribs(dm, approx=True).sum(-1) - margin).abs().max()) < tol
    inter = b.predict_interactions(dm)
    assert float((inter.sum((-1, -2)) - margin).abs().max()) < tol
    # ntree_limit: the final weights of the first N rounds
    w, X = b.weights(), dm.X
    for N in (1, 3):
        want = torch.full_like(b.predict_margin(dm), b.base_margin)
        for t in range(N * K):
            leaf = torch.from_numpy(F32(w[t]) * np.asarray(b.trees[t].leaf, dtype=np.float32))
            row = want[t % K] if K > 1 else want
            row += leaf[b.trees[t].leaf_index(X)]
        assert torch.equal(b.predict_margin(dm, N * K), want)
    # pred_leaf does not see the weights
    ids = b.predict_leaf(dm)
    keep, b.tree_w = b.tree_w, []
    try:
        assert torch.equal(b.predict_leaf(dm), ids)
        plain = b.dump()
    finally:
        b.tree_w = keep
    # the dump's leaves are the effective ones
    got = [float(v) for v in re.findall(r"leaf=([-+0-9.e]+)", b.dump())]
    want = [float("%g" % v) for t in range(len(b.trees))
            for v in _dump_order(b.trees[t], b.eff_leaf(t))]
    assert got == want and got != [float(v) for v in re.findall(r"leaf=([-+0-9.e]+)", plain)]


def _dump_order(t, leaf):
    out = []

    def rec(i):
        if t.feat[i] < 0:
            out.append(leaf[i])
        else:
            rec(t.left[i]), rec(t.right[i])
    rec(0)
    return out


# -------------------------------------------------------------- 8. the app
def _work(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WH_DEVICE", "cpu")
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)


def test_app(tmp_path, monkeypatch, capsys):
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    _work(tmp_path, monkeypatch)
    X, y = D.labels(400, 1)
    C.write_libsvm(tmp_path / "train.libsvm", X, 0.2 * y)
    C.write_libsvm(tmp_path / "test.libsvm", X[:150], 0.2 * y[:150])
    args = ["data=train.libsvm", "eval[test]=test.libsvm", "objective=reg:linear", "base_score=0",
            "eta=0.1", "max_depth=3", "max_bin=64", "num_round=4", "booster=dart",
            "rate_drop=0.5", "one_drop=1", "model_out=d.model"]
    assert main(args) == 0
    out = capsys.readouterr().out
    assert "unknown parameter" not in out
    vals = [float(v) for v in re.findall(r"test-rmse:([0-9.]+)", out)]
    assert len(vals) == 4
    b = G.Booster.load("d.model", G.GBDTParam())
    assert len(b.trees) == 4 and b.weighted()
    # the worst-case rounding bound of the kept margins against predict_margin
    # (every weight at most its first value, 1): below half the tolerance
    k_max = [min(r, 3) for r in range(4)]
    ops = sum(3 * k + 6 for k in k_max) + 2 * 4
    bound = D.rounding_bound(ops, 2.0 * D.magnitude(b, [1.0] * 4))
    assert bound < 5e-6, bound
    assert main(["task=eval", "model_in=d.model", "test:data=test.libsvm"]) == 0
    ev = float(re.search(r"test-rmse:([0-9.]+)", capsys.readouterr().out).group(1))
    assert abs(ev - vals[-1]) <= 1e-5, (ev, vals)
    # pred, pred_margin and dump agree with the model
    assert main(["task=pred", "model_in=d.model", "test:data=test.libsvm", "name_pred=p.txt",
                 "pred_margin=1"]) == 0
    dm = M.dmatrix(G, X[:150], y[:150], CPU)
    want = b.predict_margin(dm).tolist()
    got = [float(v) for v in open("p.txt").read().split()]
    assert len(got) == 150 and all(abs(a - z) <= 1e-5 * max(1.0, abs(z)) for a, z in zip(got, want))
    assert main(["task=dump", "model_in=d.model", "name_dump=d.txt"]) == 0
    assert open("d.txt").read() == b.dump() and open("d.txt").read().count("booster[") == 4


def test_app_parameters(tmp_path, monkeypatch, capsys):
    from wormhole_amd.apps.xgboost_app import main
    _work(tmp_path, monkeypatch)
    X, y = D.labels(120, 1)
    C.write_libsvm(tmp_path / "t.libsvm", X, y)
    base = ["data=t.libsvm", "max_depth=2", "num_round=2", "max_bin=32", "eval_train=1"]
    for bad, name in (("rate_drop=1.5", "rate_drop"), ("rate_drop=-0.1", "rate_drop"),
                      ("skip_drop=2", "skip_drop"), ("skip_drop=x", "skip_drop"),
                      ("one_drop=2", "one_drop"), ("sample_type=heavy", "sample_type"),
                      ("normalize_type=leaf", "normalize_type")):
        with pytest.raises(SystemExit, match=name):
            main(base + ["booster=dart", bad, "model_out=x.model"])
    with pytest.raises(SystemExit, match=r"gbtree.*dart"):
        main(base + ["booster=gblinear", "model_out=x.model"])
    # under gbtree the dart parameters are accepted and change nothing
    capsys.readouterr()
    assert main(base + ["model_out=a.model"]) == 0
    plain = capsys.readouterr().out
    assert main(base + ["booster=gbtree", "rate_drop=0.9", "skip_drop=0.1", "one_drop=1",
                        "sample_type=weighted", "normalize_type=forest", "model_out=b.model"]) == 0
    out = capsys.readouterr().out
    assert "unknown parameter" not in out + plain
    assert re.findall(r"^\[\d+\].*$", out, re.M) == re.findall(r"^\[\d+\].*$", plain, re.M)
    assert open("a.model", "rb").read() == open("b.model", "rb").read()
