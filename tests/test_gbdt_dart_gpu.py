"""booster=dart on the GPU: k_dart_walk against the forest-kernel fallback and
a torch CPU reference (bit for bit), training with the binned walk against
training with the fallback, and the GPU against the CPU through the app."""
import random
import re

import pytest
import torch

import _gbdt_dart_cases as D
import _gbdt_forest_cases as fc
import _gbdt_monotone_cases as M
import _gbdt_objective_cases as C

pytestmark = pytest.mark.gpu

GPU = torch.device("cuda")
CPU = torch.device("cpu")
COEF = [0.0, 1.0, -0.75, 0.3, 1.0 / 3.0, -1.7]
LDS_NODES = 600  # a small budget: a few trees per chunk, a depth-9 tree over it
ROWS = [1, 63, 64, 65, 255, 256, 257, 1000]


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _hip():
    from wormhole_amd import _native
    return _native.hip()


def _bsp():
    import os
    from wormhole_amd.parallel.bsp import BSP
    os.environ.pop("RANK", None)
    return BSP(GPU)


def _count(monkeypatch, name):
    hip, calls = _hip(), []
    monkeypatch.setattr(hip, name, lambda *a, _f=getattr(hip, name), **k: (calls.append(1),
                                                                             _f(*a, **k))[1])
    return calls


def _model(F, seed=2, oversize=LDS_NODES):
    """(booster of random trees with a tree over the budget in the middle,
    its table under the grid cuts with bins recovered from them)."""
    G = _G()
    trees = fc.random_forest(seed, F, 2600, max_depth=7, oversize=oversize)
    trees[1] = fc.random_tree(random.Random(seed), F, 0, 0.0)  # a single leaf
    b = fc.booster(trees, 1)
    table = G.DartForest(GPU, D.grid_cuts(F), lds_nodes=LDS_NODES)
    for t in trees:
        assert table.append(t, False)
    return b, table


def _selections(table):
    T = len(table.size)
    stump = [t for t in range(T) if table.size[t] == 1][0]
    big = [t for t in range(T) if table.size[t] > LDS_NODES]
    assert len(big) == 1 and 0 < big[0] < T - 1
    small = [t for t in range(T) if t != big[0]]
    sels = {"empty": [], "stump": [stump], "all": list(range(T)), "every other": list(range(0, T, 2)),
            "chunks": small, "over budget": [big[0] - 1, big[0], big[0] + 1]}
    plan = table.plan(small)
    # three chunks or more, the last one short of the budget by more than a stump
    assert len(plan) >= 3 and all(c[3] for c in plan) and plan[-1][2] < LDS_NODES - 1
    assert [c[3] for c in table.plan(sels["over budget"])] == [True, False, True]
    return sels


def _check(b, table, X, sel, calls=None):
    """walk == fallback == torch reference on the rows X, sentinels kept."""
    G = _G()
    n = X.shape[0]
    coef = [COEF[j % len(COEF)] for j in range(len(sel))]
    dm = G.DMatrix.from_dense(X, torch.zeros(n), GPU)
    B = D.grid_bins(X).to(GPU)
    g = torch.Generator().manual_seed(n)
    start = torch.randn(n, generator=g) + 3.0
    want = D.torch_reference(b.trees, X, sel, coef, start)
    got = []
    for table_ in (table, None):
        buf = torch.full((n + 16,), 777.0, device=GPU)
        out = buf[8:8 + n]
        out.copy_(start)
        G.dart_add(b, dm, B, table_, sel, coef, out)
        assert bool((buf[:8] == 777.0).all()) and bool((buf[8 + n:] == 777.0).all())
        got.append(out.cpu())
    assert torch.equal(got[0], want), (n, X.shape[1], float((got[0] - want).abs().max()))
    assert torch.equal(got[1], want)
    if len(sel) > 2:
        assert not torch.equal(want, start)


@pytest.mark.parametrize("nan_share", [0.0, 0.3])
@pytest.mark.parametrize("F", [1, 28, 96])
def test_walk_is_the_fallback_is_the_reference(F, nan_share, monkeypatch):
    b, table = _model(F)
    calls = _count(monkeypatch, "gbdt_dart_walk")
    sels = _selections(table)
    for n in ROWS:
        X = fc.rows(n, F, nan_share)
        for name, sel in sels.items():
            if n in (1, 257, 1000) or name in ("all", "over budget"):
                _check(b, table, X, sel)
    assert len(calls) > len(ROWS)  # (the kernel ran)


def test_walk_rows_per_tile(monkeypatch):
    """Every tile height the binding takes walks the same numbers."""
    b, table = _model(28)
    X = fc.rows(1000, 28, 0.3)
    for rows in (64, 256, 1024):
        table.rows = rows
        _check(b, table, X, list(range(len(table.size))))
    with pytest.raises(RuntimeError, match="rows per tile"):
        table.rows = 100
        _check(b, table, X, [0])


def test_walk_past_the_persistent_grid():
    """More tiles than the grid holds at once, and a partial one: every block
    goes round its tile loop more than once."""
    hip = _hip()
    b, table = _model(5, oversize=0)
    sel = [t for t in range(len(table.size))][:6]
    (first, count, nnode, staged, _), = table.plan(sel)[:1]
    assert staged and count >= 2
    grid = hip.gbdt_dart_grid(n=1 << 40, f=5, ntree=count, nnode=nnode, rows=table.rows)
    n = grid * table.rows + table.rows // 2 + 3
    assert hip.gbdt_dart_grid(n=n, f=5, ntree=count, nnode=nnode, rows=table.rows) == grid
    _check(b, table, fc.rows(n, 5, 0.3), sel[:count])


def test_wide_rows_go_to_the_fallback(monkeypatch):
    assert _hip().gbdt_dart_max_f() == 96
    b, table = _model(97)
    calls = _count(monkeypatch, "gbdt_dart_walk")
    _check(b, table, fc.rows(257, 97, 0.3), list(range(len(table.size))))
    assert not calls


# ------------------------------------------------------------- 2. training
def _train(monkeypatch, K, binned, defer):
    G = _G()
    monkeypatch.setattr(G, "DART_BIN_WALK", binned)
    monkeypatch.setattr(G, "DEFER_TREES", defer)
    p = D.param(G, K, rate_drop=0.5, one_drop=1)
    return D.train_dart(G, _bsp(), p, 3000, K, GPU, 4, evals=200)


@pytest.mark.parametrize("K", [1, 3])
def test_training_binned_walk_is_the_fallback(K, monkeypatch, tmp_path):
    calls = _count(monkeypatch, "gbdt_dart_walk")
    runs = {}
    for binned in (True, False):
        for defer in (True, False):
            before = len(calls)
            b, tr, margin, ev = _train(monkeypatch, K, binned, defer)
            assert (len(calls) > before) == binned
            assert sum(len(d) for _, d in tr.history) >= 3 and b.weighted()
            runs[binned, defer] = (D.model_bytes(b, tmp_path / "m.model"), margin.cpu(),
                                   ev[0][1].cpu())
    for defer in (True, False):  # with DEFER_TREES on and off: the same
        got, ref = runs[True, defer], runs[False, defer]
        assert got[0] == ref[0], defer
        assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]), defer
    b = _G().Booster.load(str(tmp_path / "m.model"), _G().GBDTParam())
    assert len(b.trees) == 4 * K and sum(len(t.feat) for t in b.trees) > 7 * 4 * K


def test_restart_on_the_gpu_replays_the_margins(monkeypatch):
    """A state restore: the table is rebuilt with bins recovered from the
    cuts, the kept margins are replayed bit for bit."""
    G = _G()
    from wormhole_amd.apps.xgboost_app import _booster_from_state, _booster_state
    p = D.param(G, rate_drop=0.5, one_drop=1)
    b, tr, margin, _ = D.train_dart(G, _bsp(), p, 3000, 1, GPU, 4)
    b2 = _booster_from_state(G, _booster_state(b), D.param(G, rate_drop=0.5, one_drop=1))
    calls = _count(monkeypatch, "gbdt_dart_walk")
    tr2 = G.DartTrainer(b2, tr.builder, tr.dm)
    assert torch.equal(tr2.start_margin(), margin) and calls
    assert tr2.table.size == tr.table.size and torch.equal(tr2.table.table[:tr2.table.used],
                                                           tr.table.table[:tr.table.used])


# ------------------------------------------------- 3. GPU against the CPU
@pytest.mark.parametrize("rows", ["dsparse=0", "dsparse=1"])
def test_app_dart_gpu_matches_cpu(tmp_path, capsys, monkeypatch, rows):
    """The data and tolerances of test_app_poisson_gpu_matches_cpu (there:
    why the two runs' leaves differ by the GPU histograms' fixed point);
    logistic pairs are below 1 in size, a tenth of the counts'."""
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    monkeypatch.chdir(tmp_path)
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    X, t = M.data(2000, 4)
    C.write_libsvm(tmp_path / "train.libsvm", X, (t > t.median()).float())
    args = ["data=train.libsvm", "objective=binary:logistic", "booster=dart", "rate_drop=0.5",
            "max_depth=4", "max_bin=64", "min_child_weight=25", "num_round=3", "eval_train=1",
            "eval_metric=logloss", rows]
    val, model, pred = {}, {}, {}
    for name, device in (("gpu", "auto"), ("cpu", "cpu")):
        monkeypatch.setenv("WH_DEVICE", device)
        assert main(args + ["model_out=%s.model" % name]) == 0
        out = capsys.readouterr().out
        assert "unknown parameter" not in out
        val[name] = [float(v) for v in re.findall(r"train-logloss:([0-9.]+)", out)]
        assert len(val[name]) == 3
        model[name] = G.Booster.load("%s.model" % name, G.GBDTParam())
        assert main(["task=pred", "model_in=%s.model" % name, "test:data=train.libsvm",
                     "name_pred=%s.txt" % name, rows]) == 0
        pred[name] = [float(v) for v in open("%s.txt" % name).read().split()]
    for a, b in zip(model["gpu"].trees, model["cpu"].trees):
        C.same_structure(a, b)
    assert model["gpu"].weights() == model["cpu"].weights() and model["gpu"].weighted()
    assert len(model["gpu"].trees) == 3 and all(len(t.feat) >= 7 for t in model["gpu"].trees)
    for a, b in zip(val["gpu"], val["cpu"]):
        assert abs(a - b) <= 1e-3 * abs(b), (val["gpu"], val["cpu"])
    assert len(pred["gpu"]) == len(pred["cpu"]) == 2000
    assert all(abs(a - b) <= 1e-4 * abs(b) for a, b in zip(pred["gpu"], pred["cpu"]))
