"""grow_policy=lossguide on the GPU: the device leaf loop against the Python
leaf loop on the same kernels, against the device level loop where both grow
the same tree, the app against its CPU run, the leaf refresh and dart."""
import functools
import math
import os
import re

import pytest
import torch

import _gbdt_interaction_cases as C
import _gbdt_lossguide_cases as L
import _gbdt_monotone_cases as M
import _gbdt_quantile_cases as Q

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
TREES = 3
GROUPS = ((0, 2, 4, 6, 8), (1, 3, 5, 7, 9), (4, 5, 10))  # feature 11 in none
MONO = M.cycled(12)


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _bsp(device=CPU):
    from wormhole_amd.parallel.bsp import BSP
    os.environ.pop("RANK", None)
    return BSP(device)


@functools.lru_cache(maxsize=None)
def _inputs(n, f, constant=False):
    G = _G()
    X, y = M.data(n, f)
    if constant:
        y = torch.full_like(y, 0.25)
    dm = G.DMatrix.from_dense(X, y, DEV)
    cuts = G.Cuts.build(dm, 64, _bsp())
    return dm, cuts, cuts.bin(dm)


def _grow(monkeypatch, dev_loop, n, f, max_leaves, max_depth, constant=False, groups=None,
          mono=None, policy="lossguide", **kw):
    """(trees, margins, device-loop calls) of TREES trees."""
    G = _G()
    from wormhole_amd import _native
    hip = _native.hip()
    calls = []
    monkeypatch.setattr(hip, "gbdt_grow_leaf",
                        lambda *a, _f=hip.gbdt_grow_leaf, **k: (calls.append(1), _f(*a, **k))[1])
    monkeypatch.setattr(G, "LEAF_LOOP_DEV", dev_loop)
    dm, cuts, B = _inputs(n, f, constant)
    p = C.param(G, groups, mono, max_depth=max_depth, max_bin=64, **kw)
    if policy is not None:
        assert p.set("grow_policy", policy) and p.set("max_leaves", str(max_leaves))
    obj = G.Objective(p.objective)
    tb = G.TreeBuilder(p, _bsp(), dm, cuts, B)
    margin = torch.full((dm.n,), 0.5, device=DEV)
    gen = torch.Generator().manual_seed(5)
    trees = []
    for _ in range(TREES):
        tb.sample_features(gen)
        trees.append(tb.build(obj.gpair(margin, dm.label, None), margin))
    for t in trees:
        t.feat  # (a deferred device tree builds its lists)
    return trees, margin.cpu(), len(calls)


def _agree(monkeypatch, *case, **kw):
    dev, mdev, calls = _grow(monkeypatch, True, *case, **kw)
    assert calls == TREES  # the device loop ran
    py, mpy, calls = _grow(monkeypatch, False, *case, **kw)
    assert calls == 0
    for a, b in zip(dev, py):
        L.same_structure(a, b)
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))
        assert all(abs(x - z) < 1e-6 * max(1.0, abs(z)) for x, z in zip(a.gain, b.gain))
        assert all(abs(x - z) < 1e-6 * max(1.0, abs(z)) for x, z in zip(a.cover, b.cover))
    assert torch.allclose(mdev, mpy, atol=1e-6)
    return dev


# ------------------------- 1. the device loop against the Python leaf loop
@pytest.mark.parametrize("n,f,max_leaves,max_depth,gamma", [
    (20000, 12, 32, 0, 0.0), (20000, 12, 20, 5, 0.0), (20000, 12, 32, 0, 2.0),
    (4097, 4, 8, 0, 0.0), (3000, 70, 64, 0, 0.0)])
def test_device_loop_equals_the_python_loop(n, f, max_leaves, max_depth, gamma, monkeypatch):
    """The histograms of both loops are the same fixed-point sums, so the
    picks cannot differ. 4097 rows: one past a partition tile; 70 features:
    two feature groups and leaves of a handful of rows; gamma = 2: the lists
    and segments go through the prune instead of the device walk."""
    trees = _agree(monkeypatch, n, f, max_leaves, max_depth, gamma=gamma)
    if gamma == 0:
        assert [L.n_leaves(t) for t in trees] == [max_leaves] * TREES
    else:
        assert all(1 < L.n_leaves(t) <= max_leaves for t in trees)
    if max_depth:
        assert all(L.tree_depth(t) <= max_depth for t in trees)
    else:
        assert max(L.tree_depth(t) for t in trees) > math.ceil(math.log2(max_leaves))


def test_device_loop_runs_out_of_leaves(monkeypatch):
    """min_child_weight = 1500 of 20000 unit hessians: at most 13 leaves fit,
    so the later steps of a 32-leaf budget are idle."""
    trees = _agree(monkeypatch, 20000, 12, 32, 0, min_child_weight=1500.0)
    assert all(1 < L.n_leaves(t) <= 13 for t in trees)


def test_device_loop_single_leaf(monkeypatch):
    """A constant label: no split has a gain, every step is idle and the
    tree is its root."""
    trees = _agree(monkeypatch, 4097, 4, 8, 0, constant=True)
    assert [len(t.feat) for t in trees] == [1] * TREES
    one = _agree(monkeypatch, 4097, 4, 1, 0)  # max_leaves = 1: no step at all
    assert [len(t.feat) for t in one] == [1] * TREES


@pytest.mark.parametrize("cons", ["groups", "mono", "both"])
def test_device_loop_under_constraints(cons, monkeypatch):
    """Groups alone, signs alone (with max_delta_step, which needs them) and
    both: every constrained instantiation of k_leaf_root and k_leaf_pick. A
    constraint that is off does not hold by accident (the Python leaf loop on
    the CPU: 95 of 96 splits break the groups under the signs alone, and the
    signs fail under the groups alone)."""
    groups = GROUPS if cons != "mono" else None
    kw = dict(mono=MONO, max_delta_step=0.4) if cons != "groups" else {}
    trees = _agree(monkeypatch, 20000, 12, 32, 0, groups=groups, **kw)
    assert [L.n_leaves(t) for t in trees] == [32] * TREES
    bad, total = C.broken(trees, GROUPS)
    if groups:
        assert bad == 0 and total > 3 * 4, (bad, total)
    else:
        assert bad > 0
    if cons == "groups":
        assert not M.holds(trees, MONO)
        return
    assert M.holds(trees, MONO)
    assert sum(k for k, _ in M.structure(trees, MONO).values()) > 6
    assert all(abs(v) <= 0.5 * 0.4 + 1e-12 for t in trees for v in t.leaf)
    if cons == "both":
        free, _, _ = _grow(monkeypatch, True, 20000, 12, 32, 0)
        assert C.broken(free, GROUPS)[0] > 0 and not M.holds(free, MONO)


# ------------------------------------------------ 2. equivalence on the device
@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_equals_the_device_level_loop(gamma, monkeypatch):
    """max_depth = 6 with 2^6 leaves: the leaf loop splits the nodes the level
    loop splits; the dumps are equal, digit for digit."""
    leaf, ml, calls = _grow(monkeypatch, True, 20000, 12, 64, 6, gamma=gamma)
    assert calls == TREES
    level, mv, calls = _grow(monkeypatch, True, 20000, 12, 0, 6, policy=None, gamma=gamma)
    assert calls == 0
    assert [t.dump(None, True) for t in leaf] == [t.dump(None, True) for t in level]
    assert sum(len(t.feat) for t in leaf) > 3 * 31
    assert torch.equal(ml, mv)


# ------------------------------------------------------------- 3. the app
@pytest.fixture()
def work(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    X, y = M.data(4000, 4)
    M.write_libsvm(tmp_path / "train.libsvm", X, y)
    return tmp_path


def test_app_gpu_matches_cpu(work, capsys, monkeypatch):
    """n = 4000, F = 4, max_leaves = 8, three rounds. The GPU histograms are
    rounded to 2^-17 of max|g| and the CPU's are fp64, so the order of the
    picks is defined only where no pick is a near tie: the smallest gap
    between a picked gain and the runner-up among the eligible open leaves,
    relative to max(1, |gain|), must exceed 1e-3 on the CPU run -- a condition
    on the inputs (measured: 4.9e-3), not a tolerance on the result."""
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    args = ["data=train.libsvm", "objective=reg:linear", "eta=0.5", "max_bin=64", "num_round=3",
            "eval_train=1", "grow_policy=lossguide", "max_leaves=8", "max_depth=0"]

    def run(device, model):
        monkeypatch.setenv("WH_DEVICE", device)
        assert main(args + ["model_out=" + model]) == 0
        out = capsys.readouterr().out
        assert "unknown parameter" not in out
        return ([l for l in out.splitlines() if re.match(r"^\[\d+\]\t", l)],
                G.Booster.load(model, G.GBDTParam()))

    cl, cb = run("cpu", "c.model")
    X, y = M.data(4000, 4)
    ref, gap = L.reference(G, _bsp(), M.dmatrix(G, X, y, CPU), L.param(G, 8, 0), 8, 0, 3)
    for a, b in zip(cb.trees, ref):  # the gap is that of the CPU run's own picks
        assert a.feat == b.feat and a.left == b.left and a.right == b.right
    print("smallest pick gap: %.3g" % gap)
    assert gap > 1e-3, gap
    gl, gb = run("auto", "g.model")
    assert gl == cl and len(cl) == 3
    assert len(gb.trees) == len(cb.trees) == 3
    for a, b in zip(cb.trees, gb.trees):
        assert a.feat == b.feat and a.cond == b.cond and a.defl == b.defl
        assert a.left == b.left and a.right == b.right
        assert L.n_leaves(a) == 8


# ---------------------------------------------------- 4. refresh and dart
def _qparam(G, **kw):
    return Q.param(G, "reg:quantileerror", quantile_alpha="[0.125,0.5,0.75]", eta=0.5,
                   grow_policy="lossguide", max_leaves=12, max_depth=0, **kw)


def test_quantile_refresh_matches_the_cpu_path():
    """Dyadic alphas, integer weights, as test_gbdt_quantile_gpu's training
    test: the same structure and leaves as the CPU path."""
    G = _G()
    X, y, w = Q.train_data()
    want = Q.train(G, _bsp(), Q.dmatrix(G, X, y, w, CPU), _qparam(G), TREES)[0]
    dm = Q.dmatrix(G, X, y, w, DEV)
    got, margin = Q.train(G, _bsp(), dm, _qparam(G), TREES)
    assert len(got.trees) == len(want.trees) == TREES * 3
    assert all(L.n_leaves(t) == 12 for t in got.trees)
    for a, b in zip(got.trees, want.trees):
        L.same_structure(a, b)
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))
    assert torch.allclose(margin.cpu(), got.predict_margin(dm).cpu(), atol=1e-6)


def test_app_dart(work, capsys, monkeypatch):
    from wormhole_amd.apps.xgboost_app import main
    monkeypatch.setenv("WH_DEVICE", "auto")
    args = ["data=train.libsvm", "objective=reg:linear", "base_score=0", "eta=0.3", "max_bin=64",
            "num_round=4", "eval_train=1", "booster=dart", "rate_drop=0.5", "one_drop=1",
            "grow_policy=lossguide", "max_leaves=8", "max_depth=0", "model_out=d.model"]
    assert main(args) == 0
    out = capsys.readouterr().out
    assert "unknown parameter" not in out
    vals = [float(v) for v in re.findall(r"train-rmse:([0-9.]+)", out)]
    assert len(vals) == 4
    b = _G().Booster.load("d.model", _G().GBDTParam())
    assert b.weighted() and [L.n_leaves(t) for t in b.trees] == [8] * 4
    assert main(["task=eval", "model_in=d.model", "test:data=train.libsvm"]) == 0
    ev = float(re.search(r"test-rmse:([0-9.]+)", capsys.readouterr().out).group(1))
    assert abs(ev - vals[-1]) <= 1e-5, (ev, vals)
