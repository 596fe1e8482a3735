"""grow_policy=lossguide on the CPU path: the builder's leaf loop against an
independent best-first reference, the limit and its control, equivalence with
depth-wise growth, constraints, composition with the other features, rank
count independence, the app, and the bookkeeping test program."""
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

import _gbdt_dart_cases as D
import _gbdt_interaction_cases as C
import _gbdt_lossguide_cases as L
import _gbdt_monotone_cases as M
import _gbdt_quantile_cases as Q

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 3


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


def _dm(n, f, sparse=False):
    X, y = M.data(n, f)
    return M.dmatrix(_G(), X, y, CPU, sparse)


# ------------------------------------------------------------ 1. parameters
def test_parameters():
    G, hip = _G(), _hip()
    p = G.GBDTParam()
    assert p.grow_policy == "depthwise" and p.max_leaves == 0 and p.leaf_limits() is None
    for bad in ("leafwise", "", "LossGuide"):
        with pytest.raises(SystemExit, match="grow_policy"):
            p.set("grow_policy", bad)
    for bad in ("-1", "2.5", "x", "32769", ""):
        with pytest.raises(SystemExit, match="max_leaves"):
            p.set("max_leaves", bad)
    assert p.set("max_leaves", "32768") and p.max_leaves == 32768
    # depth-wise: a limit on the leaves is refused, naming both
    with pytest.raises(SystemExit, match=r"max_leaves.*grow_policy"):
        p.leaf_limits()
    assert p.set("grow_policy", "lossguide")
    # the depth cap comes from the consumers' constants, not from a literal
    cap = hip.gbdt_leaf_depth_cap()
    assert cap == min(hip.gbdt_shap_max_path() - 1, hip.gbdt_dart_max_depth()) == 62
    p.max_depth = 0
    assert p.leaf_limits() == (32768, cap)
    p.max_leaves = 255
    assert p.leaf_limits() == (255, cap)
    p.max_depth = 8
    assert p.leaf_limits() == (255, 8)
    p.max_leaves = 0
    assert p.leaf_limits() == (256, 8)
    p.max_depth = 20
    assert p.leaf_limits() == (32768, 20)
    p.max_depth = 0
    with pytest.raises(SystemExit, match=r"max_leaves.*max_depth"):
        p.leaf_limits()


def test_pick_rule():
    hip = _hip()

    def pick(rows, cap=62):
        return hip.gbdt_leaf_pick(node=[r[0] for r in rows], depth=[r[1] for r in rows],
                                  gain=[r[2] for r in rows], rt_eps=L.RT_EPS, depth_cap=cap)

    assert pick([]) == -1
    assert pick([(3, 2, 1.0), (4, 2, 5.0), (2, 1, 2.0)]) == 1
    assert pick([(7, 3, 2.5), (4, 2, 2.5)]) == 1  # ties: the smaller node id
    assert pick([(3, 5, 9.0), (4, 4, 1.0)], cap=5) == 1  # at the depth cap: passed over
    assert pick([(0, 0, L.RT_EPS), (1, 1, -math.inf)]) == -1


def test_plan_test_binary():
    exe = os.path.join(ROOT, "bin", "native", "gbdt_leaf_plan_test")
    assert os.path.exists(exe), "native tools not built (python build_native.py)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_plan_test_binary_sanitized():
    b = subprocess.run([sys.executable, os.path.join(ROOT, "build_native.py"),
                        "--sanitize-leaf-plan"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    exe = b.stdout.strip().splitlines()[-1]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# --------------------------------- 2. the builder against the reference
CASES = [(4000, 4, 8, 0), (4000, 4, 24, 0), (20000, 12, 20, 5)]


@pytest.mark.parametrize("n,f,max_leaves,max_depth", CASES)
def test_builder_equals_the_reference(n, f, max_leaves, max_depth):
    G, bsp = _G(), _bsp()
    dm = _dm(n, f)
    p = L.param(G, max_leaves, max_depth)
    got = M.train(G, bsp, dm, p, ROUNDS)[0].trees
    want, _ = L.reference(G, bsp, dm, p, max_leaves, max_depth, ROUNDS)
    assert len(got) == len(want) == ROUNDS
    for a, b in zip(got, want):
        L.same_structure(a, b)
        assert all(abs(x - z) < 1e-9 for x, z in zip(a.leaf, b.leaf))
        assert L.n_leaves(a) == max_leaves
        if max_depth:
            assert L.tree_depth(a) <= max_depth


def test_the_limit_binds():
    """8 leaves on 4000 x 4: every tree has exactly 8 leaves, leaves that
    could still be split remain, and the trees are deeper than a balanced
    tree of 8 leaves (best-first growth, not a truncated level loop). The
    control: depth-wise growth to the same depth has more leaves."""
    G, bsp = _G(), _bsp()
    dm = _dm(4000, 4)
    p = L.param(G, 8, 0)
    trees = M.train(G, bsp, dm, p, ROUNDS)[0].trees
    assert [L.n_leaves(t) for t in trees] == [8] * ROUNDS
    assert all(len(g) > 0 for g in L.open_gains(G, bsp, dm, p, trees))
    depths = [L.tree_depth(t) for t in trees]
    assert min(depths) > math.ceil(math.log2(8)), depths
    control = M.train(G, bsp, dm, M.param(G, max_depth=max(depths)), ROUNDS)[0].trees
    assert all(L.n_leaves(t) > 8 for t in control)


# --------------------------------------------------------- 3. equivalence
@pytest.mark.parametrize("gamma,colsample", [(0.0, 1.0), (2.0, 1.0), (0.0, 0.6), (2.0, 0.6)])
def test_equals_depthwise_when_the_leaves_do_not_bind(gamma, colsample):
    """max_depth = 5 with 2^5 leaves: lossguide splits exactly the nodes the
    level loop splits, in another order; the compacted trees are the same."""
    G, bsp = _G(), _bsp()
    dm = _dm(4000, 4)
    kw = dict(gamma=gamma, colsample_bytree=colsample)
    deep = M.train(G, bsp, dm, M.param(G, max_depth=5, **kw), ROUNDS)[0]
    leaf = M.train(G, bsp, dm, L.param(G, 32, 5, **kw), ROUNDS)[0]
    assert deep.dump(None, True) == leaf.dump(None, True)
    assert deep.dump().count("yes=") > 3 * 7
    # max_leaves = 0 with a depth limit: 2^depth leaves, the same trees again
    auto = M.train(G, bsp, dm, L.param(G, 0, 5, **kw), ROUNDS)[0]
    assert auto.dump(None, True) == deep.dump(None, True)


# --------------------------------------------------------- 4. constraints
GROUPS = ((0, 2, 4, 6, 8), (1, 3, 5, 7, 9), (4, 5, 10))  # feature 11 in none
MONO = M.cycled(12)


def test_constraints_hold():
    G, bsp = _G(), _bsp()
    dm = _dm(20000, 12)

    def grow(groups, mono, **kw):
        p = C.param(G, groups, mono, max_depth=0, max_bin=64, **kw)
        assert p.set("grow_policy", "lossguide") and p.set("max_leaves", "32")
        return M.train(G, bsp, dm, p, ROUNDS)[0].trees

    trees = grow(GROUPS, MONO, max_delta_step=0.4)
    assert [L.n_leaves(t) for t in trees] == [32] * ROUNDS
    bad, total = C.broken(trees, GROUPS)
    assert bad == 0 and total > 3 * 4, (bad, total)
    assert M.holds(trees, MONO)
    s = M.structure(trees, MONO)
    assert sum(k for k, _ in s.values()) > 6, s  # constrained features were split on
    # max_delta_step: every node's weight, hence every leaf / eta, within the step
    assert all(abs(v) <= 0.5 * 0.4 + 1e-12 for t in trees for v in t.leaf)
    # the control: left alone, the same growth breaks both rules
    free = grow(None, None)
    assert C.broken(free, GROUPS)[0] > 0 and not M.holds(free, MONO)


# --------------------------------------------------------- 5. composition
def _compose_param(G, what):
    kw = dict(grow_policy="lossguide", max_leaves=12, max_depth=0, max_bin=64, eta=0.5)
    if what == "quantile":
        return Q.param(G, "reg:quantileerror", quantile_alpha="[0.125,0.5,0.75]", **kw)
    if what == "softprob":
        return Q.param(G, "multi:softprob", num_class=3, **kw)
    if what == "dart":
        return Q.param(G, "reg:linear", booster="dart", rate_drop=0.5, seed=2, **kw)
    return Q.param(G, "reg:linear", subsample=0.7, colsample_bytree=0.6, **kw)


@pytest.mark.parametrize("what", ["quantile", "softprob", "dart", "sampling"])
def test_composition_and_csr(what):
    """Each feature under lossguide trains, its trees stop at max_leaves, and
    the CSR builder (dsparse=1) grows the dense builder's trees."""
    G, bsp = _G(), _bsp()
    K = 3 if what in ("quantile", "softprob") else 1
    X, y = D.labels(2000, 3) if what == "softprob" else M.data(2000, 4)
    models = []
    for sparse in (False, True):
        dm = Q.dmatrix(G, X, y, None, CPU, sparse)
        b, margin = Q.train(G, bsp, dm, _compose_param(G, what), ROUNDS)
        assert len(b.trees) == ROUNDS * K
        assert [L.n_leaves(t) for t in b.trees] == [12] * (ROUNDS * K)
        assert torch.allclose(margin, b.predict_margin(dm), atol=1e-5)
        models.append(b)
    for a, c in zip(models[0].trees, models[1].trees):
        L.same_structure(a, c)
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, c.leaf))
    assert models[0].weights() == models[1].weights()
    if what == "quantile":
        # refreshed leaves: not eta x the Newton weight of an unit-hessian node
        t = models[0].trees[0]
        assert any(abs(t.leaf[i] - 0.5 * t.base_weight[i]) > 1e-3 for i in Q.leaves_of(t))


# ----------------------------------------------- 6. rank-count independence
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _train_rank(bsp):
    G = _G()
    X, y = M.data(4000, 4)
    rows = torch.arange(4000)[bsp.rank::bsp.world]
    dm = G.DMatrix.from_dense(X[rows], y[rows], CPU)
    b = M.train(G, bsp, dm, L.param(G, 12, 0), ROUNDS)[0]
    return [t.dump(None, True) for t in b.trees]


def _main(rank, world, port, out, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), WH_GBDT_XCHG=mode)
    torch.set_num_threads(1)
    from wormhole_amd.parallel.bsp import BSP
    bsp = BSP(CPU)
    dumps = _train_rank(bsp)
    if rank == 0:
        json.dump(dumps, open(out, "w"))
    bsp.finalize()


@pytest.mark.parametrize("mode", ["rs", "allreduce"])
def test_two_ranks_grow_the_single_rank_model(mode, tmp_path):
    one = _train_rank(_bsp())
    assert all(d.count("leaf=") == 12 for d in one)
    out = str(tmp_path / "two.json")
    mp.spawn(_main, args=(2, _free_port(), out, mode), nprocs=2, join=True)
    assert json.load(open(out)) == one


# ------------------------------------------------------------- 7. the app
@pytest.fixture()
def work(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WH_DEVICE", "cpu")
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    X, y = M.data(4000, 4)
    M.write_libsvm(tmp_path / "train.libsvm", X, y)
    return tmp_path


BASE = ["data=train.libsvm", "objective=reg:linear", "eta=0.5", "max_bin=64", "num_round=3",
        "eval_train=1"]


def test_app(work, capsys):
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    assert main(BASE + ["grow_policy=lossguide", "max_leaves=8", "max_depth=0",
                        "model_out=l.model"]) == 0
    out = capsys.readouterr().out
    assert "unknown parameter" not in out
    assert len(re.findall(r"^\[\d+\]\ttrain-rmse:", out, re.M)) == 3
    b = G.Booster.load("l.model", G.GBDTParam())
    assert [L.n_leaves(t) for t in b.trees] == [8, 8, 8]
    # the app's model is the reference's
    X, y = M.data(4000, 4)
    dm = M.dmatrix(G, X, y, CPU)
    want, _ = L.reference(G, _bsp(), dm, L.param(G, 8, 0), 8, 0, 3)
    for a, c in zip(b.trees, want):
        assert a.feat == c.feat and a.left == c.left and a.right == c.right
    # dump, pred and eval of the model need nothing about its growth
    assert main(["task=dump", "model_in=l.model", "name_dump=d.txt"]) == 0
    assert open("d.txt").read() == b.dump()
    assert main(["task=pred", "model_in=l.model", "test:data=train.libsvm",
                 "name_pred=p.txt"]) == 0
    got = [float(v) for v in open("p.txt").read().split()]
    want_m = b.predict_margin(dm).tolist()
    assert len(got) == 4000
    assert all(abs(a - z) <= 1e-5 * max(1.0, abs(z)) for a, z in zip(got, want_m))
    capsys.readouterr()
    assert main(["task=eval", "model_in=l.model", "test:data=train.libsvm"]) == 0
    ev = float(re.search(r"test-rmse:([0-9.]+)", capsys.readouterr().out).group(1))
    last = float(re.findall(r"train-rmse:([0-9.]+)", out)[-1])
    assert abs(ev - last) <= 1e-5


def test_app_refusals(work, capsys):
    from wormhole_amd.apps.xgboost_app import main
    for bad, name in ((["grow_policy=leafwise"], "grow_policy"),
                      (["grow_policy=lossguide", "max_leaves=-3"], "max_leaves"),
                      (["grow_policy=lossguide", "max_leaves=7.5"], "max_leaves"),
                      (["grow_policy=lossguide", "max_leaves=40000"], "max_leaves"),
                      (["max_leaves=8"], r"max_leaves.*grow_policy"),
                      (["grow_policy=depthwise", "max_leaves=8"], r"max_leaves.*grow_policy"),
                      (["grow_policy=lossguide", "max_depth=0"], r"max_leaves.*max_depth"),
                      (["grow_policy=lossguide", "max_leaves=0", "max_depth=0"],
                       r"max_leaves.*max_depth")):
        with pytest.raises(SystemExit, match=name):
            main(BASE + bad + ["model_out=x.model"])
        assert not os.path.exists("x.model")
    # depthwise with max_leaves=0 is the model of neither parameter
    capsys.readouterr()
    assert main(BASE + ["max_depth=3", "model_out=a.model"]) == 0
    plain = capsys.readouterr().out
    assert main(BASE + ["max_depth=3", "grow_policy=depthwise", "max_leaves=0",
                        "model_out=b.model"]) == 0
    out = capsys.readouterr().out
    assert "unknown parameter" not in out + plain
    assert re.findall(r"^\[\d+\].*$", out, re.M) == re.findall(r"^\[\d+\].*$", plain, re.M)
    assert open("a.model", "rb").read() == open("b.model", "rb").read()
