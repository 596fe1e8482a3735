"""GBDT forest prediction without a GPU: the chunk plan and the checked pack
(host C++ behind ``_hip``, which loads on a CPU-only machine), ``predict_leaf``
and ``predict_margin(ntree_limit=...)`` on the CPU against a plain Python
per-row walk, and the three prediction parameters of bin/xgboost.dmlc."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import _gbdt_forest_cases as fc
from test_gbdt_multiclass import three_class_rows, write_libsvm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKER = os.path.join(ROOT, "tracker", "dmlc_local.py")
XGB = os.path.join(ROOT, "bin", "xgboost.dmlc")


def hip():
    from wormhole_amd import _native
    return _native.hip()


# ------------------------------------------------------------------ plan
C = 100
PLAN_CASES = {
    "no trees": [],
    "one tree": [7],
    "fills exactly": [40, 60, 100, 30, 30, 40],
    "one node over": [40, 61, 100, 1, 99, 1],
    "oversize first": [101, 40, 60, 5],
    "oversize in the middle": [40, 50, 250, 50, 50, 5],
    "oversize last": [40, 60, 5, 101],
    "all oversize": [101, 500, 102],
    "single leaves": [1] * 250,
}


@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan(name):
    sizes = PLAN_CASES[name]
    chunks = hip().gbdt_forest_plan(tree_sizes=sizes, lds_nodes=C)
    tree = node = 0
    for k, (first, ntree, begin, nnode, in_lds) in enumerate(chunks):
        assert (first, begin) == (tree, node) and ntree >= 1  # in order, no gap
        assert nnode == sum(sizes[first:first + ntree])
        assert in_lds == (nnode <= C)
        if not in_lds:
            assert ntree == 1
        # as many whole trees as fit: the next tree would not have fitted
        if in_lds and first + ntree < len(sizes):
            assert nnode + sizes[first + ntree] > C
        tree, node = tree + ntree, node + nnode
    assert tree == len(sizes) and node == sum(sizes)
    assert sum(c[3] for c in chunks) == sum(sizes)
    if name == "fills exactly":
        assert [c[1] for c in chunks] == [2, 1, 3]
    if name == "one node over":
        assert [c[1] for c in chunks] == [1, 1, 1, 2, 1]
    if name == "single leaves":
        assert [c[1] for c in chunks] == [100, 100, 50]


def test_lds_capacity_fits_a_cu():
    c = hip().gbdt_forest_lds_nodes()
    assert 511 <= c and c * 16 <= 160 * 1024  # a full depth-8 tree; the CU's LDS


# ------------------------------------------------------------------ pack
def _lists(trees):
    return dict(feat=[t.feat for t in trees], cond=[t.cond for t in trees],
                left=[t.left for t in trees], right=[t.right for t in trees],
                defl=[t.defl for t in trees], leaf=[t.leaf for t in trees])


def _stump():
    from wormhole_amd.models.gbdt import RegTree
    t = RegTree()
    r = t.add(-1)
    t.feat[r], t.cond[r], t.defl[r] = 2, 0.5, 1
    t.left[r], t.right[r] = t.add(r), t.add(r)
    t.leaf[1], t.leaf[2] = -1.5, 2.25
    return t


def test_pack_layout():
    nodes, off, max_feat = hip().gbdt_forest_pack(**_lists([_stump(), _stump()]))
    assert off.tolist() == [0, 3, 6] and max_feat == 2 and nodes.shape == (6, 4)
    assert nodes[0].tolist()[0] == (2 << 1 | 1) and nodes[0].tolist()[2:] == [1, 2]
    assert nodes[3].tolist()[2:] == [1, 2]  # children numbered within the tree
    assert nodes[:, 1].view(torch.float32)[[0, 1, 2]].tolist() == [0.5, -1.5, 2.25]
    assert nodes[1].tolist()[0] < 0  # a leaf
    nodes, off, max_feat = hip().gbdt_forest_pack(**_lists([]))
    assert off.tolist() == [0] and nodes.shape == (0, 4) and max_feat == -1


@pytest.mark.parametrize("what,node,left,right", [
    ("a child equal to its parent (a cycle)", 0, 0, 2), ("the right child a cycle", 0, 1, 0),
    ("a child >= nn", 0, 1, 3), ("a child < its parent", 1, 2, 0), ("a negative child", 0, -1, 2)])
def test_pack_rejects_malformed_trees(what, node, left, right):
    bad = _stump()
    bad.feat[node], bad.left[node], bad.right[node] = 0, left, right
    with pytest.raises(ValueError, match="malformed tree 1"):
        hip().gbdt_forest_pack(**_lists([_stump(), bad]))
    from wormhole_amd.models.gbdt_tree import Forest
    with pytest.raises(ValueError, match="malformed tree 1"):
        Forest([_stump(), bad], torch.device("cpu"))


# ------------------------------------------------------- CPU predictions
def _cpu_forest():
    trees = fc.random_forest(seed=11, F=6, total_nodes=400, max_depth=5)
    assert any(len(t.feat) == 1 for t in trees) and len(trees) % 3 == 1
    return trees


@pytest.mark.parametrize("K", [1, 3])
def test_cpu_predictions_match_a_python_walk(K):
    from wormhole_amd.models import gbdt as G
    trees = _cpu_forest()
    X = fc.rows(41, 6, 0.3)
    assert bool(torch.isnan(X[20]).all())
    # values exactly on a threshold occur, and go right
    assert any(float(X[r, t.feat[0]]) == t.cond[0] for t in trees if t.feat[0] >= 0
               for r in range(41))
    b = fc.booster(trees, K)
    for dm in (G.DMatrix.from_dense(X, torch.zeros(41), torch.device("cpu")),
               G.make_dmatrix(*fc.csr_of(X), torch.zeros(41), None, 6, torch.device("cpu"),
                              sparse=True)):
        for limit in (0, 1, 2, 7, len(trees), len(trees) + 5):
            T = min(limit, len(trees)) if limit else len(trees)
            ids, margin = fc.python_reference(trees[:T], X, K, b.base_margin)
            got = b.predict_leaf(dm, limit)
            assert got.dtype == torch.int32 and got.shape == (41, T)
            assert torch.equal(got, ids)
            assert torch.equal(b.predict_margin(dm, limit), margin)
            assert torch.equal(fc.margins_from_ids(trees[:T], ids, K, b.base_margin), margin)
    with pytest.raises(ValueError):
        b.predict_margin(dm, -1)


def test_equal_goes_right_and_nan_takes_the_default():
    from wormhole_amd.models import gbdt as G
    t = _stump()  # f2 < 0.5, missing -> left
    X = torch.tensor([[0, 0, 0.25], [0, 0, 0.5], [0, 0, float("nan")]])
    dm = G.DMatrix.from_dense(X, torch.zeros(3), torch.device("cpu"))
    assert fc.booster([t], 1).predict_leaf(dm).tolist() == [[1], [2], [1]]
    t.defl[0] = 0
    assert fc.booster([t], 1).predict_leaf(dm).tolist() == [[1], [2], [2]]


# ------------------------------------------------------------------- CLI
def run(args, cwd, env_extra=None, timeout=300):
    env = dict(os.environ, WH_DEVICE="cpu")
    env.update(env_extra or {})
    return subprocess.run([sys.executable, TRACKER] + args, cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=timeout)


CONF = ["learn/xgboost/mushroom.conf", "max_depth=3", "eval_train=0"]
PRED = CONF + ["task=pred", "test:data=learn/data/agaricus.txt.test"]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """Agaricus models of 4 rounds and of 1 round, and the default pred.txt."""
    d = tmp_path_factory.mktemp("forest_cli")
    os.symlink(os.path.join(ROOT, "learn"), d / "learn")
    for rounds in (4, 1):
        r = run(["-n", "1", XGB] + CONF + ["num_round=%d" % rounds,
                                           "model_out=m%d.model" % rounds], d)
        assert r.returncode == 0, r.stderr[-2000:]
    r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "name_pred=default.txt"], d)
    assert r.returncode == 0, r.stderr[-2000:]
    return d


def floats(path):
    return [float(x) for x in open(path)]


def test_cli_pred_margin(work):
    r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "pred_margin=1",
                                       "name_pred=margin.txt"], work)
    assert r.returncode == 0 and "unknown parameter" not in r.stdout, r.stderr[-2000:]
    margin, prob = floats(work / "margin.txt"), floats(work / "default.txt")
    assert len(margin) == len(prob) == 1611
    assert all(abs(1 / (1 + math.exp(-m)) - p) <= 1e-5 for m, p in zip(margin, prob))
    assert any(m < 0 or m > 1 for m in margin)


def test_cli_ntree_limit(work):
    r = run(["-n", "2", XGB] + PRED + ["model_in=m4.model", "ntree_limit=1",
                                       "name_pred=limit1.txt"], work)
    assert r.returncode == 0 and "unknown parameter" not in r.stdout, r.stderr[-2000:]
    r = run(["-n", "1", XGB] + PRED + ["model_in=m1.model", "name_pred=one.txt"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(work / "limit1.txt").read() == open(work / "one.txt").read()
    assert open(work / "limit1.txt").read() != open(work / "default.txt").read()
    # 0 and more rounds than the model has: every tree
    for limit in ("0", "9"):
        r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "ntree_limit=" + limit,
                                           "name_pred=all.txt"], work)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(work / "all.txt").read() == open(work / "default.txt").read()
    # task=eval takes the limit too
    ev = {}
    for name, args in (("limit", ["model_in=m4.model", "ntree_limit=1"]),
                       ("one", ["model_in=m1.model"]), ("all", ["model_in=m4.model"])):
        r = run(["-n", "1", XGB] + CONF + ["task=eval", "eval_metric=logloss",
                                           "test:data=learn/data/agaricus.txt.test"] + args, work)
        assert r.returncode == 0, r.stderr[-2000:]
        ev[name] = re.findall(r"test-logloss:[\d.]+", r.stdout)
    assert ev["limit"] == ev["one"] != ev["all"] and len(ev["one"]) == 1


def test_cli_pred_leaf(work):
    r = run(["-n", "2", XGB] + PRED + ["model_in=m4.model", "pred_leaf=1",
                                       "name_pred=leaf.txt"], work)
    assert r.returncode == 0 and "unknown parameter" not in r.stdout, r.stderr[-2000:]
    lines = open(work / "leaf.txt").read().split("\n")[:-1]
    assert len(lines) == 1611 * 4 and all(re.fullmatch(r"\d+", l) for l in lines)
    r = run(["-n", "1", XGB] + CONF + ["task=dump", "model_in=m4.model"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    boosters = open(work / "dump.txt").read().split("booster[")[1:]
    leaves = [set(int(i) for i in re.findall(r"(\d+):leaf=", b)) for b in boosters]
    assert len(leaves) == 4
    for k, l in enumerate(lines):
        assert int(l) in leaves[k % 4], (k, l)
    assert len(set(lines)) > 2


def test_cli_multiclass(tmp_path):
    X, y = three_class_rows(120)
    write_libsvm(tmp_path / "train.libsvm", X, y)
    train = ["objective=multi:softprob", "num_class=3", "max_depth=3", "eta=0.5",
             "data=train.libsvm"]
    for rounds in (3, 1):
        r = run(["-n", "1", XGB] + train + ["num_round=%d" % rounds,
                                            "model_out=m%d.model" % rounds], tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
    pred = ["task=pred", "test:data=train.libsvm"]
    # one round is three trees
    r = run(["-n", "1", XGB] + pred + ["model_in=m3.model", "ntree_limit=1",
                                       "name_pred=limit1.txt"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run(["-n", "1", XGB] + pred + ["model_in=m1.model", "name_pred=one.txt"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "limit1.txt").read() == open(tmp_path / "one.txt").read()
    r = run(["-n", "1", XGB] + pred + ["model_in=m3.model", "ntree_limit=1", "pred_leaf=1",
                                       "name_pred=leaf.txt"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(open(tmp_path / "leaf.txt").read().split()) == 120 * 3
    # margins: n x 3 row-major, whose softmax is the default output
    r = run(["-n", "2", XGB] + pred + ["model_in=m3.model", "pred_margin=1",
                                       "name_pred=margin.txt"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run(["-n", "1", XGB] + pred + ["model_in=m3.model", "name_pred=prob.txt"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    margin = torch.tensor(floats(tmp_path / "margin.txt"), dtype=torch.float64)
    prob = torch.tensor(floats(tmp_path / "prob.txt"), dtype=torch.float64)
    assert margin.numel() == prob.numel() == 120 * 3
    assert float((torch.softmax(margin.view(120, 3), 1) - prob.view(120, 3)).abs().max()) < 1e-4


def test_cli_errors(work):
    r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "pred_leaf=1", "pred_margin=1"], work)
    assert r.returncode != 0 and "exclude each other" in r.stderr
    r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "ntree_limit=-1"], work)
    assert r.returncode != 0 and "ntree_limit" in r.stderr
