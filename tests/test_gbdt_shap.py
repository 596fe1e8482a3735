"""GBDT feature contributions without a GPU: the host reference (C++ behind
``_hip``, which loads on a CPU-only machine; the float64 instantiation is the
CPU path of ``Booster.predict_contribs``) against an independent Python
enumeration of the Shapley sum, the merged paths, the Saabas attribution, the
launch plan of the kernels, the stand-alone host test, and the two parameters
of bin/xgboost.dmlc."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import _gbdt_forest_cases as fc
import _gbdt_shap_cases as sc
from test_gbdt_forest import CONF, PRED, ROOT, XGB, run

CPU = torch.device("cpu")
F = 6


def hip():
    from wormhole_amd import _native
    return _native.hip()


def matrices(X, ncol):
    from wormhole_amd.models import gbdt as G
    n = X.shape[0]
    return (G.DMatrix.from_dense(X, torch.zeros(n), CPU),
            G.make_dmatrix(*fc.csr_of(X), torch.zeros(n), None, ncol, CPU, sparse=True))


def forest():
    """Ten trees over 6 features (at most 8 used per tree: the enumeration's
    bound), single leaves among them; len % 3 == 1."""
    trees = sc.random_forest(11, F, 300, max_depth=5)
    assert any(len(t.feat) == 1 for t in trees) and len(trees) % 3 == 1
    return trees


def rows(n=13):
    X = fc.rows(n, F, 0.3)
    assert bool(torch.isnan(X[n // 2]).all())
    return X


# ------------------------------------------------------- the definition
@pytest.mark.parametrize("K", [1, 3])
def test_exact_contributions_equal_the_shapley_sum(K):
    trees, X = forest(), rows()
    # values exactly on a threshold occur
    assert any(float(X[r, t.feat[0]]) == t.cond[0] for t in trees if t.feat[0] >= 0
               for r in range(X.shape[0]))
    b = fc.booster(trees, K)
    want = sc.brute(trees, X, F, K, b.base_margin)
    for dm in matrices(X, F):
        got = b.predict_contribs(dm)
        assert got.dtype == torch.float64
        assert got.shape == ((13, F + 1) if K == 1 else (3, 13, F + 1))
        got = got[None] if K == 1 else got
        assert float(np.abs(got.numpy() - want).max()) <= 1e-12
        # the bias: base margin + sum over the class's trees of sum leaf x ratios
        for k in range(K):
            bias = b.base_margin + sum(sc.expected_value(t) for t in trees[k::K])
            assert float((got[k, :, F] - bias).abs().max()) <= 1e-12
        margin = b.predict_margin(dm)
        margin = margin[None] if K == 1 else margin
        assert float((got.sum(-1) - margin).abs().max()) <= 1e-6


def test_ntree_limit_and_tree_ownership():
    trees, X = forest(), rows()
    b = fc.booster(trees, 3)
    dm = matrices(X, F)[0]
    for limit in (1, 2, 3, 7, len(trees), len(trees) + 5):
        T = min(limit, len(trees))
        got = b.predict_contribs(dm, limit)
        for k in range(3):  # class k owns trees k, k + 3, ...: alone they give its slice
            own = fc.booster(trees[k:T:3], 1).predict_contribs(dm)
            assert float((got[k] - own).abs().max()) <= 1e-12
        assert float((got.sum(-1) - b.predict_margin(dm, limit)).abs().max()) <= 1e-6
    assert torch.equal(b.predict_contribs(dm, 0), b.predict_contribs(dm, len(trees)))
    with pytest.raises(ValueError):
        b.predict_contribs(dm, -1)


def test_chain_paths_are_merged():
    """Depth 12 over 3 features: paths of at most 3 elements, and still the
    Shapley sum."""
    tree = sc.chain_tree(3, 12, [0, 1, 2])
    packed = hip().gbdt_shap_pack(num_class=1, **sc.lists([tree]))
    used, paths, elems, ecol = packed[0], packed[2], packed[3], packed[4]
    assert used.tolist() == [0, 1, 2] and paths.shape == (13, 4)
    assert 1 <= int(paths[:, 1].min()) and int(paths[:, 1].max()) == 3
    assert int(paths[:, 1].sum()) == elems.shape[0] == ecol.numel()
    for begin, ln, _, tree_id in paths.tolist():
        assert tree_id == 0 and len(set(ecol[begin:begin + ln].tolist())) == ln
    X = fc.rows(21, 3, 0.3)
    want = sc.brute([tree], X, 3, 1, 0.0)
    for dm in matrices(X, 3):
        got = fc.booster([tree], 1).predict_contribs(dm)
        assert float(np.abs(got.numpy() - want[0] - [0, 0, 0, fc.booster([], 1).base_margin]
                            ).max()) <= 1e-12


@pytest.mark.parametrize("K", [1, 3])
def test_saabas(K):
    trees, X = forest(), rows()
    b = fc.booster(trees, K)
    want = sc.saabas(trees, X, F, K, b.base_margin)
    for dm in matrices(X, F):
        got = b.predict_contribs(dm, approx=True)
        got = got[None] if K == 1 else got
        assert float(np.abs(got.numpy() - want).max()) <= 1e-12
        margin = b.predict_margin(dm)
        assert float((got.sum(-1) - (margin[None] if K == 1 else margin)).abs().max()) <= 1e-6
    # limited to two trees
    got = b.predict_contribs(dm, 2, approx=True)
    want = sc.saabas(trees[:2], X, F, K, b.base_margin)
    assert float(np.abs((got[None] if K == 1 else got).numpy() - want).max()) <= 1e-12


def test_fp32_reference_is_close():
    """The error yardstick of the GPU tests is the same algorithm in fp32."""
    trees, X = forest(), rows(40)
    kw = dict(num_class=1, base=0.5, X=X, **sc.lists(trees))
    for approx in (False, True):
        p64, used = hip().gbdt_shap_rows(approx=approx, **kw)
        p32, _ = hip().gbdt_shap_rows(approx=approx, f32=True, **kw)
        assert p64.dtype == p32.dtype == torch.float64 and used.dtype == torch.int32
        assert 0 < float((p64 - p32).abs().max()) < 1e-5


# ------------------------------------------------------------ edge cases
def test_edge_cases():
    trees, X = forest(), rows()
    for dm in matrices(X, F):
        for approx in (False, True):
            got = fc.booster([], 1).predict_contribs(dm, approx=approx)  # no trees
            base = fc.booster([], 1).base_margin
            assert got.shape == (13, F + 1) and bool((got[:, :F] == 0).all())
            assert bool((got[:, F] == base).all())
            leaves = [t for t in trees if len(t.feat) == 1]  # bias only
            got, used = fc.booster(leaves, 1).predict_contribs(dm, approx=approx, compact=True)
            assert used.numel() == 0 and got.shape == (13, 1)
            assert float((got[:, 0] - base - sum(t.leaf[0] for t in leaves)).abs().max()) < 1e-12
    for dm in matrices(X[:0], F):  # no rows
        assert fc.booster(trees, 1).predict_contribs(dm).shape == (0, F + 1)
        assert fc.booster(trees, 3).predict_contribs(dm, approx=True).shape == (3, 0, F + 1)


def test_compact_columns():
    """compact=True: only the features the trees split on, ascending."""
    rng = random.Random(5)
    remap = [2, 5, 11]
    trees = [sc.add_covers(rng, fc.random_tree(rng, 3, 4, 0.9)) for _ in range(4)]
    for t in trees:
        t.feat = [remap[f] if f >= 0 else f for f in t.feat]
    X = fc.rows(17, 14, 0.3)
    for K in (1, 3):
        b = fc.booster(trees, K)
        for dm in matrices(X, 14):
            full = b.predict_contribs(dm)
            phi, used = b.predict_contribs(dm, compact=True)
            assert used.tolist() == remap and phi.shape[-1] == 4 and full.shape[-1] == 15
            assert torch.equal(full[..., remap], phi[..., :3])
            assert torch.equal(full[..., 14], phi[..., 3])
            rest = [j for j in range(14) if j not in remap]
            assert bool((full[..., rest] == 0).all())
            part = b.predict_contribs(dm, rows=(3, 9))
            assert torch.equal(part, full[..., 3:9, :])
    with pytest.raises(ValueError):
        b.predict_contribs(dm, rows=(3, 99))


# -------------------------------------------------------------- refusals
def test_trees_without_covers_are_refused():
    trees = forest()
    bad = fc.random_forest(seed=3, F=F, total_nodes=60, max_depth=4)[0]  # cover 0 everywhere
    while len(bad.feat) == 1:
        bad = fc.random_tree(random.Random(8), F, 4, 1.0)
    dm = matrices(rows(), F)[0]
    for approx in (False, True):
        with pytest.raises(ValueError, match="tree 2 has no usable cover statistics"):
            fc.booster(trees[:2] + [bad] + trees[2:], 1).predict_contribs(dm, approx=approx)
    with pytest.raises(ValueError, match="tree 0 has no usable cover statistics"):
        hip().gbdt_shap_pack(num_class=1, **sc.lists([bad]))
    for value in (float("nan"), float("inf"), -1.0):
        t = sc.chain_tree(1, 3, [0, 1, 2])
        t.cover[t.left[0]] = value
        with pytest.raises(ValueError, match="no usable cover"):
            fc.booster([t], 1).predict_contribs(dm)


def test_a_path_of_70_features():
    """The CPU takes it; the pack that prepares it for the GPU is refused."""
    tree = sc.chain_tree(7, 70, list(range(70)))
    X = fc.rows(9, 70, 0.3)
    b = fc.booster([sc.chain_tree(8, 3, [0, 1, 2]), tree], 1)
    for dm in matrices(X, 70):
        got = b.predict_contribs(dm)
        assert float((got.sum(-1) - b.predict_margin(dm)).abs().max()) <= 1e-6
        assert int((got[:, :70] != 0).any(0).sum()) > 60
    with pytest.raises(ValueError, match=r"tree 1 has a path of \d+ distinct"):
        hip().gbdt_shap_pack(num_class=1, **sc.lists(b.trees))
    from wormhole_amd.models.gbdt_tree import ShapForest
    with pytest.raises(ValueError, match=r"tree 1 has a path of \d+ distinct"):
        ShapForest(b.trees, 1, 0.0, CPU)


# ------------------------------------------------------------------ plan
def check_plan(lens, classes, cap):
    order, chunks = hip().gbdt_shap_plan(path_len=lens, path_class=classes,
                                         path_tree=list(range(len(lens))), lds_elems=cap)
    assert sorted(order) == list(range(len(lens)))  # every path once
    width = [16 if l < 16 else 32 if l < 32 else 64 for l in lens]
    path = elem = 0
    for begin, npath, ebegin, nelem, cls, w in chunks:
        assert (begin, ebegin) == (path, elem) and npath >= 1
        ids = order[begin:begin + npath]
        assert {classes[p] for p in ids} == {cls} and {width[p] for p in ids} == {w}
        assert nelem == sum(lens[p] for p in ids) <= cap  # whole paths, within the capacity
        path, elem = path + npath, elem + nelem
    assert path == len(lens) and elem == sum(lens)
    # as many whole paths as fit: a chunk of the same class and width as its
    # predecessor starts with the path that did not fit there
    for a, c in zip(chunks, chunks[1:]):
        if a[4:] == c[4:]:
            assert a[3] + lens[order[c[0]]] > cap
    return order, chunks


def test_plan_invariants_around_the_capacity():
    C = hip().gbdt_shap_lds_elems()
    assert C >= 256 * 8 and hip().gbdt_shap_lds_cols() >= 29  # a full depth-8 tree; 28 features
    assert C * 36 + 64 * hip().gbdt_shap_lds_cols() * 4 + 260 <= 160 * 1024  # the CU's LDS
    rng = random.Random(4)
    for total in (C - 1, C, C + 1, 2 * C, int(2.5 * C)):
        for K in (1, 3):
            lens, classes = [], []
            while sum(lens) < total:
                lens.append(min(rng.choice([1, 5, 8, 15, 16, 31, 32, 63]), total - sum(lens)))
                classes.append(len(lens) % K)
            check_plan(lens, classes, C)
    order, chunks = check_plan([8] * (C // 8), [0] * (C // 8), C)  # exactly full
    assert len(chunks) == 1
    order, chunks = check_plan([8] * (C // 8) + [1], [0] * (C // 8 + 1), C)  # one element over
    assert [c[1] for c in chunks] == [C // 8, 1]
    order, chunks = check_plan([63, 15, 63, 16, 1], [1, 0, 0, 0, 0], 63)
    assert order == [1, 4, 3, 2, 0] and [c[5] for c in chunks] == [16, 32, 64, 64]
    assert check_plan([], [], C) == ([], [])
    with pytest.raises(ValueError, match="tree 1 has a path of 64"):
        hip().gbdt_shap_plan(path_len=[3, 64], path_class=[0, 0], path_tree=[0, 1], lds_elems=C)
    with pytest.raises(ValueError):
        hip().gbdt_shap_plan(path_len=[3], path_class=[0], path_tree=[0], lds_elems=62)


def test_pack_follows_the_plan():
    trees = forest()
    K = 3
    packed = hip().gbdt_shap_pack(num_class=K, lds_elems=64, **sc.lists(trees))
    used, tree_E, paths, elems, ecol, chunks, nodes, tree_off, node_m, node_col = packed
    assert used.tolist() == sorted({f for t in trees for f in t.feat if f >= 0})
    assert tree_E.dtype == torch.float64 and tree_E.numel() == len(trees)
    assert [float(e) for e in tree_E] == pytest.approx([sc.expected_value(t) for t in trees],
                                                       abs=1e-12)
    assert len(chunks) > 3 and max(c[3] for c in chunks) <= 64
    assert [c[4] for c in chunks] == sorted(c[4] for c in chunks)  # class by class
    for begin, npath, ebegin, nelem, cls, w in chunks:
        assert {t % K for t in paths[begin:begin + npath, 3].tolist()} == {cls}
        assert int(paths[begin, 0]) == ebegin and int(paths[begin:begin + npath, 1].sum()) == nelem
    assert int(ecol.max()) < used.numel() and int(ecol.min()) >= 0
    assert nodes.shape == (sum(len(t.feat) for t in trees), 4) and node_m.dtype == torch.float32
    inner = nodes[:, 0] >= 0
    assert bool((node_col[inner] >= 0).all()) and bool((node_col[~inner] == -1).all())
    assert torch.equal(used[node_col[inner].long()], nodes[inner, 0] >> 1)


# ------------------------------------------------- the stand-alone binary
def test_host_plan_test_binary(tmp_path):
    exe = os.path.join(ROOT, "bin", "native", "gbdt_shap_plan_test")
    assert os.path.exists(exe), "native tools not built (python build_native.py)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_host_plan_test_binary_sanitized():
    b = subprocess.run([sys.executable, os.path.join(ROOT, "build_native.py"),
                        "--sanitize-shap-plan"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    exe = b.stdout.strip().splitlines()[-1]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ------------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """An agaricus model of 4 rounds, its margins and its contributions."""
    d = tmp_path_factory.mktemp("shap_cli")
    os.symlink(os.path.join(ROOT, "learn"), d / "learn")
    r = run(["-n", "1", XGB] + CONF + ["num_round=4", "model_out=m4.model"], d)
    assert r.returncode == 0, r.stderr[-2000:]
    for args in (["pred_margin=1", "name_pred=margin.txt"],
                 ["pred_contribs=1", "name_pred=contribs.txt"], ["name_pred=default.txt"]):
        r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model"] + args, d)
        assert r.returncode == 0 and "unknown parameter" not in r.stdout, r.stderr[-2000:]
    return d


def parse(path):
    out = []
    for line in open(path).read().split("\n")[:-1]:
        out.append([(int(t.split(":")[0]), float(t.split(":")[1])) for t in line.split()])
    return out


def test_cli_pred_contribs(work):
    from wormhole_amd.models import gbdt as G
    b = G.Booster.load(str(work / "m4.model"), G.GBDTParam())
    margin = [float(x) for x in open(work / "margin.txt")]
    lines = parse(work / "contribs.txt")
    assert len(lines) == len(margin) == 1611
    used = {f for t in b.trees for f in t.feat if f >= 0}
    for toks, m in zip(lines, margin):
        idx = [j for j, _ in toks]
        assert idx == sorted(set(idx)) and idx[-1] == b.num_feature and set(idx[:-1]) <= used
        assert all(v != 0 for _, v in toks[:-1])
        assert abs(sum(v for _, v in toks) - m) <= 1e-5
    assert len({tuple(t) for t in map(tuple, lines)}) > 2
    assert len({toks[-1][1] for toks in lines}) == 1  # one bias
    # the default output is untouched by the new parameters' code
    r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "pred_contribs=0",
                                       "name_pred=again.txt"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(work / "again.txt").read() == open(work / "default.txt").read()


def test_cli_approx_contribs_and_ntree_limit(work):
    r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "approx_contribs=1", "ntree_limit=2",
                                       "name_pred=approx.txt"], work)
    assert r.returncode == 0 and "unknown parameter" not in r.stdout, r.stderr[-2000:]
    r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "pred_margin=1", "ntree_limit=2",
                                       "name_pred=margin2.txt"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    margin = [float(x) for x in open(work / "margin2.txt")]
    lines = parse(work / "approx.txt")
    assert len(lines) == 1611
    for toks, m in zip(lines, margin):
        # %g prints six significant digits: every printed value, the margin
        # included, is off by at most half a unit of its sixth digit
        slack = sum(0.5 * 10.0 ** (math.floor(math.log10(abs(v))) - 5)
                    for v in [v for _, v in toks] + [m] if v)
        assert abs(sum(v for _, v in toks) - m) <= 1e-6 + slack
    assert open(work / "approx.txt").read() != open(work / "contribs.txt").read()


def test_cli_two_ranks_write_the_one_rank_file(work):
    r = run(["-n", "2", XGB] + PRED + ["model_in=m4.model", "pred_contribs=1",
                                       "name_pred=contribs2.txt"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(work / "contribs2.txt").read() == open(work / "contribs.txt").read()


def test_cli_multiclass(tmp_path):
    from test_gbdt_multiclass import three_class_rows, write_libsvm
    X, y = three_class_rows(60)
    write_libsvm(tmp_path / "train.libsvm", X, y)
    r = run(["-n", "1", XGB, "objective=multi:softprob", "num_class=3", "max_depth=3", "eta=0.5",
             "data=train.libsvm", "num_round=2", "model_out=m.model"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    pred = ["-n", "1", XGB, "task=pred", "test:data=train.libsvm", "model_in=m.model"]
    for args in (["pred_contribs=1", "name_pred=c.txt"], ["pred_margin=1", "name_pred=m.txt"]):
        r = run(pred + args, tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
    margin = [float(x) for x in open(tmp_path / "m.txt")]
    lines = parse(tmp_path / "c.txt")
    assert len(lines) == len(margin) == 60 * 3  # one line per row and class, row-major
    for toks, m in zip(lines, margin):
        assert abs(sum(v for _, v in toks) - m) <= 1e-5 and toks[-1][0] == X.shape[1]


@pytest.mark.parametrize("args", [["pred_contribs=1", "pred_margin=1"],
                                  ["pred_contribs=1", "pred_leaf=1"],
                                  ["approx_contribs=1", "pred_margin=1"],
                                  ["approx_contribs=1", "pred_leaf=1"]])
def test_cli_excluded_combinations(work, args):
    r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model"] + args, work)
    assert r.returncode != 0 and "exclude each other" in r.stderr
