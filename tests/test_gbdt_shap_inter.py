"""GBDT SHAP interaction values without a GPU: the host reference (C++ behind
``_hip``; the float64 instantiation is the CPU path of
``Booster.predict_interactions``) against an independent Python enumeration
of the Shapley interaction index, the sum rules that tie the matrix to
``predict_contribs`` and ``predict_margin``, the stand-alone host test, and
pred_interactions of bin/xgboost.dmlc."""
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
import _gbdt_shap_inter_cases as ic
from test_gbdt_forest import CONF, PRED, ROOT, XGB, run
from test_gbdt_shap import F, forest, matrices, rows


def hip():
    from wormhole_amd import _native
    return _native.hip()


# ------------------------------------------------------- the definition
@pytest.mark.parametrize("K", [1, 3])
def test_interactions_equal_the_enumeration(K):
    trees, X = forest(), rows()
    assert any(float(X[r, t.feat[0]]) == t.cond[0] for t in trees if t.feat[0] >= 0
               for r in range(X.shape[0]))  # values exactly on a threshold occur
    b = fc.booster(trees, K)
    want = ic.brute(trees, X, F, K, b.base_margin)
    assert float(np.abs(want[:, :, :F, :F] - np.swapaxes(want[:, :, :F, :F], 2, 3)).max()) < 1e-13
    assert int((want[:, :, :F, :F] != 0).sum()) > 13 * F  # there are pairs
    for dm in matrices(X, F):
        got = b.predict_interactions(dm)
        assert got.dtype == torch.float64
        assert got.shape == ((13, F + 1, F + 1) if K == 1 else (3, 13, F + 1, F + 1))
        got = got[None] if K == 1 else got
        assert float(np.abs(got.numpy() - want).max()) <= 1e-12


@pytest.mark.parametrize("K", [1, 3])
def test_sum_rules_and_structure(K):
    trees, X = forest(), rows()
    b = fc.booster(trees, K)
    for dm in matrices(X, F):
        got = b.predict_interactions(dm)
        phi, margin = b.predict_contribs(dm), b.predict_margin(dm)
        assert float((got.sum(-1) - phi).abs().max()) <= 1e-12  # a row sums to the contribution
        assert float((got.sum((-1, -2)) - margin).abs().max()) <= 1e-6
        assert torch.equal(got, got.transpose(-1, -2))  # bit for bit
        assert torch.equal(got[..., F, F], phi[..., F])  # the bias
        assert bool((got[..., F, :F] == 0).all()) and bool((got[..., :F, F] == 0).all())


def test_disjoint_trees_do_not_interact():
    rng = random.Random(21)
    a = sc.add_covers(rng, fc.random_tree(rng, 3, 4, 0.9))
    c = sc.add_covers(rng, fc.random_tree(rng, 3, 4, 0.9))
    c.feat = [f + 3 if f >= 0 else f for f in c.feat]
    assert sc.used_features(a) == [0, 1, 2] and sc.used_features(c) == [3, 4, 5]
    X = rows()
    for dm in matrices(X, F):
        got = fc.booster([a, c, a], 1).predict_interactions(dm)
        assert bool((got[:, :3, 3:6] == 0).all()) and bool((got[:, 3:6, :3] == 0).all())
        assert bool((got[:, :3, :3] != 0).any()) and bool((got[:, 3:6, 3:6] != 0).any())


def test_special_trees():
    """One feature only: everything on the diagonal. Depth 12 over three
    features: the paths are merged, and still the enumeration."""
    X = fc.rows(21, 3, 0.3)
    base = fc.booster([], 1).base_margin
    one = sc.chain_tree(2, 6, [0])
    tree = sc.chain_tree(3, 12, [0, 1, 2])
    for dm in matrices(X, 3):
        got = fc.booster([one], 1).predict_interactions(dm)
        phi = fc.booster([one], 1).predict_contribs(dm)
        off = got.clone()
        off[:, 0, 0] = off[:, 3, 3] = 0
        assert bool((off == 0).all()) and torch.equal(got[:, 0, 0], phi[:, 0])
        assert bool((got[:, 0, 0] != 0).any())
        got = fc.booster([tree], 1).predict_interactions(dm)
        want = ic.brute([tree], X, 3, 1, base)
        assert float(np.abs(got.numpy() - want[0]).max()) <= 1e-12


def test_ntree_limit_and_tree_ownership():
    trees, X = forest(), rows()
    b = fc.booster(trees, 3)
    dm = matrices(X, F)[0]
    for limit in (1, 2, 3, 7, len(trees), len(trees) + 5):
        T = min(limit, len(trees))
        got = b.predict_interactions(dm, limit)
        for k in range(3):  # class k owns trees k, k + 3, ...: alone they give its slice
            own = fc.booster(trees[k:T:3], 1).predict_interactions(dm)
            assert float((got[k] - own).abs().max()) <= 1e-12
        assert float((got.sum((-1, -2)) - b.predict_margin(dm, limit)).abs().max()) <= 1e-6
    assert torch.equal(b.predict_interactions(dm, 0), b.predict_interactions(dm, len(trees)))
    with pytest.raises(ValueError):
        b.predict_interactions(dm, -1)


def test_compact_columns_and_rows():
    rng = random.Random(5)
    remap = [2, 5, 11]
    trees = [sc.add_covers(rng, fc.random_tree(rng, 3, 4, 0.9)) for _ in range(4)]
    for t in trees:
        t.feat = [remap[f] if f >= 0 else f for f in t.feat]
    X = fc.rows(17, 14, 0.3)
    for K in (1, 3):
        b = fc.booster(trees, K)
        for dm in matrices(X, 14):
            full = b.predict_interactions(dm)
            phi, used = b.predict_interactions(dm, compact=True)
            assert used.tolist() == remap and phi.shape[-2:] == (4, 4)
            assert full.shape[-2:] == (15, 15)
            idx = remap + [14]
            assert torch.equal(full[..., idx, :][..., idx], phi)
            assert int((full != 0).sum()) == int((phi != 0).sum())  # the same non-zeros
            part = b.predict_interactions(dm, rows=(3, 9))
            assert torch.equal(part, full[..., 3:9, :, :])
            part, used2 = b.predict_interactions(dm, compact=True, rows=(3, 9))
            assert torch.equal(part, phi[..., 3:9, :, :]) and used2.tolist() == remap
    with pytest.raises(ValueError):
        b.predict_interactions(dm, rows=(3, 99))


def test_edge_cases():
    trees, X = forest(), rows()
    base = fc.booster([], 1).base_margin
    for dm in matrices(X, F):
        got = fc.booster([], 1).predict_interactions(dm)  # no trees
        assert got.shape == (13, F + 1, F + 1) and bool((got[:, F, F] == base).all())
        assert int((got != 0).sum()) == 13 * (base != 0)
        leaves = [t for t in trees if len(t.feat) == 1]  # bias only
        got, used = fc.booster(leaves, 1).predict_interactions(dm, compact=True)
        assert used.numel() == 0 and got.shape == (13, 1, 1)
        assert float((got[:, 0, 0] - base - sum(t.leaf[0] for t in leaves)).abs().max()) < 1e-12
    for dm in matrices(X[:0], F):  # no rows
        assert fc.booster(trees, 1).predict_interactions(dm).shape == (0, F + 1, F + 1)
        assert fc.booster(trees, 3).predict_interactions(dm).shape == (3, 0, F + 1, F + 1)


def test_refusals():
    trees = forest()
    bad = fc.random_forest(seed=3, F=F, total_nodes=60, max_depth=4)[0]  # cover 0 everywhere
    while len(bad.feat) == 1:
        bad = fc.random_tree(random.Random(8), F, 4, 1.0)
    dm = matrices(rows(), F)[0]
    with pytest.raises(ValueError, match="tree 2 has no usable cover statistics"):
        fc.booster(trees[:2] + [bad] + trees[2:], 1).predict_interactions(dm)


def test_fp32_reference_is_close():
    """The error yardstick of the GPU tests is the same algorithm in fp32."""
    trees, X = forest(), rows(40)
    kw = dict(num_class=1, base=0.5, **sc.lists(trees))
    p64, used = hip().gbdt_shap_inter_rows(X=X, **kw)
    p32, _ = hip().gbdt_shap_inter_rows(X=X, f32=True, **kw)
    assert p64.dtype == p32.dtype == torch.float64 and used.dtype == torch.int32
    assert p64.shape == (1, 40, used.numel() + 1, used.numel() + 1)
    assert 0 < float((p64 - p32).abs().max()) < 1e-5
    assert torch.equal(p32, p32.transpose(-1, -2))
    keys, off, val = fc.csr_of(X)
    c32, _ = hip().gbdt_shap_inter_rows_csr(row_off=off, fid=keys.to(torch.int32), val=val,
                                            f32=True, **kw)
    assert torch.equal(c32, p32)


def test_accumulator_limit():
    """The packed triangles of a block's rows fit the CU's LDS beside a full
    path table up to the limit, and not with one more column."""
    U, C = hip().gbdt_shap_inter_lds_cols(), hip().gbdt_shap_lds_elems()
    assert U >= 32  # 28 features; and a group of 64 lanes can meet the LDS accumulator
    table = C * 36 + 65 * 4
    fits = [r for r in range(1, 65) if table + r * 4 * U * (U - 1) // 2 <= 160 * 1024]
    assert fits and table + max(fits) * 4 * (U + 1) * U // 2 > 160 * 1024


# ------------------------------------------------- the stand-alone binary
def test_host_inter_test_binary():
    exe = os.path.join(ROOT, "bin", "native", "gbdt_shap_inter_test")
    assert os.path.exists(exe), "native tools not built (python build_native.py)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_host_inter_test_binary_sanitized():
    b = subprocess.run([sys.executable, os.path.join(ROOT, "build_native.py"),
                        "--sanitize-shap-inter"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    exe = b.stdout.strip().splitlines()[-1]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ------------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """An agaricus model of 4 rounds, its margins, contributions and
    interactions."""
    d = tmp_path_factory.mktemp("shap_inter_cli")
    os.symlink(os.path.join(ROOT, "learn"), d / "learn")
    r = run(["-n", "1", XGB] + CONF + ["num_round=4", "model_out=m4.model"], d)
    assert r.returncode == 0, r.stderr[-2000:]
    for args in (["pred_margin=1", "name_pred=margin.txt"],
                 ["pred_contribs=1", "name_pred=contribs.txt"],
                 ["pred_interactions=1", "name_pred=inter.txt"]):
        r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model"] + args, d)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "unknown parameter" not in r.stdout + r.stderr
    return d


def parse(path):
    """Per line [(i, j, value)]."""
    out = []
    for line in open(path).read().split("\n")[:-1]:
        toks = [t.split(":") for t in line.split()]
        assert all(len(t) == 3 for t in toks)
        out.append([(int(i), int(j), float(v)) for i, j, v in toks])
    return out


def half_digit(v):
    """%g prints six significant digits: a printed value is off by at most
    half a unit of its sixth digit."""
    return 0.5 * 10.0 ** (math.floor(math.log10(abs(v))) - 5) if v else 0.0


def test_cli_pred_interactions(work):
    from wormhole_amd.models import gbdt as G
    b = G.Booster.load(str(work / "m4.model"), G.GBDTParam())
    nf = b.num_feature
    margin = [float(x) for x in open(work / "margin.txt")]
    contribs = [dict((int(t.split(":")[0]), float(t.split(":")[1])) for t in line.split())
                for line in open(work / "contribs.txt").read().split("\n")[:-1]]
    lines = parse(work / "inter.txt")
    assert len(lines) == len(margin) == len(contribs) == 1611
    used = {f for t in b.trees for f in t.feat if f >= 0}
    pairs = 0
    for toks, m, phi in zip(lines, margin, contribs):
        idx = [(i, j) for i, j, _ in toks]
        assert idx == sorted(set(idx)) and idx[-1] == (nf, nf)
        assert all(i <= j and {i, j} <= used and v != 0 for i, j, v in toks[:-1])
        pairs += sum(i < j for i, j in idx)
        # the diagonal plus twice the off-diagonal cells is the margin
        total = sum(v if i == j else 2 * v for i, j, v in toks)
        slack = sum(half_digit(v) * (1 if i == j else 2) for i, j, v in toks) + half_digit(m)
        assert abs(total - m) <= 1e-6 + slack
        # summed by row index, the cells are the contributions
        rowsum, rowslack = {}, {}
        for i, j, v in toks:
            for a in {i, j}:
                rowsum[a] = rowsum.get(a, 0.0) + v
                rowslack[a] = rowslack.get(a, 0.0) + half_digit(v)
        for a in set(rowsum) | set(phi):
            want = phi.get(a, 0.0)
            assert abs(rowsum.get(a, 0.0) - want) <= 1e-6 + rowslack.get(a, 0.0) + half_digit(want)
    assert pairs > 1611  # there are interactions
    assert len({toks[-1][2] for toks in lines}) == 1  # one bias


def test_cli_ntree_limit(work):
    for args in (["pred_interactions=1", "name_pred=inter2.txt"],
                 ["pred_margin=1", "name_pred=margin2.txt"]):
        r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "ntree_limit=2"] + args, work)
        assert r.returncode == 0 and "unknown parameter" not in r.stdout, r.stderr[-2000:]
    margin = [float(x) for x in open(work / "margin2.txt")]
    lines = parse(work / "inter2.txt")
    assert len(lines) == 1611
    for toks, m in zip(lines, margin):
        total = sum(v if i == j else 2 * v for i, j, v in toks)
        slack = sum(half_digit(v) * (1 if i == j else 2) for i, j, v in toks) + half_digit(m)
        assert abs(total - m) <= 1e-6 + slack
    assert open(work / "inter2.txt").read() != open(work / "inter.txt").read()


def test_cli_two_ranks_write_the_one_rank_file(work):
    r = run(["-n", "2", XGB] + PRED + ["model_in=m4.model", "pred_interactions=1",
                                       "name_pred=inter_2ranks.txt"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(work / "inter_2ranks.txt").read() == open(work / "inter.txt").read()


def test_cli_multiclass(tmp_path):
    from test_gbdt_multiclass import three_class_rows, write_libsvm
    X, y = three_class_rows(60)
    write_libsvm(tmp_path / "train.libsvm", X, y)
    r = run(["-n", "1", XGB, "objective=multi:softprob", "num_class=3", "max_depth=3", "eta=0.5",
             "data=train.libsvm", "num_round=2", "model_out=m.model"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    pred = ["-n", "1", XGB, "task=pred", "test:data=train.libsvm", "model_in=m.model"]
    for args in (["pred_interactions=1", "name_pred=i.txt"], ["pred_margin=1", "name_pred=m.txt"]):
        r = run(pred + args, tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
    margin = [float(x) for x in open(tmp_path / "m.txt")]
    lines = parse(tmp_path / "i.txt")
    assert len(lines) == len(margin) == 60 * 3  # one line per row and class, row-major
    for toks, m in zip(lines, margin):
        total = sum(v if i == j else 2 * v for i, j, v in toks)
        slack = sum(half_digit(v) * (1 if i == j else 2) for i, j, v in toks) + half_digit(m)
        assert abs(total - m) <= 1e-6 + slack and toks[-1][:2] == (X.shape[1], X.shape[1])


@pytest.mark.parametrize("other", ["pred_margin", "pred_leaf", "pred_contribs", "approx_contribs"])
def test_cli_excluded_combinations(work, other):
    r = run(["-n", "1", XGB] + PRED + ["model_in=m4.model", "pred_interactions=1", other + "=1"],
            work)
    assert r.returncode != 0 and "exclude each other" in r.stderr
    assert "pred_interactions=1 and %s=1" % other in r.stderr
