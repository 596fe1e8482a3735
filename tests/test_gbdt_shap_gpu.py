"""GBDT feature contributions on the GPU (csrc/hip/gbdt_shap.hip): the exact
TreeSHAP kernels (dense and CSR rows, lane groups of 16, 32 and 64, the LDS
and the global accumulator) and the Saabas kernel against the host float64
reference (csrc/host/gbdt_shap_plan.h), never against another GPU run.

Tolerance. Per case, err32 is the largest absolute difference between the
host fp32 and fp64 references over all entries of the case (257 rows, or
more); the GPU may differ from the fp64 reference by at most 8 x err32. Sub
runs of a case (fewer rows of the same matrix) use the case's err32.
Measured on one MI355X, the worst case of each family (err32 / largest GPU
error; the kernels take the fp32 reference's statements in its order, so the
two mostly meet in the same entry):
  small forests, F 1, 28, 130 (dense = CSR)  1.59e-06 / 1.59e-06 (small1)
  2.5 x capacity forest, K 1 and 3           1.37e-06 / 6.78e-07, 8.34e-07 / 8.34e-07
  chains of 15 .. 63 elements                3.78e-07 / 3.78e-07 (chain15)
  U + 1 = limit and limit + 1                4.72e-07 / 4.72e-07, 3.98e-07 / 3.98e-07
  Saabas                                     2.21e-07 / 2.21e-07 (chain33)
  largest GPU error / err32 of any run       1.07 (Saabas, small28, K = 3)
  the app's file                             8.02e-07; largest printed difference 1e-06
The app's files are compared token by token; a printed value carries six
significant digits (%g), so two printed values may differ by the bound above
plus one unit of the sixth digit of the larger one (half a unit of print
rounding each)."""
import functools
import math
import os
import random
import subprocess
import sys

import pytest
import torch

import _gbdt_forest_cases as fc
import _gbdt_shap_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.5
N = 257  # rows of a case


def dev():
    return torch.device("cuda", 0)


def hip():
    from wormhole_amd import _native
    return _native.hip()


# ------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def model(name):
    """(trees, F) of a named case."""
    C, cols = hip().gbdt_shap_lds_elems(), hip().gbdt_shap_lds_cols()
    if name.startswith("small"):  # small1, small28, small130
        F = int(name[5:])
        return tuple(sc.forest_of_elems(3 + F, F, 300)), F
    if name == "big":  # about 2.5 x the element capacity: three or more chunks
        return tuple(sc.forest_of_elems(9, 28, int(2.5 * C))), 28
    if name.startswith("chain"):  # chain15 .. chain63: the longest path, and small trees
        L = int(name[5:])
        trees = [sc.chain_tree(L, L, list(range(L)))] + sc.forest_of_elems(L, 64, 100, 4)
        return tuple(trees), 64
    if name in ("under", "over"):  # U + 1 = the LDS accumulator's limit, and one more
        U = cols - 1 if name == "under" else cols
        trees = [sc.chain_tree(1, 63, list(range(63))), sc.chain_tree(2, 20, list(range(63, 83)))]
        for k in range(83, U, 8):
            fs = list(range(k, min(k + 8, U)))
            trees.append(sc.chain_tree(k, len(fs), fs))
        return tuple(trees), U
    raise KeyError(name)


CHAINS = ["chain%d" % L for L in (15, 16, 17, 31, 32, 33, 63)]
MODELS = ["small1", "small28", "small130", "big"] + CHAINS + ["under", "over"]


def host(trees, K, X, approx=False, f32=False, base=0.5):
    """The host reference: float64 [K, n, U + 1], compact."""
    phi, _ = hip().gbdt_shap_rows(num_class=K, base=base, X=X.contiguous(), approx=approx,
                                  f32=f32, **sc.lists(trees))
    return phi


@functools.lru_cache(maxsize=None)
def reference(name, K=1, approx=False, limit=0):
    """(fp64 reference [K, N, U + 1], err32) of a case over its N rows."""
    trees, F = model(name)
    trees = trees[:limit] if limit else trees
    X = fc.rows(N, F, 0.3)
    ref = host(trees, K, X, approx)
    err32 = float((host(trees, K, X, approx, f32=True) - ref).abs().max())
    return ref, err32


def booster(trees, K, base=0.5):
    b = fc.booster(trees, K)
    b.base_margin = base
    return b


def matrix(X, F, kind):
    from wormhole_amd.models import gbdt as G
    n = X.shape[0]
    if kind == "dense":
        return G.DMatrix.from_dense(X, torch.zeros(n), dev())
    return G.make_dmatrix(*fc.csr_of(X), torch.zeros(n), None, F, dev(), sparse=True)


def run(name, n, kind, K=1, approx=False, limit=0):
    """The GPU's compact contributions [K, n, U + 1] of the case's first n
    rows, checked against the reference; also the margins they must sum to."""
    trees, F = model(name)
    X = fc.rows(N, F, 0.3)[:n]
    dm = matrix(X, F, kind)
    b = booster(trees, K)
    got, used = b.predict_contribs(dm, limit, approx=approx, compact=True)
    got = got[None] if K == 1 else got
    assert got.dtype == torch.float32 and got.is_cuda
    ref, err32 = reference(name, K, approx, limit)
    assert got.shape == (K, n, ref.shape[2]) and used.numel() + 1 == ref.shape[2]
    err = float((got.cpu().double() - ref[:, :n]).abs().max()) if n else 0.0
    print("%s n=%d %s K=%d approx=%d limit=%d: err32 %.3g gpu %.3g" % (
        name, n, kind, K, approx, limit, err32, err))
    assert err <= 8 * err32, (err, err32)
    margin = b.predict_margin(dm, limit)
    margin = margin[None] if K == 1 else margin
    # U + 1 entries within 8 x err32 each; the margin itself is an fp32 sum of
    # T leaves: every addition rounds a partial sum that is at most M
    used_trees = trees[:limit] if limit else trees
    M = 0.5 + sum(max(abs(v) for v in t.leaf) for t in used_trees)
    tol = 8 * err32 * ref.shape[2] + (len(used_trees) + 1) * 2.0 ** -24 * M
    if n:
        assert float((got.double().sum(-1) - margin.double()).abs().max()) <= tol
    return got


# ------------------------------------------------------------- the tests
def test_cases_cover_every_kernel_variant():
    """Lane groups of 16, 32 and 64 with the LDS and with the global
    accumulator; three or more chunks, the last one partial; single leaves."""
    from wormhole_amd.models.gbdt_tree import ShapForest
    C, cols = hip().gbdt_shap_lds_elems(), hip().gbdt_shap_lds_cols()
    seen = set()
    for name in MODELS:
        trees, F = model(name)
        sf = ShapForest(list(trees), 1, 0.0, dev())
        lds = sf.used.numel() + 1 <= cols
        seen |= {(c[5], lds) for c in sf.chunks}
        longest = int(sf.paths[:, 1].max())
        if name.startswith("chain"):
            assert longest == int(name[5:])
        if name == "big":
            assert len(sf.chunks) >= 3 and 0 < sf.chunks[-1][3] < C
            assert sum(c[3] for c in sf.chunks) >= 2.5 * C
            assert any(len(t.feat) == 1 for t in trees)
        if name in ("under", "over"):
            assert sf.used.numel() + 1 == cols + (name == "over")
    assert seen == {(w, a) for w in (16, 32, 64) for a in (True, False)}


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, N])
def test_row_counts(n, kind):
    """1 and 257 rows, and the rows of one wave (4 groups of 16 lanes) and of
    one block (64 groups) with one less and one more."""
    run("small28", n, kind)


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("name", ["small1", "small130"] + CHAINS + ["under", "over"])
def test_models(name, kind):
    run(name, N, kind)


@pytest.mark.parametrize("name,n", [("chain33", 1), ("chain33", 2), ("chain33", 15),
                                    ("chain33", 16), ("chain33", 17), ("chain17", 1),
                                    ("chain17", 2), ("chain17", 3), ("chain17", 31),
                                    ("chain17", 32), ("chain17", 33)])
def test_wider_groups_around_a_wave_and_a_block(name, n):
    """64 lanes: 1 row per wave, 16 per block; 32 lanes: 2 and 32."""
    run(name, n, "dense")


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("K", [1, 3])
def test_big_forest(K, kind):
    run("big", N, kind, K=K)


def test_ntree_limit_around_a_chunk_boundary():
    from wormhole_amd.models.gbdt_tree import ShapForest
    trees, F = model("big")
    sf = ShapForest(list(trees), 1, 0.0, dev())
    edge = int(sf.paths[sf.chunks[0][1] - 1, 3]) + 1  # trees with a path in the first chunk
    assert 1 < edge < len(trees)
    for limit in (edge - 1, edge, edge + 1):
        run("big", 64, "dense", limit=limit)


def test_rows_beyond_the_resident_grid():
    """The grid strides over row tiles: more tiles than resident blocks."""
    trees, F = model("small28")
    trees = trees[:3]
    n = hip().gbdt_shap_max_blocks() * 64 + 5
    X = fc.rows(n, F, 0.3)
    ref = host(trees, 1, X)
    err32 = float((host(trees, 1, X, f32=True) - ref).abs().max())
    got, _ = booster(trees, 1).predict_contribs(matrix(X, F, "dense"), compact=True)
    assert float((got.cpu().double() - ref[0]).abs().max()) <= 8 * err32


def test_wide_csr():
    """ncol = 100 000 and a handful of used features: the cost is U, not F."""
    from wormhole_amd.models import gbdt as G
    remap = [5, 77, 4096, 65536, 77777, 99999]
    trees = [sc.add_covers(random.Random(t), fc.random_tree(random.Random(50 + t), 6, 6, 0.9))
             for t in range(8)]
    for t in trees:
        t.feat = [remap[f] if f >= 0 else f for f in t.feat]
    X6 = fc.rows(N, 6, 0.3)
    keys, off, val = fc.csr_of(X6)
    keys = torch.tensor(remap)[keys]
    dm = G.make_dmatrix(keys, off, val, torch.zeros(N), None, 100000, dev(), sparse=True)
    cpu = G.make_dmatrix(keys, off, val, torch.zeros(N), None, 100000, torch.device("cpu"),
                         sparse=True)
    b = booster(trees, 1)
    got, used = b.predict_contribs(dm, compact=True)
    ref, used_cpu = b.predict_contribs(cpu, compact=True)
    assert used.tolist() == used_cpu.tolist() == sorted(set(used.tolist())) and got.shape[1] <= 7
    p32, _ = hip().gbdt_shap_rows_csr(num_class=1, base=0.5, row_off=cpu.row_off, fid=cpu.fid,
                                      val=cpu.val, f32=True, **sc.lists(trees))
    err32 = float((p32[0] - ref).abs().max())
    assert float((got.cpu().double() - ref).abs().max()) <= 8 * err32
    full = b.predict_contribs(dm)
    assert full.shape == (N, 100001) and torch.equal(full[:, used.to(dev())], got[:, :-1])
    assert torch.equal(full[:, -1], got[:, -1]) and int((full != 0).sum()) == int((got != 0).sum())


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("name,K", [("small28", 1), ("small28", 3), ("chain33", 1), ("over", 1)])
def test_saabas(name, K, kind):
    run(name, N, kind, K=K, approx=True)
    run(name, 5, kind, K=K, approx=True)


@pytest.mark.parametrize("name", ["small28", "chain63", "over"])
def test_deterministic_and_independent_of_n(name):
    a = run(name, N, "dense")
    assert torch.equal(a, run(name, N, "dense"))
    assert torch.equal(a[:, :64], run(name, 64, "dense"))
    c = run(name, N, "csr")
    assert torch.equal(c[:, :64], run(name, 64, "csr"))


@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("name", ["small28", "over"])
def test_sentinel_frame(name, approx):
    """The kernels write nothing outside [K, n, U + 1]."""
    from wormhole_amd.models.gbdt_tree import ShapForest
    trees, F = model(name)
    K, n = 3, 37
    sf = ShapForest(list(trees), K, 0.5, dev())
    U1 = sf.used.numel() + 1
    buf = torch.full((K * n * U1 + 128,), SENTINEL, device=dev())
    out = buf[64:64 + K * n * U1].view(K, n, U1)
    out.copy_(sf.new_out(n, dev()))
    X = fc.rows(N, F, 0.3)[:n].to(dev()).contiguous()
    if approx:
        hip().gbdt_saabas(X=X, nodes=sf.nodes, tree_off=sf.tree_off, node_m=sf.node_m,
                          node_col=sf.node_col, ncol=U1 - 1, max_feat=sf.max_feat, out=out)
    else:
        hip().gbdt_shap(X=X, paths=sf.paths, elems=sf.elems, ecol=sf.ecol, chunks=sf.chunks,
                        ncol=U1 - 1, max_feat=sf.max_feat, out=out)
    torch.cuda.synchronize()
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + K * n * U1:] == SENTINEL).all())
    ref = host(trees, K, X.cpu(), approx)
    err32 = float((host(trees, K, X.cpu(), approx, f32=True) - ref).abs().max())
    assert float((out.cpu().double() - ref).abs().max()) <= 8 * err32
    assert bool((out[:, :, -1] == sf.bias.float().to(dev())[:, None]).all())


def test_no_trees_and_no_rows():
    trees, F = model("small28")
    X = fc.rows(N, F, 0.3)
    for kind in ("dense", "csr"):
        for approx in (False, True):
            got = booster([], 1).predict_contribs(matrix(X[:9], F, kind), approx=approx)
            assert got.shape == (9, F + 1) and bool((got[:, :F] == 0).all())
            assert bool((got[:, F] == 0.5).all())
            got = booster(trees, 3).predict_contribs(matrix(X[:0], F, kind), approx=approx)
            assert got.shape == (3, 0, F + 1)
            leaves = [t for t in trees if len(t.feat) == 1]
            got, used = booster(leaves, 1).predict_contribs(matrix(X[:9], F, kind), approx=approx,
                                                            compact=True)
            assert used.numel() == 0 and got.shape == (9, 1)
            assert abs(float(got[0, 0]) - 0.5 - sum(t.leaf[0] for t in leaves)) < 1e-5


def test_refusals():
    trees = [sc.chain_tree(4, 64, list(range(64)))]
    X = fc.rows(9, 64, 0.3)
    with pytest.raises(ValueError, match="tree 0 has a path of 64"):
        booster(trees, 1).predict_contribs(matrix(X, 64, "dense"))
    t = sc.chain_tree(5, 3, [0, 1, 2])
    t.cover = [0.0] * len(t.feat)
    with pytest.raises(ValueError, match="tree 1 has no usable cover statistics"):
        booster([trees[0], t], 1).predict_contribs(matrix(X, 64, "dense"), approx=True)
    # a forest that splits on a feature the dense matrix does not have
    with pytest.raises(RuntimeError, match="does not have"):
        booster([sc.chain_tree(6, 5, list(range(5)))], 1).predict_contribs(
            matrix(X[:, :3].contiguous(), 3, "dense"))


# -------------------------------------------------------------------- app
def test_app_file_matches_the_cpu(tmp_path):
    """bin/xgboost.dmlc pred_contribs=1 on the GPU and on the CPU: the same
    indices on every line, values within the module's tolerance."""
    from wormhole_amd.models import gbdt as G
    tracker = os.path.join(ROOT, "tracker", "dmlc_local.py")
    xgb = os.path.join(ROOT, "bin", "xgboost.dmlc")
    os.symlink(os.path.join(ROOT, "learn"), tmp_path / "learn")
    conf = ["learn/xgboost/mushroom.conf", "max_depth=3", "eval_train=0"]

    def app(args, device):
        r = subprocess.run([sys.executable, tracker, "-n", "1", xgb] + conf + args, cwd=tmp_path,
                           env=dict(os.environ, WH_DEVICE=device), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]

    app(["num_round=4", "model_out=m.model"], "cpu")
    pred = ["task=pred", "test:data=learn/data/agaricus.txt.test", "model_in=m.model",
            "pred_contribs=1"]
    app(pred + ["name_pred=cpu.txt"], "cpu")
    app(pred + ["name_pred=gpu.txt"], "auto")
    b = G.Booster.load(str(tmp_path / "m.model"), G.GBDTParam())
    raw = G._native.host().load_split(os.path.join(ROOT, "learn/data/agaricus.txt.test"), 0, 1,
                                      "libsvm")
    dm = G.make_dmatrix(*raw, ncol=b.num_feature, device=torch.device("cpu"))
    ref, _ = b.predict_contribs(dm, compact=True)
    p32, _ = hip().gbdt_shap_rows(num_class=1, base=b.base_margin, X=dm.X, f32=True,
                                  **sc.lists(b.trees))
    err32 = float((p32[0] - ref).abs().max())
    cpu = open(tmp_path / "cpu.txt").read().split("\n")
    gpu = open(tmp_path / "gpu.txt").read().split("\n")
    assert len(cpu) == len(gpu) == dm.n + 1
    worst = 0.0
    for lc, lg in zip(cpu[:-1], gpu[:-1]):
        tc, tg = [t.split(":") for t in lc.split()], [t.split(":") for t in lg.split()]
        assert [t[0] for t in tc] == [t[0] for t in tg] and tc[-1][0] == str(b.num_feature)
        for (_, vc), (_, vg) in zip(tc, tg):
            vc, vg = float(vc), float(vg)
            big = max(abs(vc), abs(vg))
            digit = 10.0 ** (math.floor(math.log10(big)) - 5) if big else 0.0
            worst = max(worst, abs(vc - vg))
            assert abs(vc - vg) <= 8 * err32 + digit * 1.0000001, (lc, lg)
    print("app: err32 %.3g, largest printed difference %.3g" % (err32, worst))
