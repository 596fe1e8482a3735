"""GBDT SHAP interaction values on the GPU (csrc/hip/gbdt_shap.hip:
k_shap_inter over dense and CSR rows, lane groups of 16, 32 and 64, the LDS
and the global triangle, and the epilogue) against the host float64 reference
(csrc/host/gbdt_shap_plan.h), never against another GPU run.

Tolerance. Per case, err32 is the largest absolute difference between the
host fp32 and fp64 references over all cells of the case's 257 rows; the GPU
may differ from the fp64 reference by at most 8 x err32: the kernel takes the
fp32 reference's statements in its order, and differs from it only in the
order in which a row's paths are added (chunk by chunk). Sub runs of a case
(fewer rows of the same matrix) use the case's err32. Row sums are compared
with the GPU's predict_contribs within 8 x err32 x (U + 1).
Measured on one MI355X, the 257-row run with the largest GPU error of each
family (err32 / GPU error; the two mostly meet in the same cell):
  small forests, F 1, 28, 130 (dense = CSR)  1.59e-06 / 1.59e-06 (small1)
  2.5 x capacity forest, K 1 and 3           1.54e-06 / 8.29e-07, 8.72e-07 / 8.72e-07
  chains of 15 .. 63 elements                9.03e-07 / 9.03e-07 (chain31)
  U = limit, limit + 1                       5.81e-07 / 5.81e-07, 9.67e-07 / 9.91e-07
  U = limit, a full table (704 threads)      2.78e-05 / 9.44e-06
  largest GPU error / err32 of any run       1.13 (chain17, 257 rows, dense)
  the app's file                             9.08e-07; largest printed difference 1e-06
The app's files are compared token by token; a printed value carries six
significant digits (%g), so two printed values may differ by the bound above
plus one unit of the sixth digit of the larger one.
"""
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
from test_gbdt_shap_gpu import CHAINS, N, ROOT, SENTINEL, booster, dev, hip, matrix
from test_gbdt_shap_gpu import model as shap_model

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def model(name):
    """(trees, F) of a named case: those of test_gbdt_shap_gpu.py, and
    "under" / "over" anew for this kernel's accumulator limit: U = the limit
    and one more, each with a path over every feature (64 lanes at the
    limit), a chain of 20 (32 lanes) and small trees (16 lanes). "full" is
    "under" and stumps (one path element each) until a chunk's table is all
    but full: the block that still fits its rows' triangles in LDS is the
    smallest one, 704 threads; the other cases run 1024."""
    if name in ("under", "over", "full"):
        U = hip().gbdt_shap_inter_lds_cols() + (name == "over")
        trees = [sc.chain_tree(1, U, list(range(U))), sc.chain_tree(2, 20, list(range(5, 25)))]
        trees += sc.forest_of_elems(U, U, 100, 4)
        if name == "full":
            trees += [sc.chain_tree(100 + k, 1, [k % U]) for k in range(1100)]
        return tuple(trees), U
    return shap_model(name)


MODELS = ["small1", "small28", "small130", "big"] + CHAINS + ["under", "over", "full"]


def host(trees, K, X, f32=False, base=0.5):
    """The host reference: float64 [K, n, U + 1, U + 1], compact."""
    phi, _ = hip().gbdt_shap_inter_rows(num_class=K, base=base, X=X.contiguous(), f32=f32,
                                        **sc.lists(trees))
    return phi


@functools.lru_cache(maxsize=None)
def reference(name, K=1, limit=0):
    """(fp64 reference [K, N, U + 1, U + 1], err32) of a case over its N rows."""
    trees, F = model(name)
    trees = trees[:limit] if limit else trees
    X = fc.rows(N, F, 0.3)
    ref = host(trees, K, X)
    err32 = float((host(trees, K, X, f32=True) - ref).abs().max())
    return ref, err32


def run(name, n, kind, K=1, limit=0):
    """The GPU's compact interactions [K, n, U + 1, U + 1] of the case's
    first n rows, checked against the reference, for symmetry and against
    the GPU's contributions."""
    trees, F = model(name)
    X = fc.rows(N, F, 0.3)[:n]
    dm = matrix(X, F, kind)
    b = booster(trees, K)
    got, used = b.predict_interactions(dm, limit, compact=True)
    got = got[None] if K == 1 else got
    assert got.dtype == torch.float32 and got.is_cuda
    ref, err32 = reference(name, K, limit)
    U1 = ref.shape[2]
    assert got.shape == (K, n, U1, U1) and used.numel() + 1 == U1
    err = float((got.cpu().double() - ref[:, :n]).abs().max()) if n else 0.0
    print("%s n=%d %s K=%d limit=%d: err32 %.3g gpu %.3g ratio %.3g" % (
        name, n, kind, K, limit, err32, err, err / err32 if err32 else 0.0))
    assert err <= 8 * err32, (err, err32)
    assert torch.equal(got, got.transpose(-1, -2))  # bit for bit
    assert bool((got[:, :, -1, :-1] == 0).all())
    phi, _ = b.predict_contribs(dm, limit, compact=True)
    phi = phi[None] if K == 1 else phi
    assert torch.equal(got[:, :, -1, -1], phi[:, :, -1])
    if n:
        assert float((got.double().sum(-1) - phi.double()).abs().max()) <= 8 * err32 * U1
    return got


# ------------------------------------------------------------- the tests
def test_cases_cover_every_kernel_variant():
    """Lane groups of 16, 32 and 64 with the LDS and with the global
    triangle; three or more chunks; a model without pairs."""
    from wormhole_amd.models.gbdt_tree import ShapForest
    cols = hip().gbdt_shap_inter_lds_cols()
    seen = set()
    for name in MODELS:
        trees, F = model(name)
        sf = ShapForest(list(trees), 1, 0.0, dev())
        U = sf.used.numel()
        seen |= {(c[5], U <= cols) for c in sf.chunks}
        if name == "small1":
            assert U == 1
        if name == "big":
            assert len(sf.chunks) >= 3 and U <= cols
        if name in ("under", "over", "full"):
            assert U == cols + (name == "over")
            assert {c[5] for c in sf.chunks} == {16, 32, 64}
        # whole waves whose rows' triangles (threads / width rows of
        # 2 U (U - 1) bytes) fit the 160 KB beside the chunk's table
        room = 160 * 1024 - 65 * 4
        threads = {min(1024, (room - c[1] * 16 - c[3] * 20) * c[5] // (2 * U * (U - 1)) // 64 * 64)
                   for c in sf.chunks if 2 <= U <= cols}
        if name == "full":
            assert 704 in threads
        else:
            assert threads <= {1024}
    assert seen == {(w, a) for w in (16, 32, 64) for a in (True, False)}


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 43, 44, 45, 63, 64, 65, N])
def test_row_counts(n, kind):
    """1 and 257 rows, the rows of one wave (4 groups of 16 lanes) and of one
    block (64 groups, or 44 in the smallest block: test_smallest_block) with
    one less and one more."""
    run("small28", n, kind)


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("name", ["small1", "small130"] + CHAINS + ["under", "over"])
def test_models(name, kind):
    run(name, N, kind)


@pytest.mark.parametrize("name,n", [("chain33", 1), ("chain33", 2), ("chain33", 15),
                                    ("chain33", 16), ("chain33", 17), ("chain17", 1),
                                    ("chain17", 2), ("chain17", 3), ("chain17", 31),
                                    ("chain17", 32), ("chain17", 33), ("under", 15),
                                    ("under", 16), ("under", 17), ("under", 33)])
def test_wider_groups_around_a_wave_and_a_block(name, n):
    """64 lanes: 1 row per wave, 16 per block; 32 lanes: 2 and 32; with the
    global triangle (chain33, chain17) and the LDS one (under)."""
    run(name, n, "dense")


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("n", [43, 44, 45, N])
def test_smallest_block(n, kind):
    """A table that is all but full at the column limit: 704 threads, 44 rows
    a block, in the chunk of the short paths."""
    run("full", n, kind)


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
    got, _ = booster(trees, 1).predict_interactions(matrix(X, F, "dense"), compact=True)
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
    got, used = b.predict_interactions(dm, compact=True)
    ref, used_cpu = b.predict_interactions(cpu, compact=True)
    assert used.tolist() == used_cpu.tolist() == sorted(set(used.tolist()))
    assert got.shape[1] == got.shape[2] <= 7
    p32, _ = hip().gbdt_shap_inter_rows_csr(num_class=1, base=0.5, row_off=cpu.row_off,
                                            fid=cpu.fid, val=cpu.val, f32=True,
                                            **sc.lists(trees))
    err32 = float((p32[0] - ref).abs().max())
    assert float((got.cpu().double() - ref).abs().max()) <= 8 * err32


@pytest.mark.parametrize("name", ["small28", "chain63", "under", "over"])
def test_deterministic_and_independent_of_n(name):
    a = run(name, N, "dense")
    assert torch.equal(a, run(name, N, "dense"))
    assert torch.equal(a[:, :64], run(name, 64, "dense"))
    c = run(name, N, "csr")
    assert torch.equal(c[:, :64], run(name, 64, "csr"))


@pytest.mark.parametrize("name", ["small28", "over"])
def test_sentinel_frame(name):
    """The kernels write nothing outside [K, n, U + 1, U + 1], and every cell
    inside it but the bias the caller set."""
    from wormhole_amd.models.gbdt_tree import ShapForest
    trees, F = model(name)
    K, n = 3, 37
    sf = ShapForest(list(trees), K, 0.5, dev())
    U1 = sf.used.numel() + 1
    size = K * n * U1 * U1
    buf = torch.full((size + 128,), SENTINEL, device=dev())
    out = buf[64:64 + size].view(K, n, U1, U1)
    out[:, :, -1, -1] = sf.bias.float().to(dev())[:, None]
    X = fc.rows(N, F, 0.3)[:n].to(dev()).contiguous()
    hip().gbdt_shap_inter(X=X, paths=sf.paths, elems=sf.elems, ecol=sf.ecol, chunks=sf.chunks,
                          ncol=U1 - 1, max_feat=sf.max_feat, out=out)
    torch.cuda.synchronize()
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + size:] == SENTINEL).all())
    assert not bool((out == SENTINEL).any())
    ref = host(trees, K, X.cpu())
    err32 = float((host(trees, K, X.cpu(), f32=True) - ref).abs().max())
    assert float((out.cpu().double() - ref).abs().max()) <= 8 * err32
    assert bool((out[:, :, -1, -1] == sf.bias.float().to(dev())[:, None]).all())


def test_no_trees_and_no_rows():
    trees, F = model("small28")
    X = fc.rows(N, F, 0.3)
    for kind in ("dense", "csr"):
        got = booster([], 1).predict_interactions(matrix(X[:9], F, kind))
        assert got.shape == (9, F + 1, F + 1) and bool((got[:, F, F] == 0.5).all())
        assert int((got != 0).sum()) == 9
        got = booster(trees, 3).predict_interactions(matrix(X[:0], F, kind))
        assert got.shape == (3, 0, F + 1, F + 1)
        leaves = [t for t in trees if len(t.feat) == 1]
        got, used = booster(leaves, 1).predict_interactions(matrix(X[:9], F, kind), compact=True)
        assert used.numel() == 0 and got.shape == (9, 1, 1)
        assert abs(float(got[0, 0, 0]) - 0.5 - sum(t.leaf[0] for t in leaves)) < 1e-5


def test_refusals():
    trees = [sc.chain_tree(4, 64, list(range(64)))]
    X = fc.rows(9, 64, 0.3)
    with pytest.raises(ValueError, match="tree 0 has a path of 64"):
        booster(trees, 1).predict_interactions(matrix(X, 64, "dense"))
    t = sc.chain_tree(5, 3, [0, 1, 2])
    t.cover = [0.0] * len(t.feat)
    with pytest.raises(ValueError, match="tree 1 has no usable cover statistics"):
        booster([trees[0], t], 1).predict_interactions(matrix(X, 64, "dense"))
    # a forest that splits on a feature the dense matrix does not have
    with pytest.raises(RuntimeError, match="does not have"):
        booster([sc.chain_tree(6, 5, list(range(5)))], 1).predict_interactions(
            matrix(X[:, :3].contiguous(), 3, "dense"))


# -------------------------------------------------------------------- app
def test_app_file_matches_the_cpu(tmp_path):
    """bin/xgboost.dmlc pred_interactions=1 on the GPU and on the CPU: the
    same index pairs on every line, values within the module's tolerance."""
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
            "pred_interactions=1"]
    app(pred + ["name_pred=cpu.txt"], "cpu")
    app(pred + ["name_pred=gpu.txt"], "auto")
    b = G.Booster.load(str(tmp_path / "m.model"), G.GBDTParam())
    raw = G._native.host().load_split(os.path.join(ROOT, "learn/data/agaricus.txt.test"), 0, 1,
                                      "libsvm")
    dm = G.make_dmatrix(*raw, ncol=b.num_feature, device=torch.device("cpu"))
    ref, _ = b.predict_interactions(dm, compact=True)
    p32, _ = hip().gbdt_shap_inter_rows(num_class=1, base=b.base_margin, X=dm.X, f32=True,
                                        **sc.lists(b.trees))
    err32 = float((p32[0] - ref).abs().max())
    cpu = open(tmp_path / "cpu.txt").read().split("\n")
    gpu = open(tmp_path / "gpu.txt").read().split("\n")
    assert len(cpu) == len(gpu) == dm.n + 1
    worst = 0.0
    for lc, lg in zip(cpu[:-1], gpu[:-1]):
        tc, tg = [t.split(":") for t in lc.split()], [t.split(":") for t in lg.split()]
        assert [t[:2] for t in tc] == [t[:2] for t in tg]
        assert tc[-1][:2] == [str(b.num_feature)] * 2
        for (_, _, vc), (_, _, vg) in zip(tc, tg):
            vc, vg = float(vc), float(vg)
            big = max(abs(vc), abs(vg))
            digit = 10.0 ** (math.floor(math.log10(big)) - 5) if big else 0.0
            worst = max(worst, abs(vc - vg))
            assert abs(vc - vg) <= 8 * err32 + digit * 1.0000001, (lc, lg)
    print("app: err32 %.3g, largest printed difference %.3g" % (err32, worst))
