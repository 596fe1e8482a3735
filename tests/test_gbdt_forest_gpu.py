"""GBDT forest prediction on the GPU: the forest kernels (dense and CSR,
margins and leaf ids) make the decisions of the per-tree kernels and add the
same fp32 leaf values in the same order, so every comparison is
``torch.equal``: with one ``predict_tree`` per tree on the GPU, and with the
CPU path.

The forests hold about 2.5 x the LDS capacity in nodes (three or more chunks,
the last one partial); a second forest has one complete tree larger than the
capacity in the middle (the chunk walked from global memory)."""
import functools

import pytest
import torch

import _gbdt_forest_cases as fc

pytestmark = pytest.mark.gpu
# 70 001 rows: many blocks and a partial last one (the rows beyond what the
# persistent blocks hold at once: test_rows_beyond_the_resident_blocks)
NS = (1, 63, 64, 65, 257, 70_001)
FS = (1, 28, 130)
NANS = (0.0, 0.3)
SENTINEL = -12345.5


def dev():
    return torch.device("cuda", 0)


def capacity():
    from wormhole_amd import _native
    return _native.hip().gbdt_forest_lds_nodes()


@functools.lru_cache(maxsize=None)
def forest_trees(F, oversize):
    C = capacity()
    return tuple(fc.random_forest(seed=100 + F, F=F, total_nodes=int(2.5 * C),
                                  oversize=C if oversize else 0))


@functools.lru_cache(maxsize=2)
def cpu_leaf_ids(n, F, nan, oversize):
    """The CPU path's leaf ids [n, T] of a case (one torch walk per tree)."""
    from wormhole_amd.models import gbdt as G
    dm = G.DMatrix.from_dense(fc.rows(n, F, nan), torch.zeros(n), torch.device("cpu"))
    return fc.booster(forest_trees(F, oversize), 1).predict_leaf(dm)


def matrices(n, F, nan):
    from wormhole_amd.models import gbdt as G
    X = fc.rows(n, F, nan)
    dense = G.DMatrix.from_dense(X, torch.zeros(n), dev())
    csr = G.make_dmatrix(*fc.csr_of(X), torch.zeros(n), None, F, dev(), sparse=True)
    assert csr.sparse and not dense.sparse
    return dense, csr


def margin_view(K, n, base):
    """[n] or [K, n] filled with base, a view into a sentinel-filled buffer."""
    buf = torch.full((K, n + 16), SENTINEL, device=dev())
    out = buf[:, 8:8 + n]
    out.fill_(base)
    return buf, (out[0] if K == 1 else out)


def sentinels_intact(buf, n):
    return bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + n:] == SENTINEL).all())


def test_forests_cover_every_kernel_path():
    from wormhole_amd.models.gbdt_tree import Forest
    C = capacity()
    for F in FS:
        plain, big = forest_trees(F, False), forest_trees(F, True)
        assert len(plain) == len(big) and len(plain) % 3 == 1
        assert any(len(t.feat) == 1 for t in plain)
        assert {d for t in plain for d in t.defl} == {0, 1}
        assert max(t.depth(len(t.feat) - 1) for t in plain) == 8
        f = Forest(plain, dev())
        assert len(f.chunks) >= 3 and all(c[4] for c in f.chunks)
        assert f.chunks[-1][3] < C and f.max_feat < F
        g = Forest(big, dev())
        assert [c[4] for c in g.chunks].count(False) == 1
        k = [c[4] for c in g.chunks].index(False)
        assert 0 < k < len(g.chunks) - 1 and g.chunks[k][3] > C


@pytest.mark.parametrize("nan", NANS)
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("n", NS)
def test_forest_equals_per_tree_and_cpu(n, F, nan):
    from wormhole_amd.models.gbdt_tree import Forest
    dense, csr = matrices(n, F, nan)
    assert bool(torch.isnan(dense.X[n // 2]).all())
    for oversize in (False, True):
        trees = forest_trees(F, oversize)
        T = len(trees)
        ids_cpu = cpu_leaf_ids(n, F, nan, oversize)
        forest = Forest(trees, dev())
        for K in (1, 3):
            base = 0.5 if K == 1 else -0.25
            want_cpu = fc.margins_from_ids(trees, ids_cpu, K, base)
            for dm in (dense, csr):
                # the per-tree GPU loop, the parent's prediction
                loop = torch.full((K, n), base, device=dev())
                for t, tree in enumerate(trees):
                    dm.predict_tree(tree, loop[t % K])
                loop = loop[0] if K == 1 else loop
                buf, out = margin_view(K, n, base)
                dm.predict_forest(forest, out)
                assert torch.equal(out, loop), (K, dm.sparse, oversize)
                assert torch.equal(out.cpu(), want_cpu), (K, dm.sparse, oversize)
                assert sentinels_intact(buf, n)
        for dm in (dense, csr):
            ids = torch.full((n, T), -7, dtype=torch.int32, device=dev())
            dm.predict_forest(forest, ids, leaf=True)
            assert torch.equal(ids.cpu(), ids_cpu), (dm.sparse, oversize)


def test_derived_cpu_margins_are_the_cpu_path():
    """The reference above derives its margins from the CPU leaf ids; here
    that is checked to be Booster.predict_margin on the CPU, bit for bit, and
    the booster's own GPU route (forest cache included) against both."""
    from wormhole_amd.models import gbdt as G
    n, F, nan = 257, 28, 0.3
    X = fc.rows(n, F, nan)
    cpu = G.DMatrix.from_dense(X, torch.zeros(n), torch.device("cpu"))
    dense, csr = matrices(n, F, nan)
    for oversize in (False, True):
        trees = forest_trees(F, oversize)
        ids = cpu_leaf_ids(n, F, nan, oversize)
        for K in (1, 3):
            b = fc.booster(trees, K)
            want = b.predict_margin(cpu)
            assert torch.equal(fc.margins_from_ids(trees, ids, K, b.base_margin), want)
            assert torch.equal(b.predict_margin(dense).cpu(), want)
            assert torch.equal(b.predict_margin(csr).cpu(), want)
            assert torch.equal(b.predict_leaf(dense).cpu(), ids)
            assert torch.equal(b.predict_leaf(csr).cpu(), ids)


def test_one_tree_no_tree_no_row():
    from wormhole_amd.models import gbdt as G
    from wormhole_amd.models.gbdt_tree import Forest
    n, F = 65, 28
    dense, csr = matrices(n, F, 0.3)
    trees = forest_trees(F, False)
    deep = max(trees, key=lambda t: len(t.feat))
    ids_cpu = cpu_leaf_ids(n, F, 0.3, False)[:, trees.index(deep)]
    for dm in (dense, csr):
        for K in (1, 3):
            # T = 1: only class 0 moves
            buf, out = margin_view(K, n, 1.0)
            dm.predict_forest(Forest([deep], dev()), out)
            want = fc.margins_from_ids([deep], ids_cpu[:, None], K, 1.0)
            assert torch.equal(out.cpu(), want) and sentinels_intact(buf, n)
            # T = 0: nothing is launched, nothing moves
            buf, out = margin_view(K, n, 1.0)
            dm.predict_forest(Forest([], dev()), out)
            assert bool((out == 1.0).all()) and sentinels_intact(buf, n)
        assert fc.booster([], 1).predict_leaf(dm).shape == (n, 0)
    # n = 0
    empty, empty_csr = matrices(0, F, 0.0)
    forest = Forest(list(trees), dev())
    for dm in (empty, empty_csr):
        assert dm.predict_forest(forest, torch.empty(0, device=dev())).shape == (0,)
        assert dm.predict_forest(forest, torch.empty(3, 0, device=dev())).shape == (3, 0)
        ids = torch.empty((0, len(trees)), dtype=torch.int32, device=dev())
        assert dm.predict_forest(forest, ids, leaf=True).shape == (0, len(trees))
    # a forest that splits on a feature the matrix does not have is refused
    narrow = G.DMatrix.from_dense(fc.rows(5, 3, 0.0), torch.zeros(5), dev())
    with pytest.raises(RuntimeError, match="feature"):
        narrow.predict_forest(forest, torch.zeros(5, device=dev()))


def test_rows_beyond_the_resident_blocks():
    """The launch keeps at most two blocks (of at most 1024 rows) per CU and
    strides them over the rows: more rows than that, so every block takes
    further tiles and the last tile is partial. Seven trees keep the CPU walk
    short."""
    from wormhole_amd.models import gbdt as G
    from wormhole_amd.models.gbdt_tree import Forest
    F = 28
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 1024 * cus + 1025
    trees = list(forest_trees(F, False)[:7])
    X = fc.rows(n, F, 0.3)
    b = fc.booster(trees, 3)
    cpu = G.DMatrix.from_dense(X, torch.zeros(n), torch.device("cpu"))
    dense = G.DMatrix.from_dense(X, torch.zeros(n), dev())
    forest = Forest(trees, dev())
    assert len(forest.chunks) == 1
    loop = torch.full((3, n), b.base_margin, device=dev())
    for t, tree in enumerate(trees):
        dense.predict_tree(tree, loop[t % 3])
    buf, out = margin_view(3, n, b.base_margin)
    dense.predict_forest(forest, out)
    assert torch.equal(out, loop) and sentinels_intact(buf, n)
    assert torch.equal(out.cpu(), b.predict_margin(cpu))
    ids = torch.full((n, 7), -7, dtype=torch.int32, device=dev())
    dense.predict_forest(forest, ids, leaf=True)
    assert torch.equal(ids.cpu(), b.predict_leaf(cpu))


@pytest.mark.parametrize("K", [1, 3])
def test_ntree_limit_around_a_chunk_boundary(K):
    n, F, nan = 257, 28, 0.3
    dense, csr = matrices(n, F, nan)
    trees = forest_trees(F, False)
    ids_cpu = cpu_leaf_ids(n, F, nan, False)
    b = fc.booster(trees, K)
    edge = b.forest(dev()).chunks[0][1]  # trees in the first chunk
    assert 1 < edge < len(trees) - 1
    for limit in (edge - 1, edge, edge + 1, len(trees) + 3):
        T = min(limit, len(trees))
        want = fc.margins_from_ids(trees[:T], ids_cpu[:, :T], K, b.base_margin)
        for dm in (dense, csr):
            assert torch.equal(b.predict_margin(dm, limit).cpu(), want), limit
            assert b.forest(dev(), limit).ntree == T
            assert torch.equal(b.predict_leaf(dm, limit).cpu(), ids_cpu[:, :T]), limit


def test_xgboost_app_predictions_gpu(tmp_path, monkeypatch):
    """task=pred on the GPU writes the CPU app's pred.txt from the same model:
    default, pred_margin=1 and pred_leaf=1."""
    import os
    from wormhole_amd.apps.xgboost_app import main
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.symlink(os.path.join(root, "learn"), tmp_path / "learn")
    monkeypatch.chdir(tmp_path)
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    conf = ["learn/xgboost/mushroom.conf", "max_depth=3"]
    monkeypatch.setenv("WH_DEVICE", "auto")
    assert main(conf + ["num_round=4", "model_out=g.model"]) == 0
    for mode in ([], ["pred_margin=1"], ["pred_leaf=1"], ["pred_margin=1", "ntree_limit=2"]):
        for device in ("auto", "cpu"):
            monkeypatch.setenv("WH_DEVICE", device)
            assert main(conf + ["task=pred", "model_in=g.model",
                                "test:data=learn/data/agaricus.txt.test",
                                "name_pred=%s.txt" % device] + mode) == 0
        gpu, cpu = open(tmp_path / "auto.txt").read(), open(tmp_path / "cpu.txt").read()
        assert gpu.splitlines() == cpu.splitlines(), mode
        assert len(gpu.splitlines()) == (1611 * 4 if mode == ["pred_leaf=1"] else 1611)
