"""Multi-class GBDT on the GPU: the softmax gradient / prediction / evaluation
kernels against the formulas evaluated in fp64, the per-class plumbing through
the dense and CSR builders, and the app end to end.

Element tolerance of the kernels: the fp32 plain-torch fallback (the CPU path
of ``Objective``) is measured against fp64 on the same inputs; a kernel may be
at most 4x as far off (its expf and division may round differently from
torch's), with a floor of 1e-6 x the row weight. The bound comes from the
fallback, never from the kernel."""
import functools
import math
import re

import pytest
import torch

from test_gbdt_multiclass import three_class_rows, write_libsvm

pytestmark = pytest.mark.gpu
NLL_MAX = -math.log(1e-16)
# n = 300 001: more than one grid-stride pass of the 1024 x 256 threads, so
# the stride loop and the last-block reduction over all 1024 blocks both run
NS = (1, 63, 64, 65, 257, 300_001)
# K <= 8: the register path (margins read once); 33: the any-K path; 256 and
# 300 (n = 65 only): one full LDS pass of classes, and a second partial one
CASES = [(n, k) for n in NS for k in (2, 3, 7, 33)] + [(65, 256), (65, 300)]


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=4)
def inputs(n, K, weighted, wide):
    """CPU inputs of a case and their fp64 softmax. wide: margins over +-80
    with exact +-80 entries and row 0 all equal; else N(0, 3)."""
    g = torch.Generator().manual_seed(1000 * K + n % 997 + 2 * weighted + wide)
    if wide:
        margin = (torch.rand(K, n, generator=g) * 160 - 80)
        margin[torch.rand(K, n, generator=g) < 0.1] = 80.0
        margin[torch.rand(K, n, generator=g) < 0.1] = -80.0
        margin[:, 0] = 80.0
    else:
        margin = torch.randn(K, n, generator=g) * 3
    label = torch.randint(0, K, (n,), generator=g).float()
    weight = (torch.rand(n, generator=g) * 1.5 + 0.5) if weighted else None
    p64 = torch.softmax(margin.double(), 0)
    return margin, label, weight, p64


def gpair64(p64, label, weight):
    K = p64.shape[0]
    hit = (label[None, :] == torch.arange(K)[:, None].float()).double()
    w = weight.double()[None, :] if weight is not None else 1.0
    return torch.stack([(p64 - hit) * w, torch.clamp(2 * p64 * (1 - p64), min=1e-16) * w], 2)


def first_argmax(margin):
    """The lowest class among a row's maxima (explicit about exact ties)."""
    K = margin.shape[0]
    ids = torch.arange(K)[:, None].expand_as(margin)
    return torch.where(margin == margin.max(0).values, ids, torch.full_like(ids, K)).min(0).values


def bound(fallback, ref, weight, shape_like):
    """max(4 x the fallback's own max error, 1e-6 x row weight), per element."""
    e = float((fallback.double() - ref).abs().max()) if ref.numel() else 0.0
    w = weight.double() if weight is not None else torch.ones(shape_like.shape[1]).double()
    return torch.maximum(torch.full_like(w, 4 * e), 1e-6 * w), e


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,K", CASES)
def test_gpair_softmax_kernel(n, K, weighted, wide):
    from wormhole_amd import _native
    from wormhole_amd.models import gbdt as G
    margin, label, weight, p64 = inputs(n, K, weighted, wide)
    ref = gpair64(p64, label, weight)
    obj = G.Objective("multi:softprob", K)
    fb = obj.gpair(margin, label, weight)  # the plain-torch fp32 path (CPU tensors)
    assert fb.shape == (K, n, 2) and fb.dtype == torch.float32
    d = dev()
    wd = weight.to(d) if weight is not None else None
    gp, st = _native.hip().gbdt_gpair_softmax(margin.to(d), label.to(d), wd)
    gp2, st2 = _native.hip().gbdt_gpair_softmax(margin.to(d), label.to(d), wd)
    gp, st = gp.cpu(), st.cpu()
    assert gp.shape == (K, n, 2) and st.shape == (K, 4) and st.dtype == torch.float64
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(st).all())
    tol, e_fb = bound(fb, ref, weight, margin)
    err = (gp.double() - ref).abs()
    print("n=%d K=%d fallback max err %.3g, kernel max err %.3g" % (n, K, e_fb, float(err.max())))
    assert bool((err <= tol[None, :, None]).all()), (float(err.max()), e_fb)
    if wide:  # row 0: all K margins equal -> p = 1 / K
        assert torch.allclose(gp[:, 0, 1].double(), ref[:, 0, 1], rtol=1e-6, atol=0)
    # root statistics: fp64 sums of the kernel's own outputs, exact maxima
    own = gp.double()
    sums, mass = own.sum(1), own.abs().sum(1)
    assert bool(((st[:, 0:2] - sums).abs() <= 1e-12 * mass).all()), (st[:, 0:2], sums)
    assert torch.equal(st[:, 2:4], own.abs().amax(1))
    # the same bits on every run
    assert torch.equal(st, st2.cpu()) and torch.equal(gp, gp2.cpu())
    # what Objective.gpair hands a builder: class slices carrying their stats
    got = obj.gpair(margin.to(d), label.to(d), wd)
    gk = G.class_gpair(got, K - 1)
    assert gk.is_contiguous() and gk.shape == (n, 2)
    s2, m2 = G.gpair_stats(gk)
    assert torch.equal(s2.cpu(), st[K - 1, :2]) and torch.equal(m2.cpu(), st[K - 1, 2:].float())


def test_gpair_softmax_no_rows():
    from wormhole_amd import _native
    d = dev()
    gp, st = _native.hip().gbdt_gpair_softmax(torch.zeros(3, 0, device=d),
                                              torch.zeros(0, device=d), None)
    assert gp.shape == (3, 0, 2) and torch.equal(st.cpu(), torch.zeros(3, 4, dtype=torch.float64))
    ev = _native.hip().gbdt_multi_eval(torch.zeros(3, 0, device=d), torch.zeros(0, device=d), None)
    assert torch.equal(ev.cpu(), torch.zeros(3, dtype=torch.float64))
    assert _native.hip().gbdt_softmax_out(torch.zeros(3, 0, device=d), True).shape == (0, 3)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n,K", [(65, 3), (65, 33), (300_001, 3), (300_001, 33)])
def test_softmax_out_and_multi_eval(n, K, wide):
    from wormhole_amd import _native
    from wormhole_amd.models import gbdt as G
    margin, label, weight, p64 = inputs(n, K, True, wide)
    d = dev()
    md = margin.to(d)
    # class ids: the fp64 arg-max wherever the top two margins are > 1e-5 apart
    ids = _native.hip().gbdt_softmax_out(md, False).cpu()
    top2 = margin.double().topk(2, 0).values
    clear = (top2[0] - top2[1]) > 1e-5
    assert ids.shape == (n,) and bool((ids[clear] == first_argmax(margin.double())[clear].float()).all())
    if wide:  # row 0 is an exact K-way tie: the lowest class wins
        assert float(ids[0]) == 0.0
    # probabilities [n, K] row-major, the fallback's tolerance rule (w = 1)
    prob = _native.hip().gbdt_softmax_out(md, True).cpu()
    fb = G.Objective("multi:softprob", K).pred(margin)
    assert prob.shape == fb.shape == (n, K)
    e_fb = float((fb.double() - p64.t()).abs().max())
    err = float((prob.double() - p64.t()).abs().max())
    print("n=%d K=%d softprob: fallback max err %.3g, kernel max err %.3g" % (n, K, e_fb, err))
    assert err <= max(4 * e_fb, 1e-6)
    assert torch.equal(G.Objective("multi:softmax", K).pred(md).cpu(), ids)
    # evaluation sums, one row labelled K (out of range): an error with the
    # clamped nll, never an index
    lab = label.clone()
    lab[n // 2] = float(K)
    ok = lab < K
    yi = torch.where(ok, lab, torch.zeros_like(lab)).long()
    py = p64.gather(0, yi[None, :])[0]
    nll = torch.where(ok, -torch.log(py.clamp(min=1e-16)), torch.full_like(py, NLL_MAX))
    wrong = torch.where(ok, (first_argmax(margin.double()) != yi).double(), torch.ones_like(py))
    w = weight.double()
    want = torch.stack([(w * wrong).sum(), (w * nll).sum(), w.sum()])
    got = _native.hip().gbdt_multi_eval(md, lab.to(d), weight.to(d)).cpu()
    got2 = _native.hip().gbdt_multi_eval(md, lab.to(d), weight.to(d)).cpu()
    print("eval sums", got.tolist(), "fp64", want.tolist())
    assert bool(((got - want).abs() <= 1e-6 * want.abs()).all()), (got, want)
    assert torch.equal(got, got2)
    # Objective.metrics: the same sums through the CPU formulas
    from wormhole_amd.parallel.bsp import BSP
    bsp = BSP(torch.device("cpu"))
    obj = G.Objective("multi:softmax", K)
    a = obj.metrics(["merror", "mlogloss"], margin, lab, weight, bsp)
    assert abs(a[0] - float(want[0] / want[2])) < 1e-9 and abs(a[1] - float(want[1] / want[2])) < 1e-6


# ------------------------------------------------------------- plumbing
def _quantile_classes(score, K):
    q = torch.quantile(score, torch.arange(1, K) / K)
    return torch.bucketize(score, q).float()


def _dense_rows():
    g = torch.Generator().manual_seed(3)
    n, f = 20000, 20
    X = torch.randn(n, f, generator=g)
    X[torch.rand(n, f, generator=g) < 0.1] = float("nan")
    X[:, 3] = torch.randint(0, 3, (n,), generator=g).float()
    Z = torch.nan_to_num(X)
    return X, _quantile_classes(Z[:, 0] + Z[:, 5] - 0.5 * Z[:, 7] * Z[:, 3], 3)


def _sparse_rows():
    """2 000 rows, 30 columns, ~1/3 of the cells stored, integer values."""
    g = torch.Generator().manual_seed(4)
    n, f = 2000, 30
    V = torch.randint(0, 6, (n, f), generator=g).float()
    keep = torch.rand(n, f, generator=g) < 0.35
    keep[:, 0] = True
    Z = V * keep
    y = _quantile_classes(Z[:, 0] + Z[:, 4] - Z[:, 9] + 0.01 * torch.rand(n, generator=g), 3)
    rows, cols = keep.nonzero(as_tuple=True)
    off = torch.zeros(n + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(keep.sum(1), 0)
    return cols.to(torch.int64), off, V[rows, cols], y, f


def _check_plumbing(make, p, sparse):
    """Round 0 through the app's loop (``boost_round``) on the GPU: class k's
    tree has the first 7 nodes of a tree built from the fp64-derived class-k
    pairs; after 3 rounds the log-loss is that of the CPU path to 1e-3
    (the criterion of test_gbdt_kernels_match_cpu for one output)."""
    from wormhole_amd.models import gbdt as G
    from wormhole_amd.parallel.bsp import BSP
    bsp = BSP(torch.device("cpu"))
    K = p.num_class
    obj = G.Objective(p.objective, K)
    loss = []
    for device, sparse in ((torch.device("cpu"), False), (dev(), sparse)):
        # (the CPU reference always takes the dense matrix: absent = missing)
        dm = make(device, sparse)
        booster = G.Booster(p, dm.ncol)
        margin = booster.predict_margin(dm)
        if device.type == "cpu":
            cuts = G.Cuts.build(dm, p.max_bin, bsp)
        builder = G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
        if device.type == "cuda":
            p64 = torch.softmax(margin.double().cpu(), 0)
            ref_pairs = gpair64(p64, dm.label.cpu(), None).float().to(device)
            other = G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
            scratch = margin.clone()  # (the reference trees' margins: not compared)
            want = [other.build(ref_pairs[k].contiguous(), scratch[k]) for k in range(K)]
        for r in range(3):
            new = G.boost_round(obj, builder, dm, margin)
            assert len(new) == K
            if device.type == "cuda" and r == 0:
                for k in range(K):
                    assert new[k].feat[:7] == want[k].feat[:7], k
                    assert new[k].cond[:7] == want[k].cond[:7], k
        loss.append(obj.metrics(["mlogloss"], margin, dm.label, None, bsp)[0])
    print("mlogloss cpu %.6f gpu %.6f" % tuple(loss))
    assert abs(loss[0] - loss[1]) < 1e-3 * loss[0], loss


def _param(depth):
    from wormhole_amd.models import gbdt as G
    p = G.GBDTParam()
    p.objective, p.num_class, p.max_depth, p.max_bin = "multi:softprob", 3, depth, 64
    return p


def test_dense_builder_per_class():
    from wormhole_amd.models import gbdt as G
    X, y = _dense_rows()

    def make(device, sparse):
        return G.DMatrix.from_dense(X, y, device)
    _check_plumbing(make, _param(6), False)


def test_csr_builder_per_class():
    from wormhole_amd.models import gbdt as G
    keys, off, val, y, f = _sparse_rows()

    def make(device, sparse):
        return G.make_dmatrix(keys, off, val, y, None, f, device, sparse=sparse)
    _check_plumbing(make, _param(4), True)


@pytest.mark.parametrize("rows", ["dsparse=0", "dsparse=1"])
def test_xgboost_app_multiclass_gpu(tmp_path, capsys, monkeypatch, rows):
    from wormhole_amd.apps.xgboost_app import main
    monkeypatch.chdir(tmp_path)
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    X, y = three_class_rows()
    write_libsvm(tmp_path / "train.libsvm", X, y)
    args = ["objective=multi:softmax", "num_class=3", "max_depth=3", "eta=0.5",
            "num_round=6", "eval_train=1", "eval_metric=merror", "eval_metric=mlogloss",
            "data=train.libsvm", rows]
    out = {}
    for name, device in (("gpu", "auto"), ("cpu", "cpu")):
        monkeypatch.setenv("WH_DEVICE", device)
        assert main(args + ["model_out=%s.model" % name]) == 0
        out[name] = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[")]
        assert main(["task=pred", "model_in=%s.model" % name, "test:data=train.libsvm",
                     "name_pred=%s.txt" % name, rows]) == 0
        assert main(["task=eval", "model_in=%s.model" % name,
                     "test:data=train.libsvm", rows]) == 0
        assert "test-merror:0.000000" in capsys.readouterr().out
    assert len(out["gpu"]) == 6 and re.search(r"train-merror:0\.000000\t", out["gpu"][-1])
    assert open(tmp_path / "gpu.txt").read() == open(tmp_path / "cpu.txt").read()
    assert len(open(tmp_path / "gpu.txt").read().split()) == 600
