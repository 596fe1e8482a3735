"""reg:absoluteerror and reg:quantileerror on the GPU: the radix select against
``leaf_quantiles_ref`` bit for bit (one rank and two emulated ones), the
gradient kernel and the ``quantile`` evaluation against their torch forms,
training against the CPU path through every grower, the app, and the unchanged
bytes of a reg:squarederror model."""
import functools
import os
import re

import pytest
import torch

import _gbdt_objective_cases as C
import _gbdt_quantile_cases as Q

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
CHUNKS = (64, 1 << 14)  # a segment spans 1, 2 and many chunks
NS = (0, 1, 65, 300_001)  # (the gradient kernel's sizes of test_gbdt_objectives_gpu)


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _hip():
    from wormhole_amd import _native
    return _native.hip()


def _bsp():
    from wormhole_amd.parallel.bsp import BSP
    return BSP(CPU)


def _on(t):
    return t.to(DEV) if t is not None else None


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------ 1. the select
def _reference(case, alpha, keep=None):
    G = _G()
    ridx, segs, label, at, w = case
    rows = ridx.long()
    r = (label - at)[rows]
    scale = G.weight_scale(w, keep, _bsp()) if w is not None else None
    u = G.round_weights(w[rows] if w is not None else None,
                        keep[rows] if keep is not None else None, scale, rows.numel(), CPU)
    return G.leaf_quantiles_ref(r, u, segs, alpha)


def _select(case, alpha, chunk, keep=None):
    ridx, segs, label, at, w = case
    return _G().leaf_quantiles(_on(ridx), segs, _on(label), _on(at), _on(w), _on(keep), alpha,
                               _bsp(), chunk=chunk)


def _same(got, want):
    (q, empty), (wq, wempty) = got, want
    assert torch.equal(empty, wempty)
    assert torch.equal(_bits(q)[~empty], _bits(wq)[~wempty]), (q[~empty], wq[~wempty])


@pytest.mark.parametrize("L", [1, 2, 256, 1500])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_select_against_the_reference(n, L):
    """Rows x leaves (uneven segments, empty ones included; 1500 leaves: the
    per-level host grower's range) x chunk sizes x weights, ridx a permutation."""
    for wi, weights in enumerate(("none", "int", "zeros", "frac")):
        case = Q.select_case(n, L, 1000 * n + 10 * L + wi, weights)
        for alpha in (0.5, 0.125):
            want = _reference(case, alpha)
            for chunk in CHUNKS:
                _same(_select(case, alpha, chunk), want)


@pytest.mark.parametrize("keys", ["top", "bottom", "boundary", "equal", "zeros"])
def test_select_key_patterns(keys):
    """Keys that differ only in the top byte, only in the bottom byte,
    duplicates across a digit boundary, all equal, +-0.0 and denormals."""
    case = Q.select_case(1000, 6, 77, "int", keys)
    for alpha in (0.5, 0.25, 0.75):
        want = _reference(case, alpha)
        for chunk in CHUNKS:
            _same(_select(case, alpha, chunk), want)
    if keys == "zeros":
        q, empty = _select(case, 0.5, 64)
        assert bool(((_bits(q) != -2 ** 31) | empty).all())  # never -0.0


def test_select_keep_mask_and_lower_median():
    case = Q.select_case(1000, 5, 3, "int")
    keep = torch.rand(1000, generator=torch.Generator().manual_seed(9)) < 0.5
    _same(_select(case, 0.75, 64, keep), _reference(case, 0.75, keep))
    # an even unweighted count at alpha = 0.5: the lower median
    ridx = torch.arange(4, dtype=torch.int32)
    q, _ = _select((ridx, [(0, 4)], torch.tensor([4.0, 1.0, 3.0, 2.0]), torch.zeros(4), None), 0.5,
                   64)
    assert float(q[0]) == 2.0


@pytest.mark.parametrize("weights", ["int", "frac"])
def test_select_two_emulated_ranks(weights):
    """Rows split in two, gbdt_qsel_hist on each half, histograms added, one
    pick: the single-rank state after every one of the four passes."""
    G, hip = _G(), _hip()
    n, L, alpha = 1000, 7, 0.25
    ridx, segs, label, at, w = Q.select_case(n, L, 21, weights)
    scale = _on(G.weight_scale(w, None, _bsp()))
    halves = []
    for par in (0, 1):  # rank `par` holds every second position of every segment
        pos = torch.cat([torch.arange(b + par, e, 2) for b, e in segs if e - b > par])
        cnt = [len(range(b + par, e, 2)) if e - b > par else 0 for b, e in segs]
        off = [0]
        for c in cnt:
            off.append(off[-1] + c)
        halves.append((ridx[pos], list(zip(off[:-1], off[1:]))))
    whole = [(ridx, segs)] + halves
    keys = []
    for rx, sg in whole:
        keys.append(hip.gbdt_qsel_key(ridx=_on(rx), label=_on(label), at=_on(at), weight=_on(w),
                                      keep=None, scale=scale))
    one = torch.zeros(L, 2, dtype=torch.int64, device=DEV)
    two = torch.zeros(L, 2, dtype=torch.int64, device=DEV)
    for p in range(4):
        h = [hip.gbdt_qsel_hist(key=k, u=u, seg_beg=[b for b, _ in sg], seg_end=[e for _, e in sg],
                                chunk=64, state=one if i == 0 else two, radix_pass=p)
             for i, ((k, u), (_, sg)) in enumerate(zip(keys, whole))]
        assert torch.equal(h[0], h[1] + h[2])
        hip.gbdt_qsel_pick(hist=h[0], state=one, radix_pass=p, alpha=alpha)
        hip.gbdt_qsel_pick(hist=h[1] + h[2], state=two, radix_pass=p, alpha=alpha)
        assert torch.equal(one, two), p
    out = hip.gbdt_qsel_value(state=two).cpu()
    _same((out[0], out[1] != 0), _reference((ridx, segs, label, at, w), alpha))


# ------------------------------------------- 2. gradients and the metric
def _inputs(n, weighted, K, seed):
    g = torch.Generator().manual_seed(seed + n % 991)
    label = torch.randn(n, generator=g)
    margin = torch.randn(K, n, generator=g)
    if n > 8:
        margin[:, :8] = label[:8]  # d = 0
    weight = torch.rand(n, generator=g) * 1.5 + 0.5 if weighted else None
    return margin, label, weight


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["reg:absoluteerror", "reg:quantileerror"])
def test_gpair_kernel(name, n, weighted):
    """As test_gbdt_objectives_gpu.test_gpair_kernel: against fp64 relative
    to w, at most 4x as far off as the fp32 torch form (floor 1e-6); the
    root statistics are sums of the kernel's own outputs."""
    G = _G()
    alphas = [0.5] if name == "reg:absoluteerror" else [0.1, 0.5, 0.9]
    K = len(alphas)
    margin, label, weight = _inputs(n, weighted, K, 5)
    p = G.GBDTParam()
    p.set("quantile_alpha", str(alphas))
    obj = G.make_objective(name, 0, p)
    m = margin if K > 1 else margin[0]
    fb = obj.gpair(m, label, weight)  # the fp32 torch path (CPU tensors)
    got = obj.gpair(_on(m), _on(label), _on(weight))
    got2 = obj.gpair(_on(m), _on(label), _on(weight))
    assert got.shape == fb.shape and got.dtype == torch.float32
    st = got._wh_stats.cpu().reshape(K, 4)
    assert torch.equal(got, got2) and torch.equal(got._wh_stats, got2._wh_stats)
    for k, a in enumerate(alphas):
        gk, fk = got.reshape(K, n, 2)[k].cpu(), fb.reshape(K, n, 2)[k]
        ref = Q.gpair64(a, margin[k], label, weight, absolute=name == "reg:absoluteerror")
        if n:
            scale = (weight.double() if weighted else torch.ones(n, dtype=torch.float64))[:, None]
            e_fb = float(((fk.double() - ref).abs() / scale).max())
            e_k = float(((gk.double() - ref).abs() / scale).max())
            print("%s n=%d alpha=%g: |err| / w: fallback %.3g, kernel %.3g" % (name, n, a, e_fb, e_k))
            assert e_k <= max(4 * e_fb, 1e-6), (e_k, e_fb)
            assert torch.equal(gk, fk)  # the same fp32 operations
            own = gk.double()
            assert bool(((st[k, :2] - own.sum(0)).abs() <= 1e-12 * own.abs().sum(0)).all())
            assert torch.equal(st[k, 2:], own.abs().amax(0))
        else:
            assert torch.equal(st[k], torch.zeros(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="quantile_alpha"):
        _hip().gbdt_gpair_obj(torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), None,
                              objective=G.OBJ_QUANTILE, quantile_alpha=1.0)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", NS)
def test_quantile_eval_kernel(n, K):
    G = _G()
    alphas = [0.25] if K == 1 else [0.1, 0.5, 0.9]
    margin, label, weight = _inputs(n, True, K, 11)
    m = margin if K > 1 else margin[0]
    got = G.pinball_sums(alphas, _on(m), _on(label), _on(weight)).cpu()
    got2 = G.pinball_sums(alphas, _on(m), _on(label), _on(weight)).cpu()
    want = G.pinball_sums(alphas, m, label, weight)  # torch on margin.double()
    assert got.shape == (2,) and got.dtype == torch.float64 and torch.equal(got, got2)
    mass = max(float(want[0]), 1e-300)  # (every term is >= 0)
    print("n=%d K=%d kernel %.17g torch %.17g" % (n, K, float(got[0]), float(want[0])))
    assert abs(float(got[0]) - float(want[0])) <= 1e-9 * mass
    assert abs(float(got[1]) - float(want[1])) <= 1e-9 * max(float(want[1]), 1e-300)
    if n:
        p = G.GBDTParam()
        p.set("quantile_alpha", str(alphas))
        obj = G.make_objective("reg:quantileerror", 0, p)
        (v,) = obj.metrics(["quantile"], _on(m), _on(label), _on(weight), _bsp())
        assert abs(v - Q.pinball64(alphas, m, label, weight)) <= 1e-9 * max(1.0, v)


# ------------------------------------------------------------- 3. training
ROUNDS = 3


@functools.lru_cache(maxsize=None)
def _cpu_model(depth, K, booster):
    """The CPU path's model (dense rows), trained once per parameter set."""
    G = _G()
    X, y, w = Q.train_data()
    return Q.train(G, _bsp(), Q.dmatrix(G, X, y, w, CPU), _param(depth, K, booster), ROUNDS)[0]


def _param(depth, K, booster):
    G = _G()
    extra = dict(booster=booster, rate_drop=0.5, seed=2) if booster == "dart" else {}
    if K == 1:
        return Q.param(G, "reg:absoluteerror", max_depth=depth, eta=0.5, **extra)
    return Q.param(G, "reg:quantileerror", quantile_alpha="[0.125,0.5,0.75]", max_depth=depth,
                   eta=0.5, **extra)


@pytest.mark.parametrize("sparse,depth,K,booster", [
    (False, 6, 1, "gbtree"), (False, 6, 3, "dart"), (False, 11, 3, "gbtree"),
    (False, 11, 1, "dart"), (True, 6, 3, "gbtree"), (True, 6, 1, "dart"),
    (True, 11, 1, "gbtree")])
def test_training_matches_the_cpu_path(sparse, depth, K, booster):
    """Dyadic alphas, integer weights: the same structure and leaves as the
    CPU path (compared as test_gbdt_objectives_gpu compares a GPU model with
    a CPU one); depth 6: the device level loop, depth 11: the per-level host
    grower; sparse: the CSR builder."""
    G = _G()
    X, y, w = Q.train_data()
    want = _cpu_model(depth, K, booster)
    dm = Q.dmatrix(G, X, y, w, DEV, sparse)
    got, margin = Q.train(G, _bsp(), dm, _param(depth, K, booster), ROUNDS)
    assert len(got.trees) == len(want.trees) == ROUNDS * K
    assert sum(len(t.feat) for t in got.trees) > 3 * 7 * K
    for a, b in zip(got.trees, want.trees):
        C.same_structure(a, b)
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))
    assert got.weights() == want.weights()
    assert torch.allclose(margin.cpu(), got.predict_margin(dm).cpu(), atol=1e-6)


def test_training_margins_equal_the_saved_model(tmp_path):
    G = _G()
    X, y, w = Q.train_data()
    dm = Q.dmatrix(G, X, y, w, DEV)
    p = Q.param(G, "reg:quantileerror", quantile_alpha="[0.25,0.75]", max_depth=6, eta=0.5,
                subsample=0.8, colsample_bytree=0.75, gamma=0.05,
                interaction_constraints="[[0,1,2],[2,3]]")
    b, margin = Q.train(G, _bsp(), dm, p, 5)
    path = str(tmp_path / "q.model")
    b.save(path)
    loaded = G.Booster.load(path, G.GBDTParam())
    assert loaded.obj.n_group == 2 and len(loaded.trees) == 10
    # (the tolerance of test_gbdt_monotone_gpu's margins against predict_margin)
    assert torch.allclose(margin.cpu(), loaded.predict_margin(dm).cpu(), atol=1e-6)


def test_app_absolute_error_on_the_gpu(tmp_path, capsys, monkeypatch):
    from wormhole_amd.apps.xgboost_app import main
    monkeypatch.chdir(tmp_path)
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WH_DEVICE", "auto")
    X, y, w = Q.train_data()
    C.write_libsvm(tmp_path / "train.libsvm", X, y, w)
    assert main(["data=train.libsvm", "objective=reg:absoluteerror", "max_depth=4", "max_bin=64",
                 "num_round=10", "eval_train=1", "model_out=abs.model"]) == 0
    out = capsys.readouterr().out
    assert "unknown parameter" not in out
    mae = [float(v) for v in re.findall(r"train-mae:([0-9.]+)", out)]
    assert len(mae) == 10 and all(b < a for a, b in zip(mae, mae[1:])), mae
    assert len(_G().Booster.load("abs.model", _G().GBDTParam()).trees) == 10


# --------------------------------------------------- 4. unchanged behaviour
def test_squarederror_model_bytes_are_unchanged(tmp_path):
    got = Q.squarederror_model(_G(), _bsp(), DEV, str(tmp_path / "m.model"))
    assert got == open(os.path.join(Q.GOLDEN, "gbdt_squarederror_gpu.model"), "rb").read()
