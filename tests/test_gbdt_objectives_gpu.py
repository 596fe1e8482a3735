"""The objectives' gradient kernel and the one-launch metric kernel against
fp64 formulas, max_delta_step through the three growers and the CSR builder,
the per-objective plumbing and the app against its CPU run.

Element tolerance of the gradient kernel: with M the sum of the absolute
values of a formula's terms at fp64 (tests/_gbdt_objective_cases.py), the fp32
plain-torch path (the CPU path of ``Objective``) is measured against fp64 on
the same inputs as |err| / (w M); the kernel may be at most 4x as far off (its
expf, log1pf and divisions may round differently from torch's), with a floor of
1e-6 (tests/test_gbdt_objectives.py derives it). The bound comes from the
fallback, never from the kernel."""
import functools
import re

import pytest
import torch

import _gbdt_monotone_cases as M
import _gbdt_objective_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
# 300 001 rows pass the 1024 blocks x 256 threads of one grid-stride step, so
# the stride loop, a partial wave and the reduction over all blocks run
NS = (0, 1, 65, 300_001)


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _hip():
    from wormhole_amd import _native
    return _native.hip()


def _bsp():
    from wormhole_amd.parallel.bsp import BSP
    return BSP(CPU)


@functools.lru_cache(maxsize=8)
def inputs(name, n, weighted, lo=-6.0, hi=6.0):
    g = torch.Generator().manual_seed(100 * C.OBJECTIVES.index(name) + n % 991 + weighted)
    margin = torch.rand(n, generator=g) * (hi - lo) + lo
    label = C.labels(name, n, g)
    weight = torch.rand(n, generator=g) * 1.5 + 0.5 if weighted else None
    return margin, label, weight


def _on(t):
    return t.to(DEV) if t is not None else None


def _check_stats(gp, st, st2, gp2):
    """Root statistics: fp64 sums of the kernel's own outputs, exact maxima,
    the same bits on every run."""
    own = gp.double()
    sums, mass = own.sum(0), own.abs().sum(0)
    assert st.shape == (4,) and st.dtype == torch.float64
    assert bool(((st[:2] - sums).abs() <= 1e-12 * mass).all()), (st[:2], sums)
    if gp.shape[0]:
        assert torch.equal(st[2:], own.abs().amax(0))
    assert torch.equal(st, st2) and torch.equal(gp, gp2)


# ------------------------------------------------------ 1. gradient kernel
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", C.OBJECTIVES)
def test_gpair_kernel(name, n, weighted):
    G = _G()
    margin, label, weight = inputs(name, n, weighted)
    obj = G.Objective(name)
    # (the squared log error's clamp is an input like the margins: fp32 holds
    # -1 + 1e-6 as SLE_MIN32, 1.3 % further from -1, and the reference clamps
    # there too -- else that one constant, not the arithmetic, sets the bound)
    ref, scale = C.weighted64(name, margin, label, weight, sle_min=C.SLE_MIN32)
    fb = obj.gpair(margin, label, weight)  # the plain-torch fp32 path (CPU tensors)
    assert fb.shape == (n, 2) and fb.dtype == torch.float32
    kw = dict(objective=G.OBJ_IDS[name], max_delta_step=obj.max_delta_step)
    gp, st = _hip().gbdt_gpair_obj(_on(margin), _on(label), _on(weight), **kw)
    gp2, st2 = _hip().gbdt_gpair_obj(_on(margin), _on(label), _on(weight), **kw)
    gp, st = gp.cpu(), st.cpu()
    assert gp.shape == (n, 2) and gp.dtype == torch.float32
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(st).all())
    if n == 0:
        assert torch.equal(st, torch.zeros(4, dtype=torch.float64))
    else:
        e_fb = float(((fb.double() - ref).abs() / scale).max())
        e_k = float(((gp.double() - ref).abs() / scale).max())
        print("%s n=%d weighted=%d: |err| / (w M): fallback %.3g, kernel %.3g"
              % (name, n, weighted, e_fb, e_k))
        assert e_k <= max(4 * e_fb, 1e-6), (e_k, e_fb)
        if name == "binary:hinge":
            assert torch.equal(gp, ref.float()) and torch.equal(gp, fb)
            if n > 1:  # both kinds of row
                assert bool((gp[:, 1] == C.FLT_MIN).any()) and bool((gp[:, 1] != C.FLT_MIN).any())
    _check_stats(gp, st, st2.cpu(), gp2.cpu())
    # what Objective.gpair hands a builder: the pairs carrying their statistics
    got = obj.gpair(_on(margin), _on(label), _on(weight))
    assert torch.equal(got.cpu(), gp) and torch.equal(got._wh_stats.cpu(), st)
    s2, m2 = G.gpair_stats(got)
    assert torch.equal(s2.cpu(), st[:2]) and torch.equal(m2.cpu(), st[2:].float())


def test_gpair_kernel_scalars():
    """The scalars travel: another variance power, slope and step."""
    G = _G()
    for name, step, rho, delta in (("reg:tweedie", 0.0, 1.2, 1.0),
                                   ("reg:pseudohubererror", 0.0, 1.5, 2.5),
                                   ("count:poisson", 0.0, 1.5, 1.0)):
        margin, label, weight = inputs(name, 65, True)
        ref, scale = C.weighted64(name, margin, label, weight, d=step, rho=rho, delta=delta)
        fb = G.obj_gpair_torch(G.OBJ_IDS[name], margin, label, weight, step, rho, delta)
        gp, _ = _hip().gbdt_gpair_obj(_on(margin), _on(label), _on(weight),
                                      objective=G.OBJ_IDS[name], max_delta_step=step,
                                      tweedie_variance_power=rho, huber_slope=delta)
        e_fb = float(((fb.double() - ref).abs() / scale).max())
        e_k = float(((gp.cpu().double() - ref).abs() / scale).max())
        print("%s step %g rho %g delta %g: fallback %.3g, kernel %.3g"
              % (name, step, rho, delta, e_fb, e_k))
        assert e_k <= max(4 * e_fb, 1e-6)
        other, _ = C.weighted64(name, margin, label, weight)
        assert not torch.allclose(other, ref, rtol=1e-3, atol=0)  # the scalar matters
    with pytest.raises(RuntimeError, match="unknown objective id"):
        _hip().gbdt_gpair_obj(torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), None,
                              objective=7)


# ------------------------------------------------------ 2. scale_pos_weight
@pytest.mark.parametrize("n", [65, 300_001])
def test_scale_pos_weight_kernel(n):
    G = _G()
    margin, label, weight = inputs("binary:hinge", n, True)  # labels 0 | 1
    s = torch.where(label == 1, 3.0, 1.0)
    hip = _hip()
    for w, ws in ((None, s), (weight, weight * s)):
        a, sa = hip.gbdt_gpair_obj(_on(margin), _on(label), _on(w), objective=G.OBJ_LOGISTIC,
                                   scale_pos_weight=3.0)
        b, sb = hip.gbdt_gpair_obj(_on(margin), _on(label), _on(ws), objective=G.OBJ_LOGISTIC)
        assert torch.equal(a, b) and torch.equal(sa, sb)
        assert float(a[:, 1].sum()) > float(hip.gbdt_gpair(_on(margin), _on(label), _on(w),
                                                           True)[0][:, 1].sum())
    # through the objective: s != 1 takes this kernel, s = 1 the existing entry point
    p = G.GBDTParam()
    p.objective, p.scale_pos_weight = "binary:logistic", 3.0
    got = G.Objective(p.objective, 0, p).gpair(_on(margin), _on(label), None)
    want, _ = hip.gbdt_gpair_obj(_on(margin), _on(label), None, objective=G.OBJ_LOGISTIC,
                                 scale_pos_weight=3.0)
    assert torch.equal(got, want)
    plain = G.Objective("binary:logistic").gpair(_on(margin), _on(label), _on(weight))
    assert torch.equal(plain, hip.gbdt_gpair(_on(margin), _on(label), _on(weight), True)[0])


# -------------------------------------------------------- 3. metric kernel
EVAL_CASES = [("count:poisson", C.METRICS, -6.0, 6.0),   # exp link, counts
              ("reg:gamma", C.METRICS, -6.0, 6.0),       # exp link, positive reals
              ("reg:squaredlogerror", ("mae", "mphe", "rmsle"), 0.0, 6.0)]  # the margin itself


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name,metrics,lo,hi", EVAL_CASES)
def test_obj_eval_kernel(name, metrics, lo, hi, n):
    G = _G()
    margin, label, weight = inputs(name, n, True, lo, hi)
    obj = G.Objective(name)
    slots = [G.parse_obj_metric(m)[0] for m in metrics]
    mask = sum(1 << s for s in slots)
    p64 = torch.exp(margin.double()) if obj.link == 1 else margin.double()
    args = (_on(margin), _on(label), _on(weight), obj.link, mask)
    got = _hip().gbdt_obj_eval(*args).cpu()
    got2 = _hip().gbdt_obj_eval(*args).cpu()
    assert got.shape == (8,) and got.dtype == torch.float64 and torch.equal(got, got2)
    for m, s in zip(metrics, slots):
        _, want, mass = C.metric64(m, p64, label, weight)
        print("%s n=%d %s: kernel %.17g fp64 %.17g" % (name, n, m, float(got[s]), want))
        assert abs(float(got[s]) - want) <= 1e-9 * mass, (m, float(got[s]), want)
    sw = float(weight.double().sum())
    assert abs(float(got[7]) - sw) <= 1e-9 * sw
    for s in set(range(7)) - set(slots):
        assert float(got[s]) == 0.0  # not asked for: not evaluated
    # Objective.metrics on GPU tensors: the CPU path's values
    bsp = _bsp()
    cpu = obj.metrics(list(metrics), margin, label, weight, bsp)
    gpu = obj.metrics(list(metrics), _on(margin), _on(label), _on(weight), bsp)
    for m, a, b in zip(metrics, cpu, gpu):
        assert abs(a - b) <= 1e-9 * max(1.0, abs(a)), (m, a, b)
        assert abs(a - C.metric64(m, p64, label, weight)[0]) <= 1e-9 * max(1.0, abs(a))


def test_obj_eval_links_and_scalars():
    """Sigmoid and step links, an unweighted set, another power and slope."""
    G = _G()
    margin, label, _ = inputs("binary:hinge", 65, False)
    m64 = margin.double()
    for link, p64 in ((2, torch.sigmoid(m64)), (3, (m64 > 0).double())):
        got = _hip().gbdt_obj_eval(_on(margin), _on(label), None, link, 1 << 4 | 1 << 5,
                                   huber_slope=2.0).cpu()
        for slot, name in ((4, "mae"), (5, "mphe")):
            _, want, mass = C.metric64(name, p64, label, None, delta=2.0)
            assert abs(float(got[slot]) - want) <= 1e-9 * max(mass, 1e-300)
        assert float(got[7]) == 65.0
    margin, label, weight = inputs("reg:tweedie", 65, True)
    got = _hip().gbdt_obj_eval(_on(margin), _on(label), _on(weight), 1, 1 << 3,
                               tweedie_variance_power=1.2).cpu()
    _, want, mass = C.metric64("tweedie-nloglik@1.2", torch.exp(margin.double()), label, weight,
                               rho=1.2)
    assert abs(float(got[3]) - want) <= 1e-9 * mass


# ------------------------------------------ 4. growers under max_delta_step
GN, GF, GDEPTH, GTREES = 20000, 12, 6, 3
ETA = 0.5  # (the monotone cases' parameter set)


@functools.lru_cache(maxsize=None)
def _gpu_inputs(sparse=False):
    G = _G()
    X, y = C.outlier_data(GN, GF)
    dm = M.dmatrix(G, X, y, DEV, sparse)
    cuts = G.Cuts.build(dm, 64, _bsp())
    return dm, cuts, cuts.bin(dm)


def _grow(monkeypatch, grower, gamma, colsample, step, mono=None, defer=True, sparse=False):
    """(trees, margins) of GTREES trees by the device level loop ("dev"), the
    per-level host grower ("host") or the Python level loop ("py"), all from
    the same gradient pairs. step: max_delta_step, None for its absence."""
    G = _G()
    dm, cuts, B = _gpu_inputs(sparse)
    monkeypatch.setattr(G, "HOST_GROWER", grower == "host")
    monkeypatch.setattr(G, "DEFER_TREES", defer)
    p = M.param(G, mono, max_depth=GDEPTH, gamma=gamma, colsample_bytree=colsample)
    assert p.eta == ETA
    if step is not None:
        assert p.set("max_delta_step", str(step))
    obj = G.Objective(p.objective, 0, p)
    tb = G.make_builder(p, _bsp(), dm, cuts, B)
    margin = torch.full((dm.n,), 0.5, device=DEV)
    gen = torch.Generator().manual_seed(5)
    trees = []
    for _ in range(GTREES):
        tb.sample_features(gen)
        gp = obj.gpair(margin, dm.label, None)
        trees.append(tb._build_py(gp, margin) if grower == "py" or sparse
                     else tb._build_native(gp, margin))
    for t in trees:
        t.feat  # (a deferred device tree builds its lists)
    return trees, margin.cpu()


def _dumps(trees):
    return [t.dump(None, True) for t in trees]


@pytest.mark.parametrize("gamma,colsample", [(0.0, 1.0), (2.0, 0.6)])
def test_growers_agree_under_max_delta_step(gamma, colsample, monkeypatch):
    dev, mdev = _grow(monkeypatch, "dev", gamma, colsample, C.STEP)
    host, mhost = _grow(monkeypatch, "host", gamma, colsample, C.STEP)
    py, mpy = _grow(monkeypatch, "py", gamma, colsample, C.STEP)
    assert sum(len(t.feat) for t in dev) > 3 * 7  # real trees, not stumps
    for a, b in zip(dev, host):
        C.same_structure(a, b)
        assert all(abs(x - z) < 1e-9 for x, z in zip(a.leaf, b.leaf))
        assert all(abs(x - z) < 1e-6 * max(1.0, abs(z)) for x, z in zip(a.gain, b.gain))
    assert torch.equal(mdev, mhost)
    for a, b in zip(host, py):
        C.same_structure(a, b)
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))
    assert torch.allclose(mhost, mpy, atol=1e-6)
    for trees in (dev, host, py):
        assert C.leaves_bounded(trees, ETA * C.STEP), C.largest_leaf(trees)
    assert C.largest_leaf(dev) == ETA * C.STEP  # the bound is met: it bites
    # the control: left alone, the same growers pass the bound
    free, _ = _grow(monkeypatch, "dev", gamma, colsample, None)
    assert not C.leaves_bounded(free, ETA * C.STEP), C.largest_leaf(free)
    # 0 is off: the parameter's absence, dump for dump
    zero, _ = _grow(monkeypatch, "dev", gamma, colsample, 0)
    assert _dumps(zero) == _dumps(free)
    hzero, _ = _grow(monkeypatch, "host", gamma, colsample, 0)
    hfree, _ = _grow(monkeypatch, "host", gamma, colsample, None)
    assert _dumps(hzero) == _dumps(hfree)


def test_deferred_trees_under_max_delta_step(monkeypatch):
    """gamma = 0 with DEFER_TREES: the margins come from the heap walk of the
    device node table (clamped leaf values), the host lists one tree later."""
    calls = []
    hip = _hip()
    monkeypatch.setattr(hip, "gbdt_walk_heap",
                        lambda *a, _f=hip.gbdt_walk_heap, **k: (calls.append(1), _f(*a, **k))[1])
    deferred, md = _grow(monkeypatch, "dev", 0.0, 1.0, C.STEP, defer=True)
    assert len(calls) == GTREES  # the deferred path ran
    direct, mn = _grow(monkeypatch, "dev", 0.0, 1.0, C.STEP, defer=False)
    assert len(calls) == GTREES
    for a, c in zip(deferred, direct):
        C.same_structure(a, c)
        assert a.leaf == c.leaf and a.gain == c.gain and a.cover == c.cover
    assert torch.equal(md, mn)
    assert C.leaves_bounded(deferred, ETA * C.STEP)


def test_max_delta_step_with_monotone_on_the_device(monkeypatch):
    """The children's intervals are cut inside [-d, d]."""
    mono = M.cycled(GF)
    dev, _ = _grow(monkeypatch, "dev", 0.0, 1.0, C.STEP, mono=mono)
    py, _ = _grow(monkeypatch, "py", 0.0, 1.0, C.STEP, mono=mono)
    for a, b in zip(dev, py):
        C.same_structure(a, b)
    assert C.leaves_bounded(dev, ETA * C.STEP) and M.holds(dev, mono)


def test_csr_builder_under_max_delta_step(monkeypatch):
    csr, mcsr = _grow(monkeypatch, "py", 0.0, 1.0, C.STEP, sparse=True)
    py, mpy = _grow(monkeypatch, "py", 0.0, 1.0, C.STEP)
    for a, b in zip(csr, py):
        C.same_structure(a, b)
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))
    assert torch.allclose(mcsr, mpy, atol=1e-6)
    assert C.leaves_bounded(csr, ETA * C.STEP) and C.largest_leaf(csr) == ETA * C.STEP
    free, _ = _grow(monkeypatch, "py", 0.0, 1.0, None, sparse=True)
    assert not C.leaves_bounded(free, ETA * C.STEP)
    zero, _ = _grow(monkeypatch, "py", 0.0, 1.0, 0, sparse=True)
    assert _dumps(zero) == _dumps(free)


# ------------------------------------------------------------- 5. plumbing
def _count_rows(n, f, slope=0.8):
    X, t = M.data(n, f)
    g = torch.Generator().manual_seed(9)
    return X, torch.poisson(torch.exp(slope * t.clamp(-2, 2)), generator=g)


@pytest.mark.parametrize("name", ["count:poisson", "reg:tweedie"])
def test_objective_plumbing(name):
    """Round 0 through the app's loop (``boost_round``) on the GPU: the tree
    has the first 7 nodes of a tree built from the fp64-derived pairs; after
    3 rounds the default metric is that of the CPU path to 1e-3 (the
    criterion of test_gbdt_multiclass_gpu._check_plumbing)."""
    G = _G()
    bsp = _bsp()
    X, y = _count_rows(4000, 8)
    p = G.GBDTParam()
    p.objective, p.max_depth, p.max_bin = name, 4, 64
    loss = []
    for device in (CPU, DEV):
        dm = G.DMatrix.from_dense(X, y, device)
        booster = G.Booster(p, dm.ncol)
        obj = booster.obj
        margin = booster.predict_margin(dm)
        if device.type == "cpu":
            cuts = G.Cuts.build(dm, p.max_bin, bsp)
        builder = G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
        if device.type == "cuda":
            ref_pairs = C.weighted64(name, margin.cpu(), y, None, d=obj.max_delta_step)[0]
            other = G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
            want = other.build(ref_pairs.float().to(device).contiguous(), margin.clone())
        for r in range(3):
            (new,) = G.boost_round(obj, builder, dm, margin)
            if device.type == "cuda" and r == 0:
                assert len(new.feat) >= 7
                assert new.feat[:7] == want.feat[:7] and new.cond[:7] == want.cond[:7]
        loss.append(obj.metrics([obj.default_metric()], margin, dm.label, None, bsp)[0])
    print("%s %s cpu %.6f gpu %.6f" % (name, obj.default_metric(), loss[0], loss[1]))
    assert abs(loss[0] - loss[1]) < 1e-3 * abs(loss[0]), loss


# -------------------------------------------------------------- 6. the app
@pytest.mark.parametrize("rows", ["dsparse=0", "dsparse=1"])
def test_app_poisson_gpu_matches_cpu(tmp_path, capsys, monkeypatch, rows):
    """The prediction files agree to 1e-4 relative, that is, the margins to
    1e-4 absolute. What separates the two runs' leaves is the GPU histograms'
    fixed point: a row's g is rounded to q <= 2 x 8192 x max|g| / 2^30 (the
    int32 LDS passes), a sum of n rows is off by about q sqrt(n / 12), and a
    sibling derived by subtraction inherits the error of the child that was
    built. Counts of mean <= e^0.8 keep max|g| below 10 (q < 1.6e-4, three
    deviations of 2000 rows: 6e-3), and min_child_weight = 100 keeps every
    leaf's H + lambda above 100: a leaf moves by less than eta x 6e-3 / 100 =
    2e-5 per tree, 6e-5 over the three."""
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    monkeypatch.chdir(tmp_path)
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    X, y = _count_rows(2000, 4, slope=0.4)
    assert float(y.max()) < 10
    C.write_libsvm(tmp_path / "train.libsvm", X, y)
    args = ["data=train.libsvm", "objective=count:poisson", "max_depth=4", "max_bin=64",
            "min_child_weight=100", "num_round=3", "eval_train=1", rows]
    val, model, pred = {}, {}, {}
    for name, device in (("gpu", "auto"), ("cpu", "cpu")):
        monkeypatch.setenv("WH_DEVICE", device)
        assert main(args + ["model_out=%s.model" % name]) == 0
        out = capsys.readouterr().out
        assert "unknown parameter" not in out
        val[name] = [float(v) for v in re.findall(r"train-poisson-nloglik:([0-9.]+)", out)]
        assert len(val[name]) == 3
        model[name] = G.Booster.load("%s.model" % name, G.GBDTParam())
        assert main(["task=pred", "model_in=%s.model" % name, "test:data=train.libsvm",
                     "name_pred=%s.txt" % name, rows]) == 0
        pred[name] = [float(v) for v in open("%s.txt" % name).read().split()]
    for a, b in zip(model["gpu"].trees, model["cpu"].trees):
        C.same_structure(a, b)
    assert len(model["gpu"].trees) == 3 and all(len(t.feat) >= 7 for t in model["gpu"].trees)
    for a, b in zip(val["gpu"], val["cpu"]):
        assert abs(a - b) <= 1e-3 * abs(b), (val["gpu"], val["cpu"])
    assert len(pred["gpu"]) == len(pred["cpu"]) == 2000
    assert all(abs(a - b) <= 1e-4 * abs(b) for a, b in zip(pred["gpu"], pred["cpu"]))
    for b in model.values():
        assert C.leaves_bounded(b.trees, 0.3 * 0.7), C.largest_leaf(b.trees)
