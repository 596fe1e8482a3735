"""The survival kernels against the fp64 oracles of
tests/_gbdt_survival_cases.py and against the plain-torch CPU paths, and the
app against its CPU run.

Element tolerance, as tests/test_gbdt_objectives_gpu.py: with M the error
scale of the cases file, the CPU path is measured against fp64 as |err| / (w M)
and the kernel may be at most 4x as far off, with a floor of 1e-6. The Cox
and the AFT kernels keep fp64 inside like their CPU paths, so the derived
2^-22 w M holds for them too and is asserted beside the rule."""
import math
import re

import pytest
import torch

import _gbdt_survival_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")


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


def _tile():
    return int(_hip().gbdt_cox_tile())


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


def _cox_kernel(margin, label, weight):
    """(pairs, stats) of two kernel calls on one device plan, on the CPU."""
    G = _G()
    plan = G.CoxPlan(_on(label), _on(weight))
    kw = dict(margin=_on(margin), order=plan.order, delta=plan.delta, weight=plan.weight,
              run_events=plan.run_events, ws=plan.ws, ticket=plan.ticket)
    gp, st = _hip().gbdt_gpair_cox(**kw)
    gp2, st2 = _hip().gbdt_gpair_cox(**kw)
    # the device plan is the CPU one
    cpu = G.CoxPlan(label, weight)
    for k in ("order", "delta", "head", "tail", "run_events"):
        assert torch.equal(getattr(plan, k).cpu(), getattr(cpu, k)), k
    return gp.cpu(), st.cpu(), gp2.cpu(), st2.cpu()


def _cox_compare(margin, label, weight, what):
    G = _G()
    n = margin.numel()
    ref, scale, _, _ = C.cox_oracle(margin, label, weight)
    fb = G.cox_gpair_torch(margin, label, weight)
    gp, st, gp2, st2 = _cox_kernel(margin, label, weight)
    assert gp.shape == (n, 2) and gp.dtype == torch.float32
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(st).all())
    floor = scale.clamp(min=1e-300)
    e_fb = float(((fb.double() - ref).abs() / floor).max())
    e_k = float(((gp.double() - ref).abs() / floor).max())
    print("cox %s: |err| / (w M): fallback %.3g, kernel %.3g" % (what, e_fb, e_k))
    assert e_k <= max(4 * e_fb, 1e-6), (e_k, e_fb)
    assert bool(((gp.double() - ref).abs() <= C.COX_BOUND * scale).all())
    assert bool((gp[:, 1] >= 0).all())
    _check_stats(gp, st, st2, gp2)
    return gp, st


# --------------------------------------------------------------- 1. cox
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", ["1", "2", "T-1", "T", "T+1", "3T+5"])
def test_gpair_cox_kernel(case, weighted):
    G = _G()
    T = _tile()
    n = {"1": 1, "2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[case]
    margin, label, weight = C.cox_inputs(n, weighted)
    gp, st = _cox_compare(margin, label, weight, "n=%d weighted=%d" % (n, weighted))
    # what Objective.gpair hands a builder: the pairs carrying their statistics
    dm = G.DMatrix.from_dense(torch.zeros(n, 1), label, DEV)
    dm.weight = _on(weight)
    obj = G.Objective("survival:cox")
    got = obj.gpair(_on(margin), dm.label, dm.weight, data=dm)
    assert torch.equal(got.cpu(), gp) and torch.equal(got._wh_stats.cpu(), st)
    assert dm.cox_plan() is dm.cox_plan()  # built once per matrix
    s2, m2 = G.gpair_stats(got)
    assert torch.equal(s2.cpu(), st[:2]) and torch.equal(m2.cpu(), st[2:].float())
    # the sketch's call: no weights
    bare = obj.gpair(_on(margin), dm.label, None, data=dm)
    ref, scale, _, _ = C.cox_oracle(margin, label, None)
    assert bool(((bare.cpu().double() - ref).abs() <= C.COX_BOUND * scale).all())


def test_gpair_cox_edges():
    T = _tile()
    _cox_compare(*C.cox_inputs(T + 1, True, times=1), "all tied")
    _cox_compare(*C.cox_inputs(T + 1, True, events="all"), "all events")
    gp, st = _cox_compare(*C.cox_inputs(T + 1, True, events="none"), "no events")
    assert torch.equal(gp, torch.zeros_like(gp)) and torch.equal(st, torch.zeros_like(st))
    _cox_compare(*C.cox_inputs(2 * T + 3, False, times=0), "no ties")
    # a risk set whose every e underflowed: finite, as the CPU path
    G = _G()
    margin = torch.tensor([0.0, 1.0, -2000.0, -2000.0])
    label = torch.tensor([1.0, 2.0, 3.0, -4.0])
    gp = _cox_kernel(margin, label, None)[0]
    assert torch.equal(gp, G.cox_gpair_torch(margin, label, None))
    assert torch.allclose(G.cox_eval_sums(_on(margin), _on(label)).cpu(),
                          G.cox_eval_torch(margin, label), rtol=1e-12, atol=0)
    # shift invariance in the kernel: the same bits 64 higher
    g = torch.Generator().manual_seed(3)
    margin = torch.randint(-32, 33, (T + 9,), generator=g).float() / 8
    _, label, weight = C.cox_inputs(T + 9, True)
    a = _cox_kernel(margin, label, weight)[0]
    b = _cox_kernel(margin + 64, label, weight)[0]
    assert torch.equal(a, b)


def test_gpair_cox_ties_across_tiles():
    T = _tile()
    # positions T-3 .. T+3 share one time; the kernels count their tiles from
    # the last position (boundaries at n - T, n - 2 T, ...), so lay a run over
    # such a boundary as well
    n = 2 * T + 11
    _cox_compare(*C.cox_tie_inputs(n, [(T - 3, T + 3)]), "run over positions T-3..T+3")
    _cox_compare(*C.cox_tie_inputs(n, [(n - T - 3, n - T + 3)]), "run over the boundary n-T")
    # a run that spans three tiles (n = 3 T + 5: boundaries at 5, T + 5, 2 T + 5)
    _cox_compare(*C.cox_tie_inputs(3 * T + 5, [(T // 2, 2 * T + T // 2)]), "run over three tiles")
    _cox_compare(*C.cox_tie_inputs(2 * T, [(T - 3, T + 3), (3, 9)]), "n a multiple of the tile")


def test_cox_eval_kernel():
    G = _G()
    T = _tile()
    for n, events in ((1, "all"), (T + 1, "mixed"), (3 * T + 5, "mixed"), (T + 1, "none")):
        margin, label, weight = C.cox_inputs(n, False, events=events)
        _, _, L, E = C.cox_oracle(margin, label)
        plan = G.CoxPlan(_on(label))
        v = G.cox_eval_sums(_on(margin), _on(label), plan).cpu()
        v2 = G.cox_eval_sums(_on(margin), _on(label), plan).cpu()
        fb = G.cox_eval_torch(margin, label)
        print("cox-nloglik n=%d %s: kernel %r, fallback %r, oracle %r" % (
            n, events, v.tolist(), fb.tolist(), (L, E)))
        assert v.dtype == torch.float64 and torch.equal(v, v2) and int(v[1]) == E
        assert abs(float(v[0]) - L) <= 1e-10 * max(abs(L), 1.0)
        obj = G.Objective("survival:cox")
        dm = G.DMatrix.from_dense(torch.zeros(n, 1), label, DEV)
        got = obj.metrics(["cox-nloglik"], _on(margin), dm.label, None, _bsp(), data=dm)[0]
        if E:
            assert abs(got - L / E) <= 1e-10 * abs(L / E)
        else:
            assert math.isnan(got)


# --------------------------------------------------------------- 2. aft
@pytest.mark.parametrize("dist", C.DISTS)
def test_gpair_aft_kernel(dist):
    G = _G()
    d = C.DISTS.index(dist)
    for sigma in C.SIGMAS:
        for kind in C.KINDS:
            margin, lower, upper, weight = C.aft_inputs(dist, kind, sigma, weighted=True)
            ref, raw, loss = C.aft_oracle(dist, margin, lower, upper, sigma, weight)
            scale = C.aft_scale(dist, margin, lower, upper, sigma, raw, loss, weight)
            fb = G.aft_gpair_torch(margin, lower, upper, weight, d, sigma)
            args = (_on(margin), _on(lower), _on(upper), _on(weight))
            gp, st = _hip().gbdt_gpair_aft(*args, dist=d, sigma=sigma)
            gp2, st2 = _hip().gbdt_gpair_aft(*args, dist=d, sigma=sigma)
            gp, st = gp.cpu(), st.cpu()
            e_fb = float(C.aft_rel_err(fb, ref, scale).max())
            e_k = float(C.aft_rel_err(gp, ref, scale).max())
            print("aft %s %s sigma=%g: |err| / (w M): fallback %.3g, kernel %.3g"
                  % (dist, kind, sigma, e_fb, e_k))
            assert e_k <= max(4 * e_fb, 1e-6), (e_k, e_fb)
            # both paths are fp64 inside: the derived bound holds for the kernel too
            assert e_k <= C.AFT_BOUND, e_k
            _check_stats(gp, st, st2.cpu(), gp2.cpu())
    # more than one grid-stride step, a partial wave; through the objective
    n = 300_001
    g = torch.Generator().manual_seed(d)
    margin = torch.rand(n, generator=g) * 4 - 2
    lower = torch.exp(torch.rand(n, generator=g) * 2 - 1)
    upper = torch.where(torch.rand(n, generator=g) < 0.5, lower, lower * 2)
    prm = G.GBDTParam()
    prm.set("aft_loss_distribution", dist)
    obj = G.make_objective("survival:aft", 0, prm)
    dm = G.DMatrix.from_dense(torch.zeros(n, 1), torch.zeros(n), DEV)
    dm.set_bounds(lower, upper)
    got = obj.gpair(_on(margin), dm.label, None, data=dm)
    fb = G.aft_gpair_torch(margin, lower, upper, None, d, 1.0)
    assert float((got.cpu() - fb).abs().max()) <= 1e-5
    _check_stats(got.cpu(), got._wh_stats.cpu(), got._wh_stats.cpu(), got.cpu())


@pytest.mark.parametrize("dist", C.DISTS)
def test_aft_tails_kernel(dist):
    margin, lower, upper = C.aft_tail_inputs()
    ref, _, _ = C.aft_oracle(dist, margin, lower, upper, 1.0)
    got, _ = _hip().gbdt_gpair_aft(_on(margin), _on(lower), _on(upper), None,
                                   dist=C.DISTS.index(dist), sigma=1.0)
    got = got.cpu()
    assert bool(torch.isfinite(got).all())
    assert bool(((got[:, 0] >= C.MIN_G) & (got[:, 0] <= C.MAX_G)).all())
    assert bool(((got[:, 1] >= torch.tensor(C.MIN_H).float()) & (got[:, 1] <= C.MAX_H)).all())
    for col, values in ((0, (C.MIN_G, C.MAX_G)), (1, (C.MIN_H, C.MAX_H))):
        for v in values:
            at = ref[:, col] == v
            assert bool((got[at, col] == torch.tensor(v).float()).all()), (dist, col, v)


@pytest.mark.parametrize("dist", C.DISTS)
def test_aft_eval_kernel(dist):
    G = _G()
    d, sigma = C.DISTS.index(dist), 2.0
    parts = [C.aft_inputs(dist, kind, sigma, weighted=True) for kind in C.KINDS]
    margin, lower, upper, weight = (torch.cat([p[i] for p in parts]) for i in range(4))
    _, _, loss = C.aft_oracle(dist, margin, lower, upper, sigma)
    want = float((weight.double() * loss.clamp(max=-math.log(1e-12))).sum())
    fb = G.aft_eval_torch(margin, lower, upper, weight, d, sigma)
    v = _hip().gbdt_aft_eval(_on(margin), _on(lower), _on(upper), _on(weight), dist=d,
                             sigma=sigma).cpu()
    v2 = _hip().gbdt_aft_eval(_on(margin), _on(lower), _on(upper), _on(weight), dist=d,
                              sigma=sigma).cpu()
    e_fb, e_k = abs(float(fb[0]) - want) / want, abs(float(v[0]) - want) / want
    print("aft-nloglik %s: relative error: fallback %.3g, kernel %.3g" % (dist, e_fb, e_k))
    assert torch.equal(v, v2) and e_k <= max(4 * e_fb, 1e-6)
    assert abs(float(v[1] - fb[1])) <= 1e-12 * float(fb[1]) and torch.equal(v[2:], fb[2:])


# --------------------------------------------------------------- 3. the app
def _write_bounds(base, lower, upper):
    for suffix, v in ((".label_lower_bound", lower), (".label_upper_bound", upper)):
        with open(str(base) + suffix, "w") as f:
            f.write("".join("%s\n" % ("inf" if math.isinf(x) else repr(x)) for x in v.tolist()))


@pytest.mark.parametrize("objective", ["survival:cox", "survival:aft"])
def test_app_gpu_matches_cpu(tmp_path, capsys, monkeypatch, objective):
    """As test_app_poisson_gpu_matches_cpu compares its two runs: the same
    tree structures, the metric to 1e-3 relative, the predictions to 1e-4
    relative. What separates the runs' leaves is the GPU histograms' fixed
    point; min_child_weight keeps every leaf's H + lambda above 10 at these
    400 rows (|g| <= 15 by the clamps, about 1 for survival:cox here)."""
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    monkeypatch.chdir(tmp_path)
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    X, t, event = C.survival_rows()
    t = t.clamp(min=0.125)
    C.write_libsvm(tmp_path / "train.libsvm", X, torch.where(event, t, -t))
    _write_bounds(tmp_path / "train.libsvm", t,
                  torch.where(event, t, torch.full_like(t, float("inf"))))
    metric = "cox-nloglik" if objective == "survival:cox" else "aft-nloglik"
    args = ["data=train.libsvm", "objective=" + objective, "max_depth=3", "max_bin=32",
            "min_child_weight=10", "num_round=10", "eval_train=1"]
    val, model, pred = {}, {}, {}
    for name, device in (("gpu", "auto"), ("cpu", "cpu")):
        monkeypatch.setenv("WH_DEVICE", device)
        assert main(args + ["model_out=%s.model" % name]) == 0
        out = capsys.readouterr().out
        assert "unknown parameter" not in out
        val[name] = [float(v) for v in re.findall(r"train-%s:([0-9.]+)" % metric, out)]
        assert len(val[name]) == 10 and val[name][-1] < val[name][0]
        model[name] = G.Booster.load("%s.model" % name, G.GBDTParam())
        assert main(["task=pred", "model_in=%s.model" % name, "test:data=train.libsvm",
                     "name_pred=%s.txt" % name]) == 0
        pred[name] = [float(v) for v in open("%s.txt" % name).read().split()]
    assert len(model["gpu"].trees) == len(model["cpu"].trees) == 10
    for a, b in zip(model["gpu"].trees, model["cpu"].trees):
        assert a.feat == b.feat and a.left == b.left and a.right == b.right
    for a, b in zip(val["gpu"], val["cpu"]):
        assert abs(a - b) <= 1e-3 * abs(b), (val["gpu"], val["cpu"])
    assert len(pred["gpu"]) == len(pred["cpu"]) == 400 and all(p > 0 for p in pred["gpu"])
    assert all(abs(a - b) <= 1e-4 * abs(b) for a, b in zip(pred["gpu"], pred["cpu"]))
