"""survival:cox and survival:aft without a GPU: the objectives' plumbing, the
plain-torch paths against the fp64 oracles of tests/_gbdt_survival_cases.py,
the metrics, the per-rank strata, the app and the host test binary."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import _gbdt_survival_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _bsp():
    from wormhole_amd.parallel.bsp import BSP
    return BSP(CPU)


def _tile():
    from wormhole_amd import _native
    return int(_native.hip().gbdt_cox_tile())


class _Data:
    """What an objective takes from a matrix."""

    def __init__(self, label, weight=None, lower=None, upper=None):
        self.label, self.weight, self.lower, self.upper = label, weight, lower, upper
        self._plan = None

    def cox_plan(self):
        if self._plan is None:
            self._plan = _G().CoxPlan(self.label, self.weight)
        return self._plan


# ------------------------------------------------------------- 1. plumbing
def test_objectives_construct():
    G = _G()
    cox, aft = G.Objective("survival:cox"), G.make_objective("survival:aft")
    assert cox.default_metric() == "cox-nloglik" and aft.default_metric() == "aft-nloglik"
    assert cox.n_group == 1 and aft.n_group == 1
    for obj in (cox, aft):
        assert obj.prob_to_margin(2.0) == math.log(2.0)
        with pytest.raises(ValueError, match="base_score"):
            obj.prob_to_margin(0.0)
        assert torch.equal(obj.pred(torch.tensor([0.0, 1.0])), torch.exp(torch.tensor([0.0, 1.0])))
    cox.check_metrics(["cox-nloglik", "rmse"])
    aft.check_metrics(["aft-nloglik", "interval-regression-accuracy"])
    for obj, bad in ((cox, "aft-nloglik"), (cox, "interval-regression-accuracy"),
                     (aft, "cox-nloglik"), (G.Objective("reg:squarederror"), "cox-nloglik"),
                     (G.Objective("binary:logistic"), "aft-nloglik"),
                     (G.Objective("count:poisson"), "interval-regression-accuracy")):
        with pytest.raises(ValueError, match=bad):
            obj.check_metrics([bad])
    # ids 0-10 of the row-local kernel are as they were: 7 stays refused
    assert "survival:cox" not in G.OBJ_IDS and 7 not in G.OBJ_IDS.values()


def test_parameters_refused():
    G = _G()
    p = G.GBDTParam()
    assert p.set("aft_loss_distribution", "logistic") and p.set("aft_loss_distribution_scale", "2")
    obj = G.make_objective("survival:aft", 0, p)
    assert (obj.aft_dist, obj.aft_sigma) == (1, 2.0)
    with pytest.raises(SystemExit, match="aft_loss_distribution"):
        G.GBDTParam().set("aft_loss_distribution", "weibull")
    for bad in ("0", "-1", "nan", "x"):
        with pytest.raises(SystemExit, match="aft_loss_distribution_scale"):
            G.GBDTParam().set("aft_loss_distribution_scale", bad)
    p = G.GBDTParam()
    p.set("scale_pos_weight", "2")
    for name in ("survival:cox", "survival:aft"):
        with pytest.raises(ValueError, match="scale_pos_weight"):
            G.make_objective(name, 0, p)
    with pytest.raises(ValueError, match="label_lower_bound"):
        G.Objective("survival:aft").gpair(torch.zeros(3), torch.zeros(3), None)
    with pytest.raises(ValueError, match="finite"):
        G.Objective("survival:cox").check_labels(torch.tensor([1.0, float("inf")]), _bsp())
    with pytest.raises(ValueError, match="finite"):
        G.Objective("survival:cox").check_labels(torch.tensor([float("nan"), 2.0]), _bsp())
    G.Objective("survival:cox").check_labels(torch.tensor([1.0, -2.0, 0.0]), _bsp())


# ------------------------------------------------------------------ 2. cox
def _cox_check(margin, label, weight, got=None):
    G = _G()
    ref, scale, _, _ = C.cox_oracle(margin, label, weight)
    got = got if got is not None else G.cox_gpair_torch(margin, label, weight)
    assert got.shape == (margin.numel(), 2) and got.dtype == torch.float32
    err = (got.double() - ref).abs()
    assert bool((err <= C.COX_BOUND * scale).all()), float((err / scale.clamp(min=1e-300)).max())
    assert bool((got[:, 1] >= 0).all())
    return got, ref


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", ["1", "2", "T-1", "T", "T+1", "3T+5"])
def test_cox_gpair_torch(case, weighted):
    T = _tile()
    n = {"1": 1, "2": 2, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[case]
    _cox_check(*C.cox_inputs(n, weighted))


def test_cox_edge_cases():
    G = _G()
    T = _tile()
    # all rows tied
    _cox_check(*C.cox_inputs(T + 1, True, times=1))
    # all events
    _cox_check(*C.cox_inputs(T + 1, True, events="all"))
    # no events: the pair is all zeros, the metric nan
    margin, label, weight = C.cox_inputs(T + 1, True, events="none")
    got, _ = _cox_check(margin, label, weight)
    assert torch.equal(got, torch.zeros_like(got))
    obj = G.Objective("survival:cox")
    v = obj.metrics(["cox-nloglik"], margin, label, weight, _bsp(), data=_Data(label, weight))
    assert math.isnan(v[0])
    # a row in no event's risk set (censored before the first event): h == 0
    label = torch.tensor([-1.0, 2.0, 3.0, -4.0])
    got, _ = _cox_check(torch.tensor([0.3, -0.2, 0.1, 0.0]), label, None)
    assert got[0].tolist() == [0.0, 0.0] and bool((got[1:, 1] > 0).all())
    # the closed-form Hessian of the oracle is the second autograd pass
    margin, label, _ = C.cox_inputs(40, False)
    ref, _, _, _ = C.cox_oracle(margin, label)
    assert torch.allclose(ref[:, 1], C.cox_hess_autograd(margin, label), rtol=1e-10, atol=1e-13)
    # empty
    assert G.cox_gpair_torch(torch.zeros(0), torch.zeros(0), None).shape == (0, 2)
    # a plan refuses a label that is not finite (it has no place in the sort)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="finite"):
            G.CoxPlan(torch.tensor([1.0, bad, 2.0]))
    # a risk set whose every e underflowed (margins 2000 below m*): finite, no pull
    margin = torch.tensor([0.0, 1.0, -2000.0, -2000.0])
    label = torch.tensor([1.0, 2.0, 3.0, -4.0])
    got = G.cox_gpair_torch(margin, label, None)
    assert bool(torch.isfinite(got).all()) and got[2].tolist() == [-1.0, 0.0]
    assert got[3].tolist() == [0.0, 0.0]
    assert bool(torch.isfinite(G.cox_eval_torch(margin, label)).all())


def test_cox_shift_invariance():
    G = _G()
    g = torch.Generator().manual_seed(3)
    n = 300
    margin = torch.randint(-32, 33, (n,), generator=g).float() / 8
    _, label, weight = C.cox_inputs(n, True)
    a = G.cox_gpair_torch(margin, label, weight)
    b = G.cox_gpair_torch(margin + 64, label, weight)
    assert torch.equal(a, b)


def test_cox_against_xgboost_loop():
    """Without ties the pair is xgboost's; with ties it is not (a tied row of
    xgboost's sees only the events sorted before it)."""
    G = _G()
    margin, label, weight = C.cox_inputs(500, True, times=0)
    got = G.cox_gpair_torch(margin, label, weight).double()
    ref = C.cox_xgboost_loop(margin, label, weight)
    _, scale, _, _ = C.cox_oracle(margin, label, weight)
    # (the loop works on exp(m) itself, without m*: 1e-9 M covers its fp64)
    assert bool(((got - ref).abs() <= (C.COX_BOUND + 1e-9) * scale).all())
    margin, label, weight = C.cox_inputs(500, True, times=7)
    got = G.cox_gpair_torch(margin, label, weight).double()
    ref = C.cox_xgboost_loop(margin, label, weight)
    _, scale, _, _ = C.cox_oracle(margin, label, weight)
    assert bool(((got - ref).abs() > 1e-3 * scale).any())


def test_cox_metric_and_strata():
    G = _G()
    margin, label, weight = C.cox_inputs(777, True)
    _, _, L, E = C.cox_oracle(margin, label)
    v = G.cox_eval_torch(margin, label)
    assert v.dtype == torch.float64 and int(v[1]) == E and abs(float(v[0]) - L) <= 1e-10 * abs(L)
    obj = G.Objective("survival:cox")
    got = obj.metrics(["cox-nloglik"], margin, label, weight, _bsp(), data=_Data(label, weight))
    assert abs(got[0] - L / E) <= 1e-10 * abs(L / E)  # unweighted
    # two ranks, two strata: the halves' {sum loss, E} combine to the halves' oracle
    h = 400
    La, Ea = C.cox_oracle(margin[:h], label[:h])[2:]
    Lb, Eb = C.cox_oracle(margin[h:], label[h:])[2:]
    va = G.cox_eval_torch(margin[:h], label[:h])
    vb = G.cox_eval_torch(margin[h:], label[h:])
    tot = va + vb
    assert int(tot[1]) == Ea + Eb == E
    assert abs(float(tot[0] / tot[1]) - (La + Lb) / (Ea + Eb)) <= 1e-10
    assert abs((La + Lb) - L) > 1e-3  # (the strata are not the pooled set)


# ------------------------------------------------------------------ 3. aft
@pytest.mark.parametrize("sigma", C.SIGMAS)
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dist", C.DISTS)
def test_aft_gpair_torch(dist, kind, sigma):
    G = _G()
    for weighted in (False, True):
        margin, lower, upper, weight = C.aft_inputs(dist, kind, sigma, weighted=weighted)
        assert set(C.aft_kind(lower, upper)) == {kind}
        ref, raw, loss = C.aft_oracle(dist, margin, lower, upper, sigma, weight)
        # the oracle is well conditioned on these rows
        assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(loss).all())
        scale = C.aft_scale(dist, margin, lower, upper, sigma, raw, loss, weight)
        got = G.aft_gpair_torch(margin, lower, upper, weight, C.DISTS.index(dist), sigma)
        assert got.shape == (margin.numel(), 2) and got.dtype == torch.float32
        err = C.aft_rel_err(got, ref, scale)
        print("%s %s sigma=%g weighted=%d: |err| / (2^-24 w M) = %.3g"
              % (dist, kind, sigma, weighted, float(err.max()) / 2.0 ** -24))
        assert bool((err <= C.AFT_BOUND).all())


@pytest.mark.parametrize("dist", C.DISTS)
def test_aft_tails(dist):
    G = _G()
    margin, lower, upper = C.aft_tail_inputs()
    ref, _, _ = C.aft_oracle(dist, margin, lower, upper, 1.0)
    got = G.aft_gpair_torch(margin, lower, upper, None, C.DISTS.index(dist), 1.0)
    assert bool(torch.isfinite(got).all())
    assert bool(((got[:, 0] >= C.MIN_G) & (got[:, 0] <= C.MAX_G)).all())
    assert bool(((got[:, 1] >= torch.tensor(C.MIN_H).float()) & (got[:, 1] <= C.MAX_H)).all())
    for col, values in ((0, (C.MIN_G, C.MAX_G)), (1, (C.MIN_H, C.MAX_H))):
        for v in values:
            at = ref[:, col] == v
            assert bool((got[at, col] == torch.tensor(v).float()).all()), (dist, col, v)
    assert int(((ref[:, 0].abs() == 15) | (ref[:, 1] == C.MIN_H) | (ref[:, 1] == 15)).sum()) >= 8  # (the case has rows at the clamps)


@pytest.mark.parametrize("dist", C.DISTS)
def test_aft_metrics(dist):
    G = _G()
    sigma = 2.0
    parts = [C.aft_inputs(dist, kind, sigma, weighted=True) for kind in C.KINDS]
    margin, lower, upper, weight = (torch.cat([p[i] for p in parts]) for i in range(4))
    _, _, loss = C.aft_oracle(dist, margin, lower, upper, sigma)
    loss = loss.clamp(max=-math.log(1e-12))
    want = float((weight.double() * loss).sum() / weight.double().sum())
    p = torch.exp(margin.double())
    acc = float(((lower.double() <= p) & (p <= upper.double())).double().mean())
    prm = G.GBDTParam()
    prm.set("aft_loss_distribution", dist)
    prm.set("aft_loss_distribution_scale", str(sigma))
    obj = G.make_objective("survival:aft", 0, prm)
    got = obj.metrics(["aft-nloglik", "interval-regression-accuracy"], margin, None, weight,
                      _bsp(), data=_Data(None, weight, lower, upper))
    assert abs(got[0] - want) <= 1e-9 * abs(want) and got[1] == acc and 0 < acc < 1
    # beside a metric of the prediction (the label column plays the label)
    mixed = obj.metrics(["rmse", "aft-nloglik"], margin, lower, weight, _bsp(),
                        data=_Data(lower, weight, lower, upper))
    assert mixed[1] == got[0] and math.isfinite(mixed[0])
    # the floor of the likelihood
    # (z = -60: every law's density is below 1e-12 there, the logistic's e^-60)
    far = G.aft_eval_torch(torch.tensor([60.0]), torch.tensor([1.0]), torch.tensor([1.0]), None,
                           C.DISTS.index(dist), 1.0)
    assert abs(float(far[0]) + math.log(1e-12)) < 1e-9
    near = G.aft_eval_torch(torch.tensor([0.0]), torch.tensor([1.0]), torch.tensor([1.0]), None,
                            C.DISTS.index(dist), 1.0)
    assert float(near[0]) < 2.0


# ------------------------------------------------------------------ 4. app
def _run(main, capsys, args):
    assert main(args) == 0
    out = capsys.readouterr().out
    assert "unknown parameter" not in out
    return out


def _write_bounds(base, lower, upper):
    for suffix, v in ((".label_lower_bound", lower), (".label_upper_bound", upper)):
        with open(str(base) + suffix, "w") as f:
            f.write("".join("%s\n" % ("inf" if math.isinf(x) else repr(x)) for x in v.tolist()))


APP = ["max_depth=3", "num_round=10", "eval_train=1", "max_bin=32", "min_child_weight=1"]


@pytest.fixture
def app(tmp_path, monkeypatch):
    from wormhole_amd.apps.xgboost_app import main
    monkeypatch.chdir(tmp_path)
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WH_DEVICE", "cpu")
    return main


def test_app_cox(app, tmp_path, capsys):
    X, t, event = C.survival_rows()
    C.write_libsvm(tmp_path / "train.libsvm", X, torch.where(event, t, -t))
    out = _run(app, capsys, ["data=train.libsvm", "objective=survival:cox",
                             "model_out=cox.model"] + APP)
    vals = [float(v) for v in re.findall(r"train-cox-nloglik:([0-9.]+)", out)]
    assert len(vals) == 10 and vals[-1] < vals[0]
    _run(app, capsys, ["task=pred", "model_in=cox.model", "test:data=train.libsvm",
                       "name_pred=pred.txt"])
    pred = [float(v) for v in open("pred.txt").read().split()]
    assert len(pred) == 400 and all(p > 0 for p in pred)
    out = _run(app, capsys, ["task=eval", "model_in=cox.model", "test:data=train.libsvm"])
    assert abs(float(re.search(r"test-cox-nloglik:([0-9.]+)", out).group(1)) - vals[-1]) < 2e-6
    # the hazard rises with feature 0
    hi, lo = X[:, 0] > 0.8, X[:, 0] < 0.2
    p = torch.tensor(pred)
    assert float(p[hi].mean()) > float(p[lo].mean())
    with pytest.raises(ValueError, match="cox-nloglik"):
        app(["data=train.libsvm", "objective=reg:squarederror", "eval_metric=cox-nloglik"] + APP)


@pytest.mark.parametrize("dist", C.DISTS)
def test_app_aft(app, tmp_path, capsys, dist):
    X, t, event = C.survival_rows()
    t = t.clamp(min=0.125)
    upper = torch.where(event, t, torch.full_like(t, float("inf")))
    C.write_libsvm(tmp_path / "train.libsvm", X, torch.zeros_like(t))  # (the labels are ignored)
    _write_bounds(tmp_path / "train.libsvm", t, upper)
    extra = ["aft_loss_distribution=" + dist, "aft_loss_distribution_scale=1.2"]
    out = _run(app, capsys, ["data=train.libsvm", "objective=survival:aft", "model_out=aft.model",
                             "eval_metric=aft-nloglik", "eval_metric=interval-regression-accuracy"]
               + APP + extra)
    vals = [float(v) for v in re.findall(r"train-aft-nloglik:([0-9.]+)", out)]
    assert len(vals) == 10 and vals[-1] < vals[0]
    assert len(re.findall(r"train-interval-regression-accuracy:([0-9.]+)", out)) == 10
    _run(app, capsys, ["task=pred", "model_in=aft.model", "test:data=train.libsvm",
                       "name_pred=pred.txt"])
    pred = [float(v) for v in open("pred.txt").read().split()]
    assert len(pred) == 400 and all(p > 0 for p in pred)
    out = _run(app, capsys, ["task=eval", "model_in=aft.model", "test:data=train.libsvm"] + extra)
    assert abs(float(re.search(r"test-aft-nloglik:([0-9.]+)", out).group(1)) - vals[-1]) < 2e-6


def test_app_aft_refusals(app, tmp_path):
    X, t, _ = C.survival_rows(40)
    t = t.clamp(min=0.125)
    C.write_libsvm(tmp_path / "train.libsvm", X, t)
    args = ["data=train.libsvm", "objective=survival:aft", "num_round=1"]
    with pytest.raises(SystemExit, match=r"train\.libsvm\.label_lower_bound"):
        app(args)
    with pytest.raises(ValueError, match="aft-nloglik"):
        app(["data=train.libsvm", "objective=reg:squarederror", "num_round=1", "eval_train=1",
             "eval_metric=aft-nloglik"])
    # an eval set without its files, beside a training set with them
    C.write_libsvm(tmp_path / "valid.libsvm", X, t)
    _write_bounds(tmp_path / "train.libsvm", t, t)
    with pytest.raises(SystemExit, match=r"valid\.libsvm\.label_lower_bound"):
        app(args + ["eval[v]=valid.libsvm"])
    with pytest.raises(SystemExit, match="aft_loss_distribution"):
        app(args + ["aft_loss_distribution=gumbel"])
    with pytest.raises(SystemExit, match="aft_loss_distribution_scale"):
        app(args + ["aft_loss_distribution_scale=0"])
    inf = float("inf")
    bad = {"label_upper_bound": (t, t[:-1]), "label_lower_bound": (-t, t)}
    for name, (lo, up) in bad.items():
        _write_bounds(tmp_path / "train.libsvm", lo, up)
        with pytest.raises(SystemExit, match=r"train\.libsvm\." + name):
            app(args)
    for lo, up, name in ((t, torch.zeros_like(t), "label_upper_bound"),
                         (t, t / 2, "label_upper_bound"),
                         (torch.full_like(t, inf), torch.full_like(t, inf), "label_lower_bound"),
                         (torch.full_like(t, float("nan")), t, "label_lower_bound")):
        _write_bounds(tmp_path / "train.libsvm", lo, up)
        with pytest.raises(SystemExit, match=r"train\.libsvm\." + name):
            app(args)
    # another objective does not read the files, whatever they hold
    _write_bounds(tmp_path / "train.libsvm", -t, t[:-1])
    assert app(["data=train.libsvm", "objective=reg:squarederror", "num_round=1"]) == 0
    _write_bounds(tmp_path / "train.libsvm", t, t)
    os.remove(tmp_path / "train.libsvm.label_upper_bound")
    with pytest.raises(SystemExit, match=r"train\.libsvm\.label_upper_bound"):
        app(args)


def test_app_compositions(app, tmp_path, capsys):
    """survival:cox under dart, lossguide, subsample, both constraint kinds and
    CSR rows; survival:aft under lossguide and CSR: each run's metric falls."""
    X, t, event = C.survival_rows(200)
    t = t.clamp(min=0.125)
    C.write_libsvm(tmp_path / "train.libsvm", X, torch.where(event, t, -t))
    _write_bounds(tmp_path / "train.libsvm", t,
                  torch.where(event, t, torch.full_like(t, float("inf"))))
    base = ["data=train.libsvm", "max_depth=3", "num_round=4", "eval_train=1", "max_bin=32"]
    for objective, metric, extras in (
            ("survival:cox", "cox-nloglik",
             (["booster=dart", "rate_drop=0.3"], ["grow_policy=lossguide", "max_leaves=6"],
              ["subsample=0.7"], ["monotone_constraints=(1,0,0,0)"],
              ["interaction_constraints=[[0,1],[2,3]]"], ["dsparse=1"], ["max_delta_step=0.5"])),
            ("survival:aft", "aft-nloglik",
             (["grow_policy=lossguide", "max_leaves=6"], ["dsparse=1"], ["subsample=0.7"]))):
        for extra in extras:
            out = _run(app, capsys, base + ["objective=" + objective] + extra)
            vals = [float(v) for v in re.findall(r"train-%s:([0-9.]+)" % metric, out)]
            assert len(vals) == 4 and vals[-1] < vals[0], (objective, extra, vals)


# ------------------------------------------------------ 5. host test binary
def test_plan_test_binary():
    exe = os.path.join(ROOT, "bin", "native", "gbdt_survival_plan_test")
    assert os.path.exists(exe), "native tools not built (python build_native.py)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_plan_test_binary_sanitized():
    b = subprocess.run([sys.executable, os.path.join(ROOT, "build_native.py"),
                        "--sanitize-survival-plan"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    exe = b.stdout.strip().splitlines()[-1]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
