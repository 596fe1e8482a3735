"""count:poisson, reg:gamma, reg:tweedie, binary:hinge, reg:pseudohubererror,
reg:squaredlogerror, their metrics, max_delta_step and scale_pos_weight on the
CPU path (plain torch: also the reference of the GPU kernels)."""
import math
import os
import re

import pytest
import torch

import _gbdt_monotone_cases as M
import _gbdt_objective_cases as C

CPU = torch.device("cpu")


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _bsp():
    from wormhole_amd.parallel.bsp import BSP
    os.environ.pop("RANK", None)
    return BSP(CPU)


def _param(G, **kw):
    p = G.GBDTParam()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ------------------------------------------------------- 1. the formulas
def _loss64(name, m, y):
    """The loss whose derivatives the table's pairs are, fp64, per row."""
    if name == "count:poisson":
        return torch.exp(m) - y * m
    if name == "reg:gamma":
        return y / torch.exp(m) + m
    if name == "reg:tweedie":
        return (-y * torch.exp((1 - C.RHO) * m) / (1 - C.RHO)
                + torch.exp((2 - C.RHO) * m) / (2 - C.RHO))
    if name == "reg:pseudohubererror":
        return C.DELTA ** 2 * (torch.sqrt(1 + (m - y) ** 2 / C.DELTA ** 2) - 1)
    if name == "reg:squaredlogerror":
        return 0.5 * (torch.log1p(m) - torch.log1p(y)) ** 2
    raise ValueError(name)


# fp32 against fp64 on exactly representable inputs: a pair is at most 8 fp32
# operations of <= 1 ulp (2^-24 = 6e-8) each on terms bounded by M, plus the
# rounding of exp's argument (|arg| 2^-24 with |arg| <= 4.7 here, as a relative
# error of the exponential): below 16 x 6e-8 = 1e-6 of M. This is the floor of
# the GPU kernel's bound (tests/test_gbdt_objectives_gpu.py).
FP32_REL = 1e-6


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", [o for o in C.OBJECTIVES if o != "binary:hinge"])
def test_pairs_are_the_loss_derivatives(name, weighted):
    G = _G()
    n = 257
    g = torch.Generator().manual_seed(7 + C.OBJECTIVES.index(name))
    m32 = torch.rand(n, generator=g) * 8 - 4
    y32 = C.labels(name, n, g)
    w32 = torch.rand(n, generator=g) * 1.5 + 0.5 if weighted else None
    obj = G.Objective(name, 0, _param(G, objective=name))
    assert obj.max_delta_step == (0.7 if name == "count:poisson" else 0.0)
    got = obj.gpair(m32, y32, w32)
    assert got.shape == (n, 2) and got.dtype == torch.float32
    # the point of differentiation: the margin, or for the squared log error
    # the clamped margin the formula is evaluated at (the clamp itself has no
    # derivative; fp32 holds -1 + 1e-6 as SLE_MIN32, an exact fp64 input)
    x = m32.double()
    if name == "reg:squaredlogerror":
        x = x.clamp(min=C.SLE_MIN32)
        assert bool((m32 < -1).any())  # the clamp is exercised
    x.requires_grad_(True)
    loss = _loss64(name, x, y32.double())
    (g1,) = torch.autograd.grad(loss.sum(), x, create_graph=True)
    (g2,) = torch.autograd.grad(g1.sum(), x)
    g1 = g1.detach()
    if name == "count:poisson":  # h is exp(m + max_delta_step) by definition
        g2 = torch.exp(m32.double() + 0.7)
    if name == "reg:squaredlogerror":  # floored
        g2 = g2.clamp(min=1e-6)
    w = w32.double() if weighted else torch.ones(n, dtype=torch.float64)
    want = torch.stack([g1 * w, g2 * w], 1)
    ref, scale = C.weighted64(name, m32, y32, w32, sle_min=C.SLE_MIN32)
    # the cases' own fp64 formulas are the derivatives (fp64 rounding)
    assert bool(((ref - want).abs() <= 1e-12 * scale).all())
    err = (got.double() - want).abs() / scale
    print("%s weighted=%d: largest error / (w M): g %.3g h %.3g"
          % (name, weighted, float(err[:, 0].max()), float(err[:, 1].max())))
    assert bool((err <= FP32_REL).all()), err.max(0)


def test_hinge_table():
    G = _G()
    obj = G.Objective("binary:hinge")
    #            y=1 wrong side, y=1 satisfied, y=0 wrong side, y=0 satisfied
    m = torch.tensor([0.5, 1.0, -0.5, -1.5])
    y = torch.tensor([1.0, 1.0, 0.0, 0.0])
    w = torch.tensor([2.0, 3.0, 0.5, 3.0])
    assert obj.gpair(m, y, None).tolist() == [[-1.0, 1.0], [0.0, C.FLT_MIN], [1.0, 1.0],
                                              [0.0, C.FLT_MIN]]
    assert obj.gpair(m, y, w).tolist() == [[-2.0, 2.0], [0.0, C.FLT_MIN], [0.5, 0.5],
                                           [0.0, C.FLT_MIN]]  # FLT_MIN: not times 3
    assert C.FLT_MIN == float(torch.finfo(torch.float32).tiny)
    assert obj.pred(torch.tensor([-1.0, 0.0, 2.0])).tolist() == [0.0, 0.0, 1.0]
    assert obj.default_metric() == "error"


def test_constructor_and_parameters():
    G = _G()
    assert G.Objective("reg:linear").name == "reg:linear"  # as it is called today
    assert G.Objective("multi:softmax", 3).n_group == 3
    with pytest.raises(ValueError, match="unknown objective"):
        G.Objective("reg:absoluteerror")
    p = G.GBDTParam()
    for k, v in (("max_delta_step", "0.5"), ("scale_pos_weight", "2"),
                 ("tweedie_variance_power", "1.2"), ("huber_slope", "3")):
        assert p.set(k, v) is True
    assert (p.max_delta_step, p.scale_pos_weight, p.tweedie_variance_power, p.huber_slope) == (
        0.5, 2.0, 1.2, 3.0)
    for k, v in (("max_delta_step", "-1"), ("scale_pos_weight", "0"),
                 ("tweedie_variance_power", "2"), ("tweedie_variance_power", "1"),
                 ("huber_slope", "0")):
        with pytest.raises(SystemExit, match=k):
            G.GBDTParam().set(k, v)
    # max_delta_step: 0.7 for count:poisson unless set, else 0
    assert _param(G, objective="count:poisson").delta_step() == 0.7
    assert _param(G, objective="count:poisson", max_delta_step=0.0).delta_step() == 0.0
    assert _param(G, objective="reg:gamma").delta_step() == 0.0
    assert G.Objective("count:poisson", 0, _param(G, max_delta_step=0.25)).max_delta_step == 0.25
    with pytest.raises(ValueError, match=r"scale_pos_weight.*reg:linear"):
        G.Objective("reg:linear", 0, _param(G, scale_pos_weight=2.0))
    # base_score -> margin, prediction, default metric
    for name in ("count:poisson", "reg:gamma", "reg:tweedie"):
        obj = G.Objective(name)
        assert obj.prob_to_margin(0.5) == math.log(0.5)
        with pytest.raises(ValueError, match="base_score"):
            obj.prob_to_margin(0.0)
        assert torch.equal(obj.pred(torch.tensor([0.0, 1.0])), torch.exp(torch.tensor([0.0, 1.0])))
    assert G.Objective("reg:pseudohubererror").prob_to_margin(0.5) == 0.5
    want = {"count:poisson": "poisson-nloglik", "reg:gamma": "gamma-nloglik",
            "reg:tweedie": "tweedie-nloglik@1.5", "binary:hinge": "error",
            "reg:pseudohubererror": "mphe", "reg:squaredlogerror": "rmsle"}
    assert {n: G.Objective(n).default_metric() for n in want} == want
    p = _param(G, tweedie_variance_power=1.25)
    assert G.Objective("reg:tweedie", 0, p).default_metric() == "tweedie-nloglik@1.25"


def test_label_checks():
    G = _G()
    bsp = _bsp()
    bad = {"count:poisson": -1.0, "reg:tweedie": -0.5, "reg:gamma": 0.0, "binary:hinge": 0.5,
           "reg:squaredlogerror": -1.0}
    for name, v in bad.items():
        obj = G.Objective(name)
        good = C.labels(name, 50, torch.Generator().manual_seed(1))
        obj.check_labels(good, bsp)
        obj.check_labels(good[:0], bsp)
        with pytest.raises(ValueError, match="label"):
            obj.check_labels(torch.cat([good, torch.tensor([v])]), bsp)
    G.Objective("reg:pseudohubererror").check_labels(torch.tensor([-5.0, 7.0]), bsp)


def test_scale_pos_weight_pairs():
    """Rows with y == 1 weigh s times as much, in the pairs only; s = 1 is the
    existing path."""
    G = _G()
    g = torch.Generator().manual_seed(3)
    m, y = torch.randn(100, generator=g), (torch.rand(100, generator=g) < 0.3).float()
    w = torch.rand(100, generator=g) + 0.5
    for name in ("binary:logistic", "reg:logistic", "binary:logitraw"):
        plain = G.Objective(name)
        obj = G.Objective(name, 0, _param(G, objective=name, scale_pos_weight=3.0))
        assert plain.obj_id is None and obj.obj_id == G.OBJ_LOGISTIC
        s = torch.where(y == 1, 3.0, 1.0)
        assert torch.equal(obj.gpair(m, y, None), plain.gpair(m, y, s))
        assert torch.equal(obj.gpair(m, y, w), plain.gpair(m, y, w * s))
        assert torch.equal(obj.gpair(m, y, w, pos_weight=False), plain.gpair(m, y, w))
        bsp = _bsp()
        # (binary:logitraw predicts the margin: no log-loss of it)
        names = ["error"] if name == "binary:logitraw" else ["logloss", "error"]
        assert obj.metrics(names, m, y, w, bsp) == plain.metrics(names, m, y, w, bsp)


# --------------------------------------------------------- 2. the metrics
def test_metrics_by_hand():
    G = _G()
    bsp = _bsp()
    m = torch.tensor([0.0, math.log(2.0), math.log(0.5), 1.0, -1.0])  # p = 1, 2, .5, e, 1/e
    y = torch.tensor([1.0, 3.0, 0.5, 2.0, 1.0])
    w = torch.tensor([1.0, 2.0, 1.0, 0.5, 1.5])
    p = [math.exp(float(v)) for v in m.double()]
    ys, ws = y.tolist(), w.tolist()
    W = sum(ws)

    def mean(f):
        return sum(wi * f(pi, yi) for wi, pi, yi in zip(ws, p, ys)) / W

    rho = 1.5
    want = {
        "poisson-nloglik": mean(lambda q, t: math.lgamma(t + 1) + q - t * math.log(q)),
        "gamma-nloglik": mean(lambda q, t: t / q + math.log(q)),
        "gamma-deviance": 2 * mean(lambda q, t: math.log((q + 1e-16) / (t + 1e-16))
                                   + (t + 1e-16) / (q + 1e-16) - 1),
        "tweedie-nloglik@1.5": mean(lambda q, t: -t * q ** (1 - rho) / (1 - rho)
                                    + q ** (2 - rho) / (2 - rho)),
        "mae": mean(lambda q, t: abs(q - t)),
        "mphe": mean(lambda q, t: math.sqrt(1 + (q - t) ** 2) - 1),
        "rmsle": math.sqrt(mean(lambda q, t: (math.log1p(t) - math.log1p(q)) ** 2)),
    }
    # a spot value from the round predictions (the fp32 margins hold log 2
    # and log 0.5 to 2^-24, so p is 2 and 0.5 to 1e-7)
    assert abs(mean(lambda q, t: abs(q - t)) - (0 + 2 * 1 + 0 + 0.5 * (math.e - 2)
                                                + 1.5 * (1 - 1 / math.e)) / 6) < 1e-7
    obj = G.Objective("count:poisson")
    names = list(C.METRICS)
    got = obj.metrics(names, m, y, w, bsp)
    for nm, v in zip(names, got):
        assert abs(v - want[nm]) <= 1e-12 * max(1.0, abs(want[nm])), (nm, v, want[nm])
        assert abs(C.metric64(nm, torch.exp(m.double()), y, w)[0] - want[nm]) < 1e-12
    # any order, mixed with an existing metric, and two powers at once
    mixed = obj.metrics(["rmse", "mae", "tweedie-nloglik@1.2", "tweedie-nloglik@1.5"], m, y, w, bsp)
    assert mixed[1] == got[names.index("mae")] and mixed[3] == got[3]
    assert abs(mixed[2] - C.metric64("tweedie-nloglik@1.2", torch.exp(m.double()), y, w,
                                     rho=1.2)[0]) < 1e-12
    # identity link: the margin is the prediction; mphe with another slope
    hub = G.Objective("reg:pseudohubererror", 0, _param(G, huber_slope=2.0))
    v = hub.metrics(["mphe", "mae"], m, y, None, bsp)
    assert abs(v[0] - C.metric64("mphe", m, y, None, delta=2.0)[0]) < 1e-12
    assert abs(v[1] - float((m.double() - y.double()).abs().mean())) < 1e-12
    # unweighted rmsle on a positive margin
    sle = G.Objective("reg:squaredlogerror")
    v = sle.metrics(["rmsle"], y + 0.5, y, None, bsp)[0]
    assert abs(v - C.metric64("rmsle", y + 0.5, y, None)[0]) < 1e-12


def test_metric_names():
    G = _G()
    obj = G.Objective("reg:tweedie")
    for bad in ("tweedie-nloglik", "tweedie-nloglik@2.5", "tweedie-nloglik@1", "tweedie-nloglik@x"):
        with pytest.raises(ValueError, match="tweedie-nloglik"):
            obj.check_metrics([bad])
    with pytest.raises(ValueError, match="unknown eval_metric"):
        obj.check_metrics(["mae@2"])
    for name in ("reg:linear", "binary:logistic", "rank:pairwise", "count:poisson"):
        G.Objective(name).check_metrics(list(C.METRICS))
    for m in C.METRICS:
        with pytest.raises(ValueError, match="does not fit"):
            G.Objective("multi:softmax", 3).check_metrics([m])


# ------------------------------------- 3. max_delta_step in the level loop
ROUNDS = 3


def _train(sparse=False, mono=None, **kw):
    G = _G()
    X, y = C.outlier_data()
    p = M.param(G, mono, max_depth=4, eta=1.0, **kw)
    dm = M.dmatrix(G, X, y, CPU, sparse)
    return M.train(G, _bsp(), dm, p, ROUNDS)[0].trees


def test_max_delta_step_bounds_every_leaf():
    bounded = _train(max_delta_step=C.STEP)
    assert len(bounded) == ROUNDS and sum(len(t.feat) for t in bounded) > 3 * 7
    assert C.leaves_bounded(bounded, C.STEP), C.largest_leaf(bounded)
    assert C.largest_leaf(bounded) == C.STEP  # and the bound is met: it bites
    # the control: left alone, the same rows grow leaves beyond the bound
    free = _train()
    assert not C.leaves_bounded(free, C.STEP), C.largest_leaf(free)
    # 0 is off: the same dump as the parameter's absence
    zero = _train(max_delta_step=0.0)
    assert [t.dump(None, True) for t in zero] == [t.dump(None, True) for t in free]
    assert [t.dump(None, True) for t in bounded] != [t.dump(None, True) for t in free]


def test_max_delta_step_with_monotone_constraints():
    mono = (1, -1, 0, 0, 0, 0)
    trees = _train(mono=mono, max_delta_step=C.STEP)
    assert C.leaves_bounded(trees, C.STEP)
    s = M.structure(trees, mono)
    assert all(bad == 0 for _, bad in s.values()) and sum(n for n, _ in s.values()) > 0, s
    # (the control of the structure check: without the signs it is broken)
    assert not M.holds(_train(max_delta_step=C.STEP), mono)


def test_max_delta_step_dense_and_csr_agree():
    dense = _train(max_delta_step=C.STEP)
    csr = _train(sparse=True, max_delta_step=C.STEP)
    for a, b in zip(dense, csr):
        C.same_structure(a, b)
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))
    assert C.leaves_bounded(csr, C.STEP)


def test_max_delta_step_multiclass():
    """Every class's trees are bounded (the builder is shared)."""
    G = _G()
    X, y = C.outlier_data()
    p = M.param(G, None, max_depth=3, eta=1.0, max_delta_step=0.1)
    p.objective, p.num_class = "multi:softprob", 3
    lab = (y > 0).float() + (y > 1).float()
    dm = M.dmatrix(G, X, lab, CPU)
    trees = M.train(G, _bsp(), dm, p, 2)[0].trees
    assert len(trees) == 6 and C.leaves_bounded(trees, 0.1)
    p.max_delta_step = None
    assert not C.leaves_bounded(M.train(G, _bsp(), dm, p, 2)[0].trees, 0.1)


# ------------------------------------------------------------- 4. the app
@pytest.fixture()
def work(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WH_DEVICE", "cpu")
    for k in ("DMLC_ROLE", "RANK", "WORLD_SIZE", "WH_CKPT_DIR", "WH_FAULT"):
        monkeypatch.delenv(k, raising=False)
    return tmp_path


def _count_rows(n=600):
    X, y = M.data(n, 4)
    g = torch.Generator().manual_seed(9)
    return X, torch.poisson(torch.exp(0.8 * y.clamp(-2, 2)), generator=g)


def _round_lines(out):
    return [l for l in out.splitlines() if re.match(r"^\[\d+\]\t", l)]


def test_app_poisson(work, capsys):
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    X, y = _count_rows()
    C.write_libsvm(work / "train.libsvm", X, y)
    args = ["data=train.libsvm", "objective=count:poisson", "max_depth=3", "max_bin=64",
            "num_round=3", "eval_train=1", "model_out=p.model"]
    assert main(args) == 0
    out = capsys.readouterr().out
    lines = _round_lines(out)
    vals = [float(re.search(r"train-poisson-nloglik:([0-9.]+)", l).group(1)) for l in lines]
    assert len(vals) == 3 and vals[0] >= vals[1] >= vals[2] and vals[2] < vals[0], vals
    b = G.Booster.load("p.model", G.GBDTParam())
    assert b.obj.name == "count:poisson" and len(b.trees) == 3
    assert C.leaves_bounded(b.trees, 0.3 * 0.7)  # max_delta_step defaults to 0.7
    # the three parameters are parsed, not ignored
    assert main(args + ["max_delta_step=0.7", "scale_pos_weight=1", "tweedie_variance_power=1.4",
                        "model_out=q.model"]) == 0
    out2 = capsys.readouterr().out
    assert "unknown parameter" not in out + out2
    assert _round_lines(out2) == lines
    # task=pred writes exp(margin)
    assert main(["task=pred", "model_in=p.model", "test:data=train.libsvm", "name_pred=p.txt"]) == 0
    assert main(["task=pred", "model_in=p.model", "test:data=train.libsvm", "name_pred=m.txt",
                 "pred_margin=1"]) == 0
    pred = [float(v) for v in open("p.txt").read().split()]
    marg = [float(v) for v in open("m.txt").read().split()]
    assert len(pred) == len(marg) == y.numel()
    assert all(abs(a - math.exp(z)) <= 2e-5 * a for a, z in zip(pred, marg))  # (two %g roundings)
    assert len(set(marg)) > 3
    # task=eval prints the last round's value
    capsys.readouterr()
    assert main(["task=eval", "model_in=p.model", "test:data=train.libsvm"]) == 0
    assert "test-poisson-nloglik:%f" % vals[2] in capsys.readouterr().out


def test_app_errors(work, capsys):
    from wormhole_amd.apps.xgboost_app import main
    X, y = _count_rows(100)
    C.write_libsvm(work / "ok.libsvm", X, y)
    y = y.clone()
    y[17] = -1.0
    C.write_libsvm(work / "neg.libsvm", X, y)
    base = ["max_depth=2", "num_round=1", "model_out=x.model"]
    with pytest.raises((ValueError, SystemExit), match="label must be non-negative"):
        main(["data=neg.libsvm", "objective=count:poisson"] + base)
    with pytest.raises((ValueError, SystemExit), match=r"scale_pos_weight.*reg:linear"):
        main(["data=ok.libsvm", "objective=reg:linear", "scale_pos_weight=2"] + base)
    with pytest.raises(SystemExit, match="max_delta_step"):
        main(["data=ok.libsvm", "max_delta_step=-0.5"] + base)
    with pytest.raises((ValueError, SystemExit), match="tweedie-nloglik"):
        main(["data=ok.libsvm", "objective=reg:tweedie", "eval_metric=tweedie-nloglik"] + base)


def test_app_scale_pos_weight_is_instance_weight(work, capsys):
    """scale_pos_weight=3 grows the trees of instance weights 3 on the
    positive rows (the eval lines differ: weights enter the metrics,
    scale_pos_weight does not)."""
    G = _G()
    from wormhole_amd.apps.xgboost_app import main
    X, t = M.data(800, 4)
    y = (t > t.median()).float()
    C.write_libsvm(work / "plain.libsvm", X, y)
    C.write_libsvm(work / "weighted.libsvm", X, y, torch.where(y == 1, 3.0, 1.0))
    args = ["objective=binary:logistic", "max_depth=4", "max_bin=64", "num_round=3", "eval_train=1"]
    assert main(args + ["data=plain.libsvm", "scale_pos_weight=3", "model_out=s.model"]) == 0
    ls = _round_lines(capsys.readouterr().out)
    assert main(args + ["data=weighted.libsvm", "model_out=w.model"]) == 0
    lw = _round_lines(capsys.readouterr().out)
    assert main(args + ["data=plain.libsvm", "model_out=f.model"]) == 0
    capsys.readouterr()
    dump = {k: G.Booster.load(k + ".model", G.GBDTParam()).dump(None, True) for k in "swf"}
    assert dump["s"] == dump["w"] and dump["s"] != dump["f"]
    assert len(ls) == len(lw) == 3 and ls != lw
