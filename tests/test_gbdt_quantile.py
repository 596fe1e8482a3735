"""reg:absoluteerror and reg:quantileerror on the CPU: the leaf quantile
reference against the definition, the gradient pairs and the ``quantile``
metric against fp64, the refreshed leaves of trained trees (pruned, subsampled,
dart), the app, and the unchanged bytes of a reg:squarederror model.

Weights are integers in 0..4 and the alphas dyadic unless a test says
otherwise, so every comparison of leaves is an equality of fp32 values."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _gbdt_objective_cases as C
import _gbdt_quantile_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKER = os.path.join(ROOT, "tracker", "dmlc_local.py")
XGB = os.path.join(ROOT, "bin", "xgboost.dmlc")
CPU = torch.device("cpu")
F32 = np.float32


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _bsp():
    from wormhole_amd.parallel.bsp import BSP
    return BSP(CPU)


# ------------------------------------------------- 1. the reference itself
def _ref_against_definition(r, u, segs, alpha):
    G = _G()
    q, empty = G.leaf_quantiles_ref(r, u, segs, alpha)
    q2, empty2 = G.select_torch(r, u, segs, alpha)
    assert torch.equal(q.view(torch.int32), q2.view(torch.int32)) and torch.equal(empty, empty2)
    for l, (b, e) in enumerate(segs):
        want, W = Q.brute_quantile(r[b:e].tolist(), u[b:e].tolist(), alpha)
        assert bool(empty[l]) == (W == 0)
        if W:
            got = q[l:l + 1]
            assert got.view(torch.int32).item() == torch.tensor([want], dtype=torch.float32).view(
                torch.int32).item(), (l, float(got), want)


@pytest.mark.parametrize("alpha", [0.5, 0.25, 0.75, 0.125])
def test_reference_against_the_definition(alpha):
    g = torch.Generator().manual_seed(int(alpha * 1000))
    sizes = [0, 1, 2, 63, 64, 65, 1000]
    cuts = [0]
    for s in sizes:
        cuts.append(cuts[-1] + s)
    n = cuts[-1]
    segs = list(zip(cuts[:-1], cuts[1:]))
    r = (torch.randn(n, generator=g) * 2).float()  # negative and positive
    u = torch.randint(0, 5, (n,), generator=g)
    _ref_against_definition(r, u, segs, alpha)
    # all-equal residuals; +-0.0 and denormals of both signs
    _ref_against_definition(torch.full((n,), -0.75), u, segs, alpha)
    z = torch.tensor([0.0, -0.0, 1e-42, -1e-42, 3e-45, -3e-45])[torch.randint(0, 6, (n,), generator=g)]
    _ref_against_definition(z, u, segs, alpha)
    q, _ = _G().leaf_quantiles_ref(torch.tensor([-0.0, -0.0]), torch.tensor([1, 1]), [(0, 2)], alpha)
    assert q.view(torch.int32).item() == 0  # -0.0 and +0.0 are one value: +0.0
    # an all-zero-weight segment keeps "empty"; zero-weight rows at both ends are never chosen
    r2 = torch.tensor([-9.0, 1.0, 2.0, 3.0, 9.0, 5.0, 6.0])
    u2 = torch.tensor([0, 2, 1, 1, 0, 0, 0])
    q, empty = _G().leaf_quantiles_ref(r2, u2, [(0, 5), (5, 7)], alpha)
    assert empty.tolist() == [False, True] and float(q[0]) in (1.0, 2.0, 3.0)
    _ref_against_definition(r2, u2, [(0, 5), (5, 7)], alpha)


def test_lower_median_and_fractional_weights():
    G = _G()
    # alpha = 0.5 on an even unweighted count: the lower median
    q, _ = G.leaf_quantiles_ref(torch.tensor([4.0, 1.0, 3.0, 2.0]), torch.ones(4, dtype=torch.int64),
                                [(0, 4)], 0.5)
    assert float(q[0]) == 2.0
    # fractional weights: rounded once to 2^-e, e from the global sum
    g = torch.Generator().manual_seed(2)
    w = torch.rand(200, generator=g) * 1.5
    scale = G.weight_scale(w, None, _bsp())
    assert float(scale) == 2.0 ** np.floor(np.log2(2.0 ** 61 / float(w.double().sum())))
    u = G.round_weights(w, None, scale)
    assert int(u.sum()) <= 2 ** 61 + 200 and int(u.sum()) > 2 ** 60
    r = torch.randn(200, generator=g)
    _ref_against_definition(r, u, [(0, 120), (120, 200)], 0.25)


def test_select_two_ranks_on_the_cpu():
    """Rows split in two, histograms added between count and pick: the
    single-rank result, bit for bit."""
    G = _G()
    ridx, segs, label, at, w = Q.select_case(1000, 6, 8)
    r = (label - at)[ridx.long()]
    u = G.round_weights(w[ridx.long()], None, None)
    want, wempty = G.leaf_quantiles_ref(r, u, segs, 0.75)
    # rank A holds the even positions of every segment, rank B the odd ones
    parts = []
    for par in (0, 1):
        rr, uu, ss, pos = [], [], [], 0
        for b, e in segs:
            sel = torch.arange(b + par, e, 2) if e - b > par else torch.arange(0)
            rr.append(r[sel]), uu.append(u[sel])
            ss.append((pos, pos + sel.numel()))
            pos += sel.numel()
        parts.append((torch.cat(rr), torch.cat(uu), ss))
    both_r = torch.cat([parts[0][0], parts[1][0]])
    both_u = torch.cat([parts[0][1], parts[1][1]])
    off = parts[0][0].numel()
    # one process holds both halves as two segment lists, in lock step
    segs2 = parts[0][2] + [(b + off, e + off) for b, e in parts[1][2]]
    L = len(segs)

    def fold(h):  # the "allreduce": leaf l's bins = rank A's + rank B's
        s = h[:L] + h[L:]
        h[:L], h[L:] = s, s
    got, gempty = G.select_torch(both_r, both_u, segs2, 0.75, fold)
    assert torch.equal(got[:L].view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[L:].view(torch.int32), want.view(torch.int32))
    assert torch.equal(gempty[:L], wempty)


# --------------------------------------------- 2. gradients and the metric
@pytest.mark.parametrize("weighted", [False, True])
def test_gradient_pairs_and_metric(weighted):
    G = _G()
    g = torch.Generator().manual_seed(4 + weighted)
    n = 301
    label = torch.randn(n, generator=g)
    weight = torch.randint(0, 5, (n,), generator=g).float() if weighted else None
    margin = torch.randn(3, n, generator=g)
    margin[:, :7] = label[:7]  # d = 0: sign 0 / the d >= 0 side
    obj = G.make_objective("reg:absoluteerror")
    assert obj.n_group == 1 and obj.adaptive and obj.alphas == [0.5]
    assert obj.default_metric() == "mae"
    gp = obj.gpair(margin[0], label, weight)
    assert torch.equal(gp.double(), Q.gpair64(0.5, margin[0], label, weight, absolute=True))
    assert bool((gp[:7, 0] == 0).all())
    assert torch.equal(gp, G.obj_gpair_torch(G.OBJ_ABSOLUTE, margin[0], label, weight))
    p = G.GBDTParam()
    assert p.set("quantile_alpha", "[0.125, 0.5,0.75]") and p.quantile_alpha == [0.125, 0.5, 0.75]
    obj = G.make_objective("reg:quantileerror", 0, p)
    assert obj.n_group == 3 and obj.default_metric() == "quantile"
    gp = obj.gpair(margin, label, weight)
    assert gp.shape == (3, n, 2)
    for k, a in enumerate(Q.ALPHAS):
        assert torch.equal(gp[k].double(), Q.gpair64(a, margin[k], label, weight))
        assert torch.equal(gp[k], G.obj_gpair_torch(G.OBJ_QUANTILE, margin[k], label, weight,
                                                    alpha=a))
    bsp = _bsp()
    (v,) = obj.metrics(["quantile"], margin, label, weight, bsp)
    assert abs(v - Q.pinball64(Q.ALPHAS, margin, label, weight)) < 1e-12
    with pytest.raises(ValueError, match="quantile only"):
        obj.check_metrics(["mae"])
    # K = 1: the single-output metrics stay, quantile beside them
    p1 = G.GBDTParam()
    p1.set("quantile_alpha", "0.25")
    o1 = G.make_objective("reg:quantileerror", 0, p1)
    assert o1.n_group == 1
    v = o1.metrics(["mae", "quantile", "rmse"], margin[0], label, weight, bsp)
    assert abs(v[1] - Q.pinball64([0.25], margin[0], label, weight)) < 1e-12
    assert abs(v[0] - C.metric64("mae", margin[0], label, weight)[0]) < 1e-12
    with pytest.raises(ValueError, match="quantile does not fit"):
        G.make_objective("reg:absoluteerror").check_metrics(["quantile"])
    with pytest.raises(ValueError, match="must be finite"):
        o1.check_labels(torch.tensor([1.0, float("inf")]), bsp)
    with pytest.raises(ValueError, match="must be finite"):
        G.make_objective("reg:absoluteerror").check_labels(torch.tensor([float("nan")]), bsp)


def test_parameter_parsing():
    G = _G()
    p = G.GBDTParam()
    for text, want in (("0.5", [0.5]), ("[0.1,0.5,0.9]", [0.1, 0.5, 0.9]),
                       ("\"[0.9, 0.1, 0.9]\"", [0.9, 0.1, 0.9]), (" 0.25 , 0.75 ", [0.25, 0.75])):
        assert p.set("quantile_alpha", text) and p.quantile_alpha == want
    assert p.set("quantile_alpha", ",".join(["0.5"] * 64)) and len(p.quantile_alpha) == 64
    for text in ("0", "1", "[0.5,1.5]", "[]", "", "[0.5,,0.6]", "abc", "nan",
                 ",".join(["0.5"] * 65)):
        with pytest.raises(SystemExit, match="quantile_alpha"):
            p.set("quantile_alpha", text)
    q = G.GBDTParam()
    with pytest.raises(SystemExit, match="quantile_alpha"):
        G.make_objective("reg:quantileerror", 0, q)
    # any other objective accepts and ignores it
    q.set("quantile_alpha", "0.3")
    assert G.make_objective("reg:squarederror", 0, q).n_group == 1
    assert not G.make_objective("reg:squarederror", 0, q).adaptive


# ------------------------------------------------------------- 3. training
def _check_leaves(tree, X, r, u, alpha, eta, newton=None):
    """Every leaf of weight > 0 holds float32(eta x the definition's quantile
    of its rows' residuals); one without keeps the grower's value."""
    idx = tree.leaf_index(X)
    seen = 0
    for i in Q.leaves_of(tree):
        rows = idx == i
        q, W = Q.brute_quantile(r[rows].tolist(), u[rows].tolist(), alpha)
        if W == 0:
            continue
        seen += 1
        assert F32(tree.leaf[i]) == F32(eta * float(F32(q))), (i, tree.leaf[i], q)
    return seen


def test_absolute_error_leaves_are_lower_weighted_medians():
    G = _G()
    bsp = _bsp()
    X, y, w = Q.train_data()
    dm = Q.dmatrix(G, X, y, w, CPU)
    p = Q.param(G, "reg:absoluteerror")
    b, margin = Q.train(G, bsp, dm, p, 1)
    t = b.trees[0]
    assert len(Q.leaves_of(t)) == 8
    r = y - torch.tensor(0.5)  # one fp32 subtraction at base_score
    assert _check_leaves(t, X, r, w, 0.5, 1.0) == 8
    # the same structure with Newton leaves is no better on the training mae
    m0 = b.predict_margin(dm) * 0 + 0.5
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    builder = G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
    m1 = m0.clone()
    newton = builder.build(b.obj.gpair(m0, dm.label, dm.weight), m1)  # no refresh
    C.same_structure(newton, t)
    mae = b.obj.metrics(["mae"], margin, dm.label, dm.weight, bsp)[0]
    mae_newton = b.obj.metrics(["mae"], m1, dm.label, dm.weight, bsp)[0]
    print("mae refreshed %.6f newton %.6f" % (mae, mae_newton))
    assert mae <= mae_newton
    # base_weight, gain and cover keep the grower's values
    assert t.gain == newton.gain and t.cover == newton.cover
    # the margins hold the refreshed leaves
    assert torch.equal(margin, b.predict_margin(dm))


def test_quantile_error_coverage():
    """30 rounds on y = 3 x_0 + noise independent of x: the share of rows
    with y <= p_k is within 0.03 of alpha_k."""
    G = _G()
    X, y = Q.interval_data()
    dm = Q.dmatrix(G, X, y, None, CPU)
    p = Q.param(G, "reg:quantileerror", quantile_alpha="[0.125,0.5,0.75]", eta=0.5)
    b, margin = Q.train(G, _bsp(), dm, p, 30)
    assert len(b.trees) == 90 and margin.shape == (3, dm.n)
    for k, a in enumerate(Q.ALPHAS):
        share = float((y <= margin[k]).float().mean())
        print("alpha %.3f: share %.4f" % (a, share))
        assert abs(share - a) <= 0.03, (a, share)
    assert torch.allclose(margin, b.predict_margin(dm), atol=1e-5)


def test_pruned_leaf_holds_the_quantile_of_the_merged_rows():
    G = _G()
    X, y, w = Q.train_data()
    dm = Q.dmatrix(G, X, y, w, CPU)
    bsp = _bsp()
    free, _ = Q.train(G, bsp, dm, Q.param(G, "reg:quantileerror", quantile_alpha=0.25, max_depth=4),
                      1)
    gains = sorted(g for g, f in zip(free.trees[0].gain, free.trees[0].feat) if f >= 0)
    gamma = gains[len(gains) // 2]  # about half of the splits go
    p = Q.param(G, "reg:quantileerror", quantile_alpha=0.25, max_depth=4, gamma=gamma)
    b, margin = Q.train(G, bsp, dm, p, 1)
    t = b.trees[0]
    assert 1 < len(Q.leaves_of(t)) < len(Q.leaves_of(free.trees[0]))
    assert _check_leaves(t, X, y - torch.tensor(0.5), w, 0.25, 1.0) == len(Q.leaves_of(t))
    assert torch.equal(margin, b.predict_margin(dm))


def test_feature_sampling_and_interaction_constraints_compose():
    G = _G()
    X, y, w = Q.train_data()
    dm = Q.dmatrix(G, X, y, w, CPU)
    p = Q.param(G, "reg:quantileerror", quantile_alpha=0.75, max_depth=4, colsample_bytree=0.75,
                interaction_constraints="[[0,1],[2,3]]")
    b, margin = Q.train(G, _bsp(), dm, p, 2)
    t = b.trees[0]
    assert _check_leaves(t, X, y - torch.tensor(0.5), w, 0.75, 1.0) == len(Q.leaves_of(t)) > 2
    for tree in b.trees:  # a path stays within one group
        for i in Q.leaves_of(tree):
            used, a = set(), i
            while tree.parent[a] >= 0:
                a = tree.parent[a]
                used.add(tree.feat[a])
            assert used <= {0, 1} or used <= {2, 3}, used
    assert torch.equal(margin, b.predict_margin(dm))


def test_subsample_left_out_rows_do_not_move_the_leaf():
    G = _G()
    X, y, w = Q.train_data()
    dm = Q.dmatrix(G, X, y, w, CPU)
    p = Q.param(G, "reg:absoluteerror", subsample=0.5)
    b, _ = Q.train(G, _bsp(), dm, p, 1)
    keep = torch.rand(dm.n, generator=torch.Generator().manual_seed(p.seed + 17)) < 0.5
    t = b.trees[0]
    assert _check_leaves(t, X, y - torch.tensor(0.5), w * keep, 0.5, 1.0) == len(Q.leaves_of(t))
    # ... and they would have: with every row the medians differ somewhere
    with pytest.raises(AssertionError):
        _check_leaves(t, X, y - torch.tensor(0.5), w, 0.5, 1.0)


def test_dart_residuals_at_the_margin_without_the_dropped_rounds(monkeypatch):
    G = _G()
    X, y, w = Q.train_data()
    dm = Q.dmatrix(G, X, y, w, CPU)
    p = Q.param(G, "reg:absoluteerror", booster="dart", rate_drop=0.5, eta=0.5, seed=2)
    seen = []
    real = G.grow_round

    def spy(obj, builder, dmat, at, into, gen=None, fgen=None):
        at0 = at.clone()  # (gbtree rounds update `at` in place)
        new = real(obj, builder, dmat, at, into, gen, fgen)
        seen.append((at0, new[0]))
        return new
    monkeypatch.setattr(G, "grow_round", spy)
    b = G.Booster(p, dm.ncol)
    margin = b.predict_margin(dm)
    cuts = G.Cuts.build(dm, p.max_bin, _bsp())
    tb = G.make_builder(p, _bsp(), dm, cuts, cuts.bin(dm))
    dart = G.DartTrainer(b, tb, dm)
    gen, fgen = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
    dropped = 0
    for r in range(6):
        before_w = list(b.weights())
        dart.round(r, margin, gen, fgen)
        at, tree = seen[-1]
        drop = dart.history[-1][1]
        # `at` is the model so far without the dropped rounds
        want = torch.full((dm.n,), 0.5)
        for j in range(r):
            if j not in drop:
                want += F32(before_w[j]) * torch.tensor(b.trees[j].leaf, dtype=torch.float32)[
                    b.trees[j].leaf_index(X)]
        assert torch.allclose(at, want, atol=1e-5)
        dropped += bool(drop)
        # the new tree's leaves before the dart weight: quantiles of y - at
        assert _check_leaves(tree, X, y - at, w, 0.5, 0.5) == len(Q.leaves_of(tree))
    assert dropped >= 2
    assert torch.allclose(margin, b.predict_margin(dm), atol=1e-5)


def test_refused_combinations():
    G = _G()
    X, y, w = Q.train_data()
    dm = Q.dmatrix(G, X, y, w, CPU)
    for name, extra in (("reg:absoluteerror", {}), ("reg:quantileerror", {"quantile_alpha": 0.5})):
        for key, val, both in (("monotone_constraints", "(1,0)", "monotone_constraints"),
                               ("max_delta_step", "0.5", "max_delta_step")):
            p = Q.param(G, name, **extra, **{key: val})
            with pytest.raises(SystemExit, match=both) as e:
                Q.train(G, _bsp(), dm, p, 1)
            assert name in str(e.value)
        # all-zero constraints and max_delta_step = 0 are nothing to refuse
        p = Q.param(G, name, **extra, monotone_constraints="(0,0)", max_delta_step=0)
        Q.train(G, _bsp(), dm, p, 1)


# -------------------------------------------------------------- 4. the app
def run(args, cwd, timeout=300):
    env = dict(os.environ, WH_DEVICE="cpu")
    return subprocess.run([sys.executable, TRACKER] + args, cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=timeout)


QTRAIN = ["objective=reg:quantileerror", "quantile_alpha=[0.125,0.5,0.75]", "max_depth=3",
          "eta=0.5", "num_round=4", "eval_train=1", "data=train.libsvm"]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """600 rows of 6 integer features in 0..7 (the sketch is exact on any
    rank count), integer weights, a real label."""
    d = tmp_path_factory.mktemp("quantile")
    g = torch.Generator().manual_seed(6)
    X = torch.randint(0, 8, (600, 6), generator=g).float()
    y = (0.5 * X[:, 2] - 0.25 * X[:, 4] + torch.randn(600, generator=g)).float()
    w = torch.randint(0, 5, (600,), generator=g).float()
    C.write_libsvm(d / "train.libsvm", X, y, w)
    return d


@pytest.fixture(scope="module")
def trained(work):
    r = run(["-n", "1", XGB] + QTRAIN + ["model_out=one.model"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_app_train_pred_eval_dump(work, trained):
    G = _G()
    vals = [float(v) for v in re.findall(r"train-quantile:([0-9.]+)", trained.stdout)]
    assert len(vals) == 4 and all(b < a for a, b in zip(vals, vals[1:])), trained.stdout
    b = G.Booster.load(str(work / "one.model"), G.GBDTParam())
    assert len(b.trees) == 12 and b.obj.n_group == 3 and b.obj.alphas is None
    hdr = open(work / "one.model", "rb").read(64)
    assert b"reg:quantileerror|0.5|6|12|3" in hdr
    for extra, name in (([], "pred.txt"), (["pred_margin=1"], "margin.txt")):
        r = run(["-n", "1", XGB, "task=pred", "model_in=one.model", "test:data=train.libsvm",
                 "name_pred=" + name] + extra, work)
        assert r.returncode == 0, r.stderr[-2000:]
    pred = [float(v) for v in open(work / "pred.txt").read().split()]
    assert pred == [float(v) for v in open(work / "margin.txt").read().split()]
    assert len(pred) == 600 * 3  # n x K, row-major
    rows = torch.tensor(pred).view(600, 3)
    assert float((rows[:, 0] <= rows[:, 2]).float().mean()) > 0.95
    r = run(["-n", "1", XGB, "task=eval", "model_in=one.model", "test:data=train.libsvm",
             "quantile_alpha=[0.125,0.5,0.75]"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    ev = float(re.search(r"test-quantile:([0-9.]+)", r.stdout).group(1))
    assert abs(ev - vals[-1]) < 2e-6
    for bad in ([], ["quantile_alpha=[0.5,0.75]"]):  # none, or another count than the model's K
        r = run(["-n", "1", XGB, "task=eval", "model_in=one.model", "test:data=train.libsvm"] + bad,
                work)
        assert r.returncode != 0 and "quantile_alpha" in r.stderr
    r = run(["-n", "1", XGB, "task=pred", "model_in=one.model", "test:data=train.libsvm",
             "pred_leaf=1", "name_pred=leaf.txt"], work)
    assert r.returncode == 0 and len(open(work / "leaf.txt").read().split()) == 600 * 12
    r = run(["-n", "1", XGB, "task=dump", "model_in=one.model", "name_dump=dump.txt"], work)
    assert r.returncode == 0 and open(work / "dump.txt").read().count("booster[") == 12


def test_app_two_ranks_write_the_same_bytes(work, trained):
    r = run(["-n", "2", XGB] + QTRAIN + ["model_out=two.model"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(work / "two.model", "rb").read() == open(work / "one.model", "rb").read()
    assert re.findall(r"train-quantile:[0-9.]+", r.stdout) == re.findall(
        r"train-quantile:[0-9.]+", trained.stdout)
    # CSR rows on the CPU path: the same trees and leaves (its split search
    # takes the gains in fp32, so the stored gains differ in the last bits)
    r = run(["-n", "2", XGB] + QTRAIN + ["dsparse=1", "model_out=csr.model"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    G = _G()
    a = G.Booster.load(str(work / "one.model"), G.GBDTParam())
    b = G.Booster.load(str(work / "csr.model"), G.GBDTParam())
    assert a.dump() == b.dump()
    assert [t.leaf for t in a.trees] == [t.leaf for t in b.trees]


def test_app_model_in_continuation(work, trained):
    half = [a for a in QTRAIN if not a.startswith("num_round")]
    r = run(["-n", "1", XGB] + half + ["num_round=2", "model_out=half.model"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run(["-n", "1", XGB] + half + ["num_round=4", "model_in=half.model",
                                       "model_out=cont.model"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(work / "cont.model", "rb").read() == open(work / "one.model", "rb").read()
    r = run(["-n", "1", XGB, "objective=reg:quantileerror", "quantile_alpha=0.5", "num_round=3",
             "data=train.libsvm", "model_in=half.model", "model_out=x.model"], work)
    assert r.returncode != 0 and "quantile_alpha" in r.stderr


def test_app_absolute_error_and_checkpoints(work):
    args = ["objective=reg:absoluteerror", "max_depth=3", "num_round=4", "eval_train=1",
            "data=train.libsvm"]
    r = run(["-n", "1", XGB] + args + ["model_out=abs.model"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    mae = [float(v) for v in re.findall(r"train-mae:([0-9.]+)", r.stdout)]
    assert len(mae) == 4 and all(b < a for a, b in zip(mae, mae[1:]))
    env = dict(os.environ, WH_DEVICE="cpu", WH_CKPT_DIR=str(work / "ckpt"), WH_FAULT="die:1:3")
    rr = subprocess.run([sys.executable, TRACKER, "-n", "2", "--max-restart", "1", XGB] + args
                        + ["model_out=restart.model"], cwd=work, env=env, capture_output=True,
                        text=True, timeout=300)
    assert rr.returncode == 0, rr.stderr[-2000:]
    assert "restart from version=" in rr.stdout
    assert open(work / "restart.model", "rb").read() == open(work / "abs.model", "rb").read()


@pytest.mark.parametrize("args,names", [
    (["objective=reg:quantileerror", "quantile_alpha=[0.5,1.0]"], ["quantile_alpha"]),
    (["objective=reg:quantileerror"], ["quantile_alpha", "reg:quantileerror"]),
    (["objective=reg:absoluteerror", "monotone_constraints=(1,0)"],
     ["monotone_constraints", "reg:absoluteerror"]),
    (["objective=reg:quantileerror", "quantile_alpha=0.5", "max_delta_step=1"],
     ["max_delta_step", "reg:quantileerror"]),
])
def test_app_errors(work, args, names):
    r = run(["-n", "1", XGB, "data=train.libsvm", "num_round=1"] + args, work)
    assert r.returncode != 0
    for nm in names:
        assert nm in r.stderr, r.stderr[-2000:]


# --------------------------------------------------- 5. the plan self-test
def test_plan_test_binary():
    exe = os.path.join(ROOT, "bin", "native", "gbdt_quantile_plan_test")
    assert os.path.exists(exe), "native tools not built (python build_native.py)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_plan_test_binary_sanitized():
    b = subprocess.run([sys.executable, os.path.join(ROOT, "build_native.py"),
                        "--sanitize-quantile-plan"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    exe = b.stdout.strip().splitlines()[-1]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# --------------------------------------------------- 6. unchanged behaviour
def test_squarederror_model_bytes_are_unchanged(tmp_path):
    """The bytes of a reg:squarederror model (pruned, rows and features
    sampled) from before the adaptive objectives: the refresh hook does
    nothing when it is not asked for."""
    got = Q.squarederror_model(_G(), _bsp(), CPU, str(tmp_path / "m.model"))
    assert got == open(os.path.join(Q.GOLDEN, "gbdt_squarederror_cpu.model"), "rb").read()
