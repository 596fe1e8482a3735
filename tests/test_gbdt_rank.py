"""Learning to rank on the CPU (objective=rank:pairwise | rank:ndcg, metrics
ndcg / map): the task plan of the query groups, the plain-torch gradient and
metric paths against the definitions (docs/bsp_apps.md "Ranking") evaluated
pair by pair in fp64, the app with a <data>.group file, and two ranks whose
boundary cuts a group."""
import re

import pytest
import torch

import _gbdt_rank_cases as C


def G():
    from wormhole_amd.models import gbdt
    return gbdt


def hip():
    from wormhole_amd import _native
    return _native.hip()


# ------------------------------------------------------------------- plan
def test_plan_classes_and_order():
    cap = hip().gbdt_rank_lds_rows()
    assert cap >= 64 and cap * 16 <= 160 * 1024
    sizes = [0, 1, 2, 64, 65, cap, cap + 1, 0, 3]
    off = torch.tensor(C.offsets(sizes))
    small, block, tiled, rows, tiled_rows = hip().gbdt_rank_plan(off, int(off[-1]))
    assert small.dtype == block.dtype == tiled.dtype == torch.int32
    assert small.tolist() == [3, 8, 2, 1]  # 64, 3, 2, 1 rows: larger first
    assert block.tolist() == [5, 4]  # cap, 65
    assert tiled.tolist() == [6]
    assert rows == cap and tiled_rows == cap + 1
    every = small.tolist() + block.tolist() + tiled.tolist()
    assert sorted(every) == [q for q, s in enumerate(sizes) if s > 0]
    # another capacity moves the class boundary with it
    _, block, tiled, rows, tiled_rows = hip().gbdt_rank_plan(off, int(off[-1]), lds_rows=64)
    assert block.tolist() == [] and tiled.tolist() == [6, 5, 4] and (rows, tiled_rows) == (0, cap + 1)


@pytest.mark.parametrize("off,n", [
    ([], 0),  # empty input
    ([1, 3], 3),  # a first offset other than 0
    ([0, 4, 2, 6], 6),  # a decrease
    ([0, 2, 5], 6),  # a last offset other than n
    ([0, 2 ** 31], 2 ** 31),  # n above INT32_MAX
])
def test_plan_refuses_malformed_offsets(off, n):
    with pytest.raises(ValueError):
        hip().gbdt_rank_plan(torch.tensor(off, dtype=torch.int64), n)


def test_groups_of_a_matrix():
    g = G()
    X = torch.zeros(6, 2)
    dm = g.DMatrix.from_dense(X, torch.zeros(6), torch.device("cpu"), group=[0, 2, 2, 6])
    assert dm.group.dtype == torch.int32 and dm.group.tolist() == [0, 2, 2, 6]
    assert dm.rank_groups() is dm.rank_groups() and dm.rank_groups().num_group == 3
    assert g.DMatrix.from_dense(X, torch.zeros(6), torch.device("cpu")).group is None
    with pytest.raises(ValueError):  # the last offset is not the matrix's row count
        g.DMatrix.from_dense(X, torch.zeros(6), torch.device("cpu"), group=[0, 2, 5])
    keys, offs = torch.zeros(0, dtype=torch.int64), torch.zeros(7, dtype=torch.int64)
    for sparse in (False, True):
        d = g.make_dmatrix(keys, offs, None, torch.zeros(6), None, 2, torch.device("cpu"),
                           sparse=sparse, group=torch.tensor([0, 6]))
        assert d.group.tolist() == [0, 6]
        assert g.make_dmatrix(keys, offs, None, torch.zeros(6), None, 2, torch.device("cpu"),
                              sparse=sparse).group is None


# ------------------------------------------------------------ torch paths
@pytest.mark.parametrize("ndcg", [False, True])
def test_worked_pin(ndcg):
    g = G()
    m, y = torch.tensor(C.PIN_M), torch.tensor(C.PIN_Y)
    assert C.ranks(C.PIN_M) == C.PIN_R
    want_g, want_h = C.PIN[ndcg]
    naive = C.naive_gpair(m, y, [0, 5], ndcg)
    for dt in (torch.float32, torch.float64):
        gp = g.rank_gpair_torch(m.to(dt), y.to(dt), [0, 5], ndcg)
        assert gp.dtype == dt and gp.shape == (5, 2)
        assert (gp[:, 0].double() - torch.tensor(want_g, dtype=torch.float64)).abs().max() <= 2e-6
        assert (gp[:, 1].double() - torch.tensor(want_h, dtype=torch.float64)).abs().max() <= 2e-6
        assert abs(float(gp[:, 0].double().sum())) <= 2e-6
    assert (g.rank_gpair_torch(m.double(), y.double(), [0, 5], ndcg) - naive).abs().max() <= 1e-12
    # through the objective (CPU tensors: the torch path), fp32 [n, 2]
    obj = g.Objective("rank:ndcg" if ndcg else "rank:pairwise")
    got = obj.gpair(m, y, None, torch.tensor([0, 5]))
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert (got[:, 0].double() - torch.tensor(want_g, dtype=torch.float64)).abs().max() <= 2e-6
    lr = C.ranks(C.PIN_Y)
    idcg = sum((2 ** v - 1) / torch.log2(torch.tensor(2.0 + r, dtype=torch.float64))
               for v, r in zip(C.PIN_Y, lr))
    assert abs(float(idcg) - C.PIN_IDCG) <= 2e-6


def random_groups(seed, sizes, tie=False):
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    m = torch.randn(n, generator=g) * 3
    if tie:
        m = (m * 2).round() / 2  # many exact ties
    y = torch.randint(0, 5, (n,), generator=g).float()
    return m, y, C.offsets(sizes)


@pytest.mark.parametrize("ndcg", [False, True])
@pytest.mark.parametrize("tie", [False, True])
def test_torch_path_matches_the_double_loop(ndcg, tie):
    """Random groups, sizes 0..70 so that several padded batches form, with a
    small batch budget so that rows are chunked too."""
    g = G()
    sizes = [0, 1, 2, 3, 70, 0, 17, 33, 64, 65, 5, 5, 8, 0]
    m, y, off = random_groups(5 + tie, sizes, tie)
    ref = C.naive_gpair(m, y, off, ndcg)
    for budget in (1 << 22, 300):
        got = g.rank_gpair_torch(m.double(), y.double(), off, ndcg, budget=budget)
        scale = ref.abs().max()
        assert (got - ref).abs().max() <= 1e-12 * scale
        # sum g = 0 in every group
        for a, b in zip(off[:-1], off[1:]):
            assert abs(float(got[a:b, 0].sum())) <= 1e-12 * (b - a + 1)
    # fp32 per-pair terms, fp64 row sums: only the per-pair rounding is left
    f32, mass = g.rank_gpair_torch(m, y, off, ndcg, mass=True)
    assert f32.dtype == torch.float32
    # a pair's fp32 terms are a few roundings (2^-24 each) off; ndcg: the fp32
    # difference of two discounts is 2^-24 x discount / |difference| off, at
    # ranks 69 and 70: 6e-8 x 0.16 / 5e-4 = 2e-5
    rel = 1e-4 if ndcg else 2e-6
    assert bool(((f32[:, 0].double() - ref[:, 0]).abs() <= rel * mass + 1e-12).all())
    assert bool(((f32[:, 1].double() - ref[:, 1]).abs() <= rel * ref[:, 1] + 1e-12).all())


@pytest.mark.parametrize("ndcg", [False, True])
def test_exact_cases(ndcg):
    g = G()
    zero = torch.zeros(4, 2)
    # all labels equal: no partner anywhere
    assert torch.equal(g.rank_gpair_torch(torch.tensor([1.0, -2, 3, 0]), torch.full((4,), 2.0),
                                          [0, 4], ndcg), zero)
    # single-row groups
    assert torch.equal(g.rank_gpair_torch(torch.tensor([1.0, -2, 3, 0]),
                                          torch.tensor([0.0, 1, 2, 3]), [0, 1, 2, 3, 4], ndcg), zero)
    # no rows, no groups
    assert g.rank_gpair_torch(torch.zeros(0), torch.zeros(0), [0], ndcg).shape == (0, 2)
    assert g.rank_gpair_torch(torch.zeros(0), torch.zeros(0), [0, 0, 0], ndcg).shape == (0, 2)
    # tied margins rank by row index: equal to the double loop, which says so
    m, y = torch.zeros(6), torch.tensor([0.0, 2, 1, 2, 0, 4])
    assert C.ranks(m.tolist()) == [0, 1, 2, 3, 4, 5]
    got = g.rank_gpair_torch(m.double(), y.double(), [0, 6], ndcg)
    assert (got - C.naive_gpair(m, y, [0, 6], ndcg)).abs().max() <= 1e-15
    if ndcg:
        # IDCG = 0 (every label 0) in the first group only
        got = g.rank_gpair_torch(torch.tensor([1.0, 2, 0.5, 0.1]), torch.tensor([0.0, 0, 1, 0]),
                                 [0, 2, 4], True)
        assert torch.equal(got[:2], torch.zeros(2, 2)) and bool((got[2:, 1] > 0).all())


def test_objective_surface():
    g = G()
    for name in g.RANK_OBJECTIVES:
        obj = g.Objective(name)
        assert obj.rank and obj.n_group == 1 and obj.default_metric() == "map"
        assert obj.prob_to_margin(0.5) == 0.5
        m = torch.tensor([0.3, -1.0])
        assert torch.equal(obj.pred(m), m)
        with pytest.raises(ValueError, match="group"):
            obj.gpair(m, torch.tensor([1.0, 0.0]), None)
        with pytest.raises(ValueError, match="weight"):
            obj.gpair(m, torch.tensor([1.0, 0.0]), torch.ones(2), torch.tensor([0, 2]))
        obj.check_metrics(["ndcg", "ndcg@10", "map@3-", "ndcg-", "rmse", "auc"])
        with pytest.raises(ValueError):
            obj.check_metrics(["ndcg@"])
        with pytest.raises(ValueError):
            obj.check_metrics(["merror"])
    # rank metrics go with any single-output objective, not with multi-class
    g.Objective("binary:logistic").check_metrics(["map@5", "error"])
    with pytest.raises(ValueError):
        g.Objective("multi:softmax", 3).check_metrics(["ndcg"])
    assert g.parse_rank_metric("ndcg@10-") == ("ndcg", 10, True)
    assert g.parse_rank_metric("map") == ("map", 0, False)
    assert g.parse_rank_metric("mapx") is None and g.parse_rank_metric("ndcg@-") is None


# ---------------------------------------------------------------- metrics
def test_metrics_by_hand():
    """Six rows; by prediction the order is rows 2, 0, 5, 1, 4, 3 (rows 0 and
    5 tie: the earlier row first), their labels 0, 3, 1, 0, 2, 0."""
    g = G()
    m = torch.tensor([2.0, 0.5, 3.0, -1.0, 0.0, 2.0])
    y = torch.tensor([3.0, 0.0, 0.0, 0.0, 2.0, 1.0])
    assert C.ranks(m.tolist()) == [1, 3, 0, 5, 4, 2]
    import math
    # ndcg@2: DCG = 0 / log2(2) + 7 / log2(3); ideal = 7 / log2(2) + 3 / log2(3)
    ndcg2 = (7 / math.log2(3)) / (7 + 3 / math.log2(3))
    # map@3: hits at ranks 1 and 2 (rows 0 and 5), three hits in the group
    map3 = (1 / 2 + 2 / 3) / 3
    # map: the third hit (row 4) is at rank 4
    map_all = (1 / 2 + 2 / 3 + 3 / 5) / 3
    off = [0, 6]
    for dt in (torch.float32, torch.float64):
        md, yd = m.to(dt), y.to(dt)
        assert abs(float(g.rank_eval_torch(md, yd, off, "ndcg", 2)) - ndcg2) <= 1e-12
        assert abs(float(g.rank_eval_torch(md, yd, off, "map", 3)) - map3) <= 1e-12
        assert abs(float(g.rank_eval_torch(md, yd, off, "map")) - map_all) <= 1e-12
        assert abs(float(g.rank_eval_torch(md, yd, off, "ndcg", 2, minus=True)) - ndcg2) <= 1e-12
    for kind, k in (("ndcg", 0), ("ndcg", 2), ("map", 0), ("map", 3)):
        assert abs(float(g.rank_eval_torch(m, y, off, kind, k)) -
                   C.naive_eval(m.tolist(), y.tolist(), kind, k)) <= 1e-12
    # a group without a hit: exactly 1, or 0 with '-'; an empty group: NaN
    z = torch.zeros(3)
    v = g.rank_eval_torch(torch.tensor([1.0, 2, 3]), z, [0, 0, 3], "map", 0, False)
    assert torch.isnan(v[0]) and float(v[1]) == 1.0
    for kind in ("ndcg", "map"):
        assert float(g.rank_eval_torch(torch.tensor([1.0, 2, 3]), z, [0, 3], kind, 2, True)) == 0.0
        assert float(g.rank_eval_torch(torch.tensor([1.0, 2, 3]), z, [0, 3], kind, 2)) == 1.0
    # a perfect order scores 1 (margins = labels, ties among equal labels)
    gen = torch.Generator().manual_seed(2)
    yy = torch.randint(0, 5, (50,), generator=gen).float()
    # (map@k divides by the hits of the whole group: 1 only without a cut-off)
    for kind, k in (("ndcg", 0), ("ndcg", 10), ("map", 0)):
        v = g.rank_eval_torch(yy.clone(), yy, [0, 20, 50], kind, k)
        assert bool(((v - 1.0).abs() <= 1e-12).all()), (kind, k, v)


def test_global_metric_is_the_mean_over_nonempty_groups():
    g = G()
    from wormhole_amd.parallel.bsp import BSP
    bsp = BSP(torch.device("cpu"))
    m, y, off = random_groups(9, [4, 0, 7, 9])
    obj = g.Objective("rank:pairwise")
    names = ["ndcg", "ndcg@3-", "map", "map@2", "rmse"]
    vals = obj.metrics(names, m, y, None, bsp, torch.tensor(off))
    for name, v in zip(names[:4], vals):
        kind, k, minus = g.parse_rank_metric(name)
        per = [C.naive_eval(m[a:b].tolist(), y[a:b].tolist(), kind, k, minus)
               for a, b in zip(off[:-1], off[1:]) if b > a]
        assert abs(v - sum(per) / 3) <= 1e-12
    assert abs(vals[4] - float(((m - y) ** 2).mean().sqrt())) <= 1e-6
    with pytest.raises(ValueError, match="group"):
        obj.metrics(["ndcg"], m, y, None, bsp)
    with pytest.raises(ValueError, match="group"):
        g.Objective("binary:logistic").metrics(["map"], m, y, None, bsp)


def test_boost_round_takes_the_matrix_groups():
    """CPU growers, dense and CSR: a round with rank:pairwise equals building
    on the torch path's pairs by hand."""
    g = G()
    from wormhole_amd.parallel.bsp import BSP
    bsp = BSP(torch.device("cpu"))
    X, y, sizes = C.app_data(ngroup=12)
    off = torch.tensor(C.offsets(sizes))
    dm = g.DMatrix.from_dense(X, y, torch.device("cpu"), group=off)
    p = g.GBDTParam()
    p.objective, p.max_depth, p.min_child_weight = "rank:pairwise", 3, 0.0
    obj = g.Objective(p.objective)
    cuts = g.Cuts.build(dm, p.max_bin, bsp)
    dumps = []
    for hand in (False, True):
        b = g.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
        margin = torch.zeros(dm.n)
        if hand:
            tree = b.build(g.rank_gpair_torch(margin, y, off, False), margin)
        else:
            tree = g.boost_round(obj, b, dm, margin)[0]
        dumps.append((tree.dump(with_stats=True), margin.clone()))
    assert dumps[0][0] == dumps[1][0] and torch.equal(dumps[0][1], dumps[1][1])
    assert "leaf" in dumps[0][0] and float(dumps[0][1].abs().max()) > 0


# -------------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("rank")
    X, y, sizes = C.app_data()
    C.write_libsvm(d / "train.txt", X, y)
    C.write_group(d / "train.txt.group", sizes)
    C.write_libsvm(d / "nogroup.txt", X, y)
    return d


@pytest.fixture(scope="module")
def trained(work):
    out = {}
    for name in ("rank:pairwise", "rank:ndcg"):
        r = C.run_app(["objective=" + name, "data=train.txt", "eval[test]=train.txt",
                       "eval_metric=ndcg@10-", "model_out=%s.model" % name[5:]] + C.APP_ARGS, work)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = r.stdout
    return out


@pytest.mark.parametrize("name", ["rank:pairwise", "rank:ndcg"])
def test_cli_train_learns_the_order(trained, name):
    """The CPU path reaches the thresholds within APP_ROUNDS (the GPU test
    holds the kernels to the same), from below them at round 0."""
    out = trained[name]
    last = C.APP_ROUNDS - 1
    for metric in ("train-ndcg", "train-map"):
        v = C.metric_lines(out, metric)
        assert sorted(v) == list(range(C.APP_ROUNDS)), out
        print(name, metric, "round 0 %.6f, last %.6f" % (v[0], v[last]))
        assert v[last] >= C.APP_THRESHOLD and v[0] < C.APP_THRESHOLD, (metric, v)
    # the metric's name is echoed exactly as given, for every set
    assert re.search(r"^\[0\]\ttest-ndcg@10-:\d\.\d{6}\ttest-ndcg:\d\.\d{6}\ttest-map:\d\.\d{6}"
                     r"\ttrain-ndcg@10-:\d\.\d{6}\ttrain-ndcg:\d\.\d{6}\ttrain-map:\d\.\d{6}$",
                     out, re.M), out
    # the same rows as eval set and as training set: the same values
    assert C.metric_lines(out, "test-ndcg@10-") == C.metric_lines(out, "train-ndcg@10-")


def test_cli_eval_and_pred(work, trained):
    r = C.run_app(["task=eval", "model_in=pairwise.model", "test:data=train.txt",
                   "objective=rank:pairwise", "eval_metric=ndcg@10-", "eval_metric=map@3"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"^test-ndcg@10-:(\d\.\d{6})\ttest-map@3:(\d\.\d{6})$", r.stdout, re.M)
    assert m, r.stdout
    last = C.metric_lines(trained["rank:pairwise"], "train-ndcg@10-")[C.APP_ROUNDS - 1]
    assert abs(float(m.group(1)) - last) <= 1e-6
    # ntree_limit=1: the model after round 0
    r1 = C.run_app(["task=eval", "model_in=pairwise.model", "test:data=train.txt",
                    "objective=rank:pairwise", "eval_metric=ndcg", "ntree_limit=1"], work)
    assert r1.returncode == 0, r1.stderr[-2000:]
    first = C.metric_lines(trained["rank:pairwise"], "train-ndcg")[0]
    assert abs(float(re.search(r"test-ndcg:(\S+)", r1.stdout).group(1)) - first) <= 1e-6
    # the default metric of a rank objective is map
    rd = C.run_app(["task=eval", "model_in=pairwise.model", "test:data=train.txt",
                    "objective=rank:pairwise"], work)
    assert rd.returncode == 0 and re.search(r"^test-map:\d", rd.stdout, re.M), rd.stdout
    # task=pred needs no group file; the prediction is the margin
    rp = C.run_app(["task=pred", "model_in=pairwise.model", "test:data=nogroup.txt",
                    "objective=rank:pairwise", "name_pred=pred.txt"], work)
    assert rp.returncode == 0, rp.stderr[-2000:]
    rm = C.run_app(["task=pred", "model_in=pairwise.model", "test:data=nogroup.txt",
                    "objective=rank:pairwise", "name_pred=margin.txt", "pred_margin=1"], work)
    assert rm.returncode == 0, rm.stderr[-2000:]
    pred = [float(x) for x in open(work / "pred.txt")]
    X, y, sizes = C.app_data()
    assert len(pred) == len(y) and pred == [float(x) for x in open(work / "margin.txt")]
    got = G().rank_eval_torch(torch.tensor(pred, dtype=torch.float64), y.double(),
                              C.offsets(sizes), "ndcg", 10, True)
    assert abs(float(got.mean()) - last) <= 1e-4  # (%g predictions: ties may move)


def test_cli_refusals(work, trained):
    X, y, sizes = C.app_data()
    base = ["objective=rank:pairwise", "num_round=1", "max_depth=2"]
    # a group file whose sizes do not sum to the rows: both numbers are named
    C.write_libsvm(work / "short.txt", X, y)
    C.write_group(work / "short.txt.group", sizes[:-1])
    r = C.run_app(base + ["data=short.txt"], work)
    assert r.returncode != 0
    assert "%d" % (len(y) - sizes[-1]) in r.stderr and "%d rows" % len(y) in r.stderr, r.stderr
    # instance weights with a rank objective
    C.write_libsvm(work / "weighted.txt", X, y, weight=[1.5] * len(y))
    C.write_group(work / "weighted.txt.group", sizes)
    r = C.run_app(base + ["data=weighted.txt"], work)
    assert r.returncode != 0 and "instance weights are not defined" in r.stderr, r.stderr
    # a rank objective, or a rank metric, without a group file
    r = C.run_app(base + ["data=nogroup.txt"], work)
    assert r.returncode != 0 and "nogroup.txt.group" in r.stderr, r.stderr
    r = C.run_app(["objective=binary:logistic", "num_round=1", "data=nogroup.txt",
                   "eval_train=1", "eval_metric=ndcg@5"], work)
    assert r.returncode != 0 and "eval_metric ndcg@5 needs query groups" in r.stderr, r.stderr
    r = C.run_app(["task=eval", "model_in=pairwise.model", "test:data=nogroup.txt",
                   "objective=rank:pairwise", "eval_metric=map"], work)
    assert r.returncode != 0 and "nogroup.txt.group" in r.stderr, r.stderr
    # a malformed line
    C.write_libsvm(work / "bad.txt", X, y)
    with open(work / "bad.txt.group", "w") as f:
        f.write("12\nten\n")
    r = C.run_app(base + ["data=bad.txt"], work)
    assert r.returncode != 0 and "bad.txt.group" in r.stderr, r.stderr


def test_two_ranks_cut_a_group(work, trained):
    """Two ranks read consecutive halves of the file; the group the boundary
    cuts becomes two groups. The 2-rank ndcg is the 1-rank value of a group
    file in which that group is split by hand at the boundary."""
    from wormhole_amd import _native
    X, y, sizes = C.app_data()
    n0 = _native.host().load_split(str(work / "train.txt"), 0, 2, "libsvm")[3].numel()
    off = C.offsets(sizes)
    assert 0 < n0 < len(y) and n0 not in off, "the boundary must fall inside a group"
    q = max(i for i, o in enumerate(off) if o < n0)
    C.write_libsvm(work / "cut.txt", X, y)
    C.write_group(work / "cut.txt.group", sizes[:q] + [n0 - off[q], off[q + 1] - n0] + sizes[q + 1:])
    args = ["task=eval", "model_in=pairwise.model", "objective=rank:pairwise", "ntree_limit=2",
            "eval_metric=ndcg", "eval_metric=map@4-"]
    two = C.run_app(args + ["test:data=train.txt"], work, nproc=2)
    assert two.returncode == 0, two.stderr[-2000:]
    one = C.run_app(args + ["test:data=cut.txt"], work)
    assert one.returncode == 0, one.stderr[-2000:]
    whole = C.run_app(args + ["test:data=train.txt"], work)
    pat = r"^test-ndcg:(\d\.\d{6})\ttest-map@4-:(\d\.\d{6})$"
    a, b, c = (re.search(pat, r.stdout, re.M) for r in (two, one, whole))
    assert a and b and c, (two.stdout, one.stdout)
    assert a.groups() == b.groups()
    assert a.groups() != c.groups()  # (the cut does change the value)
    # training with two ranks runs and learns (each rank ranks its own groups)
    r = C.run_app(["objective=rank:pairwise", "data=train.txt", "model_out=two.model"] + C.APP_ARGS,
                  work, nproc=2)
    assert r.returncode == 0, r.stderr[-2000:]
    v = C.metric_lines(r.stdout, "train-ndcg")
    assert v[C.APP_ROUNDS - 1] >= C.APP_THRESHOLD > v[0], v
