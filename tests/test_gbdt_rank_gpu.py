"""Learning to rank on the GPU: the gradient and evaluation kernels
(csrc/hip/gbdt_rank.hip) against the definitions evaluated in fp64, the
plumbing through the dense and CSR growers, and the app end to end.

Element tolerance of the kernels (the rule of test_gbdt_multiclass_gpu.py):
the fp32 plain-torch fallback (``rank_gpair_torch``, the CPU path) is measured
against the same formulas in fp64 on the same input; the kernel may be at most
4x as far off as the fallback's largest error, with a floor of 1e-6 x the
row's fp64 sum of W |lambda| (g) or 2 W eta (h, which is the reference's h
itself). The bound comes from the fallback, never from the kernel."""
import functools

import pytest
import torch

import _gbdt_rank_cases as C

pytestmark = pytest.mark.gpu
VARIANTS = ("normal", "wide", "equal")


def dev():
    return torch.device("cuda", 0)


def hip():
    from wormhole_amd import _native
    return _native.hip()


def G():
    from wormhole_amd.models import gbdt
    return gbdt


def cap():
    return hip().gbdt_rank_lds_rows()


def group_sizes(case):
    """One group of the sizes at which the kernels change path (a wavefront's
    64 rows, a block's 256 threads, the LDS rows C: resident / tiled, and a
    third, partial tile), or "many": 20 000 groups of 0..40 rows, more than
    one pass of the wave-per-group grid (2048 blocks x 4 waves), with empty
    groups in the middle and at both ends."""
    if case == "many":
        g = torch.Generator().manual_seed(4)
        sizes = torch.randint(0, 41, (20_000,), generator=g)
        sizes[0] = sizes[-1] = sizes[9_999] = sizes[10_000] = 0
        return sizes.tolist()
    c = cap()
    return [{"C": c, "C+1": c + 1, "2C+3": 2 * c + 3}.get(case) or int(case)]


CASES = ["1", "2", "63", "64", "65", "255", "256", "257", "C", "C+1", "2C+3", "many"]


@functools.lru_cache(maxsize=None)
def inputs(case, variant):
    """(margin, label fp32 on the GPU, offsets list). normal: margins N(0, 3),
    grades 0..4; wide: margins over +-80 with exact ties (rounded to 1/2, and
    exact +-80 entries), the first group of two or more rows fully tied;
    equal: all labels 2."""
    sizes = group_sizes(case)
    off = C.offsets(sizes)
    n = off[-1]
    g = torch.Generator().manual_seed(len(case) * 131 + sum(map(ord, case)) + VARIANTS.index(variant))
    if variant == "wide":
        m = ((torch.rand(n, generator=g) * 160 - 80) * 2).round() / 2
        m[torch.rand(n, generator=g) < 0.1] = 80.0
        m[torch.rand(n, generator=g) < 0.1] = -80.0
        for a, b in zip(off[:-1], off[1:]):
            if b - a >= 2:
                m[a:b] = 1.25
                break
    else:
        m = torch.randn(n, generator=g) * 3
    y = torch.randint(0, 5, (n,), generator=g).float()
    if variant == "equal":
        y = torch.full((n,), 2.0)
    return m.to(dev()), y.to(dev()), off


@functools.lru_cache(maxsize=None)
def plan(case):
    off = torch.tensor(group_sizes(case)).cumsum(0)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), off])
    small, block, tiled, rows, tiled_rows = hip().gbdt_rank_plan(off, int(off[-1]))
    d = dev()
    return off.to(torch.int32).to(d), small.to(d), block.to(d), tiled.to(d), rows, tiled_rows


def run_gpair(case, m, y, ndcg, flip=False):
    off, small, block, tiled, rows, tiled_rows = plan(case)
    if flip:  # another order of every task list
        small, block, tiled = (t.flip(0).contiguous() for t in (small, block, tiled))
    return hip().gbdt_gpair_rank(margin=m, label=y, group_off=off, small=small, block=block,
                                 tiled=tiled, block_rows=rows, tiled_rows=tiled_rows, ndcg=ndcg)


@pytest.mark.parametrize("ndcg", [False, True], ids=["pairwise", "ndcg"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", CASES)
def test_gpair_rank_kernel(case, variant, ndcg):
    g = G()
    m, y, off = inputs(case, variant)
    n = off[-1]
    ref, mass = g.rank_gpair_torch(m.double(), y.double(), off, ndcg, mass=True)  # fp64
    fb = g.rank_gpair_torch(m, y, off, ndcg)  # the fp32 fallback
    assert fb.dtype == torch.float32 and ref.dtype == torch.float64
    gp, st = run_gpair(case, m, y, ndcg)
    gp2, st2 = run_gpair(case, m, y, ndcg)
    gp3, st3 = run_gpair(case, m, y, ndcg, flip=True)
    assert gp.shape == (n, 2) and gp.dtype == torch.float32
    assert st.shape == (4,) and st.dtype == torch.float64
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(st).all())
    e_fb = (fb.double() - ref).abs().amax(0)  # the fallback's largest error {g, h}
    floor = torch.stack([1e-6 * mass, 1e-6 * ref[:, 1]], 1)
    tol = torch.maximum(4 * e_fb[None, :].expand_as(floor), floor)
    err = (gp.double() - ref).abs()
    print("%s %s ndcg=%d: fallback max err g %.3g h %.3g, kernel max err g %.3g h %.3g" % (
        case, variant, ndcg, float(e_fb[0]), float(e_fb[1]), float(err[:, 0].max()),
        float(err[:, 1].max())))
    assert bool((err <= tol).all()), (err.amax(0), e_fb)
    if variant == "equal":  # no partner anywhere
        assert not bool(gp.any()) and not bool(st.any())
    # root statistics: fp64 sums of the kernel's own outputs, exact maxima
    own = gp.double()
    assert bool(((st[:2] - own.sum(0)).abs() <= 1e-12 * own.abs().sum(0)).all()), (st, own.sum(0))
    assert torch.equal(st[2:], own.abs().amax(0))
    # the same bits on every run, and for any order of the task lists
    assert torch.equal(gp, gp2) and torch.equal(st, st2)
    assert torch.equal(gp, gp3) and torch.equal(st, st3)
    # sum g = 0 within the rounding of the rows: sum of |g| x 2^-24
    assert abs(float(own[:, 0].sum())) <= 2.0 ** -23 * float(own[:, 0].abs().sum()) + 1e-30


def test_objective_hands_the_kernels_output_with_its_stats():
    g = G()
    m, y, off = inputs("many", "normal")
    groups = g.RankGroups(torch.tensor(off))
    for name, ndcg in (("rank:pairwise", False), ("rank:ndcg", True)):
        got = g.Objective(name).gpair(m, y, None, groups)
        gp, st = run_gpair("many", m, y, ndcg)
        assert torch.equal(got, gp)
        s, mx = g.gpair_stats(got)  # (no torch reduction: the kernel's statistics)
        assert torch.equal(s, st[:2]) and torch.equal(mx, st[2:].float())
    # plain offsets work too (a plan per call)
    assert torch.equal(g.Objective("rank:pairwise").gpair(m, y, None, torch.tensor(off)),
                       run_gpair("many", m, y, False)[0])


def test_no_rows():
    d = dev()
    z = torch.zeros(0, device=d)
    e = torch.zeros(0, dtype=torch.int32, device=d)
    for off in ([0], [0, 0, 0]):
        o = torch.tensor(off, dtype=torch.int32, device=d)
        gp, st = hip().gbdt_gpair_rank(margin=z, label=z, group_off=o, small=e, block=e, tiled=e,
                                       block_rows=0, tiled_rows=0, ndcg=True)
        assert gp.shape == (0, 2) and torch.equal(st.cpu(), torch.zeros(4, dtype=torch.float64))
        v = hip().gbdt_rank_eval(margin=z, label=z, group_off=o, small=e, block=e, tiled=e,
                                 block_rows=0, tiled_rows=0, kind=0, k=0, minus=False)
        assert v.shape == (len(off) - 1,) and bool(torch.isnan(v).all())
    g = G()
    assert g.Objective("rank:ndcg").gpair(z, z, None, torch.tensor([0])).shape == (0, 2)


EVAL_NAMES = ["ndcg", "ndcg@1", "ndcg@10", "map", "map@5", "ndcg-", "ndcg@1-", "ndcg@10-", "map-",
              "map@5-"]


@pytest.mark.parametrize("variant", ["normal", "wide"])
@pytest.mark.parametrize("case", ["2", "64", "65", "257", "C", "C+1", "2C+3", "many"])
def test_rank_eval_kernel(case, variant):
    """Per-group values against rank_eval_torch in fp64. The fallback is the
    same counting on the fp32 inputs (exact comparisons) with fp64 terms, so
    its own error is 0 or a few fp64 roundings; the floor is 1e-12: a group's
    value is a ratio of two sums of at most 2C + 3 fp64 terms, each a few
    2^-53 off."""
    g = G()
    m, y, off = inputs(case, variant)
    o, small, block, tiled, rows, tiled_rows = plan(case)
    sizes = torch.tensor(off[1:]) - torch.tensor(off[:-1])
    yc = y.cpu()
    offs = torch.tensor(off)
    cum = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum((yc > 0).long(), 0)])
    nohit = (sizes > 0) & ((cum[offs[1:]] - cum[offs[:-1]]) == 0)
    if case == "many":
        assert int(nohit.sum()) > 10
    for name in EVAL_NAMES:
        kind, k, minus = g.parse_rank_metric(name)
        ref = g.rank_eval_torch(m.double(), y.double(), off, kind, k, minus)
        fb = g.rank_eval_torch(m, y, off, kind, k, minus)
        got = hip().gbdt_rank_eval(margin=m, label=y, group_off=o, small=small, block=block,
                                   tiled=tiled, block_rows=rows, tiled_rows=tiled_rows,
                                   kind=0 if kind == "ndcg" else 1,
                                   k=k, minus=minus)
        assert got.dtype == torch.float64 and got.shape == ref.shape
        assert torch.equal(torch.isnan(got).cpu(), sizes == 0)
        assert torch.equal(torch.isnan(ref).cpu(), sizes == 0)
        ok = ~torch.isnan(ref)
        e_fb = float((fb - ref)[ok].abs().max())
        err = float((got - ref)[ok].abs().max())
        print("%s %s %s: fallback max err %.3g, kernel max err %.3g" % (case, variant, name, e_fb, err))
        assert err <= max(4 * e_fb, 1e-12), (name, err, e_fb)
        assert torch.equal(got[ok], g.rank_eval(m, y, g.RankGroups(torch.tensor(off)), kind, k,
                                                minus)[ok])
        # groups without a hit take exactly 1, or 0 with '-'
        assert bool((got.cpu()[nohit] == (0.0 if minus else 1.0)).all())


def test_global_metric_on_the_gpu():
    g = G()
    from wormhole_amd.parallel.bsp import BSP
    m, y, off = inputs("many", "normal")
    names = ["ndcg@10", "map@5-", "rmse"]
    groups = g.RankGroups(torch.tensor(off))
    obj = g.Objective("rank:pairwise")
    got = obj.metrics(names, m, y, None, BSP(dev()), groups)
    want = obj.metrics(names, m.cpu(), y.cpu(), None, BSP(torch.device("cpu")), groups)
    assert [abs(a - b) <= 1e-9 for a, b in zip(got[:2], want[:2])] == [True, True]
    assert abs(got[2] - want[2]) <= 1e-5


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_boost_round_through_the_growers(sparse):
    """One round of rank:pairwise equals feeding the same builder the
    kernel's pairs by hand (plumbing, not numerics): 2 000 rows, 8 features,
    100 groups of 20."""
    g = G()
    from wormhole_amd.parallel.bsp import BSP
    d = dev()
    bsp = BSP(d)
    gen = torch.Generator().manual_seed(8)
    n, F = 2000, 8
    X = torch.randint(0, 32, (n, F), generator=gen).float()
    y = (X[:, 0] / 8).floor() + (torch.rand(n, generator=gen) < 0.2).float()
    off = torch.arange(0, n + 1, 20)
    keys = torch.arange(F).repeat(n)
    rowoff = torch.arange(0, n * F + 1, F)
    dm = g.make_dmatrix(keys, rowoff, X.reshape(-1), y, None, F, d, sparse=sparse, group=off)
    assert dm.sparse == sparse and dm.group.is_cuda and dm.group.dtype == torch.int32
    p = g.GBDTParam()
    p.objective, p.max_depth, p.min_child_weight = "rank:pairwise", 4, 0.0
    obj = g.Objective(p.objective)
    cuts = g.Cuts.build(dm, p.max_bin, bsp)
    res = []
    for hand in (False, True):
        b = g.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
        margin = torch.zeros(n, device=d)
        if hand:
            groups = dm.rank_groups()
            small, block, tiled, rows, tiled_rows = groups.tasks(d)
            gp, st = hip().gbdt_gpair_rank(margin=margin, label=dm.label, group_off=dm.group,
                                           small=small, block=block, tiled=tiled, block_rows=rows,
                                           tiled_rows=tiled_rows, ndcg=False)
            gp._wh_stats = st
            tree = b.build(gp, margin)
        else:
            tree = g.boost_round(obj, b, dm, margin)[0]
        if hasattr(tree, "materialize"):
            tree.materialize()
        res.append((tree.dump(with_stats=True), margin.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    assert res[0][0].count("leaf") > 4 and float(res[0][1].abs().max()) > 0


@pytest.mark.parametrize("name", ["rank:pairwise", "rank:ndcg"])
def test_app_learns_the_order_on_the_gpu(name, tmp_path, monkeypatch, capsys):
    """The set of test_gbdt_rank.py's CLI test, which holds the CPU path to
    the same thresholds after the same C.APP_ROUNDS rounds: train-ndcg and
    train-map >= 0.999 at the last round, below it after round 0."""
    from wormhole_amd.apps.xgboost_app import main
    X, y, sizes = C.app_data()
    C.write_libsvm(tmp_path / "train.txt", X, y)
    C.write_group(tmp_path / "train.txt.group", sizes)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WH_DEVICE", "auto")
    assert main(["objective=" + name, "data=train.txt", "model_out=gpu.model"] + C.APP_ARGS) == 0
    out = capsys.readouterr().out
    for metric in ("train-ndcg", "train-map"):
        v = C.metric_lines(out, metric)
        assert sorted(v) == list(range(C.APP_ROUNDS)), out
        print(name, metric, "round 0 %.6f, last %.6f" % (v[0], v[C.APP_ROUNDS - 1]))
        assert v[C.APP_ROUNDS - 1] >= C.APP_THRESHOLD, (metric, v)
        assert v[0] < C.APP_THRESHOLD, (metric, v)
