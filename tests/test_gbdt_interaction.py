"""interaction_constraints on the CPU path (the Python level loop, which is
also the native growers' reference): parsing, the masked split search against
an independent loop, the path rule on every tree (with an unconstrained
control that breaks it), the root-only rule, dense = CSR, with
monotone_constraints, multi-class, the command line, several ranks."""
import functools
import json
import math
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

import _gbdt_interaction_cases as C
import _gbdt_monotone_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKER = os.path.join(ROOT, "tracker", "dmlc_local.py")
XGB = os.path.join(ROOT, "bin", "xgboost.dmlc")
CPU = torch.device("cpu")
BIT63 = -(1 << 63)  # bit 63 alone, as an int64


def _G():
    from wormhole_amd.models import gbdt as G
    return G


def _bsp():
    from wormhole_amd.parallel.bsp import BSP
    os.environ.pop("RANK", None)
    return BSP(CPU)


# ------------------------------------------------------------------ parsing
def test_parsing():
    G = _G()
    for text in ("[[0,1,2],[2,3,4,5]]", " [ [0, 1 ,2] , [2,3,4,5] ] ", '"[[0,1,2],[2,3,4,5]]"',
                 "'[[2,1,0,1],[5,4,3,2]]'", "[[+0,1,2],[2,3,4,5,5]]"):
        p = G.GBDTParam()
        assert p.set("interaction_constraints", text) is True
        assert p.interaction == [[0, 1, 2], [2, 3, 4, 5]], text
    m = p.interaction_vector(7)
    assert m.dtype == torch.int64 and m.shape == (7,)
    # feature 2 is in both groups, feature 6 in none (the reserved bit alone)
    assert m.tolist() == [1, 1, 3, 2, 2, 2, BIT63]
    assert p.interaction_vector(9).tolist() == [1, 1, 3, 2, 2, 2, BIT63, BIT63, BIT63]  # padded
    assert p.interaction_vector(6).tolist() == [1, 1, 3, 2, 2, 2]
    with pytest.raises(SystemExit, match="interaction_constraints"):
        p.interaction_vector(5)  # feature 5 of 5 features
    # off: unset, or the empty list
    assert G.GBDTParam().interaction_vector(4) is None
    for text in ("[]", " [ ] ", '"[]"'):
        p = G.GBDTParam()
        assert p.set("interaction_constraints", text) and p.interaction == []
        assert p.interaction_vector(4) is None
    for bad in ("[[0,1],[]]", "[[]]", "[[0,a]]", "[[0.5]]", "[[0,-1]]", "[[0,1]", "[0,1]]",
                "[[0,1],[2]]]", "[[[0]]]", "[0,1]", "0,1", "[[0,]]", "[[0 1]]", "[[0],,[1]]", ""):
        with pytest.raises(SystemExit, match="interaction_constraints"):
            G.GBDTParam().set("interaction_constraints", bad)
    # 63 groups fill the word; a 64th names the limit
    p = G.GBDTParam()
    assert p.set("interaction_constraints", C.spell([(k,) for k in range(63)]))
    m = p.interaction_vector(64)
    assert m[62].item() == 1 << 62 and m[63].item() == BIT63
    with pytest.raises(SystemExit, match=r"interaction_constraints.*\b63\b"):
        G.GBDTParam().set("interaction_constraints", C.spell([(k,) for k in range(64)]))


def test_child_state_rule():
    """state(child) = state(parent) & m[f] & ~bit63, admit = state & m[f] != 0:
    the set rule of the documentation, on the shared groups."""
    G = _G()
    p = C.param(G, C.GROUPS)
    m = p.interaction_vector(C.F).tolist()
    root = G.INTERACTION_ROOT
    assert all(root & m[f] for f in range(C.F))  # the root admits every feature
    for first in range(C.F):
        for second in range(C.F):
            st = G.interaction_child(root, m[first])
            want = any({first, second} <= set(grp) for grp in C.GROUPS)
            assert bool(st & m[second]) == want, (first, second)
            for third in range(C.F):
                st2 = G.interaction_child(st, m[second])
                want3 = any({first, second, third} <= set(grp) for grp in C.GROUPS)
                assert bool(st2 & m[third]) == want3, (first, second, third)
    assert G.interaction_child(root, m[C.FREE]) == 0  # nothing below a split on feature 6


def test_quoted_value_survives_the_conf_parser(tmp_path):
    from wormhole_amd.apps.xgboost_app import parse_args
    conf = tmp_path / "m.conf"
    conf.write_text('max_depth = 3\ninteraction_constraints = "[[0, 1], [2,3]]"\n')
    items = dict(parse_args([str(conf)]))
    assert items["interaction_constraints"] == "[[0, 1], [2,3]]"
    p = _G().GBDTParam()
    assert p.set("interaction_constraints", items["interaction_constraints"])
    assert p.interaction == [[0, 1], [2, 3]]
    for arg in ("interaction_constraints=[[0,1],[2,3]]", 'interaction_constraints="[[0,1],[2,3]]"'):
        (k, v), = parse_args([arg])
        p = _G().GBDTParam()
        assert p.set(k, v) and p.interaction == [[0, 1], [2, 3]]


# ----------------------------------------------- masked search vs a loop
def _search_case():
    G = _G()
    S, F, nbin = 5, 6, 9
    g = torch.Generator().manual_seed(7)
    hist = torch.zeros(S, F, nbin, 2, dtype=torch.float64)
    hist[..., 0] = torch.randn(S, F, nbin, generator=g, dtype=torch.float64) * 3
    hist[..., 1] = torch.rand(S, F, nbin, generator=g, dtype=torch.float64) * 4 + 0.5
    totals = hist[:, 0].sum(1)
    totals[:, 0] += 0.7
    totals[:, 1] = hist[:, :, :, 1].sum(2).max(1).values + 1.5
    valid = torch.ones(F, nbin, dtype=torch.bool)
    valid[3, 7:] = False
    valid[0, 0] = False
    p = G.GBDTParam()
    # groups {0, 1, 2}, {2, 3}, {4}; feature 5 in none
    fmask = torch.tensor([1, 1, 3, 2, 4, BIT63], dtype=torch.int64)
    # slots: root, group 0, groups 0 + 1, nothing, group 2
    state = torch.tensor([-1, 1, 3, 0, 4], dtype=torch.int64)
    mono = torch.tensor([1, -1, 0, 0, 1, 0], dtype=torch.int8)
    w0 = [p.calc_weight(float(t[0]), float(t[1])) for t in totals]
    inf = math.inf
    bounds = torch.tensor([[-inf, inf], [w0[1] - 0.02, w0[1] + 0.02], [-inf, inf], [-inf, inf],
                           [w0[4] - 0.05, inf]], dtype=torch.float64)
    return p, hist, totals, valid, fmask, state, mono, bounds


@pytest.mark.parametrize("with_mono", [False, True])
def test_masked_search_matches_independent_loop(with_mono):
    G = _G()
    p, hist, totals, valid, fmask, state, mono, bounds = _search_case()
    mb = (mono, bounds) if with_mono else (None, None)
    S, F, nbin = hist.shape[:3]
    gains, left = G.split_gains(p, hist, totals, valid, *mb)  # every candidate, unmasked
    fm, st = fmask.tolist(), state.tolist()
    for s in range(S):
        for f in range(F):
            if not st[s] & fm[f]:
                gains[s, f] = -math.inf
    got = G.find_splits_ref(p, hist, totals, valid, *mb, fmask, state)
    free = G.find_splits_ref(p, hist, totals, valid, *mb)
    o = [0] + [nbin * (f + 1) for f in range(F)]
    compact = hist.reshape(S, F * nbin, 2)
    fvalid = torch.ones(F, dtype=torch.uint8)
    # (the CSR search knows features, not thresholds: the same candidates)
    got_csr = G.find_splits_csr_ref(p, compact, totals, o, fvalid, *mb, fmask, state)
    csr_want = G.find_splits_ref(p, hist, totals, torch.ones_like(valid), *mb, fmask, state)
    changed = 0
    for s in range(S):
        flat = gains[s].reshape(-1)
        k = int(flat.argmax())
        if not math.isfinite(float(flat[k])):
            assert float(got[s, 0]) == -math.inf and float(got_csr[s, 0]) == -math.inf
            continue
        f, b, d = k // (2 * nbin), (k // 2) % nbin, k % 2
        assert (int(got[s, 1]), int(got[s, 2]), int(got[s, 3])) == (f, b, d), s
        assert st[s] & fm[f]
        assert float(got[s, 0]) == float(flat[k])
        assert got[s, 4:6].tolist() == left[s, f, b, d].tolist()
        changed += int(got[s, 1]) != int(free[s, 1])
        # the CSR reference: the same split on the same bin (its unconstrained
        # gains are fp32, its bounded ones Python floats)
        assert got_csr[s, 1:4].tolist() == csr_want[s, 1:4].tolist(), s
        assert float(got_csr[s, 0]) == pytest.approx(float(csr_want[s, 0]), rel=1e-5)
    assert float(got[3, 0]) == -math.inf  # a slot that admits nothing
    assert math.isfinite(float(got[0, 0])) and torch.equal(got[0], free[0])  # the root: all
    assert changed > 0  # the mask bites


# ------------------------------------------------------------ the path rule
@functools.lru_cache(maxsize=None)
def _model(sparse, gamma, colsample, groups, c=1.0, mono=None):
    G = _G()
    X, y = C.data(c=c)
    dm = C.dmatrix(G, X, y, CPU, sparse)
    p = C.param(G, groups, mono, gamma=float(gamma), colsample_bytree=colsample)
    return C.train(G, _bsp(), dm, p)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("gamma", [0, 2])
@pytest.mark.parametrize("colsample", [1.0, 0.6])
def test_path_rule_on_every_tree(sparse, gamma, colsample):
    b = _model(sparse, gamma, colsample, C.GROUPS)
    bad, total = C.broken(b.trees)
    print("constrained", bad, total)
    assert len(b.trees) == C.ROUNDS and bad == 0 and total > 2 * C.ROUNDS
    # the control: the same data need the constraint
    bad, total = C.broken(_model(sparse, gamma, colsample, None).trees)
    print("free", bad, total)
    assert bad > 0


def test_control_breaks_every_path():
    """The figures of the shared data: 46 of the unconstrained model's 46
    paths break the rule, dense and CSR alike."""
    for sparse in (False, True):
        assert C.broken(_model(sparse, 0, 1.0, None).trees) == (46, 46)


def test_csr_builder_grows_the_dense_trees():
    dense, csr = _model(False, 0, 1.0, C.GROUPS), _model(True, 0, 1.0, C.GROUPS)
    for a, b in zip(dense.trees, csr.trees):
        assert a.feat == b.feat and a.cond == b.cond and a.defl == b.defl
        assert all(abs(x - z) < 1e-6 for x, z in zip(a.leaf, b.leaf))


def test_root_only_rule():
    """c = 3: feature 6, in no group, wins every root; below it nothing is
    admitted, so the constrained trees have exactly three nodes."""
    free = _model(False, 0, 1.0, None, c=3.0)
    assert [t.feat[0] for t in free.trees] == [C.FREE] * C.ROUNDS
    assert all(len(t.feat) > 3 for t in free.trees)
    b = _model(False, 0, 1.0, C.GROUPS, c=3.0)
    t = b.trees[0]
    assert t.feat[0] == C.FREE and len(t.feat) == 3
    assert t.feat[t.left[0]] < 0 and t.feat[t.right[0]] < 0
    assert C.broken(b.trees)[0] == 0 and C.broken(free.trees)[0] > 0


def test_one_group_of_all_features_and_the_empty_list_change_nothing():
    for sparse in (False, True):
        none = _model(sparse, 0, 1.0, None)
        everything = _model(sparse, 0, 1.0, (tuple(range(C.F)),))
        assert everything.dump(None, True) == none.dump(None, True)
        empty = _model(sparse, 0, 1.0, ())
        assert empty.dump(None, True) == none.dump(None, True)
        assert "yes=" in none.dump()


MONO = (1, -1, 0, 1, 0, 0, 0)


def test_with_monotone_constraints():
    both = _model(False, 0, 1.0, C.GROUPS, mono=MONO)
    assert C.broken(both.trees)[0] == 0
    assert M.holds(both.trees, MONO)
    s = M.structure(both.trees, MONO)
    assert sum(n for n, _ in s.values()) > 0  # constrained features are split on
    # each constraint alone leaves the other's property broken, and differs
    inter = _model(False, 0, 1.0, C.GROUPS)
    mono = _model(False, 0, 1.0, None, mono=MONO)
    assert C.broken(mono.trees)[0] > 0
    assert both.dump() != inter.dump() and both.dump() != mono.dump()


def test_multiclass_trees_are_constrained():
    G = _G()
    X, y = C.data()
    q = torch.quantile(y, torch.tensor([1 / 3, 2 / 3]))
    lab = (y > q[0]).float() + (y > q[1]).float()
    res = {}
    for groups in (C.GROUPS, None):
        p = C.param(G, groups, objective="multi:softprob", num_class=3)
        b = C.train(G, _bsp(), C.dmatrix(G, X, lab, CPU), p, rounds=3)
        assert len(b.trees) == 9
        res[groups] = [C.broken(b.trees[k::3]) for k in range(3)]
    for k in range(3):
        bad, total = res[C.GROUPS][k]
        assert bad == 0 and total > 3, (k, res)
    assert all(bad > 0 for bad, _ in res[None])  # the control, class by class


# ------------------------------------------------------------ command line
def _cli(args, cwd, n=1):
    env = dict(os.environ, WH_DEVICE="cpu")
    return subprocess.run([sys.executable, TRACKER, "-n", str(n), XGB] + args, cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=300)


def test_cli(tmp_path):
    X, y = C.data()
    C.write_libsvm(tmp_path / "train.libsvm", X, y)
    conf = tmp_path / "m.conf"
    conf.write_text('objective = "reg:linear"\nmax_depth = 4\neta = 0.5\nmax_bin = 16\n'
                    'num_round = 3\ndata = "train.libsvm"\n'
                    'interaction_constraints = "[[0,1,2], [2,3,4,5]]"\n')
    r = _cli(["m.conf", "model_out=a.model"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "unknown parameter" not in r.stdout + r.stderr
    r = _cli(["m.conf", "task=dump", "model_in=a.model", "name_dump=a.txt"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    trees = C.parse_dump(open(tmp_path / "a.txt").read())
    bad, total = C.broken(trees)
    assert len(trees) == 3 and bad == 0 and total > 6
    # the command line overrides the conf: off again, and the rule breaks
    r = _cli(["m.conf", "interaction_constraints=[]", "model_out=f.model"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    r = _cli(["m.conf", "task=dump", "model_in=f.model", "name_dump=f.txt"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert C.broken(C.parse_dump(open(tmp_path / "f.txt").read())) == (46, 46)
    # a bad value, and an id past the data's 7 features
    for k, val in enumerate(("[[0,1],[]]", "[[0,1],[2,7]]")):
        out = "bad%d.model" % k
        bad = _cli(["m.conf", "interaction_constraints=" + val, "model_out=" + out], tmp_path)
        assert bad.returncode != 0
        assert "interaction_constraints" in bad.stdout + bad.stderr
        assert not (tmp_path / out).exists()


# ------------------------------------------------ feature-sharded exchange
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _xtrain(bsp):
    G = _G()
    X, y = C.data()
    rows = torch.arange(X.shape[0])[bsp.rank::bsp.world]
    dm = G.DMatrix.from_dense(X[rows], y[rows], CPU)
    b = C.train(G, bsp, dm, C.param(G, C.GROUPS))
    return [t.dump(with_stats=True) for t in b.trees], b


def _xmain(rank, world, port, out, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), WH_GBDT_XCHG=mode)
    torch.set_num_threads(1)
    from wormhole_amd.parallel.bsp import BSP
    bsp = BSP(CPU)
    dumps, _ = _xtrain(bsp)
    if rank == 0:
        json.dump(dumps, open(out, "w"))
    bsp.finalize()


@pytest.fixture(scope="module")
def single():
    dumps, b = _xtrain(_bsp())
    assert C.broken(b.trees)[0] == 0
    return dumps


@pytest.mark.parametrize("world,mode", [(2, "rs"), (4, "rs"), (2, "allreduce"), (4, "allreduce")])
def test_feature_sharded_trees_equal_single_rank(single, world, mode, tmp_path):
    out = str(tmp_path / "x.json")
    mp.spawn(_xmain, args=(world, _free_port(), out, mode), nprocs=world, join=True)
    assert json.load(open(out)) == single
    assert any("yes=" in d for d in single)
