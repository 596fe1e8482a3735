"""Multi-class GBDT (objective=multi:softmax | multi:softprob, num_class=K):
closed-form leaves, learnable data through the tracker, rank counts and
restart, pred / eval tasks, errors, model-file compatibility."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKER = os.path.join(ROOT, "tracker", "dmlc_local.py")
XGB = os.path.join(ROOT, "bin", "xgboost.dmlc")
ROUNDS = 6  # (chosen by running it: mlogloss 0.507 -> 0.037, merror 0 from round 0)
TRAIN = ["objective=multi:softmax", "num_class=3", "max_depth=3", "eta=0.5",
         "num_round=%d" % ROUNDS, "eval_train=1", "eval_metric=merror", "eval_metric=mlogloss",
         "data=train.libsvm"]


def run(args, cwd, env_extra=None, timeout=300):
    env = dict(os.environ, WH_DEVICE="cpu")
    env.update(env_extra or {})
    return subprocess.run([sys.executable, TRACKER] + args, cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=timeout)


def three_class_rows(n=600, seed=5):
    """8 integer features in 0..7 (<= max_bin distinct values: the sketch is
    exact on any rank count); the label is a depth-2 tree of features 2, 5."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(0, 8, (n, 8), generator=g)
    y = torch.where(X[:, 2] < 4, torch.where(X[:, 5] < 3, 0, 1),
                    torch.where(X[:, 5] < 6, 2, 0))
    return X, y


def write_libsvm(path, X, y):
    with open(path, "w") as f:
        for row, lab in zip(X.tolist(), y.tolist()):
            f.write("%d %s\n" % (lab, " ".join("%d:%d" % (j, v) for j, v in enumerate(row))))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("multiclass")
    X, y = three_class_rows()
    write_libsvm(d / "train.libsvm", X, y)
    return d


@pytest.fixture(scope="module")
def trained(work):
    """The 1-rank run every other test compares against (computed once)."""
    r = run(["-n", "1", XGB] + TRAIN + ["model_out=one.model"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def rounds(out):
    return [l for l in out.splitlines() if re.match(r"^\[\d+\]\t", l)]


def load(path):
    from wormhole_amd.models.gbdt import Booster, GBDTParam
    p = GBDTParam()
    return Booster.load(str(path), p), p


def test_closed_form_leaves():
    """6 rows, x = {1,1,0,0,0,0}, y = {0,0,1,1,2,2}: at equal margins p = 1/3,
    g = -2/3 (true class) | +1/3, h = 2 p (1 - p) = 4/9; leaf = -G / (H + 1).
    Pins the factor 2, the tree-to-class order and the leaf sign."""
    from wormhole_amd.models import gbdt as G
    from wormhole_amd.parallel.bsp import BSP
    dev = torch.device("cpu")
    bsp = BSP(dev)
    X = torch.tensor([[1.], [1.], [0.], [0.], [0.], [0.]])
    y = torch.tensor([0., 0., 1., 1., 2., 2.])
    p = G.GBDTParam()
    for k, v in (("objective", "multi:softmax"), ("num_class", "3"), ("max_depth", "1"),
                 ("eta", "1"), ("lambda", "1"), ("min_child_weight", "0"), ("base_score", "0.5")):
        assert p.set(k, v)
    dm = G.DMatrix.from_dense(X, y, dev)
    booster = G.Booster(p, 1)
    assert booster.obj.n_group == 3 and G.Objective("binary:logistic").n_group == 1
    margin = booster.predict_margin(dm)
    assert margin.shape == (3, 6) and bool((margin == 0.5).all())
    gp = booster.obj.gpair(margin, y, None)
    assert gp.shape == (3, 6, 2)
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    builder = G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
    for k in range(3):
        builder.sample_features(torch.Generator().manual_seed(0))
        booster.trees.append(builder.build(G.class_gpair(gp, k), margin[k]))
    # per class: (G, H) of the x = 1 side and of the x = 0 side
    #   class 0: x=1 both true -> G = -4/3, H = 8/9; x=0 four others -> G = 4/3, H = 16/9
    #   class 1, 2: x=1 two others -> G = 2/3, H = 8/9; x=0 two true, two others ->
    #               G = -4/3 + 2/3 = -2/3, H = 16/9
    want = [(12 / 17, -12 / 25), (-6 / 17, 6 / 25), (-6 / 17, 6 / 25)]
    for k, (hi, lo) in enumerate(want):
        t = booster.trees[k]
        assert t.feat[0] == 0 and len(t.feat) == 3, "class %d tree must split on x" % k
        # x < cond goes left: the x = 0 rows are the left child
        assert abs(t.leaf[t.left[0]] - lo) < 1e-6 and abs(t.leaf[t.right[0]] - hi) < 1e-6
        # the builder added the leaves to this class's margins in place
        assert torch.allclose(margin[k], 0.5 + torch.tensor([hi, hi, lo, lo, lo, lo]), atol=1e-6)
    assert booster.dump().count("booster[") == 3


def test_learnable_data_through_the_tracker(trained):
    lines = rounds(trained.stdout)
    assert len(lines) == ROUNDS and lines[0].startswith("[0]\ttrain-merror:")
    ll = [float(x) for x in re.findall(r"train-mlogloss:([\d.]+)", trained.stdout)]
    me = [float(x) for x in re.findall(r"train-merror:([\d.]+)", trained.stdout)]
    assert len(ll) == len(me) == ROUNDS
    assert all(b < a for a, b in zip(ll, ll[1:])), ll
    assert me[-1] == 0.0


def test_three_ranks_grow_the_same_trees(work, trained):
    r3 = run(["-n", "3", XGB] + TRAIN + ["model_out=three.model"], work)
    assert r3.returncode == 0, r3.stderr[-2000:]
    a, _ = load(work / "one.model")
    b, pb = load(work / "three.model")
    assert len(a.trees) == 3 * ROUNDS and pb.num_class == 3
    assert a.dump() == b.dump()
    assert rounds(trained.stdout) == rounds(r3.stdout)


def test_csr_rows_grow_the_same_trees(work, trained):
    r = run(["-n", "2", XGB] + TRAIN + ["dsparse=1", "model_out=csr.model"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    a, _ = load(work / "one.model")
    b, _ = load(work / "csr.model")
    assert a.dump() == b.dump() and rounds(trained.stdout) == rounds(r.stdout)


def test_restart_resumes_with_the_right_grouping(work, trained):
    rr = run(["-n", "2", "--max-restart", "1", XGB] + TRAIN + ["model_out=restart.model"], work,
             {"WH_CKPT_DIR": str(work / "ckpt"), "WH_FAULT": "die:1:3"})
    assert rr.returncode == 0, rr.stderr[-2000:]
    assert "restart from version=" in rr.stdout
    a, _ = load(work / "one.model")
    b, _ = load(work / "restart.model")
    assert len(b.trees) == 3 * ROUNDS and a.dump() == b.dump()


def test_pred_softmax_and_softprob(work, trained):
    r = run(["-n", "1", XGB, "task=pred", "model_in=one.model", "test:data=train.libsvm",
             "name_pred=cls.txt"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    cls = [float(x) for x in open(work / "cls.txt")]
    assert len(cls) == 600 and set(cls) <= {0.0, 1.0, 2.0}
    _, y = three_class_rows()
    assert cls == [float(v) for v in y.tolist()]  # (train-merror is 0)
    # the same trees read as multi:softprob: the objective rides in the model
    # header, so train the probabilities' model with the same settings
    args = [a.replace("multi:softmax", "multi:softprob") for a in TRAIN]
    rp = run(["-n", "1", XGB] + args + ["model_out=prob.model"], work)
    assert rp.returncode == 0, rp.stderr[-2000:]
    r2 = run(["-n", "2", XGB, "task=pred", "model_in=prob.model", "test:data=train.libsvm",
              "name_pred=prob.txt"], work)
    assert r2.returncode == 0, r2.stderr[-2000:]
    prob = torch.tensor([float(x) for x in open(work / "prob.txt")], dtype=torch.float64)
    assert prob.numel() == 3 * 600
    prob = prob.view(600, 3)
    assert float((prob.sum(1) - 1).abs().max()) < 1e-5
    assert prob.argmax(1).tolist() == [int(c) for c in cls]


def test_eval_task_prints_merror(work, trained):
    r = run(["-n", "2", XGB, "task=eval", "model_in=one.model", "test:data=train.libsvm"], work)
    assert r.returncode == 0, r.stderr[-2000:]
    assert re.search(r"^test-merror:0\.000000$", r.stdout, re.M), r.stdout
    r = run(["-n", "1", XGB, "task=eval", "model_in=one.model", "test:data=train.libsvm",
             "eval_metric=mlogloss", "eval_metric=merror"], work)
    m = re.search(r"^test-mlogloss:([\d.]+)\ttest-merror:0\.000000$", r.stdout, re.M)
    last = re.findall(r"train-mlogloss:([\d.]+)", trained.stdout)[-1]
    assert m and m.group(1) == last


def test_errors(work):
    X, y = three_class_rows(60)
    y[7] = 3  # == num_class, on one rank's split only
    write_libsvm(work / "bad.libsvm", X, y)
    r = run(["-n", "3", XGB] + TRAIN + ["data=bad.libsvm", "num_round=1"], work, timeout=120)
    assert r.returncode != 0 and "label must be in [0, num_class)" in r.stderr
    r = run(["-n", "1", XGB] + TRAIN + ["num_class=1", "num_round=1"], work)
    assert r.returncode != 0 and "num_class" in r.stderr
    r = run(["-n", "1", XGB] + TRAIN + ["eval_metric=error", "num_round=1"], work)
    assert r.returncode != 0 and "eval_metric error" in r.stderr
    from wormhole_amd.models import gbdt as G
    with pytest.raises(ValueError):
        G.Objective("multi:softmax", 1)
    with pytest.raises(ValueError):
        G.Objective("multi:softprob", 3).check_metrics(["auc"])
    with pytest.raises(ValueError):
        G.Objective("binary:logistic").check_metrics(["merror"])


def header(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"WHGB"
    ln = int.from_bytes(raw[4:8], "little")
    return raw[8:8 + ln].decode().split("|")


def test_model_file_compatibility(work, trained, tmp_path):
    from wormhole_amd.models import gbdt as G
    p = G.GBDTParam()
    p.objective = "binary:logistic"
    b = G.Booster(p, 4)
    t = G.RegTree()
    t.add(-1)
    t.leaf[0] = 0.25
    b.trees.append(t)
    b.save(str(tmp_path / "bin.model"))
    assert header(tmp_path / "bin.model") == ["binary:logistic", "0.5", "4", "1"]
    b2, p2 = load(tmp_path / "bin.model")
    assert p2.num_class == 0 and b2.obj.n_group == 1 and b2.dump() == b.dump()
    assert header(work / "one.model") == ["multi:softmax", "0.5", "8", str(3 * ROUNDS), "3"]
    a, pa = load(work / "one.model")
    assert pa.num_class == 3 and a.obj.n_group == 3
    a.save(str(tmp_path / "again.model"))
    assert open(tmp_path / "again.model", "rb").read() == open(work / "one.model", "rb").read()
    c, _ = load(tmp_path / "again.model")
    assert c.dump() == a.dump()


def test_single_output_margins_keep_their_shape():
    from wormhole_amd.models import gbdt as G
    dev = torch.device("cpu")
    p = G.GBDTParam()
    p.objective = "binary:logistic"
    dm = G.DMatrix.from_dense(torch.zeros(5, 2), torch.zeros(5), dev)
    assert G.Booster(p, 2).predict_margin(dm).shape == (5,)
    assert G.Objective("binary:logistic").gpair(torch.zeros(5), torch.zeros(5), None).shape == (5, 2)
