"""What the ranking tests share (test_gbdt_rank.py, test_gbdt_rank_gpu.py):
the definitions of docs/bsp_apps.md "Ranking" as naive fp64 double loops, the
worked pin, and the learnable set of the end-to-end runs."""
import math
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKER = os.path.join(ROOT, "tracker", "dmlc_local.py")
XGB = os.path.join(ROOT, "bin", "xgboost.dmlc")

# one group, from an fp64 prototype, rounded to 6 places (compare to 2e-6)
PIN_M = [0.5, -1.0, 0.5, 2.0, 0.0]
PIN_Y = [2.0, 0.0, 1.0, 0.0, 2.0]
PIN_R = [1, 4, 2, 0, 3]
PIN_IDCG = 5.392789
PIN = {
    False: ([-0.958333, 0.407326, 0.071435, 1.609166, -1.129594],
            [0.689391, 0.635015, 0.913846, 0.512858, 0.676312]),
    True: ([-0.142582, 0.023117, -0.022953, 0.342098, -0.199680],
           [0.081993, 0.037043, 0.040995, 0.101299, 0.057777]),
}

# The end-to-end set (app_data): the parameters and the round count at which
# BOTH objectives order every training group perfectly on the CPU path. Found
# by running it: rank:pairwise has train-ndcg and train-map >= 0.999 from
# round 6 on, rank:ndcg from round 11 on (and both stay there through round
# 19); after round 0 they are at 0.79 / 0.87 and 0.93 / 0.91: one depth-3
# tree has 8 leaves for the 12 steps of the grade. (rank:ndcg's hessians are
# small: with lambda = 1 its leaf weights are, too, and it needs many more rounds.)
APP_ROUNDS = 20
APP_THRESHOLD = 0.999
APP_ARGS = ["max_depth=3", "min_child_weight=0", "eta=1.0", "lambda=0.01",
            "num_round=%d" % APP_ROUNDS, "eval_train=1", "eval_metric=ndcg", "eval_metric=map"]


def ranks(x):
    """0-based descending rank of every element; ties go to the earlier one."""
    n = len(x)
    return [sum(1 for j in range(n) if x[j] > x[i] or (x[j] == x[i] and j < i)) for i in range(n)]


def naive_group(m, y, ndcg):
    """One group's (g, h, sum W |lambda|) lists in fp64, pair by pair."""
    n = len(m)
    c = [sum(1 for j in range(n) if y[j] != y[i]) for i in range(n)]
    r, lr = ranks(m), ranks(y)
    gain = [2.0 ** v - 1.0 for v in y]
    idcg = sum(gain[i] / math.log2(2 + lr[i]) for i in range(n))
    g, h, mass = [0.0] * n, [0.0] * n, [0.0] * n
    for i in range(n):
        for j in range(n):
            if not y[i] > y[j]:
                continue
            delta = 1.0
            if ndcg:
                delta = (abs(gain[i] - gain[j]) * abs(1 / math.log2(2 + r[i]) - 1 / math.log2(2 + r[j]))
                         / idcg) if idcg > 0 else 0.0
            w = (1.0 / c[i] + 1.0 / c[j]) * delta
            d = m[i] - m[j]
            # rho = sigmoid(d); 1 - rho from the same exponential
            t = math.exp(-abs(d))
            rho, q = (1 / (1 + t), t / (1 + t)) if d >= 0 else (t / (1 + t), 1 / (1 + t))
            lam, eta = -q, max(rho * q, 1e-16)
            g[i] += w * lam
            g[j] -= w * lam
            h[i] += 2 * w * eta
            h[j] += 2 * w * eta
            mass[i] += w * q
            mass[j] += w * q
    return g, h, mass


def naive_gpair(margin, label, off, ndcg):
    """fp64 [n, 2] over all groups of offsets ``off``."""
    out = torch.zeros(len(margin), 2, dtype=torch.float64)
    m, y = [float(v) for v in margin], [float(v) for v in label]
    for a, b in zip(off[:-1], off[1:]):
        g, h, _ = naive_group(m[a:b], y[a:b], ndcg)
        out[a:b, 0] = torch.tensor(g, dtype=torch.float64)
        out[a:b, 1] = torch.tensor(h, dtype=torch.float64)
    return out


def naive_eval(m, y, kind, k=0, minus=False):
    """One group's ndcg@k / map@k by the definitions (k = 0: no cut-off)."""
    n = len(m)
    k = k or n + 1
    r, lr = ranks(m), ranks(y)
    if kind == "ndcg":
        num = sum((2.0 ** y[i] - 1) / math.log2(2 + r[i]) for i in range(n) if r[i] < k)
        den = sum((2.0 ** y[i] - 1) / math.log2(2 + lr[i]) for i in range(n) if lr[i] < k)
    else:
        hits = [sum(1 for j in range(n) if y[j] > 0 and r[j] <= r[i]) for i in range(n)]
        num = sum(hits[i] / (r[i] + 1) for i in range(n) if y[i] > 0 and r[i] < k)
        den = sum(1 for v in y if v > 0)
    return num / den if den > 0 else (0.0 if minus else 1.0)


def offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + int(s))
    return off


def app_data(seed=11, ngroup=60):
    """The learnable ranking set: groups of 5 to 40 rows, 8 features in
    [0, 1) rounded to 1/64 (few distinct values: exact cuts); the grade is a
    step function of feature 0 with 5 levels over 12 steps, 7 features are noise."""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(5, 41, (ngroup,), generator=g)
    n = int(sizes.sum())
    X = torch.randint(0, 64, (n, 8), generator=g).float() / 64
    levels = torch.tensor([0, 3, 1, 4, 0, 2, 4, 0, 3, 1, 2, 0])
    y = levels[(X[:, 0] * 12).long().clamp(max=11)].float()
    return X, y, sizes.tolist()


def write_libsvm(path, X, y, weight=None):
    with open(path, "w") as f:
        for i, (row, lab) in enumerate(zip(X.tolist(), y.tolist())):
            head = "%g" % lab if weight is None else "%g:%g" % (lab, weight[i])
            f.write("%s %s\n" % (head, " ".join("%d:%g" % (j, v) for j, v in enumerate(row))))


def write_group(path, sizes):
    with open(path, "w") as f:
        f.write("".join("%d\n" % s for s in sizes))


def run_app(args, cwd, device="cpu", nproc=1, timeout=300):
    env = dict(os.environ, WH_DEVICE=device)
    return subprocess.run([sys.executable, TRACKER, "-n", str(nproc), XGB] + args, cwd=cwd,
                          env=env, capture_output=True, text=True, timeout=timeout)


def metric_lines(stdout, name):
    """{round: value} of ``<name>:<value>`` from the per-round output lines."""
    out = {}
    for line in stdout.splitlines():
        m = re.match(r"\[(\d+)\]", line)
        v = re.search(r"\t%s:([-0-9.eE]+)" % re.escape(name), line)
        if m and v:
            out[int(m.group(1))] = float(v.group(1))
    return out
