#!/usr/bin/env python3
"""Survival objectives benchmark on bench_gbdt.py's shape (Higgs-shaped
11M x 28, depth 8).

    python benchmarks/bench_gbdt_survival.py [--rows 11000000] [--reps 20]

Measures, each after warm-up calls, as ``reps`` separately timed calls (median,
min, max): the survival:cox gradient per round, split by stage (the stages run
cumulatively: 1 = m*, 2 = + e and its tile sums, 3 = + the suffix scan,
4 = + the prefix scan, the pair and the statistics; a stage's cost is the
difference to the one before), the same at 100k rows, the cox-nloglik
evaluation, the survival:aft gradient per distribution, and alongside, on the
same build, ``gbdt_gpair`` (squared error), one depth-8 tree build and a whole
survival:cox boosting round. One JSON line per measurement; the last line is
the Cox gradient as a share of a round.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wormhole_amd import _native  # noqa: E402
from wormhole_amd.models import gbdt as G  # noqa: E402
from wormhole_amd.parallel.bsp import BSP  # noqa: E402
from bench_gbdt import higgs_like  # noqa: E402


def timed(fn, reps, warmup=3):
    """ms of ``reps`` separately timed calls after ``warmup`` untimed ones."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def report(metric, ms, **extra):
    row = {"metric": metric, "value": statistics.median(ms), "unit": "ms", "min": min(ms),
           "max": max(ms), "reps": len(ms)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row["value"]


def survival_labels(X, gen_seed, dev):
    """Exponential times whose hazard rises with feature 0, 30 % censored;
    fp32 times: a few ties among the smallest values, as real data has."""
    g = torch.Generator(device=dev).manual_seed(gen_seed)
    n = X.shape[0]
    rate = torch.exp(0.5 * X[:, 0].clamp(-3, 3))
    t = -torch.log(torch.rand(n, generator=g, device=dev).clamp(min=1e-7)) / rate
    event = torch.rand(n, generator=g, device=dev) < 0.7
    return t.clamp(min=1e-3).float(), event


def cox_stages(hip, margin, plan, reps, shape):
    kw = dict(margin=margin, order=plan.order, delta=plan.delta, run_events=plan.run_events,
              ws=plan.ws, ticket=plan.ticket)
    names = ("m*", "+ e, tile sums", "+ suffix scan", "+ prefix scan, pair, statistics")
    cum = []
    for k, name in enumerate(names, 1):
        # (1..3: the benchmark's own binding; all four: the gradient call itself)
        ms = timed((lambda: hip.gbdt_cox_scan_stages(stages=k, **kw)) if k < 4 else
                   (lambda: hip.gbdt_gpair_cox(weight=plan.weight, **kw)), reps)
        cum.append(report("survival:cox gradient, stages 1..%d (%s) (%s)" % (k, name, shape), ms))
    prev = 0.0
    for name, c in zip(names, cum):
        print(json.dumps({"metric": "survival:cox gradient, stage alone: %s (%s)" % (name, shape),
                          "value": c - prev, "unit": "ms (difference of medians)"}), flush=True)
        prev = c
    return cum[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=11_000_000)
    ap.add_argument("--small-rows", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    bsp = BSP(dev)
    hip = _native.hip()
    n = a.rows
    X, y = higgs_like(n, a.features, 7, dev)
    t, event = survival_labels(X, 11, dev)
    label = torch.where(event, t, -t)
    dm = G.DMatrix.from_dense(X, label, dev)
    shape = "%dx%d" % (n, a.features)
    margin = (0.3 * torch.randn(n, device=dev)).float()

    # ---- survival:cox
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    plan = dm.cox_plan()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"metric": "survival:cox plan, once per matrix (%s)" % shape,
                      "value": e0.elapsed_time(e1), "unit": "ms", "reps": 1,
                      "events": plan.events, "tiles": -(-n // hip.gbdt_cox_tile())}), flush=True)
    cox_ms = cox_stages(hip, margin, plan, a.reps, shape)
    report("cox-nloglik evaluation (%s)" % shape,
           timed(lambda: G.cox_eval_sums(margin, label, plan), a.reps))
    ns = min(a.small_rows, n)
    small = G.CoxPlan(label[:ns].contiguous())
    cox_stages(hip, margin[:ns].contiguous(), small, a.reps, "%d rows" % ns)

    # ---- survival:aft
    upper = torch.where(event, t, torch.full_like(t, float("inf")))
    for d, dist in enumerate(G.AFT_DISTS):
        report("survival:aft gradient, %s (%s)" % (dist, shape),
               timed(lambda: hip.gbdt_gpair_aft(margin, t, upper, None, dist=d, sigma=1.0),
                     a.reps))
    report("aft-nloglik evaluation, normal (%s)" % shape,
           timed(lambda: hip.gbdt_aft_eval(margin, t, upper, None, dist=0, sigma=1.0), a.reps))

    # ---- alongside: the squared-error gradient, a tree, a whole round
    report("gbdt_gpair, squared error (%s)" % shape,
           timed(lambda: hip.gbdt_gpair(margin, label, None, False), a.reps))
    p = G.GBDTParam()
    p.objective, p.max_depth, p.eta, p.max_bin = "survival:cox", a.depth, 0.1, 256
    booster = G.Booster(p, dm.ncol)
    obj = booster.obj
    m0 = booster.predict_margin(dm)
    hess = obj.gpair(m0, dm.label, None, data=dm)[..., 1]
    cuts = G.Cuts.build(dm, p.max_bin, bsp, hess=hess)
    B = cuts.bin(dm)
    tb = G.TreeBuilder(p, bsp, dm, cuts, B)
    state = {"m": m0}

    def tree():
        gp = obj.gpair(state["m"], dm.label, None, data=dm)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tb.build(gp, state["m"]).feat  # (a deferred tree's host lists: inside the timed region)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(2):
        tree()
    tree_ms = report("one depth-%d tree build on survival:cox pairs (%s)" % (a.depth, shape),
                     [tree() for _ in range(max(3, a.reps // 2))])

    def round_():
        G.boost_round(obj, tb, dm, state["m"])[-1].feat
    round_ms = report("survival:cox boosting round, gradient + depth-%d tree (%s)"
                      % (a.depth, shape), timed(round_, max(3, a.reps // 2), warmup=1))
    print(json.dumps({"metric": "survival:cox gradient as a share of a round (%s)" % shape,
                      "value": cox_ms / round_ms, "unit": "fraction",
                      "gradient_ms": cox_ms, "tree_ms": tree_ms, "round_ms": round_ms,
                      "train-cox-nloglik": obj.metrics(["cox-nloglik"], state["m"], dm.label,
                                                       None, bsp, data=dm)[0]}), flush=True)
    bsp.finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
