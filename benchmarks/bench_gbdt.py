#!/usr/bin/env python3
"""GBDT benchmark (BASELINE.json config: hist GBDT depth 8 on Higgs-shaped
11M x 28; default 500 trees).  Strong scaling: --rows is the total, split over
the ranks (row split, histogram allreduce per level over RCCL).

    python benchmarks/bench_gbdt.py [--rows 11000000] [--trees 500] [--depth 8]

--num-class K: multi:softprob on K quantile classes of the same synthetic
score (K trees per round; reports rounds/s and trees/s, and the softmax
gradient kernel alone against its plain-torch form and the 12 K n byte floor).

--monotone PATTERN: train with monotone_constraints, PATTERN's characters
``+`` / ``-`` / ``0`` cycled over the features (``"+-0"``: feature 0 rising,
1 falling, 2 free, 3 rising, ...): the bounded split search and the weight
intervals of every grower, against the same run without the option.

--interaction GROUPS: train with interaction_constraints, GROUPS as the app
takes them (``"[[0,1,2],[2,3]]"``), or ``halves``: two groups, the lower and
the upper half of the features. Composes with --monotone.

--objective NAME: a single-output objective instead of binary:logistic
(count:poisson, reg:gamma, reg:tweedie, binary:hinge, reg:pseudohubererror,
reg:squaredlogerror), on labels of the same synthetic score that fit it
(counts for count:poisson and reg:tweedie, positive reals for reg:gamma and
reg:squaredlogerror). count:poisson brings max_delta_step = 0.7, so it takes
the bounded split kernels. train_error is the objective's default metric.
reg:squarederror, reg:absoluteerror and reg:quantileerror (--quantile-alpha, a
number or a list as the app takes it; default 0.5) train on the score plus
unit noise. The last two refresh every tree's leaves with residual quantiles
(the radix select) and give up the deferred-tree path; --gamma G > 0 takes it
from any objective too, which makes reg:squarederror --gamma 1e-9 their fair
comparison.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wormhole_amd.models import gbdt as G  # noqa: E402
from wormhole_amd.parallel.bsp import BSP  # noqa: E402
from wormhole_amd.parallel.comm import env_local_rank  # noqa: E402
from wormhole_amd.parallel import launch  # noqa: E402


OBJECTIVES = ("binary:logistic",) + tuple(G.OBJ_IDS) + ("reg:squarederror",) + G.ADAPTIVE_OBJECTIVES


def higgs_like(n, f, seed, dev, num_class=0, objective="binary:logistic"):
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn(n, f, device=dev, generator=g)
    X[:, :7] = X[:, :7].abs()  # kinematic-like positive features
    w = torch.randn(f, device=dev, generator=g)
    logit = (X * w).sum(1) * 0.3 + torch.sin(X[:, 0] * X[:, 1]) + 0.5 * (X[:, 2] > 1).float()
    y = (torch.rand(n, device=dev, generator=g) < torch.sigmoid(logit)).float()
    if num_class > 1:  # K equal-mass classes of the score
        srt = logit.sort().values
        edges = srt[[(n * k) // num_class for k in range(1, num_class)]]
        y = torch.bucketize(logit, edges).float()
    elif objective in ("count:poisson", "reg:tweedie"):  # counts of mean exp(score / 2)
        y = torch.poisson(torch.exp(0.5 * logit.clamp(-3, 3)), generator=g)
    elif objective in ("reg:gamma", "reg:squaredlogerror"):  # positive reals around it
        y = torch.exp(0.5 * logit.clamp(-3, 3)) * (0.5 + torch.rand(n, device=dev, generator=g))
    elif objective in ("reg:pseudohubererror", "reg:squarederror") + G.ADAPTIVE_OBJECTIVES:
        y = logit + torch.randn(n, device=dev, generator=g)
    return X, y


def time_gpair(obj, margin, label, dev, reps=10):
    """ms per call of the fused softmax gradient kernel and of its plain-torch
    form on the same device tensors (events around `reps` calls, after one
    warm-up call each)."""
    out = []
    for fn in (lambda: obj.gpair(margin, label, None),
               lambda: G.softmax_gpair_torch(margin, label, None)):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=11_000_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--trees", type=int, default=500)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--max-bin", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--num-class", type=int, default=0,
                    help="K > 1: multi:softprob, K trees per round (--trees counts trees)")
    ap.add_argument("--objective", default="binary:logistic", choices=OBJECTIVES,
                    help="a single-output objective (not with --num-class); labels are drawn to fit")
    ap.add_argument("--quantile-alpha", default="0.5",
                    help="reg:quantileerror: one alpha or a list, K trees per round")
    ap.add_argument("--gamma", type=float, default=0.0,
                    help="min_split_loss; > 0 prunes and turns the deferred-tree path off")
    ap.add_argument("--monotone", default="",
                    help='monotone_constraints as a pattern of + - 0 cycled over the features')
    ap.add_argument("--interaction", default="",
                    help='interaction_constraints: "[[0,1],[2,3]]", or "halves"')
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"],
                    help="cpu: the framework's PyTorch CPU path (anchor numbers)")
    ap.add_argument("--gpus", type=int, default=1,
                    help="ranks (one per GPU); > 1 without a launcher: started here")
    a = ap.parse_args()
    if a.gpus > 1 and not launch.launched():  # before any GPU call in this process
        return launch.self_launch(os.path.abspath(__file__), sys.argv[1:], a.gpus, a.device)
    if a.device == "cuda":
        torch.cuda.set_device(env_local_rank())
        dev = torch.device("cuda", env_local_rank())
    else:
        dev = torch.device("cpu")

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()
    bsp = BSP(dev)
    launch.verify_world(bsp.comm, a.gpus if launch.launched() else 1)
    n = a.rows // bsp.world
    K = a.num_class if a.num_class > 1 else 1
    if K > 1 and a.objective != "binary:logistic":
        ap.error("--objective and --num-class exclude each other")
    p = G.GBDTParam()
    if a.objective == "reg:quantileerror":
        p.set("quantile_alpha", a.quantile_alpha)
        K = len(p.quantile_alpha)
    X, y = higgs_like(n, a.features, 7 + bsp.rank, dev, a.num_class, a.objective)
    dm = G.DMatrix.from_dense(X, y, dev)
    p.objective = "multi:softprob" if a.num_class > 1 else a.objective
    p.num_class = a.num_class if K > 1 else 0
    p.max_depth = a.depth
    p.eta = 0.1
    p.gamma = a.gamma
    p.max_bin = a.max_bin
    if a.monotone:
        if set(a.monotone) - set("+-0"):
            ap.error("--monotone takes a pattern of the characters + - 0")
        sign = {"+": "1", "-": "-1", "0": "0"}
        p.set("monotone_constraints", ",".join(sign[a.monotone[j % len(a.monotone)]]
                                               for j in range(a.features)))
    if a.interaction:
        h = a.features // 2
        halves = "[[%s],[%s]]" % (",".join(map(str, range(h))),
                                  ",".join(map(str, range(h, a.features))))
        p.set("interaction_constraints", halves if a.interaction == "halves" else a.interaction)
        p.interaction_vector(a.features)  # (ids past --features end the run here)
    sync()
    t_prep = time.perf_counter()
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    B = cuts.bin(dm)
    sync()
    t_prep = time.perf_counter() - t_prep
    obj = G.make_objective(p.objective, p.num_class, p)
    tb = G.TreeBuilder(p, bsp, dm, cuts, B)
    margin = torch.zeros(n, device=dev) if K == 1 else torch.zeros(K, n, device=dev)
    rounds = max(1, a.trees // K)
    for _ in range(a.warmup):
        for t in G.boost_round(obj, tb, dm, margin):
            if hasattr(t, "materialize"):
                t.materialize()
    sync()
    bsp.barrier()
    b0 = tb.hist_bytes()
    t0 = time.perf_counter()
    tree = None
    for _ in range(rounds):
        tree = G.boost_round(obj, tb, dm, margin)[-1]
    # a device-grown tree's host lists are built one tree later: the last
    # one's inside the timed region too
    if tree is not None and hasattr(tree, "materialize"):
        tree.materialize()
    sync()
    bsp.barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    bsp.allreduce(t, "max")
    dt = float(t.item())
    ntree = rounds * K
    hb = bsp.allreduce_scalar((tb.hist_bytes() - b0) / max(ntree, 1), "max")
    err = obj.metrics([obj.default_metric()], margin, dm.label, None, bsp)[0]
    extra = {}
    if a.objective == "reg:quantileerror":
        extra = {"quantile_alpha": p.quantile_alpha, "rounds": rounds}
    elif K > 1:
        extra = {"num_class": K, "rounds": rounds, "rounds_per_s": rounds / dt}
        if dev.type == "cuda":
            ms_k, ms_t = time_gpair(obj, margin, dm.label, dev)
            extra.update({"gpair_softmax_ms": ms_k, "gpair_torch_ms": ms_t,
                          "gpair_bytes_floor": 12 * K * n,
                          "gpair_softmax_GBps": 12e-6 * K * n / ms_k})
    if bsp.rank == 0:
        print(json.dumps({"metric": "GBDT trees/s (hist, depth %d, %dx%d)" % (a.depth, a.rows, a.features),
                          "value": ntree / dt, "unit": "trees/s", "n_gpus": bsp.world if dev.type == "cuda" else 0, "ranks": bsp.world, "device": dev.type,
                          "ms_per_tree": 1000 * dt / ntree,
                          "trees": ntree, **extra, "objective": p.objective,
                          "gamma": a.gamma, "monotone": a.monotone or None,
                          "interaction": p.interaction or None,
                          "sketch_bin_s": t_prep,
                          "hist_exchange": ("feature-reduce-scatter" if tb.xchg is not None
                                            else "allreduce") if bsp.world > 1 else None,
                          "hist_bytes_per_rank_per_tree": hb,
                          "train_error": err, "scaling": "strong", "data": "synthetic Higgs-shaped"}),
              flush=True)
    bsp.finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
