#!/usr/bin/env python3
"""GBDT learning-to-rank benchmark on web-search-shaped synthetic data: 1M
rows x 136 features in query groups of 1..1250 rows (mean about 120), grades
0..4. Per boosting round it reports the gradient launch of rank:pairwise and
rank:ndcg (us, and its share of a round), the ndcg@10 evaluation (us), and
trees/s against binary:logistic on the same matrix; then the gradient launch
by task class, and one group of 1024 / 2048 / 4096 rows resident in LDS
against the same group streamed in tiles (the measurement behind
kRankLdsRows, csrc/host/gbdt_rank_plan.h).

    python benchmarks/bench_gbdt_rank.py [--rows 1000000] [--features 136] [--trees 20]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wormhole_amd import _native  # noqa: E402
from wormhole_amd.models import gbdt as G  # noqa: E402
from wormhole_amd.parallel.bsp import BSP  # noqa: E402


def web_search_like(n, f, seed, dev):
    """(X [n, f], grades [n], group sizes): group sizes log-normal, clipped to
    1..1250 (mean about 120); the grade is a skewed quantile of a noisy score
    (half the rows grade 0, 3 % grade 4)."""
    g = torch.Generator().manual_seed(seed)
    sizes = []
    total = 0
    while total < n:
        s = torch.exp(torch.randn(4096, generator=g) * 1.0 + 4.3).round().clamp(1, 1250).long()
        for v in s.tolist():
            v = min(v, n - total)
            sizes.append(v)
            total += v
            if total >= n:
                break
    gd = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn(n, f, device=dev, generator=gd)
    w = torch.randn(f, device=dev, generator=gd) / f ** 0.5
    score = (X * w).sum(1) + 0.5 * torch.sin(X[:, 0] * X[:, 1]) + \
        0.7 * torch.randn(n, device=dev, generator=gd)
    srt = score.sort().values
    edges = srt[[int(n * q) for q in (0.5, 0.75, 0.9, 0.97)]]
    return X, torch.bucketize(score, edges).float(), sizes


def us_per_call(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=136)
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--depth", type=int, default=6)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    hip = _native.hip()
    bsp = BSP(dev)
    X, y, sizes = web_search_like(a.rows, a.features, 7, dev)
    groups = G.RankGroups.from_sizes(sizes)
    dm = G.DMatrix.from_dense(X, y, dev, group=groups.off)
    n = dm.n
    st = torch.tensor(sizes, dtype=torch.float64)
    small, block, tiled, rows, tiled_rows = dm.rank_groups().tasks(dev)
    print("data: %d rows x %d features, %d groups, sizes %d..%d mean %.1f; pairs (sum of size^2) "
          "%.3g; tasks small %d block %d tiled %d (block LDS rows %d)" % (
              n, a.features, len(sizes), int(st.min()), int(st.max()), float(st.mean()),
              float((st * st).sum()), small.numel(), block.numel(), tiled.numel(), rows))
    p = G.GBDTParam()
    p.max_depth, p.eta, p.min_child_weight = a.depth, 0.1, 0.0
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    B = cuts.bin(dm)
    ybin = (y > 0).float()
    round_ms = {}
    for name in ("binary:logistic", "rank:pairwise", "rank:ndcg"):
        p.objective = name
        obj = G.Objective(name)
        dm.label = ybin if name == "binary:logistic" else y
        tb = G.TreeBuilder(p, bsp, dm, cuts, B)
        margin = torch.zeros(n, device=dev)
        for _ in range(2):
            G.boost_round(obj, tb, dm, margin)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tree = None
        for _ in range(a.trees):
            tree = G.boost_round(obj, tb, dm, margin)[-1]
        if hasattr(tree, "materialize"):
            tree.materialize()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        round_ms[name] = 1000 * dt / a.trees
        line = "%-16s %7.2f trees/s  %8.3f ms per round (depth %d)" % (
            name, a.trees / dt, round_ms[name], a.depth)
        if obj.rank:
            us = us_per_call(lambda: obj.gpair(margin, dm.label, None, dm.rank_groups()))
            ev = us_per_call(lambda: G.rank_eval(margin, dm.label, dm.rank_groups(), "ndcg", 10))
            val = obj.metrics(["ndcg@10", "map"], margin, dm.label, None, bsp, dm.rank_groups())
            line += "  gradient launch %8.1f us = %4.1f %% of a round  ndcg@10 eval %8.1f us" \
                    "  (%.2fx binary:logistic's round; train ndcg@10 %.4f map %.4f)" % (
                        us, 0.1 * us / round_ms[name], ev,
                        round_ms[name] / round_ms["binary:logistic"], val[0], val[1])
        print(line, flush=True)
    # the gradient launch by task class (each class alone, statistics included)
    margin = torch.randn(n, device=dev)
    e = torch.zeros(0, dtype=torch.int32, device=dev)
    off = dm.group
    for ndcg in (False, True):
        parts = []
        for label, lists in (("small", (small, e, e)), ("block", (e, block, e)),
                             ("tiled", (e, e, tiled)), ("none", (e, e, e))):
            us = us_per_call(lambda: hip.gbdt_gpair_rank(
                margin=margin, label=y, group_off=off, small=lists[0], block=lists[1],
                tiled=lists[2], block_rows=rows, tiled_rows=tiled_rows, ndcg=ndcg))
            parts.append("%s %.1f us" % (label, us))
        print("gradient launch by class (%s): %s  ('none': the zero fill and the statistics)" % (
            "rank:ndcg" if ndcg else "rank:pairwise", ", ".join(parts)), flush=True)
    # one group resident in LDS against the same group in tiles of half its rows
    for rows1 in (1024, 2048, 4096):
        m1 = torch.randn(rows1, device=dev) * 3
        y1 = torch.randint(0, 5, (rows1,), device=dev).float()
        o1 = torch.tensor([0, rows1], dtype=torch.int32, device=dev)
        t1 = torch.zeros(1, dtype=torch.int32, device=dev)
        res = us_per_call(lambda: hip.gbdt_gpair_rank(
            margin=m1, label=y1, group_off=o1, small=e, block=t1, tiled=e, block_rows=rows1,
            tiled_rows=0, ndcg=True), reps=5)
        til = us_per_call(lambda: hip.gbdt_gpair_rank(
            margin=m1, label=y1, group_off=o1, small=e, block=e, tiled=t1, block_rows=0,
            tiled_rows=rows1, ndcg=True, tile_rows=rows1 // 2), reps=5)
        print("one group of %d rows (rank:ndcg): resident %.1f us, tiled by %d rows "
              "%.1f us" % (rows1, res, rows1 // 2, til), flush=True)
    bsp.finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
