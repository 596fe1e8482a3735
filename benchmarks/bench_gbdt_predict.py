#!/usr/bin/env python3
"""GBDT prediction: one predict_tree per tree (what Booster.predict_margin did
before the forest kernels) against the forest path, on the same dense matrix
in the same process.

    python benchmarks/bench_gbdt_predict.py [--rows 11000000 10000] [--trees 1 8 64 500]

The matrix is synthetic (BASELINE shape: 11M x 28 fp32, 2 % NaN), the forest
is synthetic too: full depth-8 trees (511 nodes) built directly as RegTree
lists, no training. Each path is timed over whole-forest calls (device events
around one call that ends in a synchronise), after one warm-up call of each;
the two are alternated --reps times and the median, minimum and maximum are
printed, with their ratio and a bit-comparison of the two margin vectors.
The forest's one-time pack and upload (Booster.forest) is reported apart.
Needs a GPU: there is no CPU fall-back to time.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wormhole_amd.models import gbdt as G  # noqa: E402


def full_tree(rng, depth, F):
    """A complete tree in breadth-first numbering: node i splits into 2i + 1, 2i + 2."""
    inner, nn = (1 << depth) - 1, (2 << depth) - 1
    t = G.RegTree()
    t.feat = rng.integers(0, F, nn).tolist()
    t.cond = rng.normal(0, 1, nn).astype(np.float32).tolist()
    t.defl = rng.integers(0, 2, nn).tolist()
    t.left = [2 * i + 1 for i in range(nn)]
    t.right = [2 * i + 2 for i in range(nn)]
    t.leaf = (rng.normal(0, 0.1, nn).astype(np.float32)).tolist()
    t.parent = [-1] + [(i - 1) // 2 for i in range(1, nn)]
    for i in range(inner, nn):
        t.feat[i], t.left[i], t.right[i], t.cond[i], t.defl[i] = -1, -1, -1, 0.0, 0
    for i in range(inner):
        t.leaf[i] = 0.0
    t.bin = [0] * nn
    t.gain, t.cover, t.base_weight = [0.0] * nn, [0.0] * nn, [0.0] * nn
    return t


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    return "%.3f [%.3f, %.3f]" % (statistics.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[11_000_000, 10_000])
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--trees", type=int, nargs="+", default=[1, 8, 64, 500])
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gbdt_predict needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    trees = [full_tree(rng, a.depth, a.features) for _ in range(max(a.trees))]
    print("# ms per whole-forest call: median [min, max] of %d alternated calls; depth %d, "
          "%d features, chunk capacity %d nodes" % (a.reps, a.depth, a.features,
                                                    G._native.hip().gbdt_forest_lds_nodes()))
    for n in a.rows:
        g = torch.Generator(device=dev).manual_seed(n)
        X = torch.randn(n, a.features, device=dev, generator=g)
        X[torch.rand(n, a.features, device=dev, generator=g) < 0.02] = float("nan")
        dm = G.DMatrix.from_dense(X, torch.zeros(n), dev)
        for T in a.trees:
            b = G.Booster(G.GBDTParam(), a.features)
            b.trees = trees[:T]

            def per_tree():
                m = torch.full((n,), b.base_margin, dtype=torch.float32, device=dev)
                for t in b.trees:
                    dm.predict_tree(t, m)
                return m

            def forest():
                m = torch.full((n,), b.base_margin, dtype=torch.float32, device=dev)
                return dm.predict_forest(b.forest(dev), m)

            t0 = time.perf_counter()
            b.forest(dev)
            torch.cuda.synchronize()
            pack_ms = (time.perf_counter() - t0) * 1e3
            per_tree(), forest()  # warm-up
            torch.cuda.synchronize()
            lt, ft = [], []
            for _ in range(a.reps):
                ms, ml = timed(per_tree)
                lt.append(ms)
                ms, mf = timed(forest)
                ft.append(ms)
            ratio = statistics.median(lt) / statistics.median(ft)
            print("n=%d T=%d per_tree_ms=%s forest_ms=%s ratio=%.2f pack_once_ms=%.1f chunks=%d "
                  "equal=%s" % (n, T, stats(lt), stats(ft), ratio, pack_ms,
                                len(b.forest(dev).chunks), torch.equal(ml, mf)), flush=True)
        del X, dm
    return 0


if __name__ == "__main__":
    sys.exit(main())
