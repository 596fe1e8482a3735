#!/usr/bin/env python3
"""grow_policy=lossguide against depth-wise growth on bench_gbdt.py's
Higgs-shaped data (11M x 28, 256 bins), one GPU. One JSON line per
measurement:

* depth-wise, depth 8 (the device level loop);
* lossguide max_leaves=256 max_depth=8 -- the same trees: the first trees'
  dumps are compared with the depth-wise ones in the same run;
* lossguide max_leaves=255 max_depth=0 and max_leaves=64 max_depth=0, each in
  the device leaf loop and in the Python leaf loop (LEAF_LOOP_DEV = False),
  with the microseconds per step (a tree of L leaves has L - 1 steps).

    python benchmarks/bench_gbdt_lossguide.py [--rows 11000000] [--trees 20]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_gbdt import higgs_like  # noqa: E402
from wormhole_amd.models import gbdt as G  # noqa: E402
from wormhole_amd.parallel.bsp import BSP  # noqa: E402


def param(a, policy, max_leaves, max_depth):
    p = G.GBDTParam()
    p.objective, p.eta, p.max_bin, p.max_depth = "binary:logistic", 0.1, a.max_bin, max_depth
    p.set("grow_policy", policy)
    p.set("max_leaves", str(max_leaves))
    return p


def run(a, bsp, dm, cuts, B, p, trees, keep=0):
    """(ms per tree, mean leaves, the first ``keep`` trees' dumps) of ``trees``
    trees after ``a.warmup`` from zero margins."""
    obj = G.make_objective(p.objective, 0, p)
    tb = G.TreeBuilder(p, bsp, dm, cuts, B)
    margin = torch.zeros(dm.n, device=dm.device)
    grown = []
    for _ in range(a.warmup):
        grown += G.boost_round(obj, tb, dm, margin)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(trees):
        grown += G.boost_round(obj, tb, dm, margin)
    for t in grown:
        t.feat  # (a deferred device tree builds its lists: the last one's inside the timing)
    torch.cuda.synchronize()
    ms = 1000 * (time.perf_counter() - t0) / trees
    leaves = sum(sum(1 for f in t.feat if f < 0) for t in grown[a.warmup:]) / trees
    return ms, leaves, [t.dump(None, True) for t in grown[:keep]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=11_000_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--max-bin", type=int, default=256)
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--py-trees", type=int, default=3, help="trees of the Python leaf loop's runs")
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    bsp = BSP(dev)
    X, y = higgs_like(a.rows, a.features, 7, dev)
    dm = G.DMatrix.from_dense(X, y, dev)
    cuts = G.Cuts.build(dm, a.max_bin, bsp)
    B = cuts.bin(dm)
    shape = "%dx%d, %d bins" % (a.rows, a.features, a.max_bin)
    keep = a.warmup + min(3, a.trees)

    def report(name, ms, leaves, **extra):
        print(json.dumps({"metric": "GBDT ms/tree (%s; %s)" % (name, shape), "value": ms,
                          "unit": "ms/tree", "mean_leaves": leaves, **extra}), flush=True)

    d_ms, d_leaves, d_dumps = run(a, bsp, dm, cuts, B, param(a, "depthwise", 0, 8), a.trees, keep)
    report("depthwise depth 8", d_ms, d_leaves)
    ms, leaves, dumps = run(a, bsp, dm, cuts, B, param(a, "lossguide", 256, 8), a.trees, keep)
    report("lossguide max_leaves=256 max_depth=8", ms, leaves, vs_depthwise=ms / d_ms,
           us_per_step=1000 * ms / 255, dumps_equal_depthwise=dumps == d_dumps)
    for L in (255, 64):
        for dev_loop in (True, False):
            G.LEAF_LOOP_DEV = dev_loop
            trees = a.trees if dev_loop else a.py_trees
            ms, leaves, _ = run(a, bsp, dm, cuts, B, param(a, "lossguide", L, 0), trees)
            report("lossguide max_leaves=%d max_depth=0, %s leaf loop"
                   % (L, "device" if dev_loop else "Python"), ms, leaves, vs_depthwise=ms / d_ms,
                   us_per_step=1000 * ms / (L - 1))
    G.LEAF_LOOP_DEV = True
    bsp.finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
