#!/usr/bin/env python3
"""booster=dart benchmark on bench_gbdt.py's shape (Higgs-shaped 11M x 28,
depth 8): the dropout walk in isolation and a boosting round end to end.

    python benchmarks/bench_gbdt_dart.py [--rows 11000000] [--rounds 100] [--rate-drop 0.1]

In isolation: ms per dropped tree of k_dart_walk (the resident u8 bins, a
chunk of trees per pass, from LDS) at several (LDS node budget, rows per tile)
settings, and of the raw-row forest kernel on the same rows and the same trees
with the same coefficients -- both timed in this process, results compared bit
for bit. End to end: ms per round of gbtree, of dart with the binned walk and
of dart with the forest-kernel fallback. One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wormhole_amd.models import gbdt as G  # noqa: E402
from wormhole_amd.models import gbdt_dart  # noqa: E402
from wormhole_amd.models.gbdt_tree import Forest  # noqa: E402
from wormhole_amd.parallel.bsp import BSP  # noqa: E402
from bench_gbdt import higgs_like  # noqa: E402

SETTINGS = ((8192, 256), (8192, 512), (8192, 1024), (4096, 512), (4096, 1024))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=11_000_000)
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--rate-drop", type=float, default=0.1)
    ap.add_argument("--iso-trees", type=int, default=32, help="trees of the isolated walks")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    bsp = BSP(dev)
    n = a.rows
    X, y = higgs_like(n, a.features, 7, dev)
    dm = G.DMatrix.from_dense(X, y, dev)

    def param(booster):
        p = G.GBDTParam()
        p.objective, p.max_depth, p.eta, p.max_bin = "binary:logistic", a.depth, 0.1, 256
        p.set("booster", booster)
        p.set("rate_drop", str(a.rate_drop))
        return p
    p = param("gbtree")
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    B = cuts.bin(dm)
    shape = "%dx%d depth %d" % (n, a.features, a.depth)

    # ---- in isolation: the same trees, rows and coefficients
    b = G.Booster(p, dm.ncol)
    tb = G.TreeBuilder(p, bsp, dm, cuts, B)
    margin = b.predict_margin(dm)
    for _ in range(a.iso_trees):
        b.trees += G.boost_round(b.obj, tb, dm, margin)
    sel = list(range(a.iso_trees))
    coef = [1.0 / (1 + (j % 7)) for j in sel]
    nodes = sum(len(b.trees[t].feat) for t in sel)
    forest = Forest([b.trees[t] for t in sel], dev,
                    [b.eff_leaf(t, c) for t, c in zip(sel, coef)])
    out = torch.zeros(n, device=dev)
    ms = timed(lambda: dm.predict_forest(forest, out), a.reps)
    ref = torch.zeros(n, device=dev)
    dm.predict_forest(forest, ref)
    print(json.dumps({"metric": "dart dropped-tree walk, raw-row forest kernel (%s)" % shape,
                      "value": ms / len(sel), "unit": "ms/tree", "trees": len(sel),
                      "nodes": nodes}), flush=True)
    for lds_nodes, rows in SETTINGS:
        table = G.DartForest(dev, tb._cut_lists, lds_nodes=lds_nodes, rows=rows)
        for t in b.trees:
            table.append(t, True)
        chunks = table.plan(sel)

        def walk(o=out):
            table.walk(B, sel, coef, o, None)
        ms = timed(walk, a.reps)
        got = torch.zeros(n, device=dev)
        walk(got)
        print(json.dumps({"metric": "dart dropped-tree walk, k_dart_walk (%s)" % shape,
                          "value": ms / len(sel), "unit": "ms/tree", "trees": len(sel),
                          "lds_nodes": lds_nodes, "rows_per_tile": rows, "chunks": len(chunks),
                          "grid": G._native.hip().gbdt_dart_grid(
                              n=n, f=a.features, ntree=chunks[0][1], nnode=chunks[0][2], rows=rows),
                          "equal_to_forest_kernel": bool(torch.equal(got, ref))}), flush=True)
    del out, ref, got, forest

    # ---- end to end: ms per round
    if a.skip_e2e:
        return 0
    for name, booster, binned in (("gbtree", "gbtree", True), ("dart, binned walk", "dart", True),
                                  ("dart, forest-kernel fallback", "dart", False)):
        G.DART_BIN_WALK = binned
        p = param(booster)
        b = G.Booster(p, dm.ncol)
        tb = G.TreeBuilder(p, bsp, dm, cuts, B)
        margin = b.predict_margin(dm)
        tr = G.DartTrainer(b, tb, dm) if booster == "dart" else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r in range(a.rounds):
            if tr is not None:
                tr.round(r, margin)
            else:
                b.trees += G.boost_round(b.obj, tb, dm, margin)
        b.trees[-1].feat  # (a deferred tree's host lists: inside the timed region)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        err = b.obj.metrics([b.obj.default_metric()], margin, dm.label, None, bsp)[0]
        print(json.dumps({"metric": "GBDT ms/round, %s (%s)" % (name, shape),
                          "value": 1000 * dt / a.rounds, "unit": "ms/round", "rounds": a.rounds,
                          "rate_drop": a.rate_drop if tr is not None else None,
                          "dropped_trees_walked": tr.walks if tr is not None else 0,
                          "rows_per_tile": gbdt_dart.DART_WALK_ROWS if tr is not None else None,
                          "train_error": err}), flush=True)
    G.DART_BIN_WALK = True
    bsp.finalize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
