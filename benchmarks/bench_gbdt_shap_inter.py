#!/usr/bin/env python3
"""GBDT SHAP interaction values: exact contributions (predict_contribs) and
interactions (predict_interactions) on the same dense matrix and forest in
one process.

    python benchmarks/bench_gbdt_shap_inter.py [--rows 100000] [--trees 100]

Matrix and forest are those of bench_gbdt_shap.py (rows x 28 fp32, 2 % NaN;
full depth-8 trees with synthetic covers). The first 64 rows are first checked
against the host float64 reference (within 8 x the host fp32 reference's own
error). Each call is timed by device events around one whole call that ends
in a synchronise, after one warm-up call; the median, minimum and maximum of
--reps repetitions are printed, and the ratio of the medians beside the mean
length of the forest's merged paths (the work per path grows by about its
length). An interactions call includes the exact-contributions launches that
give its diagonal. Needs a GPU.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_gbdt_shap import full_tree, stats, timed  # noqa: E402
from wormhole_amd.models import gbdt as G  # noqa: E402


def check(b, X):
    """The first 64 rows against the host float64 reference."""
    hip = G._native.hip()
    kw = dict(feat=[t.feat for t in b.trees], cond=[t.cond for t in b.trees],
              left=[t.left for t in b.trees], right=[t.right for t in b.trees],
              defl=[t.defl for t in b.trees], leaf=[t.leaf for t in b.trees],
              cover=[t.cover for t in b.trees])
    Xc = X[:64].cpu().contiguous()
    ref, _ = hip.gbdt_shap_inter_rows(num_class=1, base=b.base_margin, X=Xc, **kw)
    f32, _ = hip.gbdt_shap_inter_rows(num_class=1, base=b.base_margin, X=Xc, f32=True, **kw)
    dm = G.DMatrix.from_dense(X[:64], torch.zeros(64), X.device)
    got, _ = b.predict_interactions(dm, compact=True)
    err32 = float((f32 - ref).abs().max())
    err = float((got.cpu().double() - ref[0]).abs().max())
    if err > 8 * err32:
        raise SystemExit("interactions differ from the host reference: %g > 8 x %g" % (err, err32))
    if not torch.equal(got, got.transpose(-1, -2)):
        raise SystemExit("interactions are not symmetric")
    return err32, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000])
    ap.add_argument("--features", type=int, default=28)
    ap.add_argument("--trees", type=int, nargs="+", default=[100])
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gbdt_shap_inter needs a GPU")
    dev = torch.device("cuda", 0)
    hip = G._native.hip()
    rng = np.random.default_rng(7)
    trees = [full_tree(rng, a.depth, a.features) for _ in range(max(a.trees))]
    print("# ms per whole call: median [min, max] of %d calls after one warm-up; depth %d, %d "
          "features; chunk capacity %d path elements, LDS triangle up to %d columns" % (
              a.reps, a.depth, a.features, hip.gbdt_shap_lds_elems(),
              hip.gbdt_shap_inter_lds_cols()))
    for n in a.rows:
        g = torch.Generator(device=dev).manual_seed(n)
        X = torch.randn(n, a.features, device=dev, generator=g)
        X[torch.rand(n, a.features, device=dev, generator=g) < 0.02] = float("nan")
        dm = G.DMatrix.from_dense(X, torch.zeros(n), dev)
        for T in a.trees:
            b = G.Booster(G.GBDTParam(), a.features)
            b.trees = trees[:T]
            sf = b.shap_forest(dev)
            lens = sf.paths[:, 1].double()
            err32, err = check(b, X)
            calls = {"exact": lambda: b.predict_contribs(dm, compact=True),
                     "inter": lambda: b.predict_interactions(dm, compact=True)}
            ms = {}
            for name, fn in calls.items():
                fn()  # warm-up
                torch.cuda.synchronize()
                ms[name] = [timed(fn)[0] for _ in range(a.reps)]
            med = {k: statistics.median(v) for k, v in ms.items()}
            U = sf.used.numel()
            acc = "LDS" if U <= hip.gbdt_shap_inter_lds_cols() else "global"
            print("n=%d T=%d exact_ms=%s inter_ms=%s inter/exact=%.2f mean_path_len=%.2f "
                  "mean_len_sq_over_mean_len=%.2f inter_rowtrees_per_s=%.3g chunks=%d U=%d "
                  "accumulator=%s check64: err32 %.3g gpu %.3g" % (
                      n, T, stats(ms["exact"]), stats(ms["inter"]), med["inter"] / med["exact"],
                      float(lens.mean()), float((lens * lens).sum() / lens.sum()),
                      n * T / med["inter"] * 1e3, len(sf.chunks), U, acc, err32, err), flush=True)
        del X, dm
    return 0


if __name__ == "__main__":
    sys.exit(main())
