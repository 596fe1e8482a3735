#!/usr/bin/env python3
"""GBDT feature contributions: predict_margin (the forest kernels), exact
contributions (TreeSHAP) and approximate contributions (Saabas) on the same
dense matrix and forest in one process.

    python benchmarks/bench_gbdt_shap.py [--rows 100000] [--trees 100]

The matrix is synthetic (rows x 28 fp32, 2 % NaN) and so is the forest: full
depth-8 trees built directly as RegTree lists, a child's cover a random
fraction in [0.1, 0.9] of its parent's. The first 64 rows are first checked
against the host float64 reference (within 8 x the host fp32 reference's own
error). Each call is timed by device events around one whole call that ends
in a synchronise, after one warm-up call; the median, minimum and maximum of
--reps repetitions are printed, with rows x trees per second and the ratio to
predict_margin. The one-time pack and upload is reported apart. Needs a GPU.
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
    """A complete tree in breadth-first numbering (node i splits into 2i + 1,
    2i + 2) with covers."""
    inner, nn = (1 << depth) - 1, (2 << depth) - 1
    t = G.RegTree()
    t.feat = rng.integers(0, F, nn).tolist()
    t.cond = rng.normal(0, 1, nn).astype(np.float32).tolist()
    t.defl = rng.integers(0, 2, nn).tolist()
    t.left = [2 * i + 1 for i in range(nn)]
    t.right = [2 * i + 2 for i in range(nn)]
    t.leaf = (rng.normal(0, 0.1, nn).astype(np.float32)).tolist()
    t.parent = [-1] + [(i - 1) // 2 for i in range(1, nn)]
    cover = np.zeros(nn)
    cover[0] = 1000.0
    frac = rng.uniform(0.1, 0.9, nn)
    for i in range(inner):
        cover[2 * i + 1] = np.float32(cover[i] * frac[i])
        cover[2 * i + 2] = np.float32(cover[i] * (1.0 - frac[i]))
        t.leaf[i] = 0.0
    for i in range(inner, nn):
        t.feat[i], t.left[i], t.right[i], t.cond[i], t.defl[i] = -1, -1, -1, 0.0, 0
    t.bin = [0] * nn
    t.gain, t.cover, t.base_weight = [0.0] * nn, cover.tolist(), [0.0] * nn
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


def check(b, X, approx):
    """The first 64 rows against the host float64 reference."""
    hip = G._native.hip()
    kw = dict(feat=[t.feat for t in b.trees], cond=[t.cond for t in b.trees],
              left=[t.left for t in b.trees], right=[t.right for t in b.trees],
              defl=[t.defl for t in b.trees], leaf=[t.leaf for t in b.trees],
              cover=[t.cover for t in b.trees])
    Xc = X[:64].cpu().contiguous()
    ref, _ = hip.gbdt_shap_rows(num_class=1, base=b.base_margin, X=Xc, approx=approx, **kw)
    f32, _ = hip.gbdt_shap_rows(num_class=1, base=b.base_margin, X=Xc, approx=approx, f32=True,
                                **kw)
    dm = G.DMatrix.from_dense(X[:64], torch.zeros(64), X.device)
    got, _ = b.predict_contribs(dm, approx=approx, compact=True)
    err32 = float((f32 - ref).abs().max())
    err = float((got.cpu().double() - ref[0]).abs().max())
    if err > 8 * err32:
        raise SystemExit("contributions (approx=%d) differ from the host reference: %g > 8 x %g"
                         % (approx, err, err32))
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
        raise SystemExit("bench_gbdt_shap needs a GPU")
    dev = torch.device("cuda", 0)
    hip = G._native.hip()
    rng = np.random.default_rng(7)
    trees = [full_tree(rng, a.depth, a.features) for _ in range(max(a.trees))]
    print("# ms per whole call: median [min, max] of %d calls after one warm-up; depth %d, %d "
          "features; chunk capacity %d path elements, LDS accumulator up to %d columns" % (
              a.reps, a.depth, a.features, hip.gbdt_shap_lds_elems(), hip.gbdt_shap_lds_cols()))
    for n in a.rows:
        g = torch.Generator(device=dev).manual_seed(n)
        X = torch.randn(n, a.features, device=dev, generator=g)
        X[torch.rand(n, a.features, device=dev, generator=g) < 0.02] = float("nan")
        dm = G.DMatrix.from_dense(X, torch.zeros(n), dev)
        for T in a.trees:
            b = G.Booster(G.GBDTParam(), a.features)
            b.trees = trees[:T]
            t0 = time.perf_counter()
            sf = b.shap_forest(dev)
            torch.cuda.synchronize()
            pack_ms = (time.perf_counter() - t0) * 1e3
            b.forest(dev)
            e_exact, e_approx = check(b, X, False), check(b, X, True)
            calls = {"margin": lambda: b.predict_margin(dm),
                     "exact": lambda: b.predict_contribs(dm, compact=True),
                     "approx": lambda: b.predict_contribs(dm, approx=True, compact=True)}
            ms = {}
            for name, fn in calls.items():
                fn()  # warm-up
                torch.cuda.synchronize()
                ms[name] = [timed(fn)[0] for _ in range(a.reps)]
            med = {k: statistics.median(v) for k, v in ms.items()}
            acc = "LDS" if sf.used.numel() + 1 <= hip.gbdt_shap_lds_cols() else "global"
            print("n=%d T=%d margin_ms=%s exact_ms=%s approx_ms=%s exact_rowtrees_per_s=%.3g "
                  "approx_rowtrees_per_s=%.3g exact/margin=%.1f approx/margin=%.2f "
                  "pack_once_ms=%.1f chunks=%d accumulator=%s check64: exact err32 %.3g gpu %.3g, "
                  "approx err32 %.3g gpu %.3g" % (
                      n, T, stats(ms["margin"]), stats(ms["exact"]), stats(ms["approx"]),
                      n * T / med["exact"] * 1e3, n * T / med["approx"] * 1e3,
                      med["exact"] / med["margin"], med["approx"] / med["margin"], pack_ms,
                      len(sf.chunks), acc, *e_exact, *e_approx), flush=True)
        del X, dm
    return 0


if __name__ == "__main__":
    sys.exit(main())
