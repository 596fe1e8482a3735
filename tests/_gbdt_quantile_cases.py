"""Data, fp64 checks and the training recipes shared by the absolute / quantile
error tests (CPU and GPU).

Unless a case says otherwise the row weights are integers in 0..4 and every
alpha is dyadic, so each weight sum and each threshold alpha * W is exact in
fp64 and in any power-of-two fixed point: the tests ask for equality."""
import functools
import math
import os

import torch

import _gbdt_monotone_cases as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALPHAS = (0.125, 0.5, 0.75)


# ------------------------------------------------------ the definition, fp64
def brute_quantile(r, u, alpha):
    """The definition of docs/bsp_apps.md "Absolute and quantile error" on one
    segment, in Python floats: (q, W). r: fp32 residuals, u: the (rounded)
    weights; q is None when W = 0."""
    r, u = [float(x) for x in r], [float(x) for x in u]
    W = math.fsum(u)
    if W == 0:
        return None, 0.0
    best = None
    for v in r:
        if math.fsum(ui for ri, ui in zip(r, u) if ri <= v) >= alpha * W:
            best = v if best is None or v < best else best
    return best + 0.0, W  # (-0.0 and +0.0 are one value: +0.0)


def check_thresholds(weight_sums, alphas):
    """The case builder's guard for non-dyadic alphas: alpha * W is not within
    1e-9 of an integer for any leaf."""
    for W in weight_sums:
        for a in alphas:
            t = a * W
            assert abs(t - round(t)) > 1e-9 or float(a * 1024).is_integer(), (a, W)


def pinball64(alphas, margin, label, weight):
    """The ``quantile`` metric in fp64 from margins [K, n] (or [n])."""
    m = margin.double().reshape(len(alphas), -1)
    y = label.double()
    w = weight.double() if weight is not None else torch.ones_like(y)
    tot = 0.0
    for k, a in enumerate(alphas):
        d = y - m[k]
        tot += float((w * torch.where(d >= 0, a * d, (a - 1) * d)).sum())
    return tot / (len(alphas) * float(w.sum()))


def gpair64(alpha, margin, label, weight, absolute=False):
    """The gradient pairs [n, 2] in fp64 (d = m - y taken in fp32)."""
    d = (margin.float() - label.float()).double()
    w = weight.double() if weight is not None else torch.ones_like(d)
    if absolute:
        g = torch.sign(d)
    else:
        g = torch.where(d >= 0, torch.full_like(d, 1 - alpha), torch.full_like(d, -alpha))
    return torch.stack([g * w, w], 1)


# --------------------------------------------------------------- the select
def select_case(n, L, seed, weights="int", keys="random"):
    """(ridx int32 [n] a permutation, segs [(b, e)] x L tiling [0, n) unevenly
    with empty segments, label, at, weight or None): inputs of the select."""
    g = torch.Generator().manual_seed(seed)
    ridx = torch.randperm(n, generator=g).to(torch.int32)
    if L == 1:
        cuts = [0, n]
    else:
        c = torch.sort(torch.randint(0, n + 1, (L - 1,), generator=g)).values.tolist()
        if L > 2:
            c[1] = c[0]  # an empty segment for certain
        cuts = [0] + c + [n]
    segs = list(zip(cuts[:-1], cuts[1:]))
    if keys == "top":  # residuals that differ only in the top byte of the key
        r = torch.tensor([1.0, 2.0 ** 64, -1.0, -(2.0 ** 64), 2.0 ** -64])[
            torch.randint(0, 5, (n,), generator=g)]
    elif keys == "bottom":  # ... only in the bottom byte
        base = torch.tensor([1.5]).view(torch.int32)
        r = (base + torch.randint(0, 200, (n,), generator=g).to(torch.int32)).view(torch.float32)
    elif keys == "boundary":  # duplicates on both sides of a digit boundary
        base = torch.tensor([2.0]).view(torch.int32)  # 0x40000000: bytes below are 0
        r = (base + torch.randint(-2, 2, (n,), generator=g).to(torch.int32) * 128).view(
            torch.float32)
    elif keys == "equal":
        r = torch.full((n,), -0.75)
    elif keys == "zeros":  # -0.0, +0.0 and denormals of both signs
        r = torch.tensor([0.0, -0.0, 1e-42, -1e-42, 3e-45])[torch.randint(0, 5, (n,), generator=g)]
    else:
        r = torch.randn(n, generator=g) * 3
    at = torch.randn(n, generator=g)
    if keys != "random":
        at = torch.zeros(n)
    label = r if keys != "random" else (r + at)
    if weights == "none":
        w = None
    elif weights == "int":
        w = torch.randint(0, 5, (n,), generator=g).float()
    elif weights == "zeros":
        w = (torch.rand(n, generator=g) < 0.3).float() * 2
    else:  # fractional
        w = torch.rand(n, generator=g) * 1.5
    return ridx, segs, label.float(), at.float(), w


# ---------------------------------------------------------------- training
@functools.lru_cache(maxsize=None)
def train_data(n=2000, f=4, seed=3):
    """(X with NaN, y, integer weights 0..4); never written to."""
    X, y = M.data(n, f)
    g = torch.Generator().manual_seed(seed)
    return X, y, torch.randint(0, 5, (n,), generator=g).float()


@functools.lru_cache(maxsize=None)
def interval_data(n=4000, seed=5):
    """Rows whose label is 3 x_0 plus noise that does not depend on x."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, 3, generator=g)
    return X, (3 * X[:, 0] + torch.randn(n, generator=g)).float()


def dmatrix(G, X, y, w, device, sparse=False):
    if not sparse:
        dm = G.DMatrix.from_dense(X, y, device)
        dm.weight = w.to(device) if w is not None else None
        return dm
    keys, off, val = M.csr_of(X)
    return G.make_dmatrix(keys, off, val, y, w, X.shape[1], device, sparse=True)


def param(G, objective, **kw):
    p = G.GBDTParam()
    p.objective, p.max_depth, p.eta, p.max_bin = objective, 3, 1.0, 64
    for k, v in kw.items():
        assert p.set(k, str(v)), k
    return p


def train(G, bsp, dm, p, rounds):
    """(booster, training margins) the way the app trains."""
    b = G.Booster(p, dm.ncol)
    margin = b.predict_margin(dm)
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    tb = G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
    gen, fgen = torch.Generator().manual_seed(p.seed + 17), torch.Generator().manual_seed(p.seed)
    dart = G.DartTrainer(b, tb, dm) if p.booster == "dart" else None
    for r in range(rounds):
        if dart is not None:
            dart.round(r, margin, gen, fgen)
        else:
            b.trees += G.boost_round(b.obj, tb, dm, margin, gen, fgen)
    for t in b.trees:
        t.feat  # (a deferred device tree builds its lists)
    return b, margin


def leaves_of(tree):
    return [i for i in range(len(tree.feat)) if tree.feat[i] < 0]


def squarederror_model(G, bsp, device, path):
    """The model whose bytes tests/golden keeps from before the adaptive
    objectives: reg:squarederror with pruning, row and feature sampling."""
    X, y, w = train_data()
    p = param(G, "reg:squarederror", max_depth=5, eta=0.5, gamma=0.05, subsample=0.8,
              colsample_bytree=0.75, seed=4)
    b, _ = train(G, bsp, dmatrix(G, X, y, w, device), p, 4)
    b.save(path)
    return open(path, "rb").read()
