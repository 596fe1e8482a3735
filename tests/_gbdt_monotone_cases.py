"""Data, training and checks shared by the monotone_constraints tests (CPU
and GPU).

The recipe: integer levels 0..47 per feature (few distinct values, so the
quantile cuts are exact for any rank count), 8 % missing, and a target that
rises with feature 0 and falls with feature 1 only on average -- the sin / cos
ripples make an unconstrained model break the guarantee many times over
(n=4000, f=4, reg:linear, depth 5, eta 0.5, 64 bins, 4 rounds: 25 of its 37
splits on feature 0 and 17 of its 31 on feature 1 -- counted with this
module's ``data()``, whose generator draws the levels, then the missing mask,
then the noise; another draw order gives other counts), so a test that passes only
because nothing was at stake is caught by its unconstrained control."""
import functools

import torch

SEED, N, F, LEVELS = 11, 4000, 4, 48
MONO = (1, -1, 0, 0)
ROUNDS = 4


@functools.lru_cache(maxsize=None)
def data(n=N, f=F):
    """(X [n, f] float32 with NaN, y [n]); never written to."""
    g = torch.Generator().manual_seed(SEED)
    X = torch.randint(0, LEVELS, (n, f), generator=g).float()
    X[torch.rand(n, f, generator=g) < 0.08] = float("nan")
    x = torch.nan_to_num(X, LEVELS / 2) / LEVELS
    y = (x[:, 0] + 0.35 * torch.sin(12 * x[:, 0]) - x[:, 1] + 0.35 * torch.cos(10 * x[:, 1])
         + x[:, 2] * x[:, 3] + 0.1 * torch.randn(n, generator=g))
    return X, y


def cycled(f, pattern=(1, -1, 0)):
    return tuple(pattern[j % len(pattern)] for j in range(f))


def param(G, mono=None, **kw):
    p = G.GBDTParam()
    p.objective, p.max_depth, p.eta, p.max_bin = "reg:linear", 5, 0.5, 64
    for k, v in kw.items():
        setattr(p, k, v)
    if mono is not None:
        assert p.set("monotone_constraints", "(%s)" % ",".join(str(c) for c in mono))
    return p


def csr_of(X):
    """(keys, offset, val) of the non-NaN cells: absent stands for NaN."""
    keep = ~torch.isnan(X)
    r, c = keep.nonzero(as_tuple=True)
    off = torch.zeros(X.shape[0] + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(keep.sum(1), 0)
    return c.to(torch.int64), off, X[r, c]


def dmatrix(G, X, y, device, sparse=False):
    if not sparse:
        return G.DMatrix.from_dense(X, y, device)
    keys, off, val = csr_of(X)
    return G.make_dmatrix(keys, off, val, y, None, X.shape[1], device, sparse=True)


def train(G, bsp, dm, p, rounds=ROUNDS):
    """(booster, training margins) after ``rounds`` boosting rounds."""
    b = G.Booster(p, dm.ncol)
    margin = b.predict_margin(dm)
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    tb = G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
    gen, fgen = torch.Generator().manual_seed(p.seed + 17), torch.Generator().manual_seed(p.seed)
    for _ in range(rounds):
        b.trees += G.boost_round(b.obj, tb, dm, margin, gen, fgen)
    for t in b.trees:
        t.feat  # (a deferred device tree builds its lists)
    return b, margin


def _leaves(t, i):
    if t.feat[i] < 0:
        return [t.leaf[i]]
    return _leaves(t, t.left[i]) + _leaves(t, t.right[i])


def structure(trees, mono):
    """{feature: (splits on it, splits that break the guarantee)} over the
    constrained features: a split on a +1 feature holds when every leaf of its
    left subtree is <= every leaf of its right one (-1: >=)."""
    out = {j: [0, 0] for j, c in enumerate(mono) if c}
    for t in trees:
        for i, f in enumerate(t.feat):
            if f < 0 or f >= len(mono) or not mono[f]:
                continue
            l, r = _leaves(t, t.left[i]), _leaves(t, t.right[i])
            bad = max(l) > min(r) if mono[f] > 0 else min(l) < max(r)
            out[f][0] += 1
            out[f][1] += int(bad)
    return {j: tuple(v) for j, v in out.items()}


def holds(trees, mono):
    s = structure(trees, mono)
    return all(bad == 0 for _, bad in s.values())


def sweep(G, booster, X, feat, device, rows=50):
    """Margins [rows, LEVELS] of the first rows with feature ``feat`` set to
    every level in turn (class 0 of a multi-class model)."""
    base = X[:rows].clone()
    grid = base[:, None, :].repeat(1, LEVELS, 1)
    grid[:, :, feat] = torch.arange(LEVELS, dtype=torch.float32)[None, :]
    dm = G.DMatrix.from_dense(grid.reshape(-1, X.shape[1]), torch.zeros(rows * LEVELS), device)
    m = booster.predict_margin(dm)
    return (m if m.dim() == 1 else m[0]).cpu().reshape(rows, LEVELS)


def write_libsvm(path, X, y):
    with open(path, "w") as f:
        for row, lab in zip(X.tolist(), y.tolist()):
            f.write("%r %s\n" % (lab, " ".join("%d:%g" % (j, v) for j, v in enumerate(row)
                                                if v == v)))
