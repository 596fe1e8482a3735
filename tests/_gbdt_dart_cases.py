"""Data, training and bounds shared by the booster=dart tests (CPU and GPU)."""
import functools

import numpy as np
import torch

import _gbdt_forest_cases as fc
import _gbdt_monotone_cases as M

F32 = np.float32


def param(G, K=1, **kw):
    p = M.param(G, max_depth=3, booster="dart")
    if K > 1:
        p.objective, p.num_class = "multi:softprob", K
    for k, v in kw.items():
        assert p.set(k, str(v)), k
    return p


@functools.lru_cache(maxsize=None)
def labels(n, K):
    """The regression target of the monotone recipe, or its K quantile classes."""
    X, y = M.data(n, 4)
    if K == 1:
        return X, y
    q = torch.quantile(y, torch.arange(1, K) / K)
    return X, torch.bucketize(y, q).float()


def setup(G, bsp, p, n, K, device, sparse=False):
    """(matrix, booster, builder) ready for round 0."""
    X, y = labels(n, K)
    dm = M.dmatrix(G, X, y, device, sparse)
    b = G.Booster(p, dm.ncol)
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    return dm, b, G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))


def gens(p):
    return torch.Generator().manual_seed(p.seed + 17), torch.Generator().manual_seed(p.seed)


def train_dart(G, bsp, p, n, K, device, rounds, sparse=False, evals=0, each=None):
    """(booster, trainer, training margins, eval margins) after ``rounds``
    dart rounds; the eval sets are the first ``evals`` rows of the data.
    each(booster, trainer): called after every round."""
    dm, b, tb = setup(G, bsp, p, n, K, device, sparse)
    ev = []
    if evals:
        X, y = labels(n, K)
        d = M.dmatrix(G, X[:evals], y[:evals], device, sparse)
        ev = [(d, b.predict_margin(d))]
    tr = G.DartTrainer(b, tb, dm, ev)
    margin = b.predict_margin(dm)
    gen, fgen = gens(p)
    for r in range(rounds):
        tr.round(r, margin, gen, fgen)
        if each is not None:
            each(b, tr)
    return b, tr, margin, ev


def train_gbtree(G, bsp, p, n, K, device, rounds, sparse=False):
    dm, b, tb = setup(G, bsp, p, n, K, device, sparse)
    margin = b.predict_margin(dm)
    gen, fgen = gens(p)
    for _ in range(rounds):
        b.trees += G.boost_round(b.obj, tb, dm, margin, gen, fgen)
    return b


def model_bytes(b, path):
    b.save(str(path))
    with open(path, "rb") as f:
        return f.read()


def magnitude(b, weights=None):
    """|base| + sum_t |w_t| max|leaf_t|: what bounds every margin and partial
    sum of the model (weights: others than the model's own)."""
    w = b.weights() if weights is None else weights
    return abs(b.base_margin) + sum(abs(wt) * max(abs(v) for v in t.leaf)
                                    for wt, t in zip(w, b.trees))


def fp32_ops(history, ntree):
    """fp32 operations per row on both paths to a margin: the kept one (per
    round with k dropped rounds: a product per coefficient, a product and a
    sum per walked tree, the new tree's sum, and the update's two products
    and two sums: at most 3 k + 6) and predict_margin's (a product and a sum
    per tree)."""
    return sum(3 * len(drop) + 6 for _, drop in history) + 2 * ntree


def rounding_bound(ops, S):
    return 2.0 ** -23 * ops * S


# ------------------------------------------------- the walk kernel's cases
def grid_cuts(F):
    """Cuts on the forest cases' grid: every tree threshold is a cut, and a
    row on the grid goes left by its bin exactly as by its value."""
    top = fc.GRID[-1] + abs(fc.GRID[-1]) + 1.0
    vals = (fc.GRID + [top]) * F
    off = [j * (len(fc.GRID) + 1) for j in range(F + 1)]
    return vals, off


def grid_bins(X):
    """uint8 [n, F]: the bins of rows on the grid under grid_cuts (255 = NaN)."""
    c = torch.tensor(fc.GRID + [fc.GRID[-1] + abs(fc.GRID[-1]) + 1.0])
    B = torch.searchsorted(c, torch.nan_to_num(X, 0.0).contiguous(), right=True)
    B = B.clamp(max=c.numel() - 1).to(torch.uint8)
    B[torch.isnan(X)] = 255
    return B


def torch_reference(trees, X, sel, coef, out):
    """out + sum_j float32(coef_j) * float32(leaf_j(row)), in order, fp32."""
    acc = out.clone()
    for t, c in zip(sel, coef):
        tree = trees[t]
        leaf = torch.from_numpy(F32(c) * np.asarray(tree.leaf, dtype=np.float32))
        acc = acc + leaf[tree.leaf_index(X)]
    return acc
