"""Random forests and rows for the forest prediction tests (CPU and GPU), and
a plain Python per-row walk to compare against.

Thresholds and feature values come from one grid of quarter-integers, so a
value equal to its threshold (which goes right) happens all the time; leaf
values are arbitrary fp32 numbers, so the order of the additions shows."""
import functools
import random

import numpy as np
import torch

GRID = [q / 4.0 for q in range(-6, 7)]


def random_tree(rng, F, max_depth, split_p):
    """A RegTree of random shape (depth <= max_depth; split_p = 0: a single
    leaf; 1: complete), renumbered breadth-first as every model tree is."""
    from wormhole_amd.models.gbdt import RegTree
    t = RegTree()
    todo = [(t.add(-1), 0)]
    while todo:
        i, d = todo.pop()
        if d < max_depth and rng.random() < split_p:
            t.feat[i] = rng.randrange(F)
            t.cond[i] = rng.choice(GRID)
            t.defl[i] = rng.randrange(2)
            t.left[i], t.right[i] = t.add(i), t.add(i)
            todo += [(t.left[i], d + 1), (t.right[i], d + 1)]
        else:
            t.leaf[i] = float(np.float32(rng.gauss(0.0, 1.0)))
    return t.compact()


def random_forest(seed, F, total_nodes, max_depth=8, oversize=0, multiple_of_3_plus=1):
    """Trees of depth <= max_depth, single leaves among them, until about
    total_nodes nodes; oversize > 0: one complete tree with more than that
    many nodes in the middle. len(forest) % 3 == multiple_of_3_plus."""
    rng = random.Random(seed)
    trees, nn = [], 0
    while nn < total_nodes or len(trees) % 3 != multiple_of_3_plus:
        p = rng.choice([0.0, 0.6, 0.8, 0.9, 0.97])
        trees.append(random_tree(rng, F, max_depth, p))
        nn += len(trees[-1].feat)
    if oversize:
        depth = 1
        while (2 << depth) - 1 <= oversize:
            depth += 1
        trees[len(trees) // 2] = random_tree(rng, F, depth, 1.0)
    return trees


@functools.lru_cache(maxsize=None)
def rows(n, F, nan_share, seed=0):
    """fp32 [n, F] on the grid, nan_share of the cells NaN, row n // 2 all NaN."""
    g = torch.Generator().manual_seed(seed + 31 * n + F)
    X = torch.tensor(GRID)[torch.randint(0, len(GRID), (n, F), generator=g)]
    if nan_share:
        X[torch.rand(n, F, generator=g) < nan_share] = float("nan")
    if n:
        X[n // 2] = float("nan")
    return X


def csr_of(X):
    """(keys, offset, val) of the non-NaN cells: absent stands for NaN."""
    keep = ~torch.isnan(X)
    r, c = keep.nonzero(as_tuple=True)
    off = torch.zeros(X.shape[0] + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(keep.sum(1), 0)
    return c.to(torch.int64), off, X[r, c]


def walk(tree, row):
    """The leaf's node id: NaN takes the default, v < thr goes left."""
    i = 0
    while tree.feat[i] >= 0:
        v = row[tree.feat[i]]
        left = bool(tree.defl[i]) if v != v else v < np.float32(tree.cond[i])
        i = tree.left[i] if left else tree.right[i]
    return i


def python_reference(trees, X, K, base):
    """(leaf ids [n, T], margins [n] or [K, n]) by the per-row walk, margins
    added in fp32 in tree order, tree t to class t % K."""
    Xl = X.tolist()
    ids = np.zeros((len(Xl), len(trees)), dtype=np.int32)
    margin = np.full((K, len(Xl)), base, dtype=np.float32)
    for r, row in enumerate(Xl):
        for t, tree in enumerate(trees):
            ids[r, t] = walk(tree, row)
            margin[t % K, r] = margin[t % K, r] + np.float32(tree.leaf[ids[r, t]])
    m = torch.from_numpy(margin)
    return torch.from_numpy(ids), (m[0] if K == 1 else m)


def margins_from_ids(trees, ids, K, base):
    """The statement of RegTree.predict_margin (margin += leaf[leaf index]) per
    tree, in tree order, on leaf ids already known."""
    n = ids.shape[0]
    margin = torch.full((K, n), base, dtype=torch.float32)
    for t, tree in enumerate(trees):
        margin[t % K] += torch.tensor(tree.leaf)[ids[:, t].long()]
    return margin[0] if K == 1 else margin


def booster(trees, K):
    from wormhole_amd.models import gbdt as G
    p = G.GBDTParam()
    if K > 1:
        p.objective, p.num_class = "multi:softprob", K
    b = G.Booster(p, 0)
    b.trees = list(trees)
    return b
