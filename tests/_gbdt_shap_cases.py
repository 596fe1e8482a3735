"""Trees with cover statistics for the contribution tests (CPU and GPU), and
independent Python statements of what the contributions are: the Shapley sum
over subsets, the bias, and the Saabas walk.

Shapes, thresholds, leaf values and rows are those of _gbdt_forest_cases.py
(quarter-integer grid: a value equal to its threshold is common). A child's
cover is a fraction in [0.1, 0.9] of its parent's, rounded to fp32 as the
model file stores it."""
import itertools
import math
import random

import numpy as np

import _gbdt_forest_cases as fc


def add_covers(rng, tree):
    """Covers down from the root (children lie beyond their parent)."""
    tree.cover = [0.0] * len(tree.feat)
    tree.cover[0] = float(np.float32(rng.uniform(50.0, 500.0)))
    for i in range(len(tree.feat)):
        if tree.feat[i] >= 0:
            frac = rng.uniform(0.1, 0.9)
            tree.cover[tree.left[i]] = float(np.float32(tree.cover[i] * frac))
            tree.cover[tree.right[i]] = float(np.float32(tree.cover[i] * (1.0 - frac)))
    return tree


def random_forest(seed, F, total_nodes, max_depth=8, multiple_of_3_plus=1):
    rng = random.Random(seed + 7)
    return [add_covers(rng, t) for t in
            fc.random_forest(seed, F, total_nodes, max_depth, 0, multiple_of_3_plus)]


def forest_of_elems(seed, F, elems, max_depth=8):
    """Trees, single leaves among them, until their merged paths hold at
    least ``elems`` elements (counted by ``count_elems``)."""
    rng = random.Random(seed)
    trees, total = [], 0
    while total < elems or len(trees) % 3 != 1:
        p = rng.choice([0.0, 0.6, 0.8, 0.9, 0.97])
        trees.append(add_covers(rng, fc.random_tree(rng, F, max_depth, p)))
        total += count_elems(trees[-1])
    return trees


def count_elems(tree):
    """Path elements of the tree: distinct features per root-to-leaf path."""
    total, todo = 0, [(0, frozenset())]
    while todo:
        i, seen = todo.pop()
        if tree.feat[i] < 0:
            total += len(seen)
        else:
            seen = seen | {tree.feat[i]}
            todo += [(tree.left[i], seen), (tree.right[i], seen)]
    return total


def chain_tree(seed, depth, feats):
    """depth inner nodes in a chain, node k splitting on feats[k % len(feats)],
    the chain going left or right at random: the longest path has
    min(depth, len(feats)) distinct features."""
    from wormhole_amd.models.gbdt import RegTree
    rng = random.Random(seed)
    t = RegTree()
    i = t.add(-1)
    for k in range(depth):
        t.feat[i] = feats[k % len(feats)]
        t.cond[i] = rng.choice(fc.GRID)
        t.defl[i] = rng.randrange(2)
        t.left[i], t.right[i] = t.add(i), t.add(i)
        nxt, leaf = (t.left[i], t.right[i]) if rng.random() < 0.5 else (t.right[i], t.left[i])
        t.leaf[leaf] = float(np.float32(rng.gauss(0.0, 1.0)))
        i = nxt
    t.leaf[i] = float(np.float32(rng.gauss(0.0, 1.0)))
    return add_covers(rng, t)


def used_features(tree):
    return sorted({f for f in tree.feat if f >= 0})


def game(tree, row, known, i=0):
    """v(S): the expected value of the tree with only `known` features known."""
    if tree.feat[i] < 0:
        return float(np.float32(tree.leaf[i]))
    l, r = tree.left[i], tree.right[i]
    if tree.feat[i] in known:
        v = row[tree.feat[i]]
        left = bool(tree.defl[i]) if v != v else v < float(np.float32(tree.cond[i]))
        return game(tree, row, known, l if left else r)
    return (tree.cover[l] / tree.cover[i] * game(tree, row, known, l) +
            tree.cover[r] / tree.cover[i] * game(tree, row, known, r))


def brute_tree(tree, row, F):
    """[F + 1]: the Shapley values of one tree for one row by the sum over
    subsets of the features it splits on, and v(empty) last."""
    feats = used_features(tree)
    u = len(feats)
    assert u <= 8
    v = {}
    for k in range(u + 1):
        for S in itertools.combinations(feats, k):
            v[frozenset(S)] = game(tree, row, frozenset(S))
    phi = np.zeros(F + 1)
    for f in feats:
        rest = [g for g in feats if g != f]
        for k in range(u):
            wgt = math.factorial(k) * math.factorial(u - k - 1) / math.factorial(u)
            for S in itertools.combinations(rest, k):
                S = frozenset(S)
                phi[f] += wgt * (v[S | {f}] - v[S])
    phi[F] = v[frozenset()]
    return phi


def brute(trees, X, F, K, base):
    """[K, n, F + 1] in float64."""
    rows = X.double().tolist()
    out = np.zeros((K, len(rows), F + 1))
    out[:, :, F] = base
    for t, tree in enumerate(trees):
        for r, row in enumerate(rows):
            out[t % K, r] += brute_tree(tree, row, F)
    return out


def expected_value(tree, i=0):
    """sum over the leaves of leaf x the product of the ratios on its path."""
    if tree.feat[i] < 0:
        return float(np.float32(tree.leaf[i]))
    l, r = tree.left[i], tree.right[i]
    return (tree.cover[l] / tree.cover[i] * expected_value(tree, l) +
            tree.cover[r] / tree.cover[i] * expected_value(tree, r))


def saabas(trees, X, F, K, base):
    """[K, n, F + 1]: phi[feat(node)] += m(child) - m(node) along each walk."""
    rows = X.double().tolist()
    out = np.zeros((K, len(rows), F + 1))
    out[:, :, F] = base
    for t, tree in enumerate(trees):
        m = [expected_value(tree, i) for i in range(len(tree.feat))]
        out[t % K, :, F] += m[0]
        for r, row in enumerate(rows):
            i = 0
            while tree.feat[i] >= 0:
                v = row[tree.feat[i]]
                left = bool(tree.defl[i]) if v != v else v < float(np.float32(tree.cond[i]))
                c = tree.left[i] if left else tree.right[i]
                out[t % K, r, tree.feat[i]] += m[c] - m[i]
                i = c
    return out


def lists(trees):
    return dict(feat=[t.feat for t in trees], cond=[t.cond for t in trees],
                left=[t.left for t in trees], right=[t.right for t in trees],
                defl=[t.defl for t in trees], leaf=[t.leaf for t in trees],
                cover=[t.cover for t in trees])
