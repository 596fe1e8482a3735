"""An independent Python statement of the SHAP interaction values for the
interaction tests: the Shapley interaction index of every pair of a tree's
features by the sum over subsets, halved; the diagonal as the Shapley value
minus the rest of its row; the bias. The game is ``_gbdt_shap_cases.game``."""
import itertools
import math

import numpy as np

import _gbdt_shap_cases as sc


def brute_tree(tree, row, F):
    """[F + 1, F + 1] of one tree for one row."""
    feats = sc.used_features(tree)
    u = len(feats)
    assert u <= 8
    v = {}
    for k in range(u + 1):
        for S in itertools.combinations(feats, k):
            v[frozenset(S)] = sc.game(tree, row, frozenset(S))
    out = np.zeros((F + 1, F + 1))
    for i in feats:  # the Shapley values, on the diagonal for now
        rest = [g for g in feats if g != i]
        for k in range(u):
            wgt = math.factorial(k) * math.factorial(u - k - 1) / math.factorial(u)
            for S in map(frozenset, itertools.combinations(rest, k)):
                out[i, i] += wgt * (v[S | {i}] - v[S])
    for i, j in itertools.permutations(feats, 2):
        rest = [g for g in feats if g not in (i, j)]
        for k in range(u - 1):
            wgt = (math.factorial(k) * math.factorial(u - k - 2) /
                   (2 * math.factorial(u - 1)))
            for S in map(frozenset, itertools.combinations(rest, k)):
                out[i, j] += wgt * (v[S | {i, j}] - v[S | {i}] - v[S | {j}] + v[S])
    for i in feats:
        out[i, i] -= sum(out[i, j] for j in feats if j != i)
    out[F, F] = v[frozenset()]
    return out


def brute(trees, X, F, K, base):
    """[K, n, F + 1, F + 1] in float64."""
    rows = X.double().tolist()
    out = np.zeros((K, len(rows), F + 1, F + 1))
    out[:, :, F, F] = base
    for t, tree in enumerate(trees):
        for r, row in enumerate(rows):
            out[t % K, r] += brute_tree(tree, row, F)
    return out
