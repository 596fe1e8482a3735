"""Data, training and checks shared by the interaction_constraints tests (CPU
and GPU).

The recipe: n = 600 rows of F = 7 features, integer levels 0..15 (few distinct
values, so the quantile cuts are exact for any rank count), 8 % missing, and

    y = x0 + x3 + 2 x1 x4 + 0.5 x2 x5 + c x6 + 0.05 noise

whose products pair features of different groups: under the groups
[[0, 1, 2], [2, 3, 4, 5]] (feature 6 in none) an unconstrained model
(reg:linear, depth 4, eta 0.5, 16 bins, 3 rounds) breaks the path rule on 46
of its 46 root-to-leaf paths with c = 1, dense and CSR alike (48 of 48 at
n = 2000), and with c = 3 all three of its trees have root feature 6 --
counted with this module's ``data()``, whose generator draws the levels, then
the missing mask, then the noise. A test that passes only because nothing was
at stake is caught by its unconstrained control."""
import functools

import torch

from _gbdt_monotone_cases import csr_of, dmatrix, write_libsvm  # noqa: F401

SEED, N, F, LEVELS = 23, 600, 7, 16
GROUPS = ((0, 1, 2), (2, 3, 4, 5))
FREE = 6  # the feature in no group
ROUNDS = 3


@functools.lru_cache(maxsize=None)
def data(n=N, c=1.0):
    """(X [n, F] float32 with NaN, y [n]); never written to."""
    g = torch.Generator().manual_seed(SEED)
    X = torch.randint(0, LEVELS, (n, F), generator=g).float()
    X[torch.rand(n, F, generator=g) < 0.08] = float("nan")
    x = torch.nan_to_num(X, LEVELS / 2) / LEVELS
    y = (x[:, 0] + x[:, 3] + 2 * x[:, 1] * x[:, 4] + 0.5 * x[:, 2] * x[:, 5] + c * x[:, 6]
         + 0.05 * torch.randn(n, generator=g))
    return X, y


def spell(groups):
    return "[%s]" % ",".join("[%s]" % ",".join(str(f) for f in grp) for grp in groups)


def param(G, groups=None, mono=None, **kw):
    p = G.GBDTParam()
    p.objective, p.max_depth, p.eta, p.max_bin = "reg:linear", 4, 0.5, 16
    for k, v in kw.items():
        setattr(p, k, v)
    if groups is not None:
        assert p.set("interaction_constraints", spell(groups))
    if mono is not None:
        assert p.set("monotone_constraints", "(%s)" % ",".join(str(c) for c in mono))
    return p


def train(G, bsp, dm, p, rounds=ROUNDS):
    """The booster after ``rounds`` boosting rounds."""
    b = G.Booster(p, dm.ncol)
    margin = b.predict_margin(dm)
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    tb = G.make_builder(p, bsp, dm, cuts, cuts.bin(dm))
    gen, fgen = torch.Generator().manual_seed(p.seed + 17), torch.Generator().manual_seed(p.seed)
    for _ in range(rounds):
        b.trees += G.boost_round(b.obj, tb, dm, margin, gen, fgen)
    for t in b.trees:
        t.feat  # (a deferred device tree builds its lists)
    return b


def paths(feat, left, right):
    """The list of split features (with repeats, root first) of every
    root-to-leaf path of a tree given as lists (feat < 0: a leaf)."""
    out, stack = [], [(0, ())]
    while stack:
        i, above = stack.pop()
        if feat[i] < 0:
            out.append(list(above))
            continue
        stack.append((right[i], above + (feat[i],)))
        stack.append((left[i], above + (feat[i],)))
    return out


def path_ok(path, groups=GROUPS):
    """The path rule: the distinct features lie within one group, or the path
    is a single split on a feature of no group."""
    fs = set(path)
    if any(fs <= set(grp) for grp in groups):  # (an empty path: a lone leaf)
        return True
    return len(path) == 1 and not any(path[0] in grp for grp in groups)


def broken(trees, groups=GROUPS):
    """(paths that break the rule, paths) over ``trees`` (RegTree-like: feat,
    left, right)."""
    all_ = [pth for t in trees for pth in paths(t.feat, t.left, t.right)]
    return sum(not path_ok(pth, groups) for pth in all_), len(all_)


class DumpTree:
    """feat / left / right of one ``booster[i]:`` block of a text dump
    (``nid:[fJ<cond] yes=L,no=R,...`` | ``nid:leaf=...``), re-indexed so that
    node 0 is the root."""

    def __init__(self, lines):
        import re
        nodes = {}
        for ln in lines:
            m = re.match(r"\s*(\d+):\[f(\d+)<[^\]]*\] yes=(\d+),no=(\d+)", ln)
            if m:
                nodes[int(m.group(1))] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
                continue
            m = re.match(r"\s*(\d+):leaf=", ln)
            assert m, ln
            nodes[int(m.group(1))] = (-1, -1, -1)
        n = max(nodes) + 1
        self.feat = [nodes.get(i, (-1, -1, -1))[0] for i in range(n)]
        self.left = [nodes.get(i, (-1, -1, -1))[1] for i in range(n)]
        self.right = [nodes.get(i, (-1, -1, -1))[2] for i in range(n)]


def parse_dump(text):
    """The trees of a model dump as :class:`DumpTree` objects."""
    trees, cur = [], None
    for ln in text.splitlines():
        if ln.startswith("booster["):
            cur = []
            trees.append(cur)
        elif ln.strip():
            cur.append(ln)
    return [DumpTree(t) for t in trees]
