"""Data, training and an independent reference shared by the
grow_policy=lossguide tests (CPU and GPU).

The data is the recipe of ``_gbdt_monotone_cases``: integer levels 0..47 per
feature (exact cuts for any rank count), 8 % missing.

:func:`reference` is a best-first loop of its own -- row masks instead of a
partitioned row index, one torch histogram per node built directly (no sibling
subtraction), ``find_splits_ref`` for a node's best split, a plain scan for
the pick -- that never calls the builder's leaf loop. It also records, per
pick, the gap to the runner-up among the eligible open leaves: the condition
under which runs that sum their histograms differently (fp64 on the CPU,
fixed point on the GPU) must pick in the same order."""
import math

import torch

import _gbdt_monotone_cases as M

RT_EPS = 1e-6
MISSING = 255


def param(G, max_leaves, max_depth, policy="lossguide", **kw):
    p = M.param(G, **kw)
    p.max_depth = max_depth
    if policy is not None:
        assert p.set("grow_policy", policy)
    assert p.set("max_leaves", str(max_leaves))
    return p


def n_leaves(t):
    return sum(1 for f in t.feat if f < 0)


def tree_depth(t):
    def rec(i):
        return 0 if t.feat[i] < 0 else 1 + max(rec(t.left[i]), rec(t.right[i]))
    return rec(0)


def same_structure(a, b):
    assert a.feat == b.feat and a.cond == b.cond and a.defl == b.defl
    assert a.left == b.left and a.right == b.right


def _hist(B, gp, mask, F, nbin):
    rows = mask.nonzero()[:, 0]
    bins = B[rows].long()
    gh = gp[rows].double()
    ok = bins != MISSING
    flat = torch.arange(F)[None, :] * nbin + bins.clamp(max=nbin - 1)
    h = torch.zeros(F * nbin, 2, dtype=torch.float64)
    for c in range(2):
        h[:, c].index_add_(0, flat[ok], gh[:, c][:, None].expand_as(flat)[ok])
    return h.view(1, F, nbin, 2)


def reference(G, bsp, dm, p, max_leaves, max_depth, rounds):
    """(trees, smallest pick gap) of ``rounds`` rounds of best-first growth on
    a dense CPU matrix, reg:linear-like single-output objectives, no
    constraints, gamma = 0. max_depth = 0: no depth limit."""
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    B = cuts.bin(dm)
    F, nbin = dm.ncol, max(1, cuts.nbin_max)
    off = cuts.offsets.tolist()
    vals = cuts.values.tolist()
    valid = torch.arange(nbin)[None, :] < torch.tensor([b - a for a, b in zip(off, off[1:])])[:, None]
    b = G.Booster(p, dm.ncol)
    margin = b.predict_margin(dm)
    cap = max_depth if max_depth > 0 else 10 ** 9
    trees, min_gap = [], math.inf
    for _ in range(rounds):
        gp = b.obj.gpair(margin, dm.label, dm.weight, None)
        t = G.RegTree()
        t.add(-1)
        masks = {0: torch.ones(dm.n, dtype=torch.bool)}
        depth = {0: 0}
        best = {}

        def open_leaf(nd):
            tot = gp[masks[nd]].double().sum(0)
            t.cover[nd] = float(tot[1])
            t.base_weight[nd] = p.calc_weight(float(tot[0]), float(tot[1]))
            t.leaf[nd] = p.eta * t.base_weight[nd]
            row = G.find_splits_ref(p, _hist(B, gp, masks[nd], F, nbin), tot[None], valid)[0]
            best[nd] = [float(v) for v in row]

        open_leaf(0)
        leaves = 1
        while leaves < max_leaves:
            elig = sorted(((-best[nd][0], nd) for nd in best
                           if best[nd][0] > RT_EPS and depth[nd] < cap))
            if not elig:
                break
            if len(elig) > 1:
                g0, g1 = -elig[0][0], -elig[1][0]
                min_gap = min(min_gap, (g0 - g1) / max(1.0, abs(g0)))
            nd = elig[0][1]
            gain, f, bn, d = best.pop(nd)[:4]
            f, bn = int(f), int(bn)
            t.feat[nd], t.bin[nd], t.cond[nd] = f, bn, vals[off[f] + bn]
            t.defl[nd], t.gain[nd] = int(d), gain
            l, r = t.add(nd), t.add(nd)
            t.left[nd], t.right[nd] = l, r
            col = B[:, f].long()
            go_left = torch.where(col == MISSING, torch.full_like(col, int(d)).bool(), col <= bn)
            m = masks.pop(nd)
            masks[l], masks[r] = m & go_left, m & ~go_left
            depth[l] = depth[r] = depth[nd] + 1
            open_leaf(l), open_leaf(r)
            leaves += 1
        for nd, m in masks.items():
            margin[m] += t.leaf[nd]
        trees.append(t.compact())
    return trees, min_gap


def open_gains(G, bsp, dm, p, trees):
    """For each tree of a model trained on ``dm`` (single output, the rounds in
    order): the gains > RT_EPS of the best splits of its leaves -- what a
    limit on the leaves left unsplit."""
    cuts = G.Cuts.build(dm, p.max_bin, bsp)
    B = cuts.bin(dm)
    F, nbin = dm.ncol, max(1, cuts.nbin_max)
    off = cuts.offsets.tolist()
    valid = torch.arange(nbin)[None, :] < torch.tensor([b - a for a, b in zip(off, off[1:])])[:, None]
    b = G.Booster(p, dm.ncol)
    margin = b.predict_margin(dm)
    out = []
    for t in trees:
        gp = b.obj.gpair(margin, dm.label, dm.weight, None)
        at = t.leaf_index(dm.X)
        gains = []
        for nd in range(len(t.feat)):
            if t.feat[nd] >= 0:
                continue
            m = at == nd
            row = G.find_splits_ref(p, _hist(B, gp, m, F, nbin), gp[m].double().sum(0)[None],
                                    valid)[0]
            if float(row[0]) > RT_EPS:
                gains.append(float(row[0]))
        out.append(gains)
        margin += torch.tensor(t.leaf)[at]
    return out
