"""booster=dart (dropout additive regression trees) on the GBDT growers of
models/gbdt.py: the draw of the dropped rounds, the weight update, the
bin-space tree table that the dropout walk reads (csrc/hip/gbdt_dart.hip) and
the boosting round.

The unit of dropout is a boosting round: its K trees (one per class) are
dropped together and share one fp32 weight ``w_t``; a tree's effective leaf is
``float32(w_t) * float32(leaf)`` (Booster.eff_leaf). Round r with R earlier
rounds: the dropped rounds are drawn from a generator seeded by (seed, r)
alone; D_c = sum of w_t * tree_t(x) over the dropped trees of class c, in
ascending t; the gradients are taken at m - D; the growers add the new trees'
outputs delta to a zero scratch; with k dropped rounds the dropped weights are
scaled by f and the new trees weigh w_new (normalize_type=tree: f = k / (k +
eta), w_new = 1 / (k + eta); forest: both 1 / (1 + eta); k = 0: 1 and 1), and
every kept margin becomes m + (f - 1) D + w_new delta.
"""
import numpy as np
import torch

from .. import _native
from .gbdt_tree import Forest, _DeviceTree

_F32 = np.float32
# rows per tile (= lanes per block) of k_dart_walk; profiles/gbdt_dart.txt
DART_WALK_ROWS = 1024


# ------------------------------------------------------------------ the draw
def dart_seed(seed, r):
    """The seed of round r's draw: a function of ``seed`` and ``r`` only (no
    rank term: every rank drops the same rounds, a restart repeats them)."""
    return (int(seed) * 0x9E3779B1 + int(r) * 1000003 + 0xDA27) & 0x7FFFFFFFFFFFFFFF


def dart_draw(seed, r, weights, p):
    """The rounds that round r drops, ascending: a pure function of (seed, r,
    the R earlier rounds' weights, the parameters p: rate_drop, skip_drop,
    one_drop, sample_type). With probability skip_drop nothing; else round j
    with probability rate_drop (uniform) or min(1, rate_drop R w_j / sum w)
    (weighted); one_drop: when that chose nothing, one round, uniformly or in
    proportion to w."""
    R = len(weights)
    if R == 0:
        return []
    g = torch.Generator().manual_seed(dart_seed(seed, r))
    u = torch.rand(R + 2, generator=g, dtype=torch.float64).tolist()
    if u[0] < p.skip_drop:
        return []
    total = float(sum(weights))
    weighted = p.sample_type == "weighted" and total > 0
    if weighted:
        prob = [min(1.0, p.rate_drop * R * w / total) for w in weights]
    else:
        prob = [p.rate_drop] * R
    drop = [j for j in range(R) if u[2 + j] < prob[j]]
    if not drop and p.one_drop:
        if weighted:
            target, acc, pick = u[1] * total, 0.0, R - 1
            for j, w in enumerate(weights):
                acc += w
                if target < acc:
                    pick = j
                    break
        else:
            pick = min(R - 1, int(u[1] * R))
        drop = [pick]
    return drop


def dart_scales(k, eta, normalize_type):
    """(f, w_new) as fp32 values after a round that dropped k rounds: the
    factor of the dropped weights and the new trees' weight."""
    if k == 0:
        return 1.0, 1.0
    if normalize_type == "forest":
        return float(_F32(1.0 / (1.0 + eta))), float(_F32(1.0 / (1.0 + eta)))
    return float(_F32(k / (k + eta))), float(_F32(1.0 / (k + eta)))


def dart_update(round_w, drop, eta, normalize_type):
    """The rounds' weights after a round that dropped ``drop``: the dropped
    ones times f, the new round's appended, each rounded to fp32."""
    f, w_new = dart_scales(len(drop), eta, normalize_type)
    out = list(round_w)
    for j in drop:
        out[j] = float(_F32(out[j]) * _F32(f))
    return out + [w_new]


# ----------------------------------------------------------- the tree table
class DartForest:
    """The device table of the model's trees in bin space (csrc/host/
    gbdt_dart_plan.h): 8-byte nodes, appended once per tree and never
    re-packed (the capacity doubles when it fills); the weights are not in it,
    they come in per walk. ``size[t]`` is tree t's node count, 0 for a tree
    the table does not admit (feature id >= 65535, more than 65535 nodes, a
    split bin >= 255 or unknown, a walk deeper than 64): such a tree and one
    larger than the LDS budget are walked by the caller's fallback."""

    def __init__(self, device, cut_lists, lds_nodes=None, rows=None):
        self.device = torch.device(device)
        self.cut_vals, self.cut_off = cut_lists
        self.lds_nodes = lds_nodes or _native.hip().gbdt_dart_lds_nodes()
        self.rows = rows or DART_WALK_ROWS
        self.table = None
        self.used = 0
        self.off, self.size = [], []

    def append(self, tree, bins_known):
        """Tree t = len(self.size). bins_known: ``tree.bin`` holds the split
        bins under these cuts (a tree grown on them); else they are recovered
        by finding each ``cond`` exactly among its feature's cuts."""
        nodes = _native.hip().gbdt_dart_pack(
            feat=tree.feat, bin=tree.bin if bins_known else None, cond=tree.cond, left=tree.left,
            right=tree.right, defl=tree.defl, leaf=tree.leaf, cut_vals=self.cut_vals,
            cut_off=self.cut_off)
        if nodes is None:
            self.off.append(-1), self.size.append(0)
            return False
        nn = int(nodes.shape[0])
        cap = 0 if self.table is None else int(self.table.shape[0])
        if self.used + nn > cap:
            grown = torch.empty((max(2 * cap, self.used + nn, 4096), 2), dtype=torch.int32,
                                device=self.device)
            if self.used:
                grown[:self.used] = self.table[:self.used]
            self.table = grown
        src = nodes.pin_memory() if self.device.type == "cuda" else nodes
        self.table[self.used:self.used + nn].copy_(src, non_blocking=True)
        self.off.append(self.used), self.size.append(nn)
        self.used += nn
        return True

    def plan(self, sel):
        """The selection's chunks (first, count, nnode, staged, stage_off)."""
        return _native.hip().gbdt_dart_plan(tree_sizes=self.size, sel=list(sel),
                                            lds_nodes=self.lds_nodes)

    def walk(self, B, sel, coef, out, fallback):
        """out[i] += coef[j] * tree_sel[j](row i of the bin matrix B) for
        every j, in order (each product and sum rounded to fp32): staged
        chunks by k_dart_walk, every other tree by ``fallback(trees, coefs)``."""
        for first, count, nnode, staged, stage_off in self.plan(sel):
            ts, cs = list(sel[first:first + count]), list(coef[first:first + count])
            if not staged:
                fallback(ts, cs)
                continue
            _native.hip().gbdt_dart_walk(
                B=B, table=self.table, tree_off=[self.off[t] for t in ts],
                tree_nn=[self.size[t] for t in ts], stage_off=stage_off, coef=cs, out=out,
                rows=self.rows)


def forest_add(booster, dm, sel, coef, out):
    """The same sum by the model's own prediction paths: out += the trees
    ``sel`` of the booster with leaves float32(coef[j]) * float32(leaf), in
    order -- the forest kernels on that sub-forest on the GPU, one torch
    gather per tree on the CPU. Bit-equal to :meth:`DartForest.walk`."""
    if not len(sel) or dm.n == 0:
        return out
    if torch.device(dm.device).type == "cuda":
        forest = Forest([booster.trees[t] for t in sel], dm.device,
                        [booster.eff_leaf(t, c) for t, c in zip(sel, coef)])
        dm.predict_forest(forest, out)
        return out
    for t, c in zip(sel, coef):
        dm.predict_tree(_scaled(booster, t, c), out)
    return out


def dart_add(booster, dm, B, table, sel, coef, out):
    """out += sum_j coef[j] * tree_sel[j] on the rows of ``dm``, in order: by
    the binned walk over ``table`` (a :class:`DartForest` of the booster's
    trees under the cuts that binned ``B``) when the switch DART_BIN_WALK is
    on and B is a resident u8 bin matrix [n, F] on the GPU with F within the
    kernel's limit; else (and for the trees the walk cannot take) by
    :func:`forest_add`."""
    from . import gbdt as G
    if (G.DART_BIN_WALK and table is not None and torch.is_tensor(B) and B.is_cuda
            and B.dtype == torch.uint8 and B.dim() == 2 and B.shape[0] == dm.n
            and 1 <= B.shape[1] <= _native.hip().gbdt_dart_max_f()):
        table.walk(B, sel, coef, out, lambda ts, cs: forest_add(booster, dm, ts, cs, out))
    else:
        forest_add(booster, dm, sel, coef, out)
    return out


def _scaled(booster, t, c):
    """Tree t with leaves float32(c) * float32(leaf) (also for c == 1: the
    CPU gather then adds the fp32 leaves, as the kernels do)."""
    from .gbdt_tree import RegTree
    tree = booster.trees[t]
    v = RegTree()
    leaf = (_F32(c) * np.asarray(tree.leaf, dtype=np.float32)).astype(np.float64).tolist()
    v.__dict__.update(tree.__dict__)
    v.leaf = leaf
    return v


# ---------------------------------------------------------------- the round
class DartTrainer:
    """booster=dart training of ``booster`` by ``builder`` on ``dtrain``.
    ``evals``: [(matrix, kept margin)] updated with every round."""

    def __init__(self, booster, builder, dtrain, evals=()):
        self.b, self.builder, self.dm = booster, builder, dtrain
        self.evals = list(evals)
        self.p = booster.param
        self.K = booster.obj.n_group
        self.table = None  # DartForest of the training matrix, built on first use
        self.walks = 0  # dropped trees walked on the training rows so far
        self.history = []  # (round, the rounds it dropped) of every round so far

    # -- the walk on the training rows
    def _binned(self):
        """True when the training rows are walked on their bins."""
        from . import gbdt as G
        bd = self.builder
        return bool(G.DART_BIN_WALK and isinstance(bd, G.TreeBuilder) and bd._walks(self.dm.n)
                    and 1 <= bd.F <= _native.hip().gbdt_dart_max_f())

    def _table(self):
        """The table with every tree of the model so far (trees that came
        from a file or a checkpoint: bins recovered from the cuts)."""
        if self.table is None:
            self.table = DartForest(self.dm.device, self.builder._cut_lists)
        while len(self.table.size) < len(self.b.trees):
            t = self.b.trees[len(self.table.size)]
            self.table.append(t, bool(getattr(t, "_dart_bins", False)))
        return self.table

    def train_add(self, sel, coef, out):
        """out += sum_j coef[j] * tree_sel[j] on the training rows, in order."""
        self.walks += len(sel)
        binned = self._binned()
        dart_add(self.b, self.dm, self.builder.B if binned else None,
                 self._table() if binned else None, sel, coef, out)

    def _rows(self, m, c):
        return m[c] if self.K > 1 else m

    # -- one round
    def round(self, r, margin, gen=None, fgen=None):
        """Boosting round r on the training margins (updated in place, as the
        kept eval margins are); appends the K new trees and their weight to
        the booster and returns them."""
        from . import gbdt as G
        b, K, p = self.b, self.K, self.p
        b.tree_w = b.weights()
        drop = dart_draw(p.seed, r, b.tree_w[::K], p)
        ntree = len(b.trees)
        self.history.append((r, list(drop)))
        if not drop:
            new = G.grow_round(b.obj, self.builder, self.dm, margin, margin, gen, fgen)
            self._commit(new, [])
            for d, em in self.evals:
                for c in range(K):
                    forest_add(b, d, [ntree + c], [1.0], self._rows(em, c))
            return new
        D = torch.zeros_like(margin)
        for c in range(K):
            sel = [j * K + c for j in drop]
            self.train_add(sel, [b.tree_w[t] for t in sel], self._rows(D, c))
        delta = torch.zeros_like(margin)
        new = G.grow_round(b.obj, self.builder, self.dm, margin - D, delta, gen, fgen)
        f, w_new = dart_scales(len(drop), p.eta, p.normalize_type)
        fm1 = float(_F32(f) - _F32(1.0))
        margin.add_(D, alpha=fm1).add_(delta, alpha=w_new)
        old = list(b.tree_w)
        self._commit(new, drop)
        for d, em in self.evals:  # one walk: the dropped trees and the new one
            for c in range(K):
                sel = [j * K + c for j in drop]
                coef = [float(_F32(fm1) * _F32(old[t])) for t in sel]
                forest_add(b, d, sel + [ntree + c], coef + [w_new], self._rows(em, c))
        return new

    def _commit(self, new, drop):
        b, K = self.b, self.K
        for t in new:
            if isinstance(t, _DeviceTree):
                t.materialize()  # (its lists are appended to the table this round)
            t._dart_bins = True  # grown on the builder's cuts: tree.bin holds the split bins
        rw = dart_update(b.tree_w[::K], drop, self.p.eta, self.p.normalize_type)
        b.trees += new
        b.tree_w = [w for w in rw for _ in range(K)]
        if self.table is not None or (drop and self._binned()):
            self._table()

    # -- the training margins of a model that is continued
    def start_margin(self):
        """The training margins a run that is continued starts from. A model
        this trainer's parameters trained from its first round has its kept
        margins replayed (the same draws, the same updates, so a restart goes
        on bit for bit); any other model -- the replayed weights then differ
        from the stored ones -- starts from predict_margin."""
        b, K, p = self.b, self.K, self.p
        R = len(b.trees) // K
        stored = b.weights()[::K]
        if not b.weighted():
            return b.predict_margin(self.dm)
        shape = (self.dm.n,) if K == 1 else (K, self.dm.n)
        m = torch.full(shape, b.base_margin, dtype=torch.float32, device=self.dm.device)
        w = []
        for r in range(R):
            drop = dart_draw(p.seed, r, w, p)
            nxt = dart_update(w, drop, p.eta, p.normalize_type)
            if not drop:
                for c in range(K):
                    self.train_add([r * K + c], [1.0], self._rows(m, c))
            else:
                D, delta = torch.zeros_like(m), torch.zeros_like(m)
                for c in range(K):
                    sel = [j * K + c for j in drop]
                    self.train_add(sel, [w[j] for j in drop], self._rows(D, c))
                    self.train_add([r * K + c], [1.0], self._rows(delta, c))
                f, w_new = dart_scales(len(drop), p.eta, p.normalize_type)
                m.add_(D, alpha=float(_F32(f) - _F32(1.0))).add_(delta, alpha=w_new)
            w = nxt
        if w != stored:
            return b.predict_margin(self.dm)
        return m
