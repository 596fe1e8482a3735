"""GBDT trees and the model (models/gbdt.py grows the trees): a tree's node
lists, the device-grown tree that builds them on first use, dump, model file."""
import math
import struct

import numpy as np
import torch

from .. import _native
from ..utils.fs import open_uri  # noqa: E402
from .gbdt_objective import make_objective


# ------------------------------------------------------------------- tree
class RegTree:
    def __init__(self):
        self.feat, self.bin, self.cond, self.defl = [], [], [], []
        self.left, self.right, self.parent = [], [], []
        self.leaf, self.gain, self.cover, self.base_weight = [], [], [], []

    @staticmethod
    def from_lists(t):
        """The tree of a native grower's lists (``_hip.gbdt_tree_from_nodes``):
        feat, bin, cond, defl, left, right, parent, gain, cover, base weight, leaf."""
        tree = RegTree()
        (tree.feat, tree.bin, tree.cond, tree.defl, tree.left, tree.right, tree.parent,
         tree.gain, tree.cover, tree.base_weight, tree.leaf) = (list(v) for v in t[:11])
        return tree

    def compact(self):
        """Renumber reachable nodes in BFS order (like xgboost's node ids)."""
        order = [0]
        k = 0
        while k < len(order):
            i = order[k]
            if not self.is_leaf(i):
                order += [self.left[i], self.right[i]]
            k += 1
        remap = {old: new for new, old in enumerate(order)}
        t = RegTree()
        for old in order:
            t.add(remap.get(self.parent[old], -1) if self.parent[old] >= 0 else -1)
        for old in order:
            i = remap[old]
            t.feat[i] = self.feat[old]
            t.bin[i], t.cond[i], t.defl[i] = self.bin[old], self.cond[old], self.defl[old]
            t.leaf[i], t.gain[i], t.cover[i] = self.leaf[old], self.gain[old], self.cover[old]
            t.base_weight[i] = self.base_weight[old]
            if not self.is_leaf(old):
                t.left[i], t.right[i] = remap[self.left[old]], remap[self.right[old]]
        self.__dict__.update(t.__dict__)
        return self

    def add(self, parent):
        i = len(self.feat)
        self.feat.append(-1), self.bin.append(0), self.cond.append(0.0), self.defl.append(0)
        self.left.append(-1), self.right.append(-1), self.parent.append(parent)
        self.leaf.append(0.0), self.gain.append(0.0), self.cover.append(0.0)
        self.base_weight.append(0.0)
        return i

    def is_leaf(self, i):
        return self.feat[i] < 0

    def depth(self, i):
        d = 0
        while self.parent[i] >= 0:
            i = self.parent[i]
            d += 1
        return d

    def device_arrays(self, device):
        f = torch.tensor(self.feat, dtype=torch.int32, device=device)
        return (f, torch.tensor(self.cond, dtype=torch.float32, device=device),
                torch.tensor(self.left, dtype=torch.int32, device=device),
                torch.tensor(self.right, dtype=torch.int32, device=device),
                torch.tensor(self.defl, dtype=torch.uint8, device=device),
                torch.tensor(self.leaf, dtype=torch.float32, device=device))

    def predict_margin(self, X, margin):
        if X.is_cuda:
            _native.hip().gbdt_predict(X, *self.device_arrays(X.device), margin)
            return margin
        margin += torch.tensor(self.leaf)[self.leaf_index(X)]
        return margin

    def leaf_index(self, X):
        """The node id of the leaf each row of a CPU matrix ends in (NaN takes
        the default direction, a value equal to the threshold goes right)."""
        node = torch.zeros(X.shape[0], dtype=torch.long)
        feat = torch.tensor(self.feat)
        cond = torch.tensor(self.cond)
        left, right = torch.tensor(self.left), torch.tensor(self.right)
        defl = torch.tensor(self.defl, dtype=torch.bool)
        for _ in range(64):
            f = feat[node]
            active = f >= 0
            if not bool(active.any()):
                break
            v = X[torch.arange(X.shape[0]), f.clamp(min=0)]
            go_left = torch.where(torch.isnan(v), defl[node], v < cond[node])
            nxt = torch.where(go_left, left[node], right[node])
            node = torch.where(active, nxt, node)
        return node

    # -------------------------------------------------------------- dump
    def dump(self, fmap=None, with_stats=False):
        out = []

        def rec(i, depth):
            pad = "\t" * depth
            if self.is_leaf(i):
                s = "%s%d:leaf=%s" % (pad, i, _fmt(self.leaf[i]))
                if with_stats:
                    s += ",cover=%s" % _fmt(self.cover[i])
                out.append(s)
                return
            f = self.feat[i]
            name, typ = (fmap[f] if fmap and f < len(fmap) else ("f%d" % f, "q"))
            if typ == "i":
                # indicator: "yes" is the branch a present feature (value 1) takes
                yes, no = (self.left[i], self.right[i]) if 1.0 < self.cond[i] else (
                    self.right[i], self.left[i])
                s = "%s%d:[%s] yes=%d,no=%d" % (pad, i, name, yes, no)
            elif typ == "int":
                s = "%s%d:[%s<%d] yes=%d,no=%d" % (pad, i, name, int(math.ceil(self.cond[i])),
                                                   self.left[i], self.right[i])
            else:
                s = "%s%d:[%s<%s] yes=%d,no=%d" % (pad, i, name, _fmt(self.cond[i]),
                                                   self.left[i], self.right[i])
            if typ != "i":
                s += ",missing=%d" % (self.left[i] if self.defl[i] else self.right[i])
            if with_stats:
                s += ",gain=%s,cover=%s" % (_fmt(self.gain[i]), _fmt(self.cover[i]))
            out.append(s)
            rec(self.left[i], depth + 1)
            rec(self.right[i], depth + 1)
        rec(0, 0)
        return "\n".join(out) + "\n"


class _DeviceTree(RegTree):
    """A tree grown by the device level loop whose host lists are built on
    first use (models/gbdt.py TreeBuilder._build_native, defer): the node
    table is copied to pinned host memory right away, behind the tree's
    kernels, and renumbered breadth-first (``gbdt_tree_from_nodes``) when an
    attribute is first read -- by the builder one tree later, or by whoever
    reads the model first. Until then it holds no lists."""

    def __init__(self, nodes, cut_lists):  # noqa: D401 (no RegTree lists yet)
        host = torch.empty(nodes.shape, dtype=nodes.dtype, pin_memory=True)
        host.copy_(nodes, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.__dict__["_pend"] = (host, ev, cut_lists, nodes)

    def materialize(self):
        pend = self.__dict__.pop("_pend", None)
        if pend is None:
            return self
        host, ev, (cut_vals, cut_off), _ = pend
        ev.synchronize()
        lists = _native.hip().gbdt_tree_from_nodes(host, cut_vals, cut_off)
        self.__dict__.update(RegTree.from_lists(lists).compact().__dict__)
        return self

    def __getattr__(self, name):  # only for attributes not set yet
        if name.startswith("__") or "_pend" not in self.__dict__:
            raise AttributeError(name)
        self.materialize()
        return object.__getattribute__(self, name)

    def __getstate__(self):
        self.materialize()
        return self.__dict__


def _fmt(x):
    return "%g" % x


def load_fmap(path):
    names = []
    for line in open_uri(path):
        parts = line.rstrip("\n").split("\t")
        if len(parts) < 3:
            continue
        fid = int(parts[0])
        while len(names) <= fid:
            names.append(("f%d" % len(names), "q"))
        names[fid] = (parts[1], parts[2])
    return names


# ----------------------------------------------------------------- forest
class Forest:
    """Trees packed for the forest prediction kernels (csrc/host/
    gbdt_forest_plan.h): one node table and the trees' offsets on the device,
    and the chunks of whole trees, each walked by every row in one launch."""

    def __init__(self, trees, device, leaves=None):
        hip = _native.hip()
        # leaves: the trees' leaf lists where they are not the stored ones
        # (a weighted tree's effective leaves, Booster.eff_leaf)
        leaves = [t.leaf for t in trees] if leaves is None else leaves
        # (a tree a walk could leave or spin in: ValueError "malformed tree t")
        nodes, tree_off, self.max_feat = hip.gbdt_forest_pack(
            feat=[t.feat for t in trees], cond=[t.cond for t in trees],
            left=[t.left for t in trees], right=[t.right for t in trees],
            defl=[t.defl for t in trees], leaf=leaves)
        self.ntree = len(trees)
        self.chunks = hip.gbdt_forest_plan(tree_sizes=[len(t.feat) for t in trees],
                                           lds_nodes=hip.gbdt_forest_lds_nodes())
        self.nodes, self.tree_off = nodes.to(device), tree_off.to(device)


class ShapForest:
    """Trees packed for the contribution kernels (csrc/host/gbdt_shap_plan.h,
    csrc/hip/gbdt_shap.hip): the merged root-to-leaf paths in plan order with
    their chunks (exact TreeSHAP), the forest with every node's expected
    value and compact column beside it (Saabas), ``used`` (the distinct split
    features, ascending: the compact columns) and ``bias`` (float64 [K]: the
    base margin plus the expected values of the class's trees). Packing
    raises ValueError for a tree without usable cover statistics and for a
    path of more than 63 distinct features."""

    def __init__(self, trees, K, base_margin, device, leaves=None):
        hip = _native.hip()
        leaves = [t.leaf for t in trees] if leaves is None else leaves  # (as Forest)
        kw = dict(feat=[t.feat for t in trees], cond=[t.cond for t in trees],
                  left=[t.left for t in trees], right=[t.right for t in trees],
                  defl=[t.defl for t in trees], leaf=leaves,
                  cover=[t.cover for t in trees])
        (used, tree_E, paths, elems, ecol, self.chunks, nodes, tree_off, node_m,
         node_col) = hip.gbdt_shap_pack(num_class=K, **kw)
        self.ntree, self.K = len(trees), K
        self.used = used
        self.max_feat = int(used[-1]) if used.numel() else -1
        self.bias = torch.tensor([base_margin + float(tree_E[k::K].sum()) for k in range(K)],
                                 dtype=torch.float64)
        self.paths, self.elems, self.ecol = paths.to(device), elems.to(device), ecol.to(device)
        self.nodes, self.tree_off = nodes.to(device), tree_off.to(device)
        self.node_m, self.node_col = node_m.to(device), node_col.to(device)

    def new_out(self, n, device):
        """float32 [K, n, U + 1]: zeros, the bias in the last column."""
        out = torch.zeros((self.K, n, self.used.numel() + 1), dtype=torch.float32, device=device)
        out[:, :, -1] = self.bias.to(torch.float32).to(device)[:, None]
        return out

    def new_inter_out(self, n, device):
        """float32 [K, n, U + 1, U + 1]: zeros, the bias in cell (U, U)."""
        U1 = self.used.numel() + 1
        out = torch.zeros((self.K, n, U1, U1), dtype=torch.float32, device=device)
        out[:, :, -1, -1] = self.bias.to(torch.float32).to(device)[:, None]
        return out


# ---------------------------------------------------------------- booster
class Booster:
    MAGIC = b"WHGB"

    def __init__(self, param, num_feature, n_out=None):
        """n_out: the outputs per row of a loaded reg:quantileerror model
        (:func:`make_objective`)."""
        self.param = param
        self.num_feature = int(num_feature)
        self.trees = []
        # booster=dart: one fp32 weight per tree (the K trees of a round share
        # theirs); trees beyond the list weigh 1, as every gbtree tree does
        self.tree_w = []
        self.obj = make_objective(param.objective, param.num_class, param, n_out=n_out)
        self.base_margin = self.obj.prob_to_margin(param.base_score)

    # Trees from which a GPU matrix is predicted by the forest kernels (one
    # launch per chunk of trees) instead of one predict_tree per tree: the
    # forest path was never the slower one, at one tree included
    # (profiles/gbdt_forest_predict.txt)
    FOREST_MIN_TREES = 1

    def _ntree(self, ntree_limit):
        """How many of the model's trees a limit means (0: all of them)."""
        if ntree_limit < 0:
            raise ValueError("ntree_limit must not be negative")
        return min(ntree_limit, len(self.trees)) if ntree_limit else len(self.trees)

    # ------------------------------------------------------ tree weights
    def weights(self, ntree=None):
        """The first ``ntree`` trees' weights (default: all), as floats that
        are fp32 values; 1.0 where none was set."""
        ntree = len(self.trees) if ntree is None else ntree
        w = [float(np.float32(x)) for x in self.tree_w[:ntree]]
        return w + [1.0] * (ntree - len(w))

    def weighted(self):
        """True when some tree's weight is not 1 (a dart-trained model)."""
        return any(w != 1.0 for w in self.weights())

    def eff_leaf(self, i, coef=None):
        """Tree i's effective leaf values, what every consumer of the model's
        trees adds: float32(w_i) * float32(leaf), one fp32 multiply per leaf
        (as Python floats). A weight of 1 returns the stored list itself.
        coef: another fp32 factor in place of the tree's weight."""
        t = self.trees[i]
        if coef is None:
            coef = self.tree_w[i] if i < len(self.tree_w) else 1.0
        w = float(np.float32(coef))
        if w == 1.0:
            return t.leaf
        return (np.float32(w) * np.asarray(t.leaf, dtype=np.float32)).astype(np.float64).tolist()

    def eff_leaves(self, ntree):
        return [self.eff_leaf(i) for i in range(ntree)]

    def eff_tree(self, i, coef=None):
        """Tree i with its effective leaves in place of the stored ones (the
        tree itself at weight 1)."""
        t = self.trees[i]
        leaf = self.eff_leaf(i, coef)
        if leaf is t.leaf:
            return t
        v = RegTree()
        v.__dict__.update(t.__dict__)  # (eff_leaf has built a pending device tree)
        v.leaf = leaf
        return v

    def forest(self, device, ntree=0):
        """The first ``ntree`` trees (0: all) packed for the forest kernels on
        ``device``; kept until the model's tree count or the limit changes.
        Packing reads the trees' lists (a pending device tree is built here);
        a tree that a walk could leave raises ValueError."""
        ntree = self._ntree(ntree)
        key = (torch.device(device), len(self.trees), ntree, tuple(self.weights(ntree)))
        if self.__dict__.get("_forest_key") != key:
            self._forest = Forest(self.trees[:ntree], device, self.eff_leaves(ntree))
            self._forest_key = key
        return self._forest

    def predict_margin(self, dm, ntree_limit=0):
        """[n] margins, or [K, n] for K classes (tree t adds to row t % K)."""
        K = self.obj.n_group
        margin = torch.full((dm.n,) if K == 1 else (K, dm.n), self.base_margin,
                            dtype=torch.float32, device=dm.device)
        ntree = self._ntree(ntree_limit)
        if torch.device(dm.device).type == "cuda" and ntree >= self.FOREST_MIN_TREES:
            dm.predict_forest(self.forest(dm.device, ntree), margin)
            return margin
        for i in range(ntree):
            dm.predict_tree(self.eff_tree(i), margin if K == 1 else margin[i % K])
        return margin

    def predict_leaf(self, dm, ntree_limit=0):
        """int32 [n, T]: the node id (the dump's numbering) of the leaf each
        row ends in, per tree."""
        ntree = self._ntree(ntree_limit)
        if torch.device(dm.device).type == "cuda" and ntree:
            out = torch.empty((dm.n, ntree), dtype=torch.int32, device=dm.device)
            dm.predict_forest(self.forest(dm.device, ntree), out, leaf=True)
            return out
        X = (dm.dense_cpu() if dm.sparse else dm.X).cpu()
        cols = [t.leaf_index(X).to(torch.int32) for t in self.trees[:ntree]]
        out = torch.stack(cols, 1) if cols else torch.empty((dm.n, 0), dtype=torch.int32)
        return out.to(dm.device)

    def shap_forest(self, device, ntree=0):
        """The first ``ntree`` trees (0: all) packed for the contribution
        kernels on ``device``; kept as ``forest`` keeps its table."""
        ntree = self._ntree(ntree)
        key = (torch.device(device), len(self.trees), ntree, tuple(self.weights(ntree)))
        if self.__dict__.get("_shap_key") != key:
            self._shap = ShapForest(self.trees[:ntree], self.obj.n_group, self.base_margin, device,
                                    self.eff_leaves(ntree))
            self._shap_key = key
        return self._shap

    def predict_contribs(self, dm, ntree_limit=0, approx=False, compact=False, rows=None):
        """Per-feature contributions in margin space (docs/bsp_apps.md
        "Contributions"): [n, F + 1], or [K, n, F + 1] for K classes; column
        j < F is the sum over the (class's) trees of feature j's Shapley
        value in the tree's cover-weighted game (approx: the Saabas
        attribution along the row's walk), column F the bias; a row sums to
        its predict_margin. F is the model's num_feature (or the matrix's
        width, if larger). compact: (phi [.., U + 1], used) over the U
        features the trees split on (``used`` int64, ascending) and the bias.
        rows = (a, b): only rows [a, b). A GPU matrix goes through the HIP
        kernels (float32); a CPU matrix through the host reference (float64).
        ValueError: a tree without usable cover statistics; on the GPU, a
        path of more than 63 distinct features."""
        K = self.obj.n_group
        ntree = self._ntree(ntree_limit)
        a, b = rows if rows is not None else (0, dm.n)
        if not 0 <= a <= b <= dm.n:
            raise ValueError("rows must be a range within the matrix")
        if torch.device(dm.device).type == "cuda":
            sf = self.shap_forest(dm.device, ntree)
            phi, used = dm.predict_contribs(sf, approx=approx, rows=(a, b)), sf.used
        else:
            trees = self.trees[:ntree]
            model = dict(feat=[t.feat for t in trees], cond=[t.cond for t in trees],
                         left=[t.left for t in trees], right=[t.right for t in trees],
                         defl=[t.defl for t in trees], leaf=self.eff_leaves(ntree),
                         cover=[t.cover for t in trees], num_class=K, base=self.base_margin)
            phi, used = dm.predict_contribs_host(model, approx=approx, rows=(a, b))
        used = used.long()
        if not compact:
            F = max(self.num_feature, dm.ncol, int(used[-1]) + 1 if used.numel() else 0)
            full = torch.zeros(phi.shape[:2] + (F + 1,), dtype=phi.dtype, device=phi.device)
            full[:, :, used.to(phi.device)] = phi[:, :, :-1]
            full[:, :, F] = phi[:, :, -1]
            phi = full
        phi = phi[0] if K == 1 else phi
        return (phi, used) if compact else phi

    def predict_interactions(self, dm, ntree_limit=0, compact=False, rows=None):
        """SHAP interaction values in margin space (docs/bsp_apps.md
        "Interactions"): [n, F + 1, F + 1], or [K, n, F + 1, F + 1] for K
        classes. Cell (i, j), i != j, is half the Shapley interaction index
        of features i and j summed over the (class's) trees, the same number
        in (j, i); cell (i, i) is predict_contribs' column i minus the rest
        of row i, so a row of the matrix sums to that column and the matrix
        to the row's predict_margin; cell (F, F) is the bias, the rest of row
        and column F zero. F, compact ((Phi [.., U + 1, U + 1], used)), rows,
        the float type per device and the ValueErrors are predict_contribs'."""
        K = self.obj.n_group
        ntree = self._ntree(ntree_limit)
        a, b = rows if rows is not None else (0, dm.n)
        if not 0 <= a <= b <= dm.n:
            raise ValueError("rows must be a range within the matrix")
        if torch.device(dm.device).type == "cuda":
            sf = self.shap_forest(dm.device, ntree)
            phi, used = dm.predict_interactions(sf, rows=(a, b)), sf.used
        else:
            trees = self.trees[:ntree]
            model = dict(feat=[t.feat for t in trees], cond=[t.cond for t in trees],
                         left=[t.left for t in trees], right=[t.right for t in trees],
                         defl=[t.defl for t in trees], leaf=self.eff_leaves(ntree),
                         cover=[t.cover for t in trees], num_class=K, base=self.base_margin)
            phi, used = dm.predict_interactions_host(model, rows=(a, b))
        used = used.long()
        if not compact:
            F = max(self.num_feature, dm.ncol, int(used[-1]) + 1 if used.numel() else 0)
            full = torch.zeros(phi.shape[:2] + (F + 1, F + 1), dtype=phi.dtype, device=phi.device)
            u = used.to(phi.device)
            full[:, :, u[:, None], u[None, :]] = phi[:, :, :-1, :-1]
            full[:, :, F, F] = phi[:, :, -1, -1]
            phi = full
        phi = phi[0] if K == 1 else phi
        return (phi, used) if compact else phi

    def save(self, path):
        p = self.param
        with open_uri(path, "wb") as f:
            f.write(self.MAGIC)
            hdr = "%s|%g|%d|%d" % (p.objective, p.base_score, self.num_feature, len(self.trees))
            if self.obj.n_group > 1:  # (single-output files keep their four fields)
                hdr += "|%d" % self.obj.n_group
            hdr = hdr.encode()
            f.write(struct.pack("<I", len(hdr)) + hdr)
            for t in self.trees:
                n = len(t.feat)
                f.write(struct.pack("<I", n))
                arr = np.zeros(n, dtype=[("feat", "<i4"), ("cond", "<f4"), ("left", "<i4"),
                                         ("right", "<i4"), ("defl", "<i4"), ("leaf", "<f4"),
                                         ("gain", "<f4"), ("cover", "<f4")])
                for k in ("feat", "cond", "left", "right", "defl", "leaf", "gain", "cover"):
                    arr[k] = getattr(t, k)
                f.write(arr.tobytes())
            if self.weighted():  # (a model of unit weights keeps the gbtree bytes)
                w = np.asarray(self.weights(), dtype="<f4")
                f.write(b"DART" + struct.pack("<I", w.size) + w.tobytes())

    @staticmethod
    def load(path, param):
        with open_uri(path, "rb") as f:
            if f.read(4) != Booster.MAGIC:
                raise ValueError("invalid model file " + path)
            (ln,) = struct.unpack("<I", f.read(4))
            fields = f.read(ln).decode().split("|")
            if len(fields) not in (4, 5):
                raise ValueError("invalid model header in " + path)
            objective, base, nf, ntree = fields[:4]
            param.objective = objective
            param.base_score = float(base)
            param.num_class = int(fields[4]) if len(fields) == 5 else 0
            # (a reg:quantileerror file's fifth field is its outputs per row)
            n_out = max(1, param.num_class) if objective == "reg:quantileerror" else None
            b = Booster(param, int(nf), n_out=n_out)
            for _ in range(int(ntree)):
                (n,) = struct.unpack("<I", f.read(4))
                arr = np.frombuffer(f.read(32 * n), dtype=[
                    ("feat", "<i4"), ("cond", "<f4"), ("left", "<i4"), ("right", "<i4"),
                    ("defl", "<i4"), ("leaf", "<f4"), ("gain", "<f4"), ("cover", "<f4")])
                t = RegTree()
                for k in ("feat", "cond", "left", "right", "defl", "leaf", "gain", "cover"):
                    setattr(t, k, [x.item() for x in arr[k]])
                t.parent = [-1] * n
                for i in range(n):
                    if t.feat[i] >= 0:
                        t.parent[t.left[i]] = i
                        t.parent[t.right[i]] = i
                t.bin = [0] * n
                t.base_weight = [0.0] * n
                b.trees.append(t)
            tag = f.read(4)
            if tag == b"DART":  # the trees' weights (no trailer: all 1)
                (cnt,) = struct.unpack("<I", f.read(4))
                w = np.frombuffer(f.read(4 * cnt), dtype="<f4")
                if w.size != cnt or cnt != len(b.trees):
                    raise ValueError("invalid weight trailer in " + path)
                b.tree_w = [float(x) for x in w]
        return b

    def dump(self, fmap=None, with_stats=False):
        """(leaf values: the effective ones, :meth:`eff_leaf`)"""
        return "".join("booster[%d]:\n%s" % (i, self.eff_tree(i).dump(fmap, with_stats))
                       for i in range(len(self.trees)))
