"""GBDT input data (models/gbdt.py grows the trees on it): a rank's rows as
a dense device matrix or kept CSR, and the quantile cuts that bin them."""
import numpy as np
import torch

from .. import _native
from .gbdt_survival import SurvivalData

MISSING_BIN = 255


class _QueryGroups:
    """What both matrices keep of their rows' query groups (learning to
    rank): ``group``, the int32 offsets [Q + 1] on the matrix's device (rows
    [group[q], group[q + 1]) are group q) or None, and the ranking kernels'
    task plan, built once per matrix on first use."""

    group = None
    _rank_groups = None

    def set_group(self, group):
        """group: integer offsets [Q + 1] (any device) or None. Malformed
        offsets raise ValueError."""
        from .gbdt_objective import RankGroups
        self.group = self._rank_groups = None
        if group is not None:
            self._rank_groups = RankGroups(group, self.n)
            self.group = self._rank_groups.device_off(self.device)

    def rank_groups(self):
        """The groups with their cached task plan (objective and metrics
        take it as ``group``), or None."""
        return self._rank_groups


# ------------------------------------------------------------------- data
class DMatrix(_QueryGroups, SurvivalData):
    """A rank's rows as a dense device matrix with NaN = missing."""

    sparse = False

    def __init__(self, keys, offset, val, label, weight, ncol, device, group=None,
                 bounds=None):
        n = offset.numel() - 1
        self.n = n
        self.ncol = int(ncol)
        self.device = device
        X = torch.full((n, self.ncol), float("nan"), dtype=torch.float32, device=device)
        if keys.numel():
            rows = torch.repeat_interleave(torch.arange(n), offset[1:] - offset[:-1]).to(device)
            k = keys.to(device)
            m = k < self.ncol
            v = val.to(device) if val is not None else torch.ones(keys.numel(), device=device)
            X[rows[m], k[m]] = v[m]
        self.X = X
        self.label = label.to(device).float()
        self.weight = weight.to(device).float() if weight is not None else None
        self.B = None
        self.set_group(group)
        self.set_bounds(*(bounds or (None, None)))

    @staticmethod
    def from_dense(X, label, device, group=None):
        d = DMatrix.__new__(DMatrix)
        d.n, d.ncol = X.shape
        d.device = device
        d.X = X.to(device).float().contiguous()
        d.label = label.to(device).float()
        d.weight = None
        d.B = None
        d.set_group(group)
        return d

    def predict_tree(self, tree, margin):
        return tree.predict_margin(self.X, margin)

    def predict_forest(self, forest, out, leaf=False):
        """All trees of a packed forest (gbdt_tree.py Forest) in one pass over
        the rows, on the GPU: margins [n] or [K, n] added to ``out`` exactly
        as one predict_tree per tree would, or, leaf, leaf ids [n, T]."""
        _native.hip().gbdt_predict_forest(X=self.X, nodes=forest.nodes, tree_off=forest.tree_off,
                                          chunks=forest.chunks, max_feat=forest.max_feat,
                                          out=out, leaf=leaf)
        return out

    def predict_contribs(self, shap, approx=False, rows=None):
        """Contributions of a packed forest (gbdt_tree.py ShapForest) on the
        GPU, rows [a, b) (default: all): float32 [K, b - a, U + 1] in the
        forest's compact columns, the bias last. approx: Saabas."""
        a, b = rows if rows is not None else (0, self.n)
        X = self.X[a:b]
        out = shap.new_out(b - a, self.device)
        if approx:
            _native.hip().gbdt_saabas(X=X, nodes=shap.nodes, tree_off=shap.tree_off,
                                      node_m=shap.node_m, node_col=shap.node_col,
                                      ncol=shap.used.numel(), max_feat=shap.max_feat, out=out)
        else:
            _native.hip().gbdt_shap(X=X, paths=shap.paths, elems=shap.elems, ecol=shap.ecol,
                                    chunks=shap.chunks, ncol=shap.used.numel(),
                                    max_feat=shap.max_feat, out=out)
        return out

    def predict_contribs_host(self, model, approx=False, rows=None):
        """The same on a CPU matrix by the host reference: (float64
        [K, b - a, U + 1], used). model: the trees' lists, covers, num_class
        and base margin as gbdt_shap_rows names them."""
        a, b = rows if rows is not None else (0, self.n)
        return _native.hip().gbdt_shap_rows(X=self.X[a:b].contiguous(), approx=approx, **model)

    def predict_interactions(self, shap, rows=None):
        """Interaction values of a packed forest (gbdt_tree.py ShapForest) on
        the GPU, rows [a, b) (default: all): float32 [K, b - a, U + 1, U + 1]
        in the forest's compact columns, the bias last."""
        a, b = rows if rows is not None else (0, self.n)
        out = shap.new_inter_out(b - a, self.device)
        _native.hip().gbdt_shap_inter(X=self.X[a:b], paths=shap.paths, elems=shap.elems,
                                      ecol=shap.ecol, chunks=shap.chunks, ncol=shap.used.numel(),
                                      max_feat=shap.max_feat, out=out)
        return out

    def predict_interactions_host(self, model, rows=None):
        """The same on a CPU matrix by the host reference: (float64
        [K, b - a, U + 1, U + 1], used). model: as predict_contribs_host."""
        a, b = rows if rows is not None else (0, self.n)
        return _native.hip().gbdt_shap_inter_rows(X=self.X[a:b].contiguous(), **model)


class CSRMatrix(_QueryGroups, SurvivalData):
    """A rank's rows kept sparse (libsvm data with a wide feature space:
    a dense n x ncol matrix would not fit). Row feature ids are sorted
    ascending within each row; a feature a row does not store is missing
    (default direction), exactly as NaN in the dense matrix."""

    sparse = True

    def __init__(self, keys, offset, val, label, weight, ncol, device, group=None,
                 bounds=None):
        n = offset.numel() - 1
        self.n, self.ncol, self.device = n, int(ncol), device
        off = offset.to(torch.int64)
        k = keys.to(torch.int64)
        v = val.float() if val is not None and val.numel() else None
        if k.numel():
            rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64), off[1:] - off[:-1])
            order = torch.argsort(rows * (self.ncol + 1) + k.clamp(0, self.ncol), stable=True)
            k = k[order]
            v = v[order] if v is not None else None
        self.row_off = off.to(device).contiguous()
        self.fid = k.to(torch.int32).to(device).contiguous()
        self.val = v.to(device).contiguous() if v is not None else None
        self.label = label.to(device).float()
        self.weight = weight.to(device).float() if weight is not None else None
        self.gbin = None
        self.set_group(group)
        self.set_bounds(*(bounds or (None, None)))

    def entry_rows(self):
        return torch.repeat_interleave(torch.arange(self.n, device=self.device),
                                       self.row_off[1:] - self.row_off[:-1])

    def predict_tree(self, tree, margin):
        if self.n == 0:
            return margin
        if self.device.type == "cuda":
            _native.hip().gbdt_predict_csr(self.row_off, self.fid, self.val,
                                           *tree.device_arrays(self.device), margin)
            return margin
        return tree.predict_margin(self.dense_cpu(), margin)

    def predict_forest(self, forest, out, leaf=False):
        """As DMatrix.predict_forest, an absent feature standing for NaN."""
        _native.hip().gbdt_predict_forest_csr(row_off=self.row_off, fid=self.fid, val=self.val,
                                              nodes=forest.nodes, tree_off=forest.tree_off,
                                              chunks=forest.chunks, out=out, leaf=leaf)
        return out

    def predict_contribs(self, shap, approx=False, rows=None):
        """As DMatrix.predict_contribs, an absent feature standing for NaN."""
        a, b = rows if rows is not None else (0, self.n)
        row_off = self.row_off[a:b + 1]  # (offsets stay absolute: fid and val are whole)
        out = shap.new_out(b - a, self.device)
        if approx:
            _native.hip().gbdt_saabas_csr(row_off=row_off, fid=self.fid, val=self.val,
                                          nodes=shap.nodes, tree_off=shap.tree_off,
                                          node_m=shap.node_m, node_col=shap.node_col,
                                          ncol=shap.used.numel(), out=out)
        else:
            _native.hip().gbdt_shap_csr(row_off=row_off, fid=self.fid, val=self.val,
                                        paths=shap.paths, elems=shap.elems, ecol=shap.ecol,
                                        chunks=shap.chunks, ncol=shap.used.numel(), out=out)
        return out

    def predict_contribs_host(self, model, approx=False, rows=None):
        """As DMatrix.predict_contribs_host, over the CSR rows themselves."""
        a, b = rows if rows is not None else (0, self.n)
        return _native.hip().gbdt_shap_rows_csr(row_off=self.row_off[a:b + 1].contiguous(),
                                                fid=self.fid, val=self.val, approx=approx,
                                                **model)

    def predict_interactions(self, shap, rows=None):
        """As DMatrix.predict_interactions, an absent feature standing for NaN."""
        a, b = rows if rows is not None else (0, self.n)
        out = shap.new_inter_out(b - a, self.device)
        _native.hip().gbdt_shap_inter_csr(row_off=self.row_off[a:b + 1], fid=self.fid,
                                          val=self.val, paths=shap.paths, elems=shap.elems,
                                          ecol=shap.ecol, chunks=shap.chunks,
                                          ncol=shap.used.numel(), out=out)
        return out

    def predict_interactions_host(self, model, rows=None):
        """As DMatrix.predict_interactions_host, over the CSR rows themselves."""
        a, b = rows if rows is not None else (0, self.n)
        return _native.hip().gbdt_shap_inter_rows_csr(row_off=self.row_off[a:b + 1].contiguous(),
                                                      fid=self.fid, val=self.val, **model)

    def dense_cpu(self):
        """(CPU reference path only: small matrices)"""
        X = torch.full((self.n, self.ncol), float("nan"))
        rows = self.entry_rows().cpu()
        ok = self.fid.cpu().long() < self.ncol
        X[rows[ok], self.fid.cpu().long()[ok]] = (self.val.cpu()[ok] if self.val is not None
                                                  else torch.ones(int(ok.sum())))
        return X


def make_dmatrix(keys, offset, val, label, weight, ncol, device, sparse=None, group=None,
                 bounds=None):
    """Dense device matrix, or CSR when asked (sparse=True) or when the dense
    form would be large and mostly missing (auto: sparse=None). group: the
    rows' query group offsets [Q + 1] (learning to rank) or None. bounds:
    survival:aft's (lower, upper), one entry per row each, or None."""
    n = offset.numel() - 1
    if sparse is None:
        cells = n * max(int(ncol), 1)
        sparse = int(ncol) > 4096 or (cells > (1 << 28) and keys.numel() < cells // 8)
    if sparse:
        return CSRMatrix(keys, offset, val, label, weight, ncol, device, group, bounds)
    return DMatrix(keys, offset, val, label, weight, ncol, device, group, bounds)


class Cuts:
    def __init__(self, values, offsets):
        self.values = values  # float32 [total]
        self.offsets = offsets  # int32 [F + 1]

    @property
    def nbin_max(self):
        o = self.offsets.tolist()
        return max(b - a for a, b in zip(o, o[1:])) if len(o) > 1 else 1

    @staticmethod
    def build(dm, max_bin, bsp, hess=None, nsummary=None):
        """Hessian-weighted quantile sketch (xgboost's WQSketch semantics):
        every stored value weighs its row's hessian (x instance weight; the
        hessian at the base margin when not given), cuts split each
        feature's weight evenly. Each rank summarises its values into <= 4 x
        max_bin weighted points per feature; the summaries are all-gathered
        and merged by the same weighted quantile rule."""
        max_bin = min(int(max_bin), 255)
        nsummary = nsummary or 4 * max_bin
        w_row = hess if hess is not None else torch.ones(dm.n, device=dm.device)
        if dm.weight is not None:
            w_row = w_row * dm.weight
        w_row = w_row.float()
        if dm.sparse:
            fid, v, w = dm.fid.long(), (dm.val if dm.val is not None else
                                        torch.ones(dm.fid.numel(), device=dm.device)), None
            w = w_row[dm.entry_rows()] if dm.n else torch.zeros(0, device=dm.device)
            ok = (fid >= 0) & (fid < dm.ncol)
            sf, sv, sw = Cuts._summary(fid[ok], v[ok].float(), w[ok], dm.ncol, nsummary)
        else:
            F = dm.ncol
            parts = []
            for j in range(F):
                col = dm.X[:, j]
                ok = ~torch.isnan(col)
                parts.append((torch.full((int(ok.sum()),), j, dtype=torch.int64,
                                         device=dm.device), col[ok], w_row[ok]))
            sf, sv, sw = Cuts._summary(torch.cat([p[0] for p in parts]),
                                       torch.cat([p[1] for p in parts]),
                                       torch.cat([p[2] for p in parts]), F, nsummary)
        local = (sf.cpu(), sv.double().cpu(), sw.double().cpu())
        gathered = bsp.comm.allgather_object(local) if bsp.world > 1 else [local]
        f_all = torch.cat([g[0] for g in gathered])
        v_all = torch.cat([g[1] for g in gathered])
        w_all = torch.cat([g[2] for g in gathered])
        order = torch.argsort(f_all * 0 + v_all, stable=True)
        order = order[torch.argsort(f_all[order], stable=True)]
        f_all, v_all, w_all = f_all[order], v_all[order], w_all[order]
        return Cuts._cuts_from_sorted(f_all, v_all, w_all, dm.ncol, max_bin)

    @staticmethod
    def _segsum(w, ids, nseg):
        """Sums of w over runs of equal, nondecreasing ids in [0, nseg): by
        prefix-sum differences -- a GPU index_add over sorted ids piles
        every row of a run onto one fp64 atomic address (seconds at 11M x 28)."""
        cnt = torch.bincount(ids, minlength=nseg)
        cwp = torch.zeros(w.numel() + 1, dtype=torch.float64, device=w.device)
        torch.cumsum(w.double(), 0, out=cwp[1:])
        end = torch.cumsum(cnt, 0)
        return cwp[end] - cwp[end - cnt]

    @staticmethod
    def _summary(fid, v, w, ncol, m):
        """Per feature: the distinct values when there are <= m, else m
        weighted quantile points each carrying its bucket's weight."""
        if fid.numel() == 0:
            z = torch.zeros(0)
            return z.long(), z, z
        order = torch.argsort(v, stable=True)
        order = order[torch.argsort(fid[order], stable=True)]
        fid, v, w = fid[order], v[order].double(), w[order].double()
        # merge equal (feature, value) runs
        new = torch.ones(fid.numel(), dtype=torch.bool, device=fid.device)
        new[1:] = (fid[1:] != fid[:-1]) | (v[1:] != v[:-1])
        grp = torch.cumsum(new.long(), 0) - 1
        ng = int(grp[-1]) + 1
        fid, v = fid[new], v[new]
        w = Cuts._segsum(w, grp, ng)
        cnt = torch.bincount(fid, minlength=ncol)
        start = torch.cumsum(cnt, 0) - cnt
        big = cnt[fid] > m
        if bool(big.any()):
            cw = torch.cumsum(w, 0)
            fw = Cuts._segsum(w, fid, ncol)
            base = cw[start[fid]] - w[start[fid]]
            q = ((cw - base) / fw[fid].clamp_min(1e-300) * m).floor().clamp(max=m - 1)
            key = fid * (m + 1) + q.long()
            keep_bkt = torch.ones_like(new[: fid.numel()])
            keep_bkt[1:] = key[1:] != key[:-1]
            # a big feature keeps the last value of each weight bucket with
            # the bucket's weight; small features keep every value
            last = torch.ones_like(keep_bkt)
            last[:-1] = key[1:] != key[:-1]
            bid = torch.cumsum(keep_bkt.long(), 0) - 1
            bw = Cuts._segsum(w, bid, int(bid[-1]) + 1)
            keep = ~big | last
            wout = torch.where(big, bw[bid], w)
            return fid[keep], v[keep], wout[keep]
        return fid, v, w

    @staticmethod
    def _cuts_from_sorted(fid, v, w, ncol, max_bin):
        vals, offs = [], [0]
        fid, v, w = fid.long(), v.double(), w.double()
        cnt = torch.bincount(fid, minlength=ncol).tolist() if fid.numel() else [0] * ncol
        pos = 0
        for j in range(ncol):
            c = cnt[j]
            if c:
                vals.extend(Cuts._feature_cuts(v[pos:pos + c], w[pos:pos + c], max_bin))
            pos += c
            offs.append(len(vals))
        return Cuts(torch.tensor(vals, dtype=torch.float32), torch.tensor(offs, dtype=torch.int32))

    @staticmethod
    def _feature_cuts(v, w, max_bin):
        if v.numel() == 0:
            return []
        order = torch.argsort(v)
        v, w = v[order].double(), w[order]
        uniq, inv = torch.unique_consecutive(v, return_inverse=True)
        uw = torch.zeros(uniq.numel(), dtype=torch.float64).index_add_(0, inv, w)
        last = float(uniq[-1])
        top = last + abs(last) + 1.0
        if uniq.numel() <= max_bin:
            cuts = uniq[1:].tolist() + [top]
        else:
            cw = torch.cumsum(uw, 0)
            total = float(cw[-1])
            cuts = []
            for b in range(1, max_bin):
                target = total * b / max_bin
                i = int(torch.searchsorted(cw, torch.tensor([target], dtype=torch.float64)))
                i = min(i + 1, uniq.numel() - 1)
                c = float(uniq[i])
                if not cuts or c > cuts[-1]:
                    cuts.append(c)
            cuts.append(top)
        return [float(np.float32(c)) for c in cuts]

    def bin(self, dm):
        if dm.sparse:
            if dm.device.type == "cuda":
                return _native.hip().gbdt_bin_csr(dm.fid, dm.val, dm.ncol,
                                                  self.values.to(dm.device),
                                                  self.offsets.to(dm.device))
            fid = dm.fid.long()
            v = dm.val if dm.val is not None else torch.ones(fid.numel())
            o = self.offsets.tolist()
            g = torch.full((fid.numel(),), -1, dtype=torch.int32)
            for j in range(dm.ncol):
                m = fid == j
                if o[j + 1] > o[j] and bool(m.any()):
                    c = self.values[o[j]:o[j + 1]]
                    b = torch.searchsorted(c, v[m], right=True).clamp(max=c.numel() - 1)
                    g[m] = (b + o[j]).to(torch.int32)
            return g
        if dm.X.is_cuda:
            return _native.hip().gbdt_bin(dm.X, self.values.to(dm.device),
                                          self.offsets.to(dm.device))
        out = torch.full(dm.X.shape, MISSING_BIN, dtype=torch.uint8)
        o = self.offsets.tolist()
        for j in range(dm.ncol):
            c = self.values[o[j]:o[j + 1]]
            col = dm.X[:, j]
            ok = ~torch.isnan(col)
            b = torch.searchsorted(c, col[ok], right=True).clamp(max=c.numel() - 1)
            out[ok, j] = b.to(torch.uint8)
        return out
