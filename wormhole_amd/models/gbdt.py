"""Distributed histogram GBDT: the xgboost learner the
reference wraps (bin/xgboost.dmlc, learn/xgboost/), built from scratch on
HIP kernels + RCCL.

Algorithm (xgboost "hist" semantics, row split ``dsplit=row``):

* quantile cuts per feature from rank-local order statistics that are
  all-gathered and merged (<= max_bin cuts; features with few distinct values
  get one bin per value); values are binned once into a uint8 matrix
  (255 = missing) that stays resident in HBM;
* per level, LDS-privatised (g, h) histograms are built only for the smaller
  child of every split (the sibling is parent - child), allreduced over the
  ranks (RCCL), and scanned for the best split of every node: gain
  G_L^2/(H_L+lambda) + G_R^2/(H_R+lambda) - G^2/(H+lambda) with L1 ``alpha``,
  ``min_child_weight`` on both children, and both default directions for
  missing values;
* rows are stably partitioned per node on the device;
* the grown tree is pruned bottom-up with ``gamma`` (xgboost's prune updater)
  and leaves store eta * weight; training margins are updated from the final
  leaf segments, other sets by a device tree walk.
"""
import os

import numpy as np
import torch

from .. import _native
# the family's other modules: parameters / objectives / metrics, the data
# matrices and cuts, the trees and the model (every public name stays
# reachable from this module)
from .gbdt_objective import (ADAPTIVE_OBJECTIVES, AdaptiveObjective, GBDTParam,  # noqa: F401
                             INTERACTION_FREE, make_objective,
                             INTERACTION_ROOT, MULTI_METRICS, NLL_MAX, OBJ_ABSOLUTE, OBJ_IDS,
                             OBJ_LOGISTIC, OBJ_METRICS, OBJ_QUANTILE, Objective,
                             RANK_OBJECTIVES, RankGroups, SINGLE_METRICS, adaptive_gpair_torch,
                             class_gpair,
                             eval_metric, first_argmax, gpair_stats, interaction_child,
                             multi_eval_sums, obj_eval_sums, obj_gpair_torch, parse_obj_metric,
                             parse_rank_metric, rank_eval, rank_eval_torch, rank_gpair_torch,
                             rank_metric, softmax_gpair_torch)
from .gbdt_survival import (AFT_DISTS, SURVIVAL_METRICS, SURVIVAL_OBJECTIVES, CoxPlan,  # noqa: F401
                            aft_eval_sums, aft_eval_torch, aft_gpair, aft_gpair_torch,
                            cox_eval_sums, cox_eval_torch, cox_gpair, cox_gpair_torch)
from .gbdt_data import MISSING_BIN, CSRMatrix, Cuts, DMatrix, make_dmatrix  # noqa: F401
from .gbdt_tree import Booster, RegTree, _DeviceTree, load_fmap  # noqa: F401
from .gbdt_quantile import (leaf_quantiles, leaf_quantiles_ref, parse_quantile_alpha,  # noqa: F401
                            pinball_sums, refresh_leaves, round_weights, select_torch,
                            weight_scale)

RT_EPS = 1e-6
_HIST32_ROWS = 8192  # rows per int32 LDS pass of the GPU histogram
# Alternate device paths, kept as the tests' cross-checks (process-wide, the
# same on every rank):
HIST32 = True  # int32 LDS histogram passes (False: int64 sums throughout)
LEAF_WALK_LDS = True  # the LDS-resident tree walk when it fits (False: global walk)
DEFER_TREES = True  # device trees: host lists one tree later (False: read every tree at once)
HOST_GROWER = False  # the per-level host grower instead of the device level loop
DART_BIN_WALK = True  # booster=dart: dropped trees walked on the bins from LDS (False: forest kernels)
LEAF_LOOP_DEV = True  # grow_policy=lossguide: the leaf loop on the device (False: the Python leaf loop)
# bytes of node histograms the device leaf loop may hold (one per node id, 2 x
# max_leaves - 1 of them); a larger tree takes the Python leaf loop
LEAF_POOL_BYTES = 4 << 30


def _h2d(t, dev):
    """Host -> device without a synchronous pageable copy: the per-level
    tables (segments, split descriptions, hist tasks) go through pinned
    memory, asynchronously on the current stream."""
    dev = torch.device(dev)
    if dev.type != "cuda":
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


# ------------------------------------------------------ histogram exchange
class HistExchange:
    """Feature-sharded histogram exchange of the multi-rank dense grower
    (xgboost's row split, ``dsplit=row``, allreduces every
    level's histograms, learn/xgboost/mushroom.hadoop.conf:33).

    Rank r owns the contiguous feature slice ``ranges[r]``. A level's built
    histograms -- the rank-local partial sums [S, F, nbin, 2] -- go out as
    ONE all-to-all-v of feature-major rows (each peer receives its slice
    only) and are summed locally in rank order: a reduce-scatter by feature,
    (P-1)/P of the histogram bytes per rank on the wire where a ring
    allreduce moves 2(P-1)/P. Each rank keeps only its slice of the node
    histograms (sibling subtraction included), searches splits over its
    features, and the per-slot best candidates [S, 6] are all-gathered and
    reduced by gain (ties: lowest rank = lowest feature index, the same
    winner as a row-major argmax over all features on one rank). Trees are
    identical to the allreduce grower's (``WH_GBDT_XCHG=allreduce`` keeps
    that path): on the GPU the histograms are exact fixed-point sums, so the
    reduction order cannot matter."""

    def __init__(self, bsp, F):
        self.comm = bsp.comm
        self.P, self.rank = bsp.world, bsp.rank
        per = -(-F // self.P) if F else 0
        self.ranges = [(min(F, r * per), min(F, (r + 1) * per)) for r in range(self.P)]
        self.lo, self.hi = self.ranges[self.rank]
        self.sent = 0  # bytes this rank sent to its peers (histograms + candidates)

    @staticmethod
    def mode(bsp, dense):
        if bsp.world <= 1 or not dense:
            return None
        return None if os.environ.get("WH_GBDT_XCHG", "rs") == "allreduce" else "rs"

    def reduce_scatter(self, h):
        """h [S, F, nbin, 2] local partials -> [S, Fr, nbin, 2] global sums
        of this rank's features."""
        S, F = int(h.shape[0]), int(h.shape[1])
        rest = tuple(h.shape[2:])
        width = S
        for d in rest:
            width *= int(d)
        x = h.transpose(0, 1).reshape(F, width)  # feature-major rows
        send = [hi - lo for lo, hi in self.ranges]
        fr = self.hi - self.lo
        out = self.comm.all_to_all_v(x, send, [fr] * self.P)
        self.sent += (F - fr) * width * x.element_size()
        acc = out[0:fr].clone()
        for q in range(1, self.P):  # rank order: deterministic on the CPU path too
            acc += out[q * fr:(q + 1) * fr]
        return acc.view((fr, S) + rest).transpose(0, 1).contiguous()

    def pick(self, cand):
        """cand [S, 6] {gain, feature (global), bin, dir, GL, HL}: this
        rank's best per slot -> the best over all ranks."""
        cand = cand.contiguous()
        allc = torch.stack(self.comm.allgather(cand))  # [P, S, 6]
        self.sent += (self.P - 1) * cand.numel() * cand.element_size()
        r = torch.argmax(allc[:, :, 0], 0)  # first maximum: lowest rank on ties
        return allc.gather(0, r[None, :, None].expand(1, cand.shape[0], cand.shape[1]))[0]


# ----------------------------------------------------------- split search
# A level's best splits, one row per slot: the float64 [S, 6] table
# {gain, feature, bin, dir, GL, HL} that the split kernels write, the feature
# exchange reduces (HistExchange.pick) and the level loop reads on the host.
def split_table(gain, feat, bin_, dir_, left):
    """[S, 6] from its fields (left: {GL, HL} [S, 2])."""
    return torch.cat([gain[:, None].double(), feat[:, None].double(), bin_[:, None].double(),
                      dir_[:, None].double(), left.double()], 1)


def split_fields(t):
    """(gain, feature, bin, dir, {GL, HL}) of a host [S, 6] table."""
    return t[:, 0], t[:, 1].long(), t[:, 2].long(), t[:, 3].long(), t[:, 4:6]


def admitted(fmask, state):
    """interaction_constraints: the bool table [S, F] of the (slot, feature)
    pairs that may split -- the slot's group set shares a bit with the
    feature's (fmask [F], state [S]: int64 bit patterns)."""
    return (state.to(fmask.device)[:, None] & fmask[None, :]) != 0


def split_gains(p, hist, totals, valid, mono=None, bounds=None, fmask=None, state=None):
    """Every candidate of a level: (gain [S, F, nbin, 2 directions] with -inf
    for what is no candidate, left sums [S, F, nbin, 2 directions, 2]); the
    arguments of :func:`find_splits_ref`."""
    cum = hist.cumsum(2)
    present = cum[:, :, -1, :]
    tot = totals[:, None, None, :]
    miss = (totals[:, None, :] - present)[:, :, None, :]
    G, H = totals[:, 0], totals[:, 1]
    if mono is None:
        parent_gain = p.calc_gain(G, H)[:, None, None]
    else:
        bounds = bounds.to(hist.device).double()
        c = mono.to(hist.device)[None, :, None]
        lo, hi = bounds[:, 0], bounds[:, 1]
        parent_gain = p.calc_gain_bounded(G, H, lo, hi)[0][:, None, None]
        lo, hi = lo[:, None, None], hi[:, None, None]
    cands = []
    for defl in (0, 1):
        L = cum + (miss if defl else 0.0)
        R = tot - L
        ok = (L[..., 1] >= p.min_child_weight) & (R[..., 1] >= p.min_child_weight)
        if mono is None:
            gain = (p.calc_gain(L[..., 0], L[..., 1]) + p.calc_gain(R[..., 0], R[..., 1])
                    - parent_gain)
        else:
            gl, wl = p.calc_gain_bounded(L[..., 0], L[..., 1], lo, hi)
            gr, wr = p.calc_gain_bounded(R[..., 0], R[..., 1], lo, hi)
            gain = gl + gr - parent_gain
            ok = ok & ~(((c > 0) & (wl > wr)) | ((c < 0) & (wl < wr)))
        gain = torch.where(ok, gain, torch.full_like(gain, -float("inf")))
        cands.append((gain, L))
    gain = torch.stack([c[0] for c in cands], -1)  # [S, F, nbin, 2dir]
    # thresholds past a feature's own bin count, and features dropped by
    # colsample_bytree, are not candidates
    gain = torch.where(valid.to(gain.device)[None, :, :, None], gain,
                       torch.full_like(gain, -float("inf")))
    if fmask is not None:
        adm = admitted(fmask.to(gain.device), state)
        gain = torch.where(adm[:, :, None, None], gain, torch.full_like(gain, -float("inf")))
    return gain, torch.stack([cands[0][1], cands[1][1]], 3)


def find_splits_ref(p, hist, totals, valid, mono=None, bounds=None, fmask=None, state=None):
    """Parameters p; hist [S, F, nbin, 2] (global sums); totals [S, 2]; valid
    [F, nbin] bool -> the host split table: the torch reference of the fused
    kernels (and the CPU path). monotone_constraints: mono [F] int8 and the
    slots' weight intervals bounds [S, 2] (float64) -- each side's gain is
    taken at its clamped weight and a candidate whose child weights are
    ordered against its feature's constraint is rejected.
    interaction_constraints: fmask [F] and the slots' states [S] (int64 bit
    sets of groups) -- a (slot, feature) pair that :func:`admitted` refuses
    has no candidate."""
    # Lall [S, F, nbin, 2dir, 2]
    gain, Lall = split_gains(p, hist, totals, valid, mono, bounds, fmask, state)
    S, nbin = gain.shape[0], gain.shape[2]
    flat = gain.reshape(S, -1)
    arg = flat.argmax(1)
    bg = flat.gather(1, arg[:, None])[:, 0]
    d = arg % 2
    rest = arg // 2
    b = rest % nbin
    f = rest // nbin
    Ls = Lall[torch.arange(S, device=arg.device), f, b, d]  # [S, 2]
    # one device->host transfer for the whole level
    return split_table(bg, f, b, d, Ls).cpu()


def find_splits(p, hist, totals, valid, mono=None, bounds=None, fmask=None, state=None):
    """:func:`find_splits_ref`, on the GPU by the fused split-search kernels
    (csrc/hip/gbdt.hip k_split_feat / k_split_node: scan + gain + argmax in
    two launches instead of ~40 elementwise ops per level)."""
    if hist.is_cuda and hist.shape[0] > 0 and hist.shape[2] <= 1024:
        if mono is not None:
            mono = mono.to(hist.device).contiguous()
            bounds = bounds.to(hist.device).double().contiguous()
        inter = {}
        if fmask is not None:
            inter = dict(fmask=fmask.to(hist.device).contiguous(),
                         state=state.to(hist.device).contiguous())
        return _native.hip().gbdt_split(hist.double().contiguous(), totals.double().contiguous(),
                                        valid.to(hist.device).contiguous(), float(p.alpha),
                                        float(p.reg_lambda), float(p.min_child_weight),
                                        mono=mono, bounds=bounds, **inter).cpu()
    return find_splits_ref(p, hist, totals, valid, mono, bounds, fmask, state)


def find_splits_csr_ref(p, hist, totals, cut_off, fvalid=None, mono=None, bounds=None,
                        fmask=None, state=None):
    """:func:`find_splits_ref` over compact histograms [S, total bins, 2]
    (feature f owns bins cut_off[f]:cut_off[f + 1], a list; fvalid [F]: this
    tree's candidate features, or None): the CSR builder's CPU path and the
    reference of the CSR split kernels. (Unconstrained gains are taken on
    torch scalars, in fp32; bounded ones in Python floats.) fmask / state: as
    :func:`find_splits_ref`."""
    o = cut_off
    S = hist.shape[0]
    res = torch.zeros(S, 6, dtype=torch.float64)
    for s_ in range(S):
        TG, TH = float(totals[s_, 0]), float(totals[s_, 1])
        if mono is None:
            parent = float(p.calc_gain(torch.tensor(TG), torch.tensor(TH)))
        else:
            lo, hi = float(bounds[s_, 0]), float(bounds[s_, 1])
            parent = p.side_gain_bounded(TG, TH, lo, hi)[0]
        best = (-float("inf"), 0, 0, 0, 0.0, 0.0)
        for f in range(len(o) - 1):
            if o[f + 1] <= o[f] or (fvalid is not None and not int(fvalid[f])):
                continue
            if fmask is not None and not int(state[s_]) & int(fmask[f]):
                continue
            hb = hist[s_, o[f]:o[f + 1]]
            cum = hb.cumsum(0)
            mg, mh = TG - float(cum[-1, 0]), TH - float(cum[-1, 1])
            for b in range(hb.shape[0]):
                for d in (0, 1):
                    GL = float(cum[b, 0]) + (mg if d else 0.0)
                    HL = float(cum[b, 1]) + (mh if d else 0.0)
                    GR, HR = TG - GL, TH - HL
                    if not (HL >= p.min_child_weight and HR >= p.min_child_weight):
                        continue
                    if mono is None:
                        g = (float(p.calc_gain(torch.tensor(GL), torch.tensor(HL))) +
                             float(p.calc_gain(torch.tensor(GR), torch.tensor(HR))) - parent)
                    else:
                        gl, wl = p.side_gain_bounded(GL, HL, lo, hi)
                        gr, wr = p.side_gain_bounded(GR, HR, lo, hi)
                        c = int(mono[f])
                        if (c > 0 and wl > wr) or (c < 0 and wl < wr):
                            continue
                        g = gl + gr - parent
                    if g > best[0]:
                        best = (g, f, b, d, GL, HL)
        res[s_] = torch.tensor(best, dtype=torch.float64)
    return res


def child_bounds(c, lo, hi, wl, wr):
    """The weight intervals of an accepted split's children ((lo, hi) left,
    (lo, hi) right): its feature's constraint c cuts the node's interval at
    the mean of the (clamped) child weights."""
    mid = (wl + wr) / 2
    if c > 0:
        return (lo, mid), (mid, hi)
    if c < 0:
        return (mid, hi), (lo, mid)
    return (lo, hi), (lo, hi)


def partition_ref(ridx, node_feat, node_bin, node_defl, seg_beg, seg_end, local_bin):
    """The stable per-node row partition on the CPU, the reference of the
    partition kernels -> (new ridx, left counts per node). A row of node nd
    goes left by its bin of feature node_feat[nd]: ``local_bin(f, rows)``
    (long; MISSING_BIN where a row does not store f: then by node_defl)."""
    out = ridx.clone()
    nleft = torch.zeros(node_feat.numel(), dtype=torch.int32)
    for nd in range(node_feat.numel()):
        f = int(node_feat[nd])
        if f < 0:
            continue
        b, e = int(seg_beg[nd]), int(seg_end[nd])
        bins = local_bin(f, ridx[b:e].long())
        left = torch.where(bins == MISSING_BIN, torch.full_like(bins, int(node_defl[nd])),
                           (bins <= int(node_bin[nd])).long()).bool()
        nl = int(left.sum())
        out[b:b + nl] = ridx[b:e][left]
        out[b + nl:e] = ridx[b:e][~left]
        nleft[nd] = nl
    return out, nleft


# ---------------------------------------------------------------- builder
class _LevelGrower:
    """What the dense and the CSR builder share: the collective choice of the
    grower, the Python level loop (the CPU path and the native growers'
    reference), histogram reduction, pruning and the margin update. A builder
    adds ``_build_hist``, ``_find_splits``, the partition's ``_local_bin``
    (CPU) and ``_partition_op`` (GPU) and, the dense one, ``_build_native``."""

    def __init__(self, param, bsp, dm, cuts):
        self.p, self.bsp, self.dm, self.cuts = param, bsp, dm, cuts
        self.device = torch.device(dm.device)
        self.gpu = self.device.type == "cuda"
        self.F = dm.ncol
        self.xchg = None  # feature-sharded histogram exchange (the dense builder's)
        self.ar_sent = 0  # allreduced histogram bytes per rank (ring model: 2 (P-1) / P)
        self._nglobal = self._iota_t = None
        self._native = None  # grower choice, made collectively at the first build()
        self._pending = None  # the deferred device tree whose host lists are still to build
        self._qscale = None  # this tree's fixed-point histogram scales (GPU)
        self._cut_lists = (cuts.values.tolist(), cuts.offsets.tolist())
        # monotone_constraints: int8 [F] (host), None when not set; _mono_dev
        # is the device copy the kernels read
        self.mono = param.monotone_vector(self.F)
        self._mono_dev = None
        # max_delta_step = d > 0: the root's weight interval is (-d, d) on the
        # same bounds path (an all-zero sign vector when none is set), so
        # every node's weight is clamped to it and a clamped side is scored
        # by the bounded formula; 0: off, nothing changes
        self.max_delta_step = param.delta_step()
        if self.max_delta_step > 0 and self.mono is None:
            self.mono = torch.zeros(self.F, dtype=torch.int8)
        # interaction_constraints: the features' group bit sets, int64 [F]
        # (host; gbdt_objective.py interaction_vector), None when not set
        self.fmask = param.interaction_vector(self.F)
        self._fmask_dev = None
        # grow_policy=lossguide: (leaves, depth) in effect; None: depth-wise
        self.limits = param.leaf_limits()

    def _fmask(self):
        if self.fmask is not None and self._fmask_dev is None:
            self._fmask_dev = self.fmask.to(self.device).contiguous()
        return self._fmask_dev

    def _mono(self):
        if self.mono is not None and self._mono_dev is None:
            self._mono_dev = self.mono.to(self.device).contiguous()
        return self._mono_dev

    def _draw_features(self, gen):
        """colsample_bytree: the bool mask [F] of this tree's candidate
        features (one ``randperm`` per call), or None for all of them."""
        if not (self.p.colsample_bytree < 1.0 and self.F > 0):
            return None
        k = max(1, int(round(self.p.colsample_bytree * self.F)))
        keep = torch.randperm(self.F, generator=gen)[:k]
        m = torch.zeros(self.F, dtype=torch.bool)
        m[keep] = True
        return m

    def _hist_scale(self, gpair):
        """Fixed-point scales {2^eg, 2^eh} of the GPU histograms: the largest
        powers of two with (global rows) * max|g| * 2^eg <= 2^61, so no node's
        int64 sum can overflow on any rank (see csrc/hip/gbdt.hip).  Unless
        WH_GBDT_HIST=64, a third entry R selects the int32 LDS histograms:
        every row is rounded to 2^-17 of max|g| (|q| <= 2^30 / R) and blocks
        sum <= R rows at a time with 32-bit LDS atomics, ~2x the rate of the
        int64 ones.  The rounding is the same in every block, so histograms
        stay exact sums of the rounded rows (identical for any chunking)."""
        if self._nglobal is None:
            self._nglobal = max(1, int(self.bsp.allreduce_scalar(self.dm.n)))
        m = gpair_stats(gpair)[1] if self.dm.n else torch.zeros(2, device=self.device)
        m = m.float().contiguous()
        self.bsp.allreduce(m, op="max")
        r32 = _HIST32_ROWS if HIST32 else 0
        if m.is_cuda:  # one launch (csrc/hip/gbdt.hip k_qscale), same formula as below
            return _native.hip().gbdt_qscale(m, float(self._nglobal), r32)
        e = torch.floor(torch.log2(2.0 ** 61 / (self._nglobal * m.double().clamp_min(1e-30))))
        if r32:
            # int32 LDS sums of <= R rows: |q| <= 2^30 / R per row (k_hist W32)
            e32 = torch.floor(torch.log2(2.0 ** 30 / (_HIST32_ROWS * m.double().clamp_min(1e-30))))
            e = torch.minimum(e, e32)
            rows = torch.full((1,), float(_HIST32_ROWS), dtype=torch.float64, device=e.device)
            return torch.cat([torch.pow(2.0, e.clamp(-60, 100)), rows]).float()
        scale = torch.pow(2.0, e.clamp(-60, 100))
        return scale.float()

    # ----------------------------------------------------------------- build
    def build(self, gpair, margin, refresh=None):
        """refresh: an adaptive objective's residual inputs (dict(label, at,
        weight, keep, alpha), :func:`grow_round`): the pruned tree's leaves
        become eta x the weighted quantile of their rows' residuals before
        the tree is added to the margins. None: no refresh."""
        if self._native is None:
            # every rank must take the same grower (their allreduce sequences
            # differ): native only if every rank can, decided once, together
            ok = self.gpu and self.dm.n > 0 and not self.dm.sparse
            self._native = bool(self.bsp.allreduce_scalar(1.0 if ok else 0.0, "min") > 0)
        if self.limits is not None:  # grow_policy=lossguide
            if self._native and self._leaf_dev():
                return self._build_leaf_native(gpair, margin, refresh)
            return self._build_leafwise(gpair, margin, refresh)
        if self._native:
            return self._build_native(gpair, margin, refresh)
        return self._build_py(gpair, margin, refresh)

    def _leaf_dev(self):
        """True when the device leaf loop grows this builder's trees: the
        dense GPU matrix (``_native``) on one rank, with a histogram per node
        id within LEAF_POOL_BYTES."""
        return False

    def _build_leafwise(self, gpair, margin, refresh=None):
        """grow_policy=lossguide: best-first growth, one split per step, over
        the same hooks as :meth:`_build_py` -- on the CPU, on CSR data, on
        several ranks (either histogram exchange) and, with the GPU kernels
        behind the hooks, on the GPU (there it is the device leaf loop's
        reference, :meth:`TreeBuilder._build_leaf_native`). The open leaves keep their histograms
        and best splits; a step picks the one with the largest gain (gain >
        RT_EPS, depth below the cap; ties: the smaller node id --
        csrc/host/gbdt_leaf_plan.h), makes nodes 2k + 1 and 2k + 2 of it,
        partitions its rows, builds the histogram of the child with the
        smaller global hessian, derives the sibling's and searches both. It
        ends at ``max_leaves`` leaves or when no leaf is eligible. A step
        passes over all n positions (``_pos_node`` / ``_partition``) and, on
        the GPU, waits for the host once: accepted for a host-driven loop."""
        p = self.p
        n = self.dm.n
        dev = self.device
        max_leaves, depth_cap = self.limits
        pick = _native.hip().gbdt_leaf_pick
        tree = RegTree()
        root = tree.add(-1)
        ridx = torch.arange(n, dtype=torch.int32, device=dev)
        tot = gpair_stats(gpair)[0] if n else torch.zeros(2, dtype=torch.float64, device=dev)
        self.bsp.allreduce(tot)
        totals = {root: tot.cpu()}
        top = self.max_delta_step if self.max_delta_step > 0 else float("inf")
        bounds = {root: (-top, top)} if self.mono is not None else None
        state = {root: INTERACTION_ROOT} if self.fmask is not None else None
        fmask_h = self.fmask.tolist() if self.fmask is not None else None
        seg = {root: (0, n)}  # every current leaf's ridx segment
        depth = {root: 0}
        if self.gpu:
            self._qscale = self._hist_scale(gpair)
        cuts_v, cuts_o = self._cut_lists

        def weigh(nd):
            G, H = float(totals[nd][0]), float(totals[nd][1])
            tree.cover[nd] = H
            tree.base_weight[nd] = (p.calc_weight(G, H) if bounds is None else
                                    p.calc_weight_bounded(G, H, *bounds[nd]))
            tree.leaf[nd] = p.eta * tree.base_weight[nd]

        def search(nodes, H_all):
            """The best splits of ``nodes`` (histograms H_all, in their
            order): rows of the host split table."""
            T_all = _h2d(torch.stack([totals[nd] for nd in nodes]), H_all.device)
            B_all = S_all = None
            if bounds is not None:
                B_all = torch.tensor([bounds[nd] for nd in nodes], dtype=torch.float64)
            if state is None:
                return self._find_splits(H_all, T_all, B_all)
            S_all = torch.tensor([state[nd] for nd in nodes], dtype=torch.int64)
            return self._find_splits(H_all, T_all, B_all, S_all)

        weigh(root)
        # open leaves: node -> (histogram, its row of the split table); a leaf
        # that can never be split (at the depth cap, or made by the last step)
        # is not searched and is not open
        open_ = {}
        if max_leaves > 1:
            h = self._reduce_hist(self._build_hist(ridx, gpair, [seg[root]], [0], 1))
            open_[root] = (h[0], search([root], h)[0])
        leaves = 1
        while leaves < max_leaves:
            ids = list(open_)
            k = pick(node=ids, depth=[depth[nd] for nd in ids],
                     gain=[float(open_[nd][1][0]) for nd in ids], rt_eps=RT_EPS,
                     depth_cap=depth_cap)
            if k < 0:
                break
            nd = ids[k]
            hist_nd, row = open_.pop(nd)
            bg, bf, bb, bd, bL = split_fields(row[None])
            f, b = int(bf[0]), int(bb[0])
            tree.feat[nd] = f
            tree.bin[nd] = b
            tree.cond[nd] = cuts_v[cuts_o[f] + b]
            tree.defl[nd] = int(bd[0])
            tree.gain[nd] = float(bg[0])
            l, r = tree.add(nd), tree.add(nd)
            tree.left[nd], tree.right[nd] = l, r
            totals[l] = bL[0].double()
            totals[r] = (totals[nd] - bL[0]).double()
            if bounds is not None:
                lo, hi = bounds[nd]
                wl = p.calc_weight_bounded(float(totals[l][0]), float(totals[l][1]), lo, hi)
                wr = p.calc_weight_bounded(float(totals[r][0]), float(totals[r][1]), lo, hi)
                bounds[l], bounds[r] = child_bounds(int(self.mono[f]), lo, hi, wl, wr)
            if state is not None:
                state[l] = state[r] = interaction_child(state[nd], fmask_h[f])
            depth[l] = depth[r] = depth[nd] + 1
            weigh(l), weigh(r)
            leaves += 1
            # ---- partition the node's rows (every other position stays put)
            nnode = len(tree.feat)
            node_feat = torch.full((nnode,), -1, dtype=torch.int32)
            node_bin = torch.zeros(nnode, dtype=torch.int32)
            node_defl = torch.zeros(nnode, dtype=torch.uint8)
            seg_beg = torch.zeros(nnode, dtype=torch.int32)
            seg_end = torch.zeros(nnode, dtype=torch.int32)
            node_feat[nd], node_bin[nd], node_defl[nd] = f, b, tree.defl[nd]
            beg, end = seg.pop(nd)
            seg_beg[nd], seg_end[nd] = beg, end
            ridx, nleft = self._partition(ridx, self._pos_node({nd: (beg, end)}, n), node_feat,
                                          node_bin, node_defl, seg_beg, seg_end)
            nl = int(nleft[nd])
            seg[l], seg[r] = (beg, beg + nl), (beg + nl, end)
            # ---- the children's histograms and best splits, unless neither
            # can be split again (the same decision on every rank)
            if leaves == max_leaves or depth[l] >= depth_cap:
                continue
            small = l if float(totals[l][1]) <= float(totals[r][1]) else r
            hsmall = self._reduce_hist(self._build_hist(ridx, gpair, [seg[small]], [0], 1))[0]
            hbig = hist_nd - hsmall
            hl, hr = (hsmall, hbig) if small == l else (hbig, hsmall)
            found = search([l, r], torch.stack([hl, hr]))
            open_[l], open_[r] = (hl, found[0]), (hr, found[1])
        self._finish(tree, ridx, margin, n, seg, refresh)
        return tree

    def _build_py(self, gpair, margin, refresh=None):
        p = self.p
        n = self.dm.n
        dev = self.device
        tree = RegTree()
        root = tree.add(-1)
        ridx = torch.arange(n, dtype=torch.int32, device=dev)
        tot = gpair_stats(gpair)[0] if n else torch.zeros(2, dtype=torch.float64, device=dev)
        self.bsp.allreduce(tot)
        totals = {root: tot.cpu()}
        # monotone_constraints: every node's weight interval, beside its totals
        # (the root's: max_delta_step on either side of 0, else unbounded)
        top = self.max_delta_step if self.max_delta_step > 0 else float("inf")
        bounds = {root: (-top, top)} if self.mono is not None else None
        # interaction_constraints: every node's set of still possible groups
        state = {root: INTERACTION_ROOT} if self.fmask is not None else None
        fmask_h = self.fmask.tolist() if self.fmask is not None else None
        seg = {root: (0, n)}
        done = {}  # finished leaves -> their final ridx segment
        if self.gpu:
            self._qscale = self._hist_scale(gpair)
        hist_root = self._reduce_hist(self._build_hist(ridx, gpair, [seg[root]], [0], 1))
        H_front = hist_root  # [len(frontier), F, nbin, 2], frontier order
        frontier = [root]
        cuts_v, cuts_o = self._cut_lists
        for depth in range(p.max_depth + 1):
            if not frontier:
                break
            for nd in frontier:
                G, H = float(totals[nd][0]), float(totals[nd][1])
                tree.cover[nd] = H
                tree.base_weight[nd] = (p.calc_weight(G, H) if bounds is None else
                                        p.calc_weight_bounded(G, H, *bounds[nd]))
                tree.leaf[nd] = p.eta * tree.base_weight[nd]
            if depth == p.max_depth:
                break
            S = len(frontier)
            H_all = H_front
            T_all = _h2d(torch.stack([totals[nd] for nd in frontier]), H_all.device)
            B_all = None
            if bounds is not None:
                B_all = torch.tensor([bounds[nd] for nd in frontier], dtype=torch.float64)
            if state is None:
                found = self._find_splits(H_all, T_all, B_all)
            else:
                S_all = torch.tensor([state[nd] for nd in frontier], dtype=torch.int64)
                found = self._find_splits(H_all, T_all, B_all, S_all)
            bg, bf, bb, bd, bL = split_fields(found)
            split_nodes = []
            for k, nd in enumerate(frontier):
                if float(bg[k]) > RT_EPS:
                    f, b = int(bf[k]), int(bb[k])
                    tree.feat[nd] = f
                    tree.bin[nd] = b
                    tree.cond[nd] = cuts_v[cuts_o[f] + b]
                    tree.defl[nd] = int(bd[k])
                    tree.gain[nd] = float(bg[k])
                    l, r = tree.add(nd), tree.add(nd)
                    tree.left[nd], tree.right[nd] = l, r
                    totals[l] = bL[k].double()
                    totals[r] = (totals[nd] - bL[k]).double()
                    if bounds is not None:
                        lo, hi = bounds[nd]
                        wl = p.calc_weight_bounded(float(totals[l][0]), float(totals[l][1]), lo, hi)
                        wr = p.calc_weight_bounded(float(totals[r][0]), float(totals[r][1]), lo, hi)
                        bounds[l], bounds[r] = child_bounds(int(self.mono[f]), lo, hi, wl, wr)
                    if state is not None:
                        state[l] = state[r] = interaction_child(state[nd], fmask_h[f])
                    split_nodes.append(nd)
            if not split_nodes:
                break
            # ---- partition rows of the split nodes
            nnode = len(tree.feat)
            node_feat = torch.full((nnode,), -1, dtype=torch.int32)
            node_bin = torch.zeros(nnode, dtype=torch.int32)
            node_defl = torch.zeros(nnode, dtype=torch.uint8)
            seg_beg = torch.zeros(nnode, dtype=torch.int32)
            seg_end = torch.zeros(nnode, dtype=torch.int32)
            for nd in split_nodes:
                node_feat[nd] = tree.feat[nd]
                node_bin[nd] = tree.bin[nd]
                node_defl[nd] = tree.defl[nd]
            for nd, (b, e) in seg.items():
                seg_beg[nd], seg_end[nd] = b, e
            pos_node = self._pos_node(seg, n)
            ridx, nleft = self._partition(ridx, pos_node, node_feat, node_bin, node_defl,
                                          seg_beg, seg_end)
            nleft = nleft.tolist()
            new_frontier = []
            build_segs, build_slots, small, big = [], [], [], []
            for nd in split_nodes:
                b, e = seg.pop(nd)
                l, r = tree.left[nd], tree.right[nd]
                seg[l] = (b, b + nleft[nd])
                seg[r] = (b + nleft[nd], e)
                new_frontier += [l, r]
                # build the child with the smaller GLOBAL hessian, derive the other
                s_, g_ = (l, r) if float(totals[l][1]) <= float(totals[r][1]) else (r, l)
                small.append(s_)
                big.append(g_)
                build_segs.append(seg[s_])
                build_slots.append(len(build_slots))
            for nd in frontier:
                if nd not in split_nodes and nd in seg:
                    done[nd] = seg.pop(nd)  # finished leaf: its rows are final
            hsmall = self._reduce_hist(self._build_hist(ridx, gpair, build_segs, build_slots,
                                                        len(build_slots)))
            # sibling subtraction for every split node at once; the new
            # frontier is [l, r] per split node, in split order
            fpos = {nd: i for i, nd in enumerate(frontier)}
            par = _h2d(torch.tensor([fpos[nd] for nd in split_nodes], dtype=torch.int64),
                       H_front.device)
            hbig = H_front.index_select(0, par) - hsmall
            small_is_left = _h2d(torch.tensor([small[k] == tree.left[nd]
                                               for k, nd in enumerate(split_nodes)]),
                                 H_front.device)
            sil = small_is_left.view(-1, *([1] * (hsmall.dim() - 1)))
            hl = torch.where(sil, hsmall, hbig)
            hr = torch.where(sil, hbig, hsmall)
            # (a rank that owns no feature of a sharded exchange holds [S, 0, ...])
            H_front = torch.stack([hl, hr], 1).reshape(2 * len(split_nodes), *H_front.shape[1:])
            frontier = new_frontier
        # margins of the training rows from the final leaf segments
        done.update(seg)
        self._finish(tree, ridx, margin, n, done, refresh)
        return tree

    def _reduce_hist(self, h):
        """Rank partials -> global histograms: allreduced (all features), or
        this rank's feature slice (:class:`HistExchange`)."""
        if self.xchg is not None:
            return self.xchg.reduce_scatter(h)
        self._allreduce_hist(h)
        return h

    def _allreduce_hist(self, h):
        P = self.bsp.world
        if P > 1:
            self.ar_sent += 2 * (P - 1) * h.numel() * h.element_size() // P
        self.bsp.allreduce(h)

    def hist_bytes(self):
        """Histogram-exchange bytes this rank has sent to its peers so far
        (all-to-all bytes + candidates, or the ring model of the allreduce)."""
        return self.ar_sent + (self.xchg.sent if self.xchg is not None else 0)

    def _pos_node(self, seg, n):
        """Node id of every ridx position (-1 for rows of finished leaves),
        expanded on the device from the segment list. The host grower tiles
        [0, n) by the same rule (csrc/host/gbdt_level_plan.h gbdt_level_tiles:
        its self-test takes the expected values from this method)."""
        ids, lens = [], []
        cur = 0
        for nd, (b, e) in sorted(seg.items(), key=lambda kv: kv[1][0]):
            if b > cur:
                ids.append(-1), lens.append(b - cur)
            ids.append(nd), lens.append(e - b)
            cur = e
        if cur < n:
            ids.append(-1), lens.append(n - cur)
        dev = self.device
        if self.gpu and ids:
            begs, acc = [], 0
            for ln in lens:
                begs.append(acc)
                acc += ln
            seg = _h2d(torch.tensor([begs, ids], dtype=torch.int32), dev)
            return _native.hip().gbdt_seg_fill(seg[0].contiguous(), seg[1].contiguous(), n)
        return torch.repeat_interleave(torch.tensor(ids, dtype=torch.int32, device=dev),
                                       torch.tensor(lens, dtype=torch.int64, device=dev),
                                       output_size=n)

    def _partition(self, ridx, pos_node, node_feat, node_bin, node_defl, seg_beg, seg_end):
        """Stable partition of the split nodes' rows -> (new ridx, host left
        counts per node); GPU: the node table goes down in one copy."""
        if not self.gpu:
            return partition_ref(ridx, node_feat, node_bin, node_defl, seg_beg, seg_end,
                                 self._local_bin)
        nleft = torch.zeros(node_feat.numel(), dtype=torch.int32, device=self.device)
        pk = _h2d(torch.stack([node_feat, node_bin, node_defl.to(torch.int32), seg_beg,
                               seg_end]), self.device)
        out = self._partition_op(ridx, pos_node, pk[0], pk[1], pk[2].to(torch.uint8), pk[3],
                                 pk[4], nleft)
        return out, nleft.cpu()

    def _prune_mark(self, tree):
        """xgboost prune updater: collapse splits whose loss_chg < gamma, node
        ids unchanged (see :meth:`RegTree.compact`)."""
        if self.p.gamma <= 0:  # accepted splits have gain > RT_EPS > 0: nothing to prune
            return
        changed = True
        while changed:
            changed = False
            for i in range(len(tree.feat)):
                if tree.is_leaf(i):
                    continue
                l, r = tree.left[i], tree.right[i]
                if tree.is_leaf(l) and tree.is_leaf(r) and tree.gain[i] < self.p.gamma:
                    tree.feat[i] = -1
                    tree.leaf[i] = self.p.eta * tree.base_weight[i]
                    changed = True

    def _walks(self, n):
        """True when :meth:`_finish` adds the leaf values by walking each
        row's bins (the dense GPU matrix ``self.B``)."""
        return False

    def _finish(self, tree, ridx, margin, n, leaf_segs, refresh=None):
        """Prune; refresh the leaves when an adaptive objective asks for it
        (``refresh``, :meth:`build`); then add the leaf values to the training
        margins and renumber."""
        self._prune_mark(tree)
        if refresh is not None:
            refresh_leaves(tree, ridx, leaf_segs, n, refresh, self.p.eta, self.bsp)
        self._add_leaves(tree, ridx, margin, n, leaf_segs)

    def _add_leaves(self, tree, ridx, margin, n, leaf_segs):
        """Add the (pruned) tree's leaf values to the training margins from the
        final (pre-prune) leaf segments, then renumber: a pruned-away
        subtree's rows take the value of its nearest ancestor that is a leaf
        after pruning, looked up BEFORE the BFS renumbering changes ids."""
        if self._walks(n):
            # walk the pruned tree per row on its bins (a pruned-away
            # subtree's rows stop at its collapsed root, whose leaf value
            # _prune_mark set): coalesced, instead of a scatter by ridx
            # the six node arrays in ONE upload (six small copies cost ~20 us
            # of queue time each between the level loop and the walk)
            nn = len(tree.feat)
            h = np.empty(6 * nn, dtype=np.int32)
            for q, v in enumerate((tree.feat, tree.bin, tree.left, tree.right, tree.defl)):
                h[q * nn:(q + 1) * nn] = v
            h[5 * nn:].view(np.float32)[:] = tree.leaf
            d = torch.from_numpy(h).to(self.device, non_blocking=True)
            _native.hip().gbdt_leaf_walk(
                self.B, d[:nn], d[nn:2 * nn], d[4 * nn:5 * nn].to(torch.uint8), d[2 * nn:3 * nn],
                d[3 * nn:4 * nn], d[5 * nn:].view(torch.float32), margin, lds=LEAF_WALK_LDS)
        elif n and self.gpu:
            val = torch.zeros(len(tree.feat), dtype=torch.float32)
            for nd in leaf_segs:
                a, top = nd, nd
                while tree.parent[a] >= 0:
                    a = tree.parent[a]
                    if tree.is_leaf(a):
                        top = a
                val[nd] = tree.leaf[top]
            pos = self._pos_node(leaf_segs, n)
            _native.hip().gbdt_leaf_add(ridx, pos, val.to(self.device), margin)
        tree.compact()
        if n and not self.gpu:
            self.dm.predict_tree(tree, margin)


class TreeBuilder(_LevelGrower):
    """Depth-wise histogram tree growth on one DMatrix split per rank."""

    def __init__(self, param, bsp, dm, cuts, B):
        super().__init__(param, bsp, dm, cuts)
        self.B = B.contiguous()
        self.nbin = max(1, cuts.nbin_max)
        # features per LDS histogram block: int64 (g, h) per bin in <= 160 KB
        fg = max(1, (160 * 1024) // (self.nbin * 16))
        fg = min(fg, 64)
        if fg >= 4:
            fg -= fg % 4  # 4-aligned groups let the kernel load 4 bins per dword
        self.fgroups = [(j, min(fg, self.F - j)) for j in range(0, self.F, fg)]
        self.max_fcnt = max(c for _, c in self.fgroups) if self.fgroups else 1
        o = self._cut_lists[1]
        nb = torch.tensor([b - a for a, b in zip(o, o[1:])])
        self.bin_mask = torch.arange(self.nbin)[None, :] < nb[:, None]  # [F, nbin]
        self.valid_mask = self.bin_mask.clone()
        self._valid_dev = None
        self._Bc = None  # feature-major copy of B for the partition gathers
        if HistExchange.mode(bsp, True):
            self.xchg = HistExchange(bsp, self.F)

    def sample_features(self, gen):
        """colsample_bytree: restrict this tree's candidate features."""
        self.valid_mask = self.bin_mask.clone()
        m = self._draw_features(gen)
        if m is not None:
            self.valid_mask &= m[:, None]

    def _valid(self):
        """This tree's candidate mask [F, nbin] on the device, uploaded once."""
        if self._valid_dev is None or self._valid_dev[0] is not self.valid_mask:
            self._valid_dev = (self.valid_mask, self.valid_mask.to(self.device).contiguous())
        return self._valid_dev[1]

    def _feature_major(self):
        if self._Bc is None:
            self._Bc = self.B.t().contiguous()
        return self._Bc

    def _walks(self, n):
        """(then the grower may skip the last level's partition and histograms)"""
        return bool(n and self.gpu and self.B.dim() == 2 and self.B.shape[0] == n
                    and self.B.dtype == torch.uint8)

    def _local_bin(self, f, rows):
        return self.B[rows, f].long()

    def _partition_op(self, ridx, pos_node, *table_and_nleft):
        return _native.hip().gbdt_partition(self.B, ridx, pos_node, *table_and_nleft,
                                            self._feature_major())

    # ----------------------------------------------------------- histograms
    def _build_hist(self, ridx, gpair, segs, slots, nslot):
        """segs: list of (beg, end) local row ranges; slots: output slot of each."""
        hist = torch.zeros(nslot, self.F, self.nbin, 2, dtype=torch.float64, device=self.device)
        if self.gpu:
            # ~512 row chunks per call (two rounds of the 256 resident
            # 1024-thread blocks); partials are summed per (slot, group)
            total = sum(max(0, e - b) for b, e in segs)
            chunk = max(8192, -(-total // 512))
            G = len(self.fgroups)
            tasks, red = [], []
            for (b, e), s in zip(segs, slots):
                if e <= b:
                    continue
                t0, nch = len(tasks), 0
                for r in range(b, e, chunk):
                    nch += 1
                    for fb, fc in self.fgroups:
                        tasks.append((s, fb, fc, r, min(e, r + chunk)))
                for g, (fb, fc) in enumerate(self.fgroups):
                    red.append((s, fb, fc, t0 + g, nch, G))
            if tasks:
                both = torch.tensor(tasks, dtype=torch.int32).reshape(-1)
                both = torch.cat([both, torch.tensor(red, dtype=torch.int32).reshape(-1)])
                both = _h2d(both, self.device)
                t = both[:5 * len(tasks)].view(-1, 5)
                rd = both[5 * len(tasks):].view(-1, 6)
                _native.hip().gbdt_hist(B=self.B, nbin=self.nbin, ridx=ridx, gpair=gpair,
                                        qscale=self._qscale, tasks=t, red=rd,
                                        max_fcnt=self.max_fcnt, hist=hist)
        else:
            for (b, e), s in zip(segs, slots):
                if e <= b:
                    continue
                rows = ridx[b:e].long()
                bins = self.B[rows].long()  # [r, F]
                gh = gpair[rows].double()  # [r, 2]
                ok = bins != MISSING_BIN
                flat = (torch.arange(self.F)[None, :] * self.nbin + bins.clamp(max=self.nbin - 1))
                for c in range(2):
                    val = gh[:, c][:, None].expand_as(flat)[ok]
                    hist[s].view(-1, 2)[:, c].index_add_(0, flat[ok], val)
        return hist

    # -------------------------------------------------------- split search
    def _find_splits(self, hist, totals, bounds=None, state=None):
        """hist [S, F, nbin, 2] (global); totals [S, 2] -> the host split
        table. With a feature-sharded exchange, hist holds this rank's feature
        slice only: the local best goes through :meth:`HistExchange.pick`.
        bounds [S, 2]: the slots' weight intervals under monotone_constraints,
        state [S]: their group sets under interaction_constraints (the same
        on every rank: each derives them from the picked table)."""
        x = self.xchg
        mono = self._mono() if bounds is not None else None
        fmask = self._fmask() if state is not None else None
        if x is None:
            return find_splits(self.p, hist, totals, self._valid(), mono, bounds, fmask, state)
        if x.hi > x.lo:
            cand = find_splits(self.p, hist, totals, self._valid()[x.lo:x.hi],
                               mono[x.lo:x.hi] if mono is not None else None, bounds,
                               fmask[x.lo:x.hi] if fmask is not None else None, state)
            cand[:, 1] += x.lo  # global feature ids
        else:  # (more ranks than features: this rank owns none)
            cand = torch.zeros(hist.shape[0], 6, dtype=torch.float64)
            cand[:, 0] = -float("inf")
        return x.pick(cand.to(self.device)).cpu()

    def _build_native(self, gpair, margin, refresh=None):
        """The level loop in C++ (``_hip.gbdt_grow``): one host sync per
        level, device-derived child segments, fused sibling subtraction.
        Same tree as :meth:`_build_py` (which stays the CPU path and the
        reference)."""
        p = self.p
        n = self.dm.n
        tot = gpair_stats(gpair)[0]
        self.bsp.allreduce(tot)
        self._qscale = self._hist_scale(gpair)
        ar = self._allreduce_hist if self.bsp.world > 1 else None
        # the level loop on the device (one host read per tree) unless the
        # per-level host grower is asked for (HOST_GROWER, or trees deeper
        # than the device loop's heap numbering)
        host = HOST_GROWER or p.max_depth > 10
        kw = dict(B=self.B, Bc=self._feature_major(), valid=self._valid(), ridx0=self._iota(n),
                  gpair=gpair, qscale=self._qscale, nbin=self.nbin, fgroups=self.fgroups,
                  max_fcnt=self.max_fcnt, cut_vals=self._cut_lists[0],
                  cut_off=self._cut_lists[1], eta=float(p.eta), alpha=float(p.alpha),
                  reg_lambda=float(p.reg_lambda), min_child_weight=float(p.min_child_weight),
                  max_depth=int(p.max_depth), rt_eps=RT_EPS, allreduce=ar, mono=self._mono())
        if self.fmask is not None:
            kw["fmask"] = self._fmask()
        if self.max_delta_step > 0:  # the root's weight interval (else unbounded)
            kw["max_delta_step"] = self.max_delta_step
        # deferred: the tree stays a device node table, the margins are
        # walked from it on the device, and its host lists are built one tree
        # later (no GPU idle between trees); needs the row walk and no
        # pruning (gamma <= 0: every accepted split has gain > RT_EPS)
        # A leaf refresh needs every final leaf's rows as a ridx segment and
        # the tree's lists at once: the last level is partitioned too (walk
        # off) and nothing is deferred.
        defer = (not host and self._walks(n) and p.gamma <= 0 and DEFER_TREES
                 and refresh is None)
        # both return (the tree as ``gbdt_tree_from_nodes`` lists it, the final
        # ridx); deferred: (the device node table, ridx)
        if host:  # (the per-level host grower allreduces whole histograms)
            grown, ridx = _native.hip().gbdt_grow(root_tot=tot.cpu().tolist(), **kw)
        else:  # root totals as a device tensor: no host wait
            x = self.xchg
            grown, ridx = _native.hip().gbdt_grow_dev(
                root_tot=tot.contiguous(), **kw,
                reduce_scatter=x.reduce_scatter if x is not None else None,
                pick=x.pick if x is not None else None, f_lo=x.lo if x is not None else 0,
                walk=self._walks(n) and refresh is None, defer=defer)
        if defer:
            _native.hip().gbdt_walk_heap(self.B, grown, margin, lds=LEAF_WALK_LDS)
            tree = _DeviceTree(grown, self._cut_lists)
            prev, self._pending = self._pending, tree
            if prev is not None:
                prev.materialize()  # (its copy finished during this tree's levels)
            return tree
        tree = RegTree.from_lists(grown)
        self._finish(tree, ridx, margin, n, {nd: (b, e) for nd, b, e in grown[11]}, refresh)
        return tree

    def _leaf_dev(self):
        slots = 2 * self.limits[0] - 1
        return (LEAF_LOOP_DEV and self.bsp.world == 1
                and slots * self.F * self.nbin * 16 <= LEAF_POOL_BYTES)

    def _build_leaf_native(self, gpair, margin, refresh=None):
        """The leaf loop on the device (``_hip.gbdt_grow_leaf``): every step
        of the tree enqueued without a host wait, the node table read once.
        Same tree as :meth:`_build_leafwise`. Without pruning and without a
        leaf refresh the margins are walked from the device table before
        that read; else :meth:`_finish` takes the lists and the leaves' row
        segments. (Trees are not deferred: the host lists are built at once.)"""
        p = self.p
        n = self.dm.n
        tot = gpair_stats(gpair)[0]
        self.bsp.allreduce(tot)
        self._qscale = self._hist_scale(gpair)
        walk = self._walks(n) and p.gamma <= 0 and refresh is None
        extra = {}
        if self.fmask is not None:
            extra["fmask"] = self._fmask()
        if self.max_delta_step > 0:
            extra["max_delta_step"] = self.max_delta_step
        grown, ridx = _native.hip().gbdt_grow_leaf(
            B=self.B, Bc=self._feature_major(), ridx0=self._iota(n), gpair=gpair,
            qscale=self._qscale, valid=self._valid(), nbin=self.nbin, fgroups=self.fgroups,
            max_fcnt=self.max_fcnt, root_tot=tot.contiguous(), cut_vals=self._cut_lists[0],
            cut_off=self._cut_lists[1], eta=float(p.eta), alpha=float(p.alpha),
            reg_lambda=float(p.reg_lambda), min_child_weight=float(p.min_child_weight),
            max_leaves=int(self.limits[0]), depth_cap=int(self.limits[1]), rt_eps=RT_EPS,
            mono=self._mono(), walk_margin=margin if walk else None, lds=LEAF_WALK_LDS, **extra)
        tree = RegTree.from_lists(grown)
        if walk:  # (gamma <= 0: nothing to prune; the table is breadth-first already)
            return tree.compact()
        self._finish(tree, ridx, margin, n, {nd: (b, e) for nd, b, e in grown[11]}, refresh)
        return tree

    def _iota(self, n):
        """0..n-1 as int32 on the device (the grower only reads it)."""
        t = self._iota_t
        if t is None or t.numel() != n:
            t = self._iota_t = torch.arange(n, dtype=torch.int32, device=self.device)
        return t


class CSRTreeBuilder(_LevelGrower):
    """Tree growth on a :class:`CSRMatrix`: the same depth-wise level loop
    (smaller-child histograms, sibling subtraction, both default directions)
    over compact [slots][total bins][2] histograms -- no F x max_bin padding
    and no dense n x F bin matrix."""

    def __init__(self, param, bsp, dm, cuts, gbin):
        # (the compact global-bin histograms are allreduced: HistExchange is
        # dense-only, xchg stays None)
        super().__init__(param, bsp, dm, cuts)
        self.gbin = gbin
        self.tb = int(cuts.offsets[-1]) if cuts.offsets.numel() else 0
        self.cut_off = cuts.offsets.to(self.device).contiguous()
        self.fvalid = None
        self._rows = None

    def sample_features(self, gen):
        m = self._draw_features(gen)
        self.fvalid = m.to(torch.uint8).to(self.device) if m is not None else None

    def _entry_rows(self):
        if self._rows is None:
            self._rows = self.dm.entry_rows()
        return self._rows

    def _build_hist(self, ridx, gpair, segs, slots, nslot):
        if self.gpu:
            chunk, tasks = 16384, []
            for (b, e), sl in zip(segs, slots):
                for r in range(b, e, chunk):
                    tasks += [sl, r, min(e, r + chunk)]
            t = _h2d(torch.tensor(tasks or [0, 0, 0], dtype=torch.int32), self.device)
            return _native.hip().gbdt_hist_csr(self.dm.row_off, self.gbin, ridx, gpair,
                                               self._qscale, t, chunk if tasks else 0, self.tb,
                                               nslot)
        hist = torch.zeros(nslot, self.tb, 2, dtype=torch.float64)
        rows = self._entry_rows()
        for (b, e), sl in zip(segs, slots):
            if e <= b:
                continue
            inseg = torch.zeros(self.dm.n, dtype=torch.bool)
            inseg[ridx[b:e].long()] = True
            m = inseg[rows] & (self.gbin >= 0)
            gb = self.gbin[m].long()
            gh = gpair[rows[m]].double()
            for c in range(2):
                hist[sl, :, c].index_add_(0, gb, gh[:, c])
        return hist

    def _find_splits(self, hist, totals, bounds=None, state=None):
        p = self.p
        mono = self._mono() if bounds is not None else None
        fmask = self._fmask() if state is not None else None
        if self.gpu:
            if bounds is not None:
                bounds = bounds.to(self.device).double().contiguous()
            inter = {}
            if state is not None:
                inter = dict(fmask=fmask, state=state.to(self.device).contiguous())
            return _native.hip().gbdt_split_csr(hist.contiguous(), totals.double().contiguous(),
                                                self.cut_off, self.fvalid, float(p.alpha),
                                                float(p.reg_lambda), float(p.min_child_weight),
                                                mono=mono, bounds=bounds, **inter).cpu()
        return find_splits_csr_ref(p, hist, totals, self._cut_lists[1], self.fvalid, mono, bounds,
                                   fmask, state)

    def _local_bin(self, f, rows):
        lb = torch.full((self.dm.n,), MISSING_BIN, dtype=torch.long)
        m = (self.dm.fid.long() == f) & (self.gbin >= 0)
        lb[self._entry_rows()[m]] = self.gbin[m].long() - self._cut_lists[1][f]
        return lb[rows]

    def _partition_op(self, ridx, pos_node, *table_and_nleft):
        return _native.hip().gbdt_partition_csr(self.dm.row_off, self.dm.fid, self.gbin,
                                                self.cut_off, ridx, pos_node, *table_and_nleft)


def make_builder(param, bsp, dm, cuts, B):
    return (CSRTreeBuilder if dm.sparse else TreeBuilder)(param, bsp, dm, cuts, B)


def boost_round(obj, builder, dm, margin, gen=None, fgen=None):
    """One boosting round on the training margins (updated in place): one
    gradient call, then one tree per class on its own slice of the pairs and
    margins (a single tree for a single-output objective). ``subsample``
    (rows, from ``gen``) and ``colsample_bytree`` (features, from ``fgen``)
    are drawn per tree. A rank objective takes the rows' query groups from
    ``dm.group``. Returns the new trees in class order."""
    return grow_round(obj, builder, dm, margin, margin, gen, fgen)


def grow_round(obj, builder, dm, at, into, gen=None, fgen=None):
    """:func:`boost_round` with the gradients taken at the margins ``at`` and
    the new trees' outputs added to ``into`` (the same tensor for gbtree; the
    dart round takes them at the margins without the dropped trees and has
    the outputs added to a scratch)."""
    p = builder.p
    K = obj.n_group
    obj.check_combination(p)
    # (a rank objective's query groups: the matrix's, with their cached task plan)
    # (survival:cox takes the matrix's plan, survival:aft its bounds)
    gp = obj.gpair(at, dm.label, dm.weight, dm.rank_groups(), data=dm)
    new = []
    for k in range(K):
        gk, mk = (class_gpair(gp, k), into[k]) if K > 1 else (gp, into)
        keep = None
        if p.subsample < 1.0:
            keep = (torch.rand(dm.n, generator=gen) < p.subsample).to(dm.device)
            gk = gk * keep[:, None].float()
        if p.colsample_bytree < 1.0:  # (else the builder's mask stays all-features)
            builder.sample_features(fgen)
        if not obj.adaptive:
            new.append(builder.build(gk, mk))
            continue
        # the leaves become quantiles of the residuals at the margins the
        # gradients were taken at (dart: those without the dropped rounds)
        rf = dict(label=dm.label, at=at[k] if K > 1 else at, weight=dm.weight, keep=keep,
                  alpha=obj.alphas[k])
        new.append(builder.build(gk, mk, rf))
    return new


# booster=dart: the draw, the weight update, the tree table and the round
# (imported last: the module reads this one's switches and growers when called)
from .gbdt_dart import (DartForest, DartTrainer, dart_add, dart_draw, dart_scales,  # noqa: E402,F401
                        dart_seed, dart_update, forest_add)

