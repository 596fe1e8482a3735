"""The adaptive objectives' leaf refresh (reg:absoluteerror,
reg:quantileerror; docs/bsp_apps.md "Absolute and quantile error"): after a
tree is grown and pruned, every leaf becomes eta x the exact weighted
alpha-quantile of the residuals y - a of the training rows that reach it, over
all ranks.

    q = min { v in {r_i} : sum of u_i over r_i <= v  >=  ceil(alpha W) }

with u_i = w_i keep_i rounded once to a multiple of 2^-e (e: the largest
exponent that keeps the global sum of u 2^e within 2^61) and W the leaf's sum
of u. The sums are integers, so the result does not depend on the rank count,
the row order or the chunking. On the GPU a radix select
(csrc/hip/gbdt_quantile.hip; the passes' int64 histograms are allreduced); the
sort in :func:`leaf_quantiles_ref` is its reference and the one-rank CPU path.
"""
import numpy as np
import torch

from .. import _native

QSEL_CHUNK = 1 << 14  # key positions per histogram task
MAX_ALPHAS = 64


def parse_quantile_alpha(val):
    """``0.5`` | ``[0.1,0.5,0.9]`` | ``0.1, 0.5`` (brackets optional, spaces
    and outer quotes allowed) -> the list, in the order given."""
    def bad(why):
        raise SystemExit("quantile_alpha=%s: %s" % (val, why))

    s = str(val).strip()
    if len(s) >= 2 and s[0] == s[-1] and s[0] in "\"'":
        s = s[1:-1].strip()
    if (s.startswith("[") and s.endswith("]")) or (s.startswith("(") and s.endswith(")")):
        s = s[1:-1]
    out = []
    for tok in s.split(","):
        tok = tok.strip()
        if not tok:
            bad("an empty list" if not s.strip() else "an empty entry")
        try:
            a = float(tok)
        except ValueError:
            bad("every entry is a number, got %r" % tok)
        if not 0.0 < a < 1.0:
            bad("every entry lies strictly inside (0, 1), got %r" % tok)
        out.append(a)
    if len(out) > MAX_ALPHAS:
        bad("%d entries, at most %d are supported" % (len(out), MAX_ALPHAS))
    return out


# ------------------------------------------------------------ fixed point
def weight_scale(weight, keep, bsp):
    """2^e as a float64 tensor [1] on the weights' device: the largest power
    of two (e in [-60, 100]) with (global sum of w keep) 2^e <= 2^61 -- the
    rule of the histograms' scales; no host read."""
    w = weight.double().clamp(min=0)
    if keep is not None:
        w = w * keep.to(w.dtype)
    tot = w.sum().reshape(1)
    bsp.allreduce(tot)
    e = torch.floor(torch.log2(2.0 ** 61 / tot.clamp(min=1e-30))).clamp(-60, 100)
    return torch.exp2(e)


def round_weights(weight, keep, scale, n=None, device=None):
    """u [n] int64: w keep scale rounded to nearest (ties to even); a
    negative or NaN weight counts 0. weight None: 1 per row (scale None)."""
    if weight is None:
        u = torch.ones(n, dtype=torch.int64, device=device)
    else:
        w = torch.where(weight > 0, weight, torch.zeros_like(weight)).double()
        u = torch.round(w * (scale if scale is not None else 1.0)).long()
    if keep is not None:
        u = u * keep.to(torch.int64)
    return u


def threshold(alpha, W):
    """ceil(alpha W) in fp64, kept within [1, W] (W: int64 tensor, > 0)."""
    t = torch.ceil(alpha * W.double()).long()
    return torch.maximum(torch.minimum(t, W), torch.ones_like(W))


# -------------------------------------------------------------- reference
def leaf_quantiles_ref(r, u, segs, alpha):
    """r fp32 [m] residuals and u int64 [m] weights in segment order, segs
    [(begin, end)] per leaf -> (q fp32 [L], empty bool [L]): per segment a
    sort, the cumulative sum of u, the first position reaching the threshold.
    An empty leaf (W = 0) has q = 0."""
    L = len(segs)
    q = torch.zeros(L, dtype=torch.float32)
    empty = torch.ones(L, dtype=torch.bool)
    r, u = r.cpu(), u.cpu()
    for l, (b, e) in enumerate(segs):
        if e <= b:
            continue
        uu = u[b:e]
        W = uu.sum()
        if int(W) <= 0:
            continue
        rs, order = torch.sort(r[b:e])
        cum = uu[order].cumsum(0)
        pos = int((cum < threshold(alpha, W)).sum())
        q[l] = rs[pos] + 0.0  # (-0.0 -> +0.0)
        empty[l] = False
    return q, empty


# ------------------------------------------- the radix select in plain torch
def _keys(r):
    """The order-preserving 32-bit keys of fp32 r, as int64."""
    b = r.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    return torch.where((b & 0x80000000) != 0, ~b & 0xFFFFFFFF, b | 0x80000000)


def _unkeys(k):
    b = torch.where((k & 0x80000000) != 0, k & 0x7FFFFFFF, ~k & 0xFFFFFFFF)
    b = torch.where(b >= 0x80000000, b - (1 << 32), b)
    return b.to(torch.int32).view(torch.float32)


def select_torch(r, u, segs, alpha, allreduce=None):
    """:func:`leaf_quantiles_ref` by the kernels' algorithm (four passes of
    256-bin int64 histograms, ``allreduce``d between count and pick): the CPU
    path of several ranks."""
    L, dev = len(segs), r.device
    leaf = torch.full((r.numel(),), -1, dtype=torch.int64, device=dev)
    for l, (b, e) in enumerate(segs):
        leaf[b:e] = l
    key = _keys(r)
    prefix = torch.zeros(L, dtype=torch.int64, device=dev)
    rem = torch.zeros(L, dtype=torch.int64, device=dev)
    for p in range(4):
        shift = 24 - 8 * p
        ok = leaf >= 0
        if p:
            ok = ok & ((key >> (shift + 8)) == (prefix[leaf.clamp(min=0)] >> (shift + 8)))
        hist = torch.zeros(L * 256, dtype=torch.int64, device=dev)
        hist.index_add_(0, (leaf * 256 + ((key >> shift) & 255))[ok], u[ok])
        hist = hist.view(L, 256)
        if allreduce is not None:
            allreduce(hist)
        if p == 0:
            W = hist.sum(1)
            rem = torch.where(W > 0, threshold(alpha, W.clamp(min=1)), torch.zeros_like(W))
        cum = hist.cumsum(1)
        d = (cum < rem[:, None]).sum(1).clamp(max=255)
        below = torch.where(d > 0, cum.gather(1, (d - 1).clamp(min=0)[:, None])[:, 0],
                            torch.zeros_like(rem))
        on = rem > 0
        prefix = torch.where(on, prefix | (d << shift), prefix)
        rem = torch.where(on, rem - below, rem)
    empty = rem <= 0
    q = torch.where(empty, torch.zeros(L, device=dev), _unkeys(prefix))
    return q.cpu(), empty.cpu()


# ------------------------------------------------------------ the refresh
def leaf_quantiles(ridx, segs, label, at, weight, keep, alpha, bsp, chunk=QSEL_CHUNK):
    """(q fp32 [L], empty bool [L]) on the host: the global weighted
    alpha-quantile of label - at over the rows ridx[b:e] of every segment
    (b, e) of ``segs`` (this rank's rows of the leaves; every rank lists the
    same leaves). keep: the rows of this tree's subsample draw (bool), or
    None. Collective when bsp.world > 1."""
    L = len(segs)
    scale = weight_scale(weight, keep, bsp) if weight is not None else None
    if ridx.is_cuda:
        hip = _native.hip()
        key, u = hip.gbdt_qsel_key(
            ridx=ridx.contiguous(), label=label.contiguous(), at=at.contiguous(),
            weight=weight.contiguous() if weight is not None else None,
            keep=keep.contiguous() if keep is not None else None, scale=scale)
        seg_beg, seg_end = [b for b, _ in segs], [e for _, e in segs]
        state = torch.zeros(L, 2, dtype=torch.int64, device=ridx.device)
        for p in range(4):
            hist = hip.gbdt_qsel_hist(key=key, u=u, seg_beg=seg_beg, seg_end=seg_end,
                                      chunk=int(chunk), state=state, radix_pass=p)
            if bsp.world > 1:
                bsp.allreduce(hist)
            hip.gbdt_qsel_pick(hist=hist, state=state, alpha=float(alpha), radix_pass=p)
        out = hip.gbdt_qsel_value(state=state).cpu()
        return out[0], out[1] != 0
    rows = ridx.long()
    r = (label.float() - at.float())[rows]
    u = round_weights(weight[rows] if weight is not None else None,
                      keep[rows] if keep is not None else None, scale, rows.numel(), ridx.device)
    if bsp.world > 1:
        return select_torch(r, u, segs, alpha, bsp.allreduce)
    return leaf_quantiles_ref(r, u, segs, alpha)


def refresh_leaves(tree, ridx, leaf_segs, n, rf, eta, bsp):
    """The refresh of a pruned tree whose node ids are still the grower's:
    ``leaf_segs`` {node: (begin, end)} are the final ridx segments of the
    leaves before pruning. A pruned-away subtree's segments are adjacent (the
    partition is stable inside the parent's segment) and merge into the
    segment of the ancestor that is a leaf after pruning. Every such leaf of
    weight W > 0 takes float32(eta q); base_weight, gain and cover stay.
    rf: dict(label, at, weight, keep, alpha) from :func:`grow_round`."""
    merged = {}
    for nd, (b, e) in leaf_segs.items():
        a, top = nd, nd
        while tree.parent[a] >= 0:
            a = tree.parent[a]
            if tree.is_leaf(a):
                top = a
        lo, hi, cnt = merged.get(top, (b, e, 0))
        merged[top] = (min(lo, b), max(hi, e), cnt + e - b)
    leaves = sorted(i for i in range(len(tree.feat)) if tree.is_leaf(i) and _reachable(tree, i))
    if sorted(merged) != leaves or any(hi - lo != cnt for lo, hi, cnt in merged.values()) or \
            sum(cnt for _, _, cnt in merged.values()) != n:
        raise RuntimeError("leaf refresh: the leaf segments do not tile the training rows")
    segs = [merged[i][:2] for i in leaves]
    q, empty = leaf_quantiles(ridx, segs, rf["label"], rf["at"], rf["weight"], rf["keep"],
                              rf["alpha"], bsp)
    for i, v, none in zip(leaves, q.tolist(), empty.tolist()):
        if not none:
            tree.leaf[i] = float(np.float32(float(eta) * v))


def _reachable(tree, i):
    """True unless an ancestor of node i is a leaf (pruned away above it)."""
    while tree.parent[i] >= 0:
        i = tree.parent[i]
        if tree.is_leaf(i):
            return False
    return True


def pinball_sums(alphas, margin, label, weight):
    """fp64 [2] = {sum_i w_i sum_k pinball_{alpha_k}(y_i, m_ki), sum_i w_i} of
    this rank's rows, margin [K, n] (or [n]): on the GPU one evaluation
    kernel, else (and as its reference) torch on ``margin.double()``."""
    K = len(alphas)
    if (margin.is_cuda and margin.dtype == torch.float32 and label.dtype == torch.float32
            and (weight is None or weight.dtype == torch.float32)):
        a = torch.tensor(alphas, dtype=torch.float64).to(margin.device)
        return _native.hip().gbdt_quantile_eval(
            margin=margin.contiguous(), label=label.contiguous(),
            weight=weight.contiguous() if weight is not None else None, alphas=a)
    out = torch.zeros(2, dtype=torch.float64, device=margin.device)
    if label.numel() == 0:
        return out
    m, y = margin.double().reshape(K, -1), label.double()
    w = weight.double() if weight is not None else torch.ones_like(y)
    a = torch.tensor(alphas, dtype=torch.float64, device=margin.device)[:, None]
    d = y[None, :] - m
    out[0] = (w * torch.where(d >= 0, a * d, (a - 1.0) * d).sum(0)).sum()
    out[1] = w.sum()
    return out

