"""GBDT parameters, objectives (single-output, multi-class softmax and
learning to rank over query groups, with their gradient pairs) and globally
reduced metrics; models/gbdt.py grows the trees."""
import math
import re

import torch

from .. import _native


# ------------------------------------------------------------------ params
class GBDTParam:
    ALIASES = {"learning_rate": "eta", "min_split_loss": "gamma", "reg_lambda": "lambda",
               "reg_alpha": "alpha", "n_estimators": "num_round"}

    def __init__(self):
        self.booster = "gbtree"
        self.objective = "reg:linear"
        self.eta = 0.3
        self.gamma = 0.0
        self.min_child_weight = 1.0
        self.max_depth = 6
        self.reg_lambda = 1.0
        self.alpha = 0.0
        self.base_score = 0.5
        self.max_bin = 256
        self.subsample = 1.0
        self.colsample_bytree = 1.0
        self.seed = 0
        self.num_class = 0  # multi:softmax / multi:softprob: classes (trees per round)
        self.eval_metric = []
        self.silent = 0
        self.monotone = []  # monotone_constraints: -1 | 0 | 1 per feature id (rest: 0)
        self.interaction = []  # interaction_constraints: groups of feature ids ([]: off)

    def set(self, name, val):
        name = self.ALIASES.get(name, name)
        if name == "lambda":
            self.reg_lambda = float(val)
        elif name == "monotone_constraints":
            self.monotone = parse_monotone(val)
        elif name == "interaction_constraints":
            self.interaction = parse_interaction(val)
        elif name in ("eta", "gamma", "min_child_weight", "alpha", "base_score", "subsample",
                      "colsample_bytree"):
            setattr(self, name, float(val))
        elif name in ("max_depth", "max_bin", "seed", "silent", "num_class"):
            setattr(self, name, int(val))
        elif name in ("objective", "booster"):
            setattr(self, name, val)
        elif name == "eval_metric":
            self.eval_metric.append(val)
        else:
            return False
        return True

    def calc_gain(self, G, H):
        g = _threshold_l1(G, self.alpha)
        out = g * g / (H + self.reg_lambda)
        return torch.where(H < self.min_child_weight, torch.zeros_like(out), out)

    def calc_weight(self, G, H):
        if H < self.min_child_weight:
            return 0.0
        g = G
        if self.alpha > 0:
            g = G - self.alpha if G > self.alpha else (G + self.alpha if G < -self.alpha else 0.0)
        return -g / (H + self.reg_lambda)

    # ---- monotone_constraints: a node's weight is clamped to its interval
    # (lo, hi); a side whose weight is clamped scores -(2 T(G) w + (H + lambda)
    # w w), an unclamped one keeps the closed form above, evaluated as above
    # (so infinite bounds change nothing). Every path -- these, the host
    # grower, the kernels -- evaluates the same operations in the same order.
    def monotone_vector(self, F):
        """The constraints of F features, zero-padded -> int8 [F], or None
        when monotone_constraints is not set."""
        if not self.monotone:
            return None
        if len(self.monotone) > F:
            raise SystemExit("monotone_constraints has %d entries, the data has %d features"
                             % (len(self.monotone), F))
        return torch.tensor(self.monotone + [0] * (F - len(self.monotone)), dtype=torch.int8)

    def calc_weight_bounded(self, G, H, lo, hi):
        """:meth:`calc_weight` clamped to [lo, hi] (floats)."""
        w = self.calc_weight(G, H)
        return lo if w < lo else (hi if w > hi else w)

    def side_gain_bounded(self, G, H, lo, hi):
        """(gain, weight) of one side under the bounds, in floats."""
        w0 = self.calc_weight(G, H)
        w = lo if w0 < lo else (hi if w0 > hi else w0)
        g = G
        if self.alpha > 0:
            g = G - self.alpha if G > self.alpha else (G + self.alpha if G < -self.alpha else 0.0)
        d = H + self.reg_lambda
        if w == w0:
            return (0.0 if H < self.min_child_weight else g * g / d), w
        return -(2.0 * g * w + d * w * w), w

    def calc_gain_bounded(self, G, H, lo, hi):
        """:meth:`calc_gain` under the bounds, on tensors -> (gain, weight)."""
        g = _threshold_l1(G, self.alpha)
        d = H + self.reg_lambda
        w0 = torch.where(H < self.min_child_weight, torch.zeros_like(d), -g / d)
        w = torch.where(w0 < lo, lo, torch.where(w0 > hi, hi, w0))
        return torch.where(w == w0, self.calc_gain(G, H), -(2.0 * g * w + d * w * w)), w

    # ---- interaction_constraints: feature f carries the bit set m[f] of the
    # groups that contain it (bit 63 alone when none does), a node the bit set
    # of the groups that contain every feature split on above it.
    def interaction_vector(self, F):
        """The group bit sets of F features -> int64 [F] (bit i: group i
        contains the feature; a feature in no group holds INTERACTION_FREE,
        bit 63, alone), or None when interaction_constraints is not set."""
        if not self.interaction:
            return None
        m = [0] * F
        for i, grp in enumerate(self.interaction):
            for f in grp:
                if f >= F:
                    raise SystemExit("interaction_constraints names feature %d, the data has %d "
                                     "features" % (f, F))
                m[f] |= 1 << i
        return torch.tensor([v if v else INTERACTION_FREE for v in m], dtype=torch.int64)


# interaction_constraints on one 64-bit word per feature and per node (int64
# bit patterns): bits 0..62 are the groups, bit 63 marks a feature in no group.
# A root holds INTERACTION_ROOT and admits every feature; a node admits feature
# f iff state & m[f] != 0; its children hold interaction_child(state, m[f]),
# which drops bit 63: below a split on an ungrouped feature nothing is admitted.
INTERACTION_MAX_GROUPS = 63
INTERACTION_FREE = -(1 << 63)
INTERACTION_ROOT = -1


def interaction_child(state, m):
    """The children's state of a node of state ``state`` split on a feature
    of mask ``m`` (Python ints as int64 bit patterns)."""
    return state & m & ~INTERACTION_FREE


def parse_interaction(val):
    """``[[0,1,2],[2,3]]`` (spaces and outer quotes allowed) -> [[0, 1, 2],
    [2, 3]]: sorted ids without duplicates per group; ``[]`` -> [] (off)."""
    def bad(why):
        raise SystemExit("interaction_constraints=%s: %s" % (val, why))

    s = str(val).strip()
    if len(s) >= 2 and s[0] == s[-1] and s[0] in "\"'":
        s = s[1:-1].strip()
    s = re.sub(r"\s*([\[\],])\s*", r"\1", s)
    if len(s) < 2 or s[0] != "[" or s[-1] != "]":
        bad("expected a list of lists of feature ids, like [[0,1],[2,3]]")
    body = s[1:-1]
    if not body:
        return []
    if not re.fullmatch(r"\[[^\[\]]*\](,\[[^\[\]]*\])*", body):
        bad("unbalanced brackets, or not a list of lists")
    groups = []
    for inner in re.findall(r"\[([^\[\]]*)\]", body):
        if not inner:
            bad("empty group")
        ids = set()
        for tok in inner.split(","):
            if not re.fullmatch(r"\+?\d+", tok):
                bad("every feature id is a non-negative integer, got %r" % tok)
            ids.add(int(tok))
        groups.append(sorted(ids))
    if len(groups) > INTERACTION_MAX_GROUPS:
        bad("%d groups, at most %d are supported" % (len(groups), INTERACTION_MAX_GROUPS))
    return groups


def parse_monotone(val):
    """``(1,0,-1)`` | ``1,0,-1`` (spaces and quotes allowed) -> [1, 0, -1]."""
    s = str(val).strip()
    if len(s) >= 2 and s[0] == s[-1] and s[0] in "\"'":
        s = s[1:-1].strip()
    if s.startswith("(") and s.endswith(")"):
        s = s[1:-1]
    out = []
    for tok in s.split(","):
        tok = tok.strip()
        if tok not in ("-1", "0", "1", "+1"):
            raise SystemExit("monotone_constraints=%s: every entry is -1, 0 or 1, got %r"
                             % (val, tok))
        out.append(int(tok))
    return out


def _threshold_l1(G, alpha):
    if alpha == 0:
        return G
    return torch.where(G > alpha, G - alpha, torch.where(G < -alpha, G + alpha, torch.zeros_like(G)))


# ---------------------------------------------------------------- objective
MULTI_METRICS = ("merror", "mlogloss")
SINGLE_METRICS = ("error", "logloss", "rmse", "auc")
RANK_OBJECTIVES = ("rank:pairwise", "rank:ndcg")
NLL_MAX = -math.log(1e-16)
_RANK_METRIC = re.compile(r"^(ndcg|map)(?:@(\d+))?(-)?$")


def parse_rank_metric(name):
    """xgboost's ranking metric names ``ndcg | map`` [``@k``] [``-``] ->
    (kind, k or 0 for no cut-off, minus), or None for any other name."""
    m = _RANK_METRIC.match(name)
    if m is None:
        return None
    return m.group(1), int(m.group(2)) if m.group(2) else 0, m.group(3) is not None


class Objective:
    """Single-output objectives keep one margin per row; multi:softmax and
    multi:softprob keep ``num_class`` margins per row, class-major
    (margin [K, n], gpair [K, n, 2]), so ``margin[k]`` / ``gpair[k]`` are the
    contiguous tensors a tree builder takes: one round grows K trees, tree t
    of the flat list belongs to class t % K. rank:pairwise and rank:ndcg keep
    one margin per row (the prediction is the margin) and need the rows'
    query groups (``DMatrix.group``) for their gradient pairs."""

    def __init__(self, name, num_class=0):
        if name not in ("binary:logistic", "reg:logistic", "reg:linear", "reg:squarederror",
                        "binary:logitraw", "multi:softmax", "multi:softprob") + RANK_OBJECTIVES:
            raise ValueError("unknown objective " + name)
        self.name = name
        self.rank = name in RANK_OBJECTIVES
        self.logistic = name in ("binary:logistic", "reg:logistic", "binary:logitraw")
        self.multi = name.startswith("multi:")
        if self.multi and int(num_class) < 2:
            raise ValueError("objective %s needs num_class >= 2 (got %d)" % (name, num_class))
        self.num_class = int(num_class) if self.multi else 0

    @property
    def n_group(self):
        """Margins per row = trees per boosting round."""
        return self.num_class if self.multi else 1

    def check_labels(self, label, bsp):
        """Multi-class labels must be integers in [0, num_class): decided on
        every rank together (the flag is allreduced before anyone raises, so
        no rank is left waiting in a collective)."""
        if not self.multi:
            return
        bad = bool(((label < 0) | (label >= self.num_class) | (label != label.floor())).any()) \
            if label.numel() else False
        if bsp.allreduce_scalar(1.0 if bad else 0.0, "max") > 0:
            raise ValueError("label must be in [0, num_class)")

    def check_metrics(self, names):
        for m in names:
            if parse_rank_metric(m) is not None:  # any single-output objective, as in xgboost
                if self.multi:
                    raise ValueError("eval_metric %s does not fit objective %s" % (m, self.name))
                continue
            if m not in MULTI_METRICS + SINGLE_METRICS:
                raise ValueError("unknown eval_metric " + m)
            if (m in MULTI_METRICS) != self.multi:
                raise ValueError("eval_metric %s does not fit objective %s" % (m, self.name))

    def prob_to_margin(self, base):
        if self.multi:
            return base  # the same for every class: cancels in the softmax
        if self.logistic:
            if not 0.0 < base < 1.0:
                raise ValueError("base_score must be in (0,1) for logistic loss")
            return -math.log(1.0 / base - 1.0)
        return base

    def gpair(self, margin, label, weight, group=None):
        """group: the rank objectives' query groups, a :class:`RankGroups`
        (``DMatrix.group``) or the int32 offsets [Q + 1]."""
        if self.rank:
            return self._gpair_rank(margin, label, weight, group)
        if self.multi:
            return self._gpair_softmax(margin, label, weight)
        if margin.is_cuda and margin.dtype == torch.float32 and label.dtype == torch.float32:
            # one launch; the root statistics ride along (gpair_stats)
            gp, st = _native.hip().gbdt_gpair(margin.contiguous(), label.contiguous(),
                                              weight.contiguous() if weight is not None else None,
                                              bool(self.logistic))
            gp._wh_stats = st
            return gp
        if self.logistic:
            p = torch.sigmoid(margin)
            g = p - label
            h = torch.clamp(p * (1.0 - p), min=1e-16)
        else:
            g = margin - label
            h = torch.ones_like(margin)
        if weight is not None:
            g, h = g * weight, h * weight
        return torch.stack([g, h], 1).float().contiguous()

    def _gpair_rank(self, margin, label, weight, group):
        """The expectation of xgboost's random partner draw over a row's
        query group (:func:`rank_gpair_torch` has the formulas). On the GPU
        one launch per task class plus the root statistics."""
        if group is None:
            raise ValueError("objective %s needs query groups (a <data>.group file)" % self.name)
        if weight is not None:
            raise ValueError("instance weights are not defined for objective " + self.name)
        group = RankGroups.of(group)
        ndcg = self.name == "rank:ndcg"
        if margin.is_cuda and margin.dtype == torch.float32 and label.dtype == torch.float32:
            small, block, tiled, rows, tiled_rows = group.tasks(margin.device)
            gp, st = _native.hip().gbdt_gpair_rank(
                margin=margin.contiguous(), label=label.contiguous(),
                group_off=group.device_off(margin.device), small=small, block=block, tiled=tiled,
                block_rows=rows, tiled_rows=tiled_rows, ndcg=ndcg)
            gp._wh_stats = st
            return gp
        return rank_gpair_torch(margin, label, group.off, ndcg).float().contiguous()

    def _gpair_softmax(self, margin, label, weight):
        """margin [K, n] -> gpair [K, n, 2]: p = softmax over the classes,
        g = w (p_k - [y = k]), h = w max(2 p_k (1 - p_k), 1e-16). On the GPU
        one launch, with every class's root statistics (:func:`class_gpair`);
        the torch form below is its reference and the CPU path."""
        K = self.num_class
        if margin.dim() != 2 or margin.shape[0] != K:
            raise ValueError("multi-class margins must be [num_class, n]")
        if (margin.is_cuda and margin.dtype == torch.float32 and label.dtype == torch.float32
                and (weight is None or weight.dtype == torch.float32)):
            gp, st = _native.hip().gbdt_gpair_softmax(
                margin.contiguous(), label.contiguous(),
                weight.contiguous() if weight is not None else None)
            gp._wh_stats = st
            return gp
        return softmax_gpair_torch(margin, label, weight)

    def pred(self, margin):
        if self.multi:
            if margin.is_cuda and margin.dtype == torch.float32:
                return _native.hip().gbdt_softmax_out(margin.contiguous(),
                                                      self.name == "multi:softprob")
            if self.name == "multi:softmax":
                return first_argmax(margin).to(margin.dtype)
            return torch.softmax(margin, 0).t().contiguous()
        if self.name in ("binary:logistic", "reg:logistic"):
            return torch.sigmoid(margin)
        return margin

    def default_metric(self):
        if self.multi:
            return "merror"
        if self.rank:
            return "map"
        return "error" if self.name == "binary:logistic" else "rmse"

    def metrics(self, names, margin, label, weight, bsp, group=None):
        """Globally reduced metrics of a set from its margins. The ranking
        metrics (ndcg, map, with ``@k`` and ``-``) are the unweighted mean of
        the per-group values over the non-empty groups of every rank: one
        evaluation (on the GPU one launch per task class, ``gbdt_rank_eval``)
        and one allreduce of {sum, count}. Multi-class:
        merror = sum w [arg-max != y] / sum w and mlogloss = sum w (-log
        max(p_y, 1e-16)) / sum w from ONE reduction {sum w err, sum w nll,
        sum w} (on the GPU one launch, ``gbdt_multi_eval``) and one allreduce
        of the three doubles. A label outside [0, K) counts as an error with
        nll = -log(1e-16)."""
        self.check_metrics(names)
        if not self.multi:
            p = self.pred(margin)
            return [rank_metric(m, margin, label, group, bsp) if parse_rank_metric(m)
                    else eval_metric(m, p, label, weight, bsp) for m in names]
        v = multi_eval_sums(margin, label, weight)
        bsp.allreduce(v)
        v = v.tolist()
        den = v[2] if v[2] > 0 else 1.0
        return [v[0] / den if m == "merror" else v[1] / den for m in names]


def first_argmax(margin):
    """Arg-max over the classes of margin [K, n]; on an exact tie the lowest
    class wins."""
    K = margin.shape[0]
    ids = torch.arange(K, device=margin.device)[:, None]
    mx = margin.max(0, keepdim=True).values
    return torch.where(margin == mx, ids, torch.full_like(ids, K)).min(0).values


def softmax_gpair_torch(margin, label, weight):
    """The softmax gradient pairs [K, n, 2] of margin [K, n] in plain torch,
    in the margins' precision: the reference of ``gbdt_gpair_softmax``."""
    K = margin.shape[0]
    p = torch.softmax(margin, 0)
    hit = label[None, :] == torch.arange(K, device=margin.device, dtype=label.dtype)[:, None]
    g = p - hit.to(p.dtype)
    h = torch.clamp(2.0 * p * (1.0 - p), min=1e-16)
    if weight is not None:
        g, h = g * weight[None, :], h * weight[None, :]
    return torch.stack([g, h], 2).float().contiguous()


def multi_eval_sums(margin, label, weight):
    """{sum w err, sum w nll, sum w} (fp64 [3]) of this rank's rows."""
    K = margin.shape[0]
    if (margin.is_cuda and margin.dtype == torch.float32 and label.dtype == torch.float32
            and (weight is None or weight.dtype == torch.float32)):
        return _native.hip().gbdt_multi_eval(margin.contiguous(), label.contiguous(),
                                             weight.contiguous() if weight is not None else None)
    w = (weight if weight is not None else torch.ones_like(label)).double()
    if label.numel() == 0:
        return torch.zeros(3, dtype=torch.float64, device=margin.device)
    ok = (label >= 0) & (label < K) & (label == label.floor())
    yi = torch.where(ok, label, torch.zeros_like(label)).long()
    m = margin.double()
    lse = torch.logsumexp(m, 0)
    nll = (lse - m.gather(0, yi[None, :])[0]).clamp(max=NLL_MAX)
    nll = torch.where(ok, nll, torch.full_like(nll, NLL_MAX))
    err = torch.where(ok, (first_argmax(m) != yi).double(), torch.ones_like(nll))
    return torch.stack([(w * err).sum(), (w * nll).sum(), w.sum()])


def class_gpair(gpair, k):
    """Class k's [n, 2] slice of a multi-class gradient tensor, carrying its
    own row of the fused kernel's root statistics (else every tree pays a
    fresh reduction and a host wait in :func:`gpair_stats`)."""
    gk = gpair[k]
    st = getattr(gpair, "_wh_stats", None)
    if st is not None:
        gk._wh_stats = st[k]
    return gk


def gpair_stats(gpair):
    """(sum g, sum h) in fp64 and (max |g|, max |h|) of a gradient-pair
    tensor: the ones the fused GPU gradient kernel computed alongside it,
    else reduced here."""
    st = getattr(gpair, "_wh_stats", None)
    if st is not None:
        return st[:2].clone(), st[2:4].float()
    if gpair.shape[0] == 0:
        z = torch.zeros(2, dtype=torch.float64, device=gpair.device)
        return z, z.float()
    return gpair.double().sum(0), gpair.abs().amax(0).float()


def eval_metric(name, pred, label, weight, bsp):
    """Globally reduced metric (xgboost CLI names)."""
    w = weight if weight is not None else torch.ones_like(label)
    if name == "error":
        s = (((pred > 0.5).float() != (label > 0.5).float()).float() * w).sum()
        v = torch.stack([s.double(), w.sum().double()])
        bsp.allreduce(v)
        return float(v[0] / v[1])
    if name == "logloss":
        p = pred.clamp(1e-16, 1 - 1e-16)
        s = (-(label * torch.log(p) + (1 - label) * torch.log(1 - p)) * w).sum()
        v = torch.stack([s.double(), w.sum().double()])
        bsp.allreduce(v)
        return float(v[0] / v[1])
    if name == "rmse":
        s = (((pred - label) ** 2) * w).sum()
        v = torch.stack([s.double(), w.sum().double()])
        bsp.allreduce(v)
        return math.sqrt(float(v[0] / v[1]))
    if name == "auc":
        from .. import ops
        parts = bsp.comm.allgather_object((pred.cpu(), label.cpu())) if bsp.world > 1 else [
            (pred.cpu(), label.cpu())]
        p = torch.cat([a for a, _ in parts])
        lab = torch.cat([b for _, b in parts])
        return float(ops.ref.auc(p, lab))
    if name in MULTI_METRICS:
        raise ValueError("eval_metric %s needs a multi-class objective (Objective.metrics)" % name)
    raise ValueError("unknown eval_metric " + name)


# ------------------------------------------------------- learning to rank
class RankGroups:
    """The query groups of a matrix: rows [off[q], off[q + 1]) are group q
    (int32 offsets [Q + 1] on the host, the first 0, non-decreasing, the last
    n; empty groups are legal). The device copy and the kernels' task plan
    (csrc/host/gbdt_rank_plan.h) are made once per device and kept."""

    def __init__(self, off, n=None):
        off = torch.as_tensor(off).detach().cpu()
        if off.dim() != 1 or off.is_floating_point():
            raise ValueError("group offsets must be an integer vector [Q + 1]")
        off = off.long()
        n = int(off[-1]) if n is None and off.numel() else int(n or 0)
        # (the plan validates: ValueError for malformed offsets)
        self._plan = _native.hip().gbdt_rank_plan(off, n)
        self.off = off.to(torch.int32)
        self.n = n
        self._dev = {}

    @staticmethod
    def of(group):
        return group if isinstance(group, RankGroups) else RankGroups(group)

    @staticmethod
    def from_sizes(sizes):
        sizes = torch.as_tensor(sizes, dtype=torch.int64)
        return RankGroups(torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]))

    @property
    def num_group(self):
        return self.off.numel() - 1

    def _on(self, device):
        device = torch.device(device)
        d = self._dev.get(device)
        if d is None:
            small, block, tiled, rows, tiled_rows = self._plan
            d = self._dev[device] = (self.off.to(device), small.to(device), block.to(device),
                                     tiled.to(device), int(rows), int(tiled_rows))
        return d

    def device_off(self, device):
        return self._on(device)[0]

    def tasks(self, device):
        """(small, block, tiled: int32 group ids on the device; the rows of
        the largest block group and of the largest tiled group)"""
        return self._on(device)[1:]


def _rank_batches(off, budget):
    """Non-empty groups, larger first, cut into batches of similar size: each
    ([group ids], L = its largest size) pads to [G, L] with G L^2 <= budget
    where it can and sizes of at least L / 2 (any size once L <= 16)."""
    sizes = (off[1:] - off[:-1]).long()
    order = torch.argsort(sizes, descending=True, stable=True)
    order = order[sizes[order] > 0]
    s, o = sizes[order].tolist(), order.tolist()
    out, a = [], 0
    while a < len(o):
        L = s[a]
        cap = max(1, budget // (L * L))
        b = a + 1
        while b < len(o) and b - a < cap and (2 * s[b] >= L or L <= 16):
            b += 1
        out.append((o[a:b], L))
        a = b
    return out


class _RankBatch:
    """A padded batch [G, L] of groups: margins M, labels Y, validity, the
    rows' global indices, and pair masks of a chunk of rows [a, b)."""

    def __init__(self, margin, label, off, gids, L):
        dev = margin.device
        g = torch.tensor(gids, dtype=torch.long, device=dev)
        beg = off[g]
        self.ar = torch.arange(L, device=dev)
        self.valid = self.ar[None, :] < (off[g + 1] - beg)[:, None]
        self.idx = (beg[:, None] + self.ar[None, :]).clamp(max=max(margin.numel() - 1, 0))
        self.M, self.Y = margin[self.idx], label[self.idx]
        self.G, self.L = len(gids), L

    def chunks(self, budget):
        step = max(1, budget // (self.G * self.L))
        return [(a, min(self.L, a + step)) for a in range(0, self.L, step)]

    def pairs(self, X, a, b):
        """(X_i [G, b - a, 1], X_j [G, 1, L])"""
        return X[:, a:b, None], X[:, None, :]

    def ranks(self, X, a, b):
        """Rows j ahead of row i by X: X_j > X_i, or equal and j before i."""
        xi, xj = self.pairs(X, a, b)
        before = self.ar[None, None, :] < self.ar[None, a:b, None]
        return ((xj > xi) | ((xj == xi) & before)) & self.valid[:, None, :]

    def scatter(self, out, val):
        out[self.idx[self.valid]] = val[self.valid]


def _discount(r):
    return 1.0 / torch.log2(2.0 + r.double())


def rank_gpair_torch(margin, label, group_off, ndcg, mass=False, budget=1 << 22):
    """Gradient pairs [n, 2] of rank:pairwise / rank:ndcg in plain torch: the
    CPU path and the reference of ``gbdt_gpair_rank`` (CPU or GPU tensors).

    Within a group, c_i = rows with another label, r_i / lr_i = rows ahead of
    i by margin / by label (ties: the earlier row is ahead), gain = 2^y - 1,
    IDCG = sum gain_i / log2(2 + lr_i). Every pair with y_i > y_j weighs
    W = (1 / c_i + 1 / c_j) * delta, delta = 1 (pairwise) or |gain_i - gain_j|
    |1 / log2(2 + r_i) - 1 / log2(2 + r_j)| / IDCG (ndcg; 0 when IDCG = 0):
    the expectation of drawing, for every row, one partner with a different
    label uniformly. With rho = sigmoid(m_i - m_j), lambda = rho - 1 and eta =
    max(rho (1 - rho), 1e-16): g_i += W lambda, g_j -= W lambda, h_i and h_j
    += 2 W eta. Per-pair terms are in the margins' precision (the discounts
    and IDCG are taken in fp64 and rounded once); a row's sums are fp64,
    rounded once to the margins' precision. mass: also return the rows' fp64
    sum of W |lambda| (the scale of g's rounding error)."""
    T = margin.dtype
    n, dev = margin.numel(), margin.device
    off = torch.as_tensor(group_off).to(dev).long()
    g_out = torch.zeros(n, dtype=torch.float64, device=dev)
    h_out, m_out = torch.zeros_like(g_out), torch.zeros_like(g_out)
    label = label.to(T)
    for gids, L in _rank_batches(off.cpu(), budget):
        bt = _RankBatch(margin, label, off, gids, L)
        vj = bt.valid[:, None, :]
        c = torch.zeros(bt.G, L, dtype=torch.long, device=dev)
        r, lr = torch.zeros_like(c), torch.zeros_like(c)
        for a, b in bt.chunks(budget):
            yi, yj = bt.pairs(bt.Y, a, b)
            c[:, a:b] = ((yj != yi) & vj).sum(-1)
            if ndcg:
                r[:, a:b] = bt.ranks(bt.M, a, b).sum(-1)
                lr[:, a:b] = bt.ranks(bt.Y, a, b).sum(-1)
        invc = torch.where(c > 0, 1.0 / c.to(T), torch.zeros((), dtype=T, device=dev))
        if ndcg:
            gain = torch.exp2(bt.Y) - 1.0
            disc = _discount(r).to(T)
            idcg = (gain.double() * _discount(lr) * bt.valid).sum(-1)
            inv_idcg = torch.where(idcg > 0, 1.0 / idcg, torch.zeros_like(idcg)).to(T)
        gs = torch.zeros(bt.G, L, dtype=torch.float64, device=dev)
        hs, ms = torch.zeros_like(gs), torch.zeros_like(gs)
        for a, b in bt.chunks(budget):
            mi, mj = bt.pairs(bt.M, a, b)
            yi, yj = bt.pairs(bt.Y, a, b)
            w = invc[:, a:b, None] + invc[:, None, :]
            if ndcg:
                gi, gj = bt.pairs(gain, a, b)
                di, dj = bt.pairs(disc, a, b)
                w = w * ((gi - gj).abs() * (di - dj).abs() * inv_idcg[:, None, None])
            part = (yi != yj) & vj
            hi = yi > yj
            d = torch.where(hi, mi - mj, mj - mi)  # m_hi - m_lo
            t = torch.exp(-d.abs())
            s = 1.0 / (1.0 + t)
            ts = t * s
            rho = torch.where(d >= 0, s, ts)
            q = torch.where(d >= 0, ts, s)  # 1 - rho, without cancellation
            eta = (rho * q).clamp(min=1e-16)
            wl = w * -q
            zero = torch.zeros((), dtype=T, device=dev)
            gs[:, a:b] = torch.where(part, torch.where(hi, wl, -wl), zero).double().sum(-1)
            hs[:, a:b] = torch.where(part, 2.0 * w * eta, zero).double().sum(-1)
            if mass:
                ms[:, a:b] = torch.where(part, w * q, zero).double().sum(-1)
        bt.scatter(g_out, gs)
        bt.scatter(h_out, hs)
        bt.scatter(m_out, ms)
    gp = torch.stack([g_out, h_out], 1).to(T).contiguous()
    return (gp, m_out) if mass else gp


def rank_eval_torch(margin, label, group_off, kind, k=0, minus=False, budget=1 << 22):
    """Per-group ndcg@k (kind "ndcg") or map@k ("map") in plain torch, fp64
    [Q] with NaN for an empty group (k = 0: no cut-off): the CPU path and the
    reference of ``gbdt_rank_eval``. ndcg@k = (sum over r_i < k of gain_i /
    log2(2 + r_i)) / (the same over lr_i < k with lr_i). map@k: a hit is
    y_i > 0, hits_i = hits j with r_j <= r_i, map = (sum over hits i with
    r_i < k of hits_i / (r_i + 1)) / (hits of the whole group). A group whose
    denominator is 0 scores 1, or, minus, 0."""
    if kind not in ("ndcg", "map"):
        raise ValueError("unknown ranking metric " + kind)
    dev = margin.device
    off = torch.as_tensor(group_off).to(dev).long()
    Q = off.numel() - 1
    out = torch.full((Q,), float("nan"), dtype=torch.float64, device=dev)
    kk = int(k) if k and k > 0 else (1 << 62)
    label = label.to(margin.dtype)
    for gids, L in _rank_batches(off.cpu(), budget):
        bt = _RankBatch(margin, label, off, gids, L)
        r = torch.zeros(bt.G, L, dtype=torch.long, device=dev)
        lr, hits = torch.zeros_like(r), torch.zeros_like(r)
        hit = (bt.Y > 0) & bt.valid
        for a, b in bt.chunks(budget):
            ahead = bt.ranks(bt.M, a, b)
            r[:, a:b] = ahead.sum(-1)
            if kind == "ndcg":
                lr[:, a:b] = bt.ranks(bt.Y, a, b).sum(-1)
            else:
                me = bt.ar[None, None, :] == bt.ar[None, a:b, None]
                hits[:, a:b] = ((ahead | me) & hit[:, None, :]).sum(-1)
        if kind == "ndcg":
            gain = torch.exp2(bt.Y.double()) - 1.0
            num = (gain * _discount(r) * (bt.valid & (r < kk))).sum(-1)
            den = (gain * _discount(lr) * (bt.valid & (lr < kk))).sum(-1)
        else:
            num = (hits.double() / (r + 1).double() * (hit & (r < kk))).sum(-1)
            den = hit.sum(-1).double()
        val = torch.where(den > 0, num / den.clamp(min=1e-300),
                          torch.full_like(num, 0.0 if minus else 1.0))
        out[torch.tensor(gids, dtype=torch.long, device=dev)] = val
    return out


def rank_eval(margin, label, group, kind, k=0, minus=False):
    """Per-group ranking metric values, fp64 [Q] (NaN: an empty group): on
    the GPU ``gbdt_rank_eval``, else :func:`rank_eval_torch`."""
    group = RankGroups.of(group)
    if margin.is_cuda and margin.dtype == torch.float32 and label.dtype == torch.float32:
        small, block, tiled, rows, tiled_rows = group.tasks(margin.device)
        return _native.hip().gbdt_rank_eval(
            margin=margin.contiguous(), label=label.contiguous(),
            group_off=group.device_off(margin.device), small=small, block=block, tiled=tiled,
            block_rows=rows, tiled_rows=tiled_rows, kind=0 if kind == "ndcg" else 1, k=int(k), minus=bool(minus))
    return rank_eval_torch(margin, label, group.off, kind, k, minus)


def rank_metric(name, margin, label, group, bsp):
    """A ranking metric's global value: the mean of the per-group values over
    the non-empty groups of all ranks (a group cut by a rank boundary counts
    as two)."""
    kind, k, minus = parse_rank_metric(name)
    if group is None:
        raise ValueError("eval_metric %s needs query groups (a <data>.group file)" % name)
    v = rank_eval(margin, label, group, kind, k, minus)
    ok = ~torch.isnan(v)
    s = torch.stack([torch.where(ok, v, torch.zeros_like(v)).sum(), ok.sum().double()])
    bsp.allreduce(s)
    s = s.tolist()
    return s[0] / s[1] if s[1] > 0 else 0.0
