"""GBDT parameters, objectives (single-output and multi-class softmax, with
their gradient pairs) and globally reduced metrics; models/gbdt.py grows the trees."""
import math

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

    def set(self, name, val):
        name = self.ALIASES.get(name, name)
        if name == "lambda":
            self.reg_lambda = float(val)
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


def _threshold_l1(G, alpha):
    if alpha == 0:
        return G
    return torch.where(G > alpha, G - alpha, torch.where(G < -alpha, G + alpha, torch.zeros_like(G)))


# ---------------------------------------------------------------- objective
MULTI_METRICS = ("merror", "mlogloss")
SINGLE_METRICS = ("error", "logloss", "rmse", "auc")
NLL_MAX = -math.log(1e-16)


class Objective:
    """Single-output objectives keep one margin per row; multi:softmax and
    multi:softprob keep ``num_class`` margins per row, class-major
    (margin [K, n], gpair [K, n, 2]), so ``margin[k]`` / ``gpair[k]`` are the
    contiguous tensors a tree builder takes: one round grows K trees, tree t
    of the flat list belongs to class t % K."""

    def __init__(self, name, num_class=0):
        if name not in ("binary:logistic", "reg:logistic", "reg:linear", "reg:squarederror",
                        "binary:logitraw", "multi:softmax", "multi:softprob"):
            raise ValueError("unknown objective " + name)
        self.name = name
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

    def gpair(self, margin, label, weight):
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
        return "error" if self.name == "binary:logistic" else "rmse"

    def metrics(self, names, margin, label, weight, bsp):
        """Globally reduced metrics of a set from its margins. Multi-class:
        merror = sum w [arg-max != y] / sum w and mlogloss = sum w (-log
        max(p_y, 1e-16)) / sum w from ONE reduction {sum w err, sum w nll,
        sum w} (on the GPU one launch, ``gbdt_multi_eval``) and one allreduce
        of the three doubles. A label outside [0, K) counts as an error with
        nll = -log(1e-16)."""
        self.check_metrics(names)
        if not self.multi:
            p = self.pred(margin)
            return [eval_metric(m, p, label, weight, bsp) for m in names]
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


