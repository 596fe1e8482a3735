"""GBDT parameters, objectives (single-output, multi-class softmax, learning
to rank over query groups and survival, with their gradient pairs) and
globally reduced metrics; models/gbdt.py grows the trees."""
import math
import re

import torch

from .. import _native
from .gbdt_survival import (SURVIVAL_METRICS, SURVIVAL_OBJECTIVES, aft_eval_sums, aft_gpair,
                            check_aft_params, cox_eval_sums, cox_gpair)


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
        # max_delta_step: every node's weight stays in [-d, d] (0: off). None:
        # not set -- 0.7 for count:poisson, else 0 (:meth:`delta_step`)
        self.max_delta_step = None
        self.scale_pos_weight = 1.0  # the logistic family: the weight of rows with y == 1
        self.tweedie_variance_power = 1.5  # reg:tweedie (and its default metric): in (1, 2)
        self.huber_slope = 1.0  # reg:pseudohubererror and mphe: > 0
        # booster=dart (models/gbdt_dart.py); read by no one under gbtree
        self.rate_drop = 0.0  # a round's chance of being dropped, in [0, 1]
        self.skip_drop = 0.0  # a round's chance of dropping nothing, in [0, 1]
        self.one_drop = 0  # 1: a round that chose nothing drops one round
        self.sample_type = "uniform"  # | weighted: chances in proportion to the weights
        self.normalize_type = "tree"  # | forest
        # reg:quantileerror: the outputs' quantiles, in the order given ([]:
        # not set); any other objective ignores them
        self.quantile_alpha = []
        # tree growth (training only, not stored in the model): depthwise grows
        # level by level; lossguide splits the open leaf of the largest gain
        # until max_leaves leaves (0: no limit of its own) -- :meth:`leaf_limits`
        self.grow_policy = "depthwise"
        self.max_leaves = 0
        # survival:aft (not stored in the model): normal | logistic | extreme, sigma > 0
        self.aft_loss_distribution = "normal"
        self.aft_loss_distribution_scale = 1.0

    def set(self, name, val):
        name = self.ALIASES.get(name, name)
        if name == "lambda":
            self.reg_lambda = float(val)
        elif name == "monotone_constraints":
            self.monotone = parse_monotone(val)
        elif name == "interaction_constraints":
            self.interaction = parse_interaction(val)
        elif name == "quantile_alpha":
            from .gbdt_quantile import parse_quantile_alpha
            self.quantile_alpha = parse_quantile_alpha(val)
        elif name in ("max_delta_step", "scale_pos_weight", "tweedie_variance_power",
                      "huber_slope"):
            setattr(self, name, float(val))
            check_objective_scalars(self)
        elif name == "aft_loss_distribution":
            self.aft_loss_distribution = str(val).strip()
            check_aft_params(self)
        elif name == "aft_loss_distribution_scale":
            try:
                self.aft_loss_distribution_scale = float(val)
            except ValueError:
                raise SystemExit("aft_loss_distribution_scale=%s: must be a positive number" % val)
            check_aft_params(self)
        elif name in ("eta", "gamma", "min_child_weight", "alpha", "base_score", "subsample",
                      "colsample_bytree"):
            setattr(self, name, float(val))
        elif name in ("max_depth", "max_bin", "seed", "silent", "num_class"):
            setattr(self, name, int(val))
        elif name == "booster":
            if val not in ("gbtree", "dart"):
                raise SystemExit("booster=%s is not supported: booster is gbtree or dart" % val)
            self.booster = val
        elif name == "grow_policy":
            if val not in ("depthwise", "lossguide"):
                raise SystemExit("grow_policy=%s is not supported: grow_policy is depthwise or "
                                 "lossguide" % val)
            self.grow_policy = val
        elif name == "max_leaves":
            try:
                x = int(str(val).strip())
            except ValueError:
                x = -1
            if not 0 <= x <= _native.hip().gbdt_leaf_max_leaves():
                raise SystemExit("max_leaves must be an integer in [0, %d], got %s"
                                 % (_native.hip().gbdt_leaf_max_leaves(), val))
            self.max_leaves = x
        elif name in ("rate_drop", "skip_drop"):
            try:
                x = float(val)
            except ValueError:
                x = float("nan")
            if not 0.0 <= x <= 1.0:
                raise SystemExit("%s must be in [0, 1], got %s" % (name, val))
            setattr(self, name, x)
        elif name == "one_drop":
            if str(val).strip() not in ("0", "1"):
                raise SystemExit("one_drop must be 0 or 1, got %s" % val)
            self.one_drop = int(val)
        elif name in ("sample_type", "normalize_type"):
            allowed = {"sample_type": ("uniform", "weighted"), "normalize_type": ("tree", "forest")}
            if val not in allowed[name]:
                raise SystemExit("%s must be %s or %s, got %s" % ((name,) + allowed[name] + (val,)))
            setattr(self, name, val)
        elif name == "objective":
            setattr(self, name, val)
        elif name == "eval_metric":
            self.eval_metric.append(val)
        else:
            return False
        return True

    def leaf_limits(self):
        """What grow_policy, max_leaves and max_depth put into effect, checked
        (training only; the same answer on every rank): None under depthwise,
        where max_leaves > 0 is refused; under lossguide (leaves, depth) -- the
        tree stops at ``leaves`` leaves and a node at depth ``depth`` is never
        split (csrc/host/gbdt_leaf_plan.h gbdt_leaf_limits: max_depth=0 is
        the deepest tree the model's consumers take, depth 62; max_leaves=0
        is min(2^max_depth, 32768); both 0 is refused)."""
        if self.grow_policy != "lossguide":
            if self.max_leaves > 0:
                raise SystemExit("max_leaves=%d needs grow_policy=lossguide: grow_policy=depthwise "
                                 "does not limit the leaves" % self.max_leaves)
            return None
        try:
            return tuple(_native.hip().gbdt_leaf_limits(max_leaves=int(self.max_leaves),
                                                        max_depth=int(self.max_depth)))
        except ValueError as e:
            raise SystemExit("grow_policy=lossguide with max_leaves=%d max_depth=%d: %s"
                             % (self.max_leaves, self.max_depth, e))

    def delta_step(self):
        """max_delta_step in effect: as set, else xgboost's 0.7 for
        count:poisson and 0 (off) for every other objective."""
        if self.max_delta_step is None:
            return 0.7 if self.objective == "count:poisson" else 0.0
        return float(self.max_delta_step)

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


def check_objective_scalars(p):
    """The ranges of the objectives' scalar parameters (docs/bsp_apps.md
    "Objectives and max_delta_step"); ``p``: anything that carries them."""
    d = getattr(p, "max_delta_step", None)
    if d is not None and not d >= 0:
        raise SystemExit("max_delta_step=%g: must not be negative (0: off)" % d)
    if not getattr(p, "scale_pos_weight", 1.0) > 0:
        raise SystemExit("scale_pos_weight=%g: must be positive" % p.scale_pos_weight)
    if not 1.0 < getattr(p, "tweedie_variance_power", 1.5) < 2.0:
        raise SystemExit("tweedie_variance_power=%g: must lie in (1, 2)"
                         % p.tweedie_variance_power)
    if not getattr(p, "huber_slope", 1.0) > 0:
        raise SystemExit("huber_slope=%g: must be positive" % p.huber_slope)


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
# The objectives of csrc/host/gbdt_objective.h (GbdtObj ids): one templated
# gradient kernel, ``gbdt_gpair_obj``; OBJ_LOGISTIC is the logistic family
# under scale_pos_weight != 1.
OBJ_LOGISTIC = 0
OBJ_IDS = {"count:poisson": 1, "reg:gamma": 2, "reg:tweedie": 3, "binary:hinge": 4,
           "reg:pseudohubererror": 5, "reg:squaredlogerror": 6}
# The adaptive objectives (their own ids of the same kernel): h = w carries no
# curvature, so a grown tree's leaves are refreshed with the weighted quantile
# of the residuals (models/gbdt_quantile.py)
OBJ_ABSOLUTE, OBJ_QUANTILE = 8, 9
ADAPTIVE_OBJECTIVES = ("reg:absoluteerror", "reg:quantileerror")
# prediction exp(margin); base_score > 0 enters as its logarithm
LOG_LINK_OBJECTIVES = ("count:poisson", "reg:gamma", "reg:tweedie") + SURVIVAL_OBJECTIVES
FLT_MIN = 1.1754943508222875e-38
SQUARED_LOG_MIN_MARGIN = -1.0 + 1e-6
# The metrics of the one-launch evaluation kernel ``gbdt_obj_eval`` (GbdtMetric
# ids, the slots of its sums; the last slot is sum w)
OBJ_METRICS = ("poisson-nloglik", "gamma-nloglik", "gamma-deviance", "tweedie-nloglik", "mae",
               "mphe", "rmsle")
_RANK_METRIC = re.compile(r"^(ndcg|map)(?:@(\d+))?(-)?$")


def parse_rank_metric(name):
    """xgboost's ranking metric names ``ndcg | map`` [``@k``] [``-``] ->
    (kind, k or 0 for no cut-off, minus), or None for any other name."""
    m = _RANK_METRIC.match(name)
    if m is None:
        return None
    return m.group(1), int(m.group(2)) if m.group(2) else 0, m.group(3) is not None


def parse_obj_metric(name):
    """``poisson-nloglik | gamma-nloglik | gamma-deviance | mae | mphe |
    rmsle`` or ``tweedie-nloglik@rho`` with rho in (1, 2) -> (slot, rho or
    None); None for any other name. tweedie-nloglik without ``@rho``, or with
    a rho outside (1, 2), is a ValueError."""
    base, at, arg = name.partition("@")
    if base not in OBJ_METRICS:
        return None
    if base != "tweedie-nloglik":
        return None if at else (OBJ_METRICS.index(base), None)
    try:
        rho = float(arg)
    except ValueError:
        rho = float("nan")
    if not at or not 1.0 < rho < 2.0:
        raise ValueError("eval_metric %s: write tweedie-nloglik@rho with rho in (1, 2)" % name)
    return OBJ_METRICS.index(base), rho


class Objective:
    """Single-output objectives keep one margin per row; multi:softmax and
    multi:softprob keep ``num_class`` margins per row, class-major
    (margin [K, n], gpair [K, n, 2]), so ``margin[k]`` / ``gpair[k]`` are the
    contiguous tensors a tree builder takes: one round grows K trees, tree t
    of the flat list belongs to class t % K. rank:pairwise and rank:ndcg keep
    one margin per row (the prediction is the margin) and need the rows'
    query groups (``DMatrix.group``) for their gradient pairs.
    reg:quantileerror keeps one margin per alpha of ``quantile_alpha`` in the
    same [K, n] layout (reg:absoluteerror: one, alpha 0.5); both are
    ``adaptive``: their trees' leaves are refreshed with residual quantiles
    (models/gbdt_quantile.py), for which :func:`grow_round` hands the growers
    the residual inputs. survival:cox and survival:aft (models/gbdt_survival.py)
    keep one margin per row and predict exp(margin); their pairs and metrics
    take the Cox plan resp. the AFT bounds from the rows' matrix (``data``)."""

    # the names a subclass adds to the ones this class takes
    EXTRA_NAMES = ()

    def __init__(self, name, num_class=0, param=None, n_out=None):
        """param: what carries max_delta_step (``delta_step()``),
        scale_pos_weight, tweedie_variance_power, huber_slope and
        quantile_alpha (a :class:`GBDTParam`); None: their defaults. n_out:
        the outputs per row of a reg:quantileerror model that is loaded (its
        file's; the alphas are not stored and may be absent)."""
        if name not in ("binary:logistic", "reg:logistic", "reg:linear", "reg:squarederror",
                        "binary:logitraw", "multi:softmax", "multi:softprob") + RANK_OBJECTIVES \
                + SURVIVAL_OBJECTIVES + self.EXTRA_NAMES and name not in OBJ_IDS:
            raise ValueError("unknown objective " + name)
        self.name = name
        # the adaptive objectives: alphas [K] (0.5 for reg:absoluteerror; None
        # for a loaded reg:quantileerror model without quantile_alpha)
        self.adaptive = name in ADAPTIVE_OBJECTIVES
        self.alphas, self.n_out = None, 1
        if name == "reg:absoluteerror":
            self.alphas = [0.5]
        elif name == "reg:quantileerror":
            given = [float(a) for a in (getattr(param, "quantile_alpha", None) or [])]
            if n_out is None and not given:
                raise SystemExit("objective reg:quantileerror needs quantile_alpha")
            self.alphas = given or None
            self.n_out = int(n_out) if n_out is not None else len(given)
        self.rank = name in RANK_OBJECTIVES
        # survival:cox takes the matrix's plan, survival:aft its bounds (``data``
        # of gpair / metrics); the AFT distribution and scale are not stored
        self.cox, self.aft = name == "survival:cox", name == "survival:aft"
        self.aft_dist, self.aft_sigma = check_aft_params(param)
        self.logistic = name in ("binary:logistic", "reg:logistic", "binary:logitraw")
        self.multi = name.startswith("multi:")
        if self.multi and int(num_class) < 2:
            raise ValueError("objective %s needs num_class >= 2 (got %d)" % (name, num_class))
        self.num_class = int(num_class) if self.multi else 0
        self.log_link = name in LOG_LINK_OBJECTIVES
        if param is not None:
            check_objective_scalars(param)
        self.rho = float(getattr(param, "tweedie_variance_power", 1.5))
        self.delta = float(getattr(param, "huber_slope", 1.0))
        self.pos_weight = float(getattr(param, "scale_pos_weight", 1.0))
        # (count:poisson's hessian is exp(m + max_delta_step); the rule of
        # GBDTParam.delta_step)
        d = getattr(param, "max_delta_step", None)
        self.max_delta_step = float(d) if d is not None else (
            0.7 if name == "count:poisson" else 0.0)
        if self.pos_weight != 1.0 and not self.logistic:
            raise ValueError("scale_pos_weight=%g does not fit objective %s (the logistic family "
                             "only)" % (self.pos_weight, name))
        # the gradient kernel's id: a new objective's, or the logistic
        # family's under scale_pos_weight (else the existing entry points)
        self.obj_id = OBJ_IDS.get(name, OBJ_LOGISTIC if self.logistic and self.pos_weight != 1.0
                                  else None)

    @property
    def n_group(self):
        """Margins per row = trees per boosting round."""
        return self.num_class if self.multi else self.n_out

    def _alphas(self, what):
        """reg:quantileerror's alphas where they are needed."""
        if self.alphas is None:
            raise SystemExit("%s of objective reg:quantileerror needs quantile_alpha" % what)
        if len(self.alphas) != self.n_out:
            raise SystemExit("quantile_alpha has %d entries, the model has %d outputs per row"
                             % (len(self.alphas), self.n_out))
        return self.alphas

    def check_combination(self, param):
        """What an adaptive objective refuses: a refreshed leaf honours
        neither monotone bounds nor max_delta_step."""
        if not self.adaptive:
            return
        if any(getattr(param, "monotone", None) or []):
            raise SystemExit("monotone_constraints does not go with objective %s (its leaves are "
                             "refreshed with residual quantiles, outside the bounds)" % self.name)
        if param.delta_step() > 0:
            raise SystemExit("max_delta_step=%g does not go with objective %s (its leaves are "
                             "refreshed with residual quantiles, outside the bound)"
                             % (param.delta_step(), self.name))

    def check_labels(self, label, bsp):
        """Multi-class labels must be integers in [0, num_class): decided on
        every rank together (the flag is allreduced before anyone raises, so
        no rank is left waiting in a collective)."""
        rule = {"count:poisson": (lambda y: y < 0, "label must be non-negative"),
                "reg:tweedie": (lambda y: y < 0, "label must be non-negative"),
                "reg:gamma": (lambda y: y <= 0, "label must be positive"),
                "binary:hinge": (lambda y: (y != 0) & (y != 1), "label must be 0 or 1"),
                "reg:squaredlogerror": (lambda y: y <= -1, "label must be greater than -1"),
                }.get(self.name)
        if self.adaptive or self.cox:  # (no place for NaN: the residuals' keys, the sort of t)
            rule = (lambda y: ~torch.isfinite(y), "label must be finite")
        if rule is not None:  # (a NaN label fails every rule's complement too)
            bad = bool((rule[0](label) | (label != label)).any()) if label.numel() else False
            if bsp.allreduce_scalar(1.0 if bad else 0.0, "max") > 0:
                raise ValueError("objective %s: %s" % (self.name, rule[1]))
        if not self.multi:
            return
        bad = bool(((label < 0) | (label >= self.num_class) | (label != label.floor())).any()) \
            if label.numel() else False
        if bsp.allreduce_scalar(1.0 if bad else 0.0, "max") > 0:
            raise ValueError("label must be in [0, num_class)")

    def check_metrics(self, names):
        for m in names:
            if m == "quantile":
                if self.name != "reg:quantileerror":
                    raise ValueError("eval_metric quantile does not fit objective %s" % self.name)
                continue
            if m in SURVIVAL_METRICS:
                if not (self.cox if m == "cox-nloglik" else self.aft):
                    raise ValueError("eval_metric %s does not fit objective %s" % (m, self.name))
                continue
            if self.n_out > 1:
                raise ValueError("eval_metric %s does not fit objective %s with %d outputs per "
                                 "row (quantile only)" % (m, self.name, self.n_out))
            # the ranking and the one-launch metrics: any single-output objective
            if parse_rank_metric(m) is not None or parse_obj_metric(m) is not None:
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
        if self.log_link:
            if not base > 0.0:
                raise ValueError("base_score must be positive for objective " + self.name)
            return math.log(base)
        return base

    def gpair(self, margin, label, weight, group=None, pos_weight=True, data=None):
        """group: the rank objectives' query groups, a :class:`RankGroups`
        (``DMatrix.group``) or the int32 offsets [Q + 1]. pos_weight=False
        leaves scale_pos_weight out, as weight=None leaves the instance
        weights out (the hessians of the quantile sketch). data: the matrix
        the rows belong to; survival:cox takes its cached plan from it (None:
        a plan is built for this call), survival:aft its bounds."""
        if self.cox:
            return cox_gpair(margin, label, weight, data.cox_plan() if data is not None else None)
        if self.aft:
            lower, upper = self._bounds(data)
            return aft_gpair(margin, lower, upper, weight, self.aft_dist, self.aft_sigma)
        if self.rank:
            return self._gpair_rank(margin, label, weight, group)
        if self.multi:
            return self._gpair_softmax(margin, label, weight)
        if self.adaptive:
            return self._gpair_adaptive(margin, label, weight)
        oid = self.obj_id if pos_weight or self.obj_id != OBJ_LOGISTIC else None
        if oid is not None:
            return self._gpair_obj(oid, margin, label, weight)
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

    def _bounds(self, data):
        if data is None or getattr(data, "lower", None) is None:
            raise ValueError("objective survival:aft and its metrics need the rows' bounds (a "
                             "<data>.label_lower_bound and a <data>.label_upper_bound file)")
        return data.lower, data.upper

    def _gpair_obj(self, oid, margin, label, weight):
        """The objectives of ``OBJ_IDS`` and the logistic family under
        scale_pos_weight: on the GPU one launch of the gradient kernel
        templated on the objective, with the root statistics; the fp32 torch
        form (:func:`obj_gpair_torch`) is its reference and the CPU path."""
        if (margin.is_cuda and margin.dtype == torch.float32 and label.dtype == torch.float32
                and (weight is None or weight.dtype == torch.float32)):
            gp, st = _native.hip().gbdt_gpair_obj(
                margin=margin.contiguous(), label=label.contiguous(),
                weight=weight.contiguous() if weight is not None else None, objective=oid,
                max_delta_step=self.max_delta_step, tweedie_variance_power=self.rho,
                huber_slope=self.delta, scale_pos_weight=self.pos_weight)
            gp._wh_stats = st
            return gp
        return obj_gpair_torch(oid, margin.float(), label.float(), weight, self.max_delta_step,
                               self.rho, self.delta, self.pos_weight)

    def _gpair_adaptive(self, margin, label, weight):
        """reg:absoluteerror: g = w sign(m - y), h = w. reg:quantileerror,
        output k: g = w (1 - alpha_k) where m_k >= y, else -w alpha_k, h = w;
        margin [K, n] -> gpair [K, n, 2] for K > 1, one launch of the
        gradient kernel per output, each with its root statistics."""
        absolute = self.name == "reg:absoluteerror"
        alphas = self._alphas("training") if not absolute else [0.5]
        K = self.n_out
        if K > 1 and (margin.dim() != 2 or margin.shape[0] != K):
            raise ValueError("reg:quantileerror margins must be [len(quantile_alpha), n]")
        gpu = (margin.is_cuda and margin.dtype == torch.float32 and label.dtype == torch.float32
               and (weight is None or weight.dtype == torch.float32))
        oid = OBJ_ABSOLUTE if absolute else OBJ_QUANTILE
        gps, sts = [], []
        for k, a in enumerate(alphas):
            mk = margin[k] if K > 1 else margin
            if gpu:
                gp, st = _native.hip().gbdt_gpair_obj(
                    margin=mk.contiguous(), label=label.contiguous(),
                    weight=weight.contiguous() if weight is not None else None, objective=oid,
                    quantile_alpha=a)
                sts.append(st)
            else:
                gp = adaptive_gpair_torch(mk.float(), label.float(), weight,
                                          None if absolute else a)
            gps.append(gp)
        if K == 1:
            gp = gps[0]
            if sts:
                gp._wh_stats = sts[0]
            return gp
        gp = torch.stack(gps)
        if sts:
            gp._wh_stats = torch.stack(sts)
        return gp

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
        if self.log_link:
            return torch.exp(margin)
        if self.name == "binary:hinge":
            return (margin > 0).to(margin.dtype)
        if self.n_out > 1:  # reg:quantileerror: n x K row-major, as multi:softprob
            return margin.t().contiguous()
        return margin

    def default_metric(self):
        if self.multi:
            return "merror"
        if self.rank:
            return "map"
        if self.adaptive:
            return "mae" if self.name == "reg:absoluteerror" else "quantile"
        if self.cox or self.aft:
            return "cox-nloglik" if self.cox else "aft-nloglik"
        own = {"count:poisson": "poisson-nloglik", "reg:gamma": "gamma-nloglik",
               "reg:tweedie": "tweedie-nloglik@%g" % self.rho, "binary:hinge": "error",
               "reg:pseudohubererror": "mphe", "reg:squaredlogerror": "rmsle"}.get(self.name)
        if own is not None:
            return own
        return "error" if self.name == "binary:logistic" else "rmse"

    @property
    def link(self):
        """How a margin becomes the prediction (a GbdtLink id of
        csrc/host/gbdt_objective.h)."""
        if self.log_link:
            return 1
        if self.name in ("binary:logistic", "reg:logistic"):
            return 2
        return 3 if self.name == "binary:hinge" else 0

    def _obj_metrics(self, parsed, margin, label, weight, bsp):
        """{name: value} of the one-launch metrics ``parsed`` = {name: (slot,
        rho)} of a set: per distinct rho (one, unless a set asks for several
        tweedie-nloglik@rho) one evaluation -- on the GPU one launch,
        ``gbdt_obj_eval`` -- and one allreduce of its sums and sum w."""
        out = {}
        rhos = sorted({rho for _, rho in parsed.values() if rho is not None}) or [None]
        for k, rho in enumerate(rhos):
            # (the metrics without a rho ride with the first one)
            names = [m for m, (_, r) in parsed.items() if r == rho or (r is None and k == 0)]
            mask = 0
            for m in names:
                mask |= 1 << parsed[m][0]
            v = obj_eval_sums(margin, label, weight, self.link, mask,
                              rho if rho is not None else self.rho, self.delta)
            bsp.allreduce(v)
            v = v.tolist()
            den = v[-1] if v[-1] > 0 else 1.0
            for m in names:
                x = v[parsed[m][0]] / den
                base = m.partition("@")[0]
                out[m] = 2.0 * x if base == "gamma-deviance" else (
                    math.sqrt(x) if base == "rmsle" else x)
        return out

    def _survival_metrics(self, names, margin, label, weight, bsp, data):
        """{name: value} of the survival metrics among ``names``. cox-nloglik:
        every rank's rows are one stratum; one allreduce of {sum loss,
        events}, nan without an event. aft-nloglik (the weighted mean) and
        interval-regression-accuracy (the unweighted share) from one
        evaluation and one allreduce of its four sums."""
        out = {}
        if "cox-nloglik" in names:
            v = cox_eval_sums(margin, label, data.cox_plan() if data is not None else None)
            bsp.allreduce(v)
            v = v.tolist()
            out["cox-nloglik"] = v[0] / v[1] if v[1] > 0 else float("nan")
        if "aft-nloglik" in names or "interval-regression-accuracy" in names:
            lower, upper = self._bounds(data)
            v = aft_eval_sums(margin, lower, upper, weight, self.aft_dist, self.aft_sigma)
            bsp.allreduce(v)
            v = v.tolist()
            out["aft-nloglik"] = v[0] / (v[1] if v[1] > 0 else 1.0)
            out["interval-regression-accuracy"] = v[2] / (v[3] if v[3] > 0 else 1.0)
        return out

    def metrics(self, names, margin, label, weight, bsp, group=None, data=None):
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
        if "quantile" in names:
            from .gbdt_quantile import pinball_sums
            alphas = self._alphas("eval_metric quantile")
            v = pinball_sums(alphas, margin, label, weight)
            bsp.allreduce(v)
            v = v.tolist()
            qv = v[0] / (len(alphas) * (v[1] if v[1] > 0 else 1.0))
            if self.n_out > 1:
                return [qv for _ in names]
            rest = [m for m in names if m != "quantile"]
            vals = iter(self.metrics(rest, margin, label, weight, bsp, group, data)
                        if rest else [])
            return [qv if m == "quantile" else next(vals) for m in names]
        if not self.multi:
            parsed = {m: parse_obj_metric(m) for m in names}
            parsed = {m: v for m, v in parsed.items() if v is not None}
            own = self._obj_metrics(parsed, margin, label, weight, bsp) if parsed else {}
            if any(m in SURVIVAL_METRICS for m in names):
                sv = self._survival_metrics(names, margin, label, weight, bsp, data)
                own.update({m: v for m, v in sv.items() if m in names})
            p = self.pred(margin) if len(own) < len(names) else None
            return [own[m] if m in own else
                    rank_metric(m, margin, label, group, bsp) if parse_rank_metric(m)
                    else eval_metric(m, p, label, weight, bsp) for m in names]
        v = multi_eval_sums(margin, label, weight)
        bsp.allreduce(v)
        v = v.tolist()
        den = v[2] if v[2] > 0 else 1.0
        return [v[0] / den if m == "merror" else v[1] / den for m in names]


def obj_gpair_torch(oid, margin, label, weight, max_delta_step=0.0, rho=1.5, delta=1.0,
                    pos_weight=1.0, alpha=0.5):
    """The gradient pairs [n, 2] of objective id ``oid`` (``OBJ_IDS``,
    ``OBJ_LOGISTIC``) in plain torch, in the margins' precision and the
    operation order of csrc/host/gbdt_objective.h: the CPU path and the
    reference of ``gbdt_gpair_obj`` (docs/bsp_apps.md "Objectives and
    max_delta_step" has the table)."""
    if oid in (OBJ_ABSOLUTE, OBJ_QUANTILE):
        return adaptive_gpair_torch(margin, label, weight, None if oid == OBJ_ABSOLUTE else alpha)
    m, y = margin, label.to(margin.dtype)
    w = weight.to(m.dtype) if weight is not None else None
    final = None  # rows whose pair the weight does not multiply
    if oid == OBJ_LOGISTIC:
        p = torch.sigmoid(m)
        g, h = p - y, torch.clamp(p * (1.0 - p), min=1e-16)
        if pos_weight != 1.0:
            s = torch.where(y == 1, torch.full_like(y, pos_weight), torch.ones_like(y))
            w = s if w is None else w * s
    elif oid == OBJ_IDS["count:poisson"]:
        g, h = torch.exp(m) - y, torch.exp(m + max_delta_step)
    elif oid == OBJ_IDS["reg:gamma"]:
        r = y / torch.exp(m)
        g, h = 1.0 - r, r
    elif oid == OBJ_IDS["reg:tweedie"]:
        c1, c2 = 1.0 - rho, 2.0 - rho
        e1, e2 = torch.exp(c1 * m), torch.exp(c2 * m)
        g, h = -y * e1 + e2, -y * c1 * e1 + c2 * e2
    elif oid == OBJ_IDS["binary:hinge"]:
        ys = 2.0 * y - 1.0
        final = ~(m * ys < 1.0)
        g = torch.where(final, torch.zeros_like(m), -ys)
        h = torch.where(final, torch.full_like(m, FLT_MIN), torch.ones_like(m))
    elif oid == OBJ_IDS["reg:pseudohubererror"]:
        z, d2 = m - y, delta * delta
        s = torch.sqrt(1.0 + z * z / d2)
        g, h = z / s, d2 / ((d2 + z * z) * s)
    elif oid == OBJ_IDS["reg:squaredlogerror"]:
        mm = torch.clamp(m, min=SQUARED_LOG_MIN_MARGIN)
        lm, ly, d = torch.log1p(mm), torch.log1p(y), mm + 1.0
        g, h = (lm - ly) / d, torch.clamp((1.0 - lm + ly) / (d * d), min=1e-6)
    else:
        raise ValueError("unknown objective id %r" % (oid,))
    if w is not None:
        gw, hw = g * w, h * w
        g, h = (gw, hw) if final is None else (torch.where(final, g, gw), torch.where(final, h, hw))
    return torch.stack([g, h], 1).float().contiguous()


class AdaptiveObjective(Objective):
    """reg:absoluteerror and reg:quantileerror: the objectives whose trees'
    leaves are refreshed after growing (``adaptive``, ``alphas``). They are a
    class of their own because the growers must be handed the residual inputs
    (:func:`grow_round` does): :class:`Objective` itself, which any builder
    can be driven with, does not take their names. :func:`make_objective`
    picks the class by name."""

    EXTRA_NAMES = ADAPTIVE_OBJECTIVES

    def __init__(self, name, num_class=0, param=None, n_out=None):
        if name not in ADAPTIVE_OBJECTIVES:
            raise ValueError("objective %s is not an adaptive one" % name)
        super().__init__(name, num_class, param, n_out=n_out)


def make_objective(name, num_class=0, param=None, n_out=None):
    """The objective of a name: an :class:`AdaptiveObjective` for
    reg:absoluteerror and reg:quantileerror, else an :class:`Objective`."""
    cls = AdaptiveObjective if name in ADAPTIVE_OBJECTIVES else Objective
    return cls(name, num_class, param, n_out=n_out)


def adaptive_gpair_torch(margin, label, weight, alpha=None):
    """The gradient pairs [n, 2] of reg:absoluteerror (alpha None) or of one
    output of reg:quantileerror in fp32 torch, in the kernel's operation
    order: d = m - y, g = sign(d) or (d >= 0 ? 1 - alpha : -alpha) with alpha
    rounded to fp32 first, h = 1, both times w."""
    m, y = margin, label.to(margin.dtype)
    d = m - y
    if alpha is None:
        g = torch.sign(d)
    else:
        a = torch.tensor(alpha, dtype=m.dtype, device=m.device)
        g = torch.where(d >= 0, 1.0 - a, -a)
    h = torch.ones_like(m)
    if weight is not None:
        w = weight.to(m.dtype)
        g, h = g * w, h * w
    return torch.stack([g, h], 1).float().contiguous()


def obj_eval_sums(margin, label, weight, link, mask, rho=1.5, delta=1.0):
    """fp64 [8]: {sum w loss_j} of this rank's rows for the ``OBJ_METRICS``
    slots j of ``mask`` (the others 0), then sum w; link: 0 the margin is the
    prediction, 1 exp, 2 sigmoid, 3 [margin > 0]. On the GPU one launch
    (``gbdt_obj_eval``: every loss in double from the fp32 inputs); the torch
    form on ``margin.double()`` is its reference and the CPU path."""
    if (margin.is_cuda and margin.dtype == torch.float32 and label.dtype == torch.float32
            and (weight is None or weight.dtype == torch.float32)):
        return _native.hip().gbdt_obj_eval(
            margin=margin.contiguous(), label=label.contiguous(),
            weight=weight.contiguous() if weight is not None else None, link=link, mask=mask,
            tweedie_variance_power=rho, huber_slope=delta)
    out = torch.zeros(len(OBJ_METRICS) + 1, dtype=torch.float64, device=margin.device)
    if label.numel() == 0:
        return out
    m, y = margin.double(), label.double()
    w = weight.double() if weight is not None else torch.ones_like(y)
    p = (m, torch.exp(m), torch.sigmoid(m), (m > 0).double())[link]
    q = p.clamp(min=1e-16)
    d2 = delta * delta
    loss = (lambda: torch.lgamma(y + 1.0) + q - y * torch.log(q),
            lambda: y / q + torch.log(q),
            lambda: torch.log((p + 1e-16) / (y + 1e-16)) + (y + 1e-16) / (p + 1e-16) - 1.0,
            lambda: -y * torch.pow(p, 1.0 - rho) / (1.0 - rho) + torch.pow(p, 2.0 - rho) / (2.0 - rho),
            lambda: (p - y).abs(),
            lambda: d2 * (torch.sqrt(1.0 + (p - y) ** 2 / d2) - 1.0),
            lambda: (torch.log1p(y) - torch.log1p(p)) ** 2)
    for j, f in enumerate(loss):
        if mask >> j & 1:
            out[j] = (w * f()).sum()
    out[-1] = w.sum()
    return out


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
