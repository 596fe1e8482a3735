"""bin/xgboost.dmlc: ``<conf> [name=value ...]`` -- distributed GBDT with the
xgboost CLI surface the reference drives (learn/xgboost/mushroom.hadoop.conf,
learn/xgboost/run_yarn.sh; SURVEY §2.2 "xgboost"):

tasks ``train | pred | dump | eval``; parameters booster (gbtree | dart),
rate_drop, skip_drop, one_drop, sample_type, normalize_type (booster=dart,
below), objective
(binary:logistic, binary:logitraw, reg:logistic, reg:linear,
reg:squarederror, multi:softmax, multi:softprob, rank:pairwise, rank:ndcg,
count:poisson, reg:gamma, reg:tweedie, binary:hinge, reg:pseudohubererror,
reg:squaredlogerror, reg:absoluteerror, reg:quantileerror, survival:cox,
survival:aft), quantile_alpha, aft_loss_distribution,
aft_loss_distribution_scale, num_class (the multi:
objectives: K >= 2, labels 0..K-1, K trees per round, tree t of the model
belongs to class t % K; metrics merror | mlogloss; task=pred writes n class
ids for multi:softmax, n x K row-major probabilities for multi:softprob), eta,
gamma, min_child_weight, max_depth, grow_policy, max_leaves, lambda, alpha,
base_score, max_bin,
subsample, colsample_bytree, monotone_constraints, interaction_constraints,
max_delta_step, scale_pos_weight, tweedie_variance_power, huber_slope, seed,
eval_metric, num_round, save_period,
eval_train, eval[name]=path, data, test:data, model_in, model_out, model_dir,
fmap, name_dump, name_pred, dump_stats, dsplit=row, dsparse (keep the rows CSR:
wide libsvm data; default when num_feature > 4096), nthread (ignored),
num_feature; for task=pred and task=eval ntree_limit (use the first N
boosting rounds, N x num_class trees; 0 or more than the model has: all), for
task=pred pred_margin (write the untransformed margins: n lines, or n x K
row-major for a multi: objective) and pred_leaf (write n x T row-major leaf
node ids, numbered as in task=dump; not together with pred_margin),
pred_contribs (per-feature contributions in margin space, exact TreeSHAP over
the trees' stored covers) and approx_contribs (the same by the Saabas
attribution; implies pred_contribs); neither goes with pred_margin or
pred_leaf. They write one line per row (per row and class, row-major, for a
multi: objective): ``j:value`` for every feature j with a non-zero
contribution, ascending, then ``num_feature:bias``; a line's values sum to the
row's margin (docs/bsp_apps.md "Contributions"). pred_interactions (SHAP
interaction values, the matrix of which pred_contribs is the row sums; with
none of pred_margin, pred_leaf, pred_contribs, approx_contribs) writes lines
of the same count and order: ``i:j:value`` for every non-zero cell with
i <= j, ascending by (i, j), then ``num_feature:num_feature:bias``; an
off-diagonal token is one of the pair's two equal cells, so a line's diagonal
tokens plus twice its off-diagonal tokens sum to the row's margin
(docs/bsp_apps.md "Interactions").

Monotone constraints: ``monotone_constraints=(1,0,-1)`` (task=train only)
lists -1, 0 or 1 per feature id from 0, comma-separated; the parentheses are
optional, spaces are allowed, and in a conf file the value is quoted
(``monotone_constraints = "(1,0,-1)"``). Missing trailing entries are 0; more
entries than the data has features, or any other value, ends the run with an
error. With +1 (-1) on feature j no tree's output falls (rises) when x_j
rises and the other features stay put, for rows that store x_j: in every
split on j every leaf of the left subtree is <= (>=) every leaf of the
right one. Rows missing x_j follow the splits' default directions and are
outside the guarantee. Every class's trees of a multi: objective are
constrained; the model file, task=dump, pred and eval are unchanged
(docs/bsp_apps.md "Monotone constraints").

Interaction constraints: ``interaction_constraints=[[0,1,2],[2,3,4,5]]``
(task=train only) lists groups of feature ids, which may overlap; spaces are
allowed, and in a conf file the value is quoted (``interaction_constraints =
"[[0,1],[2,3]]"``); ``[]`` is off. The root of a tree may split on any
feature; any other node may split on feature f iff one group contains f and
every feature split on above the node, so the distinct features of a
root-to-leaf path lie within one group. A feature in no group can be split on
at the root only, and the children of that root are leaves. At most 63
groups; an empty group, an id that is no non-negative integer or not below
the data's feature count, unbalanced brackets or a 64th group end the run
with an error. Composes with colsample_bytree and monotone_constraints;
every class's trees of a multi: objective are constrained (docs/bsp_apps.md
"Interaction constraints").

Objectives and max_delta_step: count:poisson, reg:gamma and reg:tweedie
predict exp(margin) (base_score > 0 enters as its logarithm), binary:hinge
predicts 0 or 1, reg:pseudohubererror and reg:squaredlogerror the margin;
labels must be >= 0 (count:poisson, reg:tweedie), > 0 (reg:gamma), 0 or 1
(binary:hinge), > -1 (reg:squaredlogerror), else the run ends with an error.
Their default metrics are poisson-nloglik, gamma-nloglik,
tweedie-nloglik@<tweedie_variance_power>, error, mphe and rmsle; these, with
gamma-deviance and mae, go with any single-output objective
(tweedie-nloglik needs its ``@rho``, rho in (1, 2)). tweedie_variance_power
(in (1, 2), default 1.5) and huber_slope (> 0, default 1) are not stored in
the model: task=eval takes them from the command line or their defaults.
max_delta_step=d (d >= 0; 0: off; 0.7 by default for count:poisson) clamps
every node's weight to [-d, d] before eta. scale_pos_weight=s (s > 0)
multiplies the weight of the rows with label 1 by s in the gradient pairs of
the logistic objectives (not in the metrics); with another objective s != 1
is an error (docs/bsp_apps.md "Objectives and max_delta_step").

Absolute and quantile error: reg:absoluteerror (metric mae) and
reg:quantileerror with ``quantile_alpha=0.5`` or a list,
``quantile_alpha=[0.1,0.5,0.9]`` (brackets optional, spaces allowed, quoted in
a conf file; every entry strictly inside (0, 1), at most 64, kept in the order
given; any other value, or reg:quantileerror at task=train without it, ends
the run with an error; other objectives ignore it). K = the number of alphas
(1 for reg:absoluteerror) takes num_class's place: K trees per round, tree t
belongs to output t % K, task=pred writes n x K row-major values. The
prediction is the margin; base_score enters as it is and is not fitted. After
a tree is grown and pruned, each leaf becomes eta x the exact weighted
alpha-quantile (lower-bound rule) of the residuals of the training rows that
reach it, over all ranks: the model does not depend on the rank count. The
alphas are not stored in the model: task=eval with the ``quantile`` metric
(the mean pinball loss over rows and alphas; reg:quantileerror only, its
default, and the only metric when K > 1) takes them from the command line.
monotone_constraints and max_delta_step > 0 are refused with either objective
(docs/bsp_apps.md "Absolute and quantile error").

DART: ``booster=dart`` (task=train) drops earlier boosting rounds before it
grows the next one. rate_drop (in [0, 1], default 0) is a round's chance of
being dropped, skip_drop (in [0, 1], default 0) a round's chance of dropping
nothing, one_drop=1 (0 | 1) drops one round when the draw chose none,
sample_type=uniform | weighted (chances in proportion to the rounds' weights),
normalize_type=tree | forest (with k dropped rounds the dropped weights are
scaled by k / (k + eta) and the new trees weigh 1 / (k + eta); forest: both
1 / (1 + eta)). An out-of-range or unknown value ends the run with an error
that names the parameter; under booster=gbtree they are accepted and ignored.
The unit of dropout is a round: the K trees of a multi: objective's round are
dropped together (xgboost drops single trees across classes). The draw
depends on seed and the round alone, so every rank drops the same rounds. A
dart model stores one weight per tree after the trees; task=pred, eval and
dump need no booster=, and task=dump prints the effective leaf values
(weight x leaf; xgboost prints the unweighted ones). model_in continues a
gbtree model with dart and a dart model with gbtree (docs/bsp_apps.md "DART").

Growth policy: ``grow_policy=depthwise`` (default) grows level by level to
max_depth; ``grow_policy=lossguide`` (task=train) grows best-first: of the open
leaves whose best split has a gain, the one with the largest gain is split
next (ties: the smaller node id), until the tree has max_leaves leaves or no
leaf can be split. max_leaves is an integer in [0, 32768], default 0 (no limit
of its own). Under lossguide max_depth=0 means no depth limit (the deepest tree
the model's consumers take: depth 62), max_depth=D > 0 never splits a node at
depth D, max_leaves=0 with max_depth=D means min(2^D, 32768) leaves, and
max_leaves=0 with max_depth=0 is an error; so are an unknown grow_policy, a
max_leaves that is no integer in range, and max_leaves > 0 under depthwise.
With max_depth=D and max_leaves >= 2^D the model equals the depth-wise one.
Neither parameter is stored in the model: task=pred, eval and dump need none
(docs/bsp_apps.md "Growth policy").

Survival: survival:cox reads a label y > 0 as an event at time y and y <= 0
as a row right-censored at |y| (labels must be finite). Its gradient is that
of the Breslow partial likelihood; rows with equal times share one risk set
(xgboost gives a tied row only the events sorted before it: without ties the
two agree). The prediction is exp(margin), the hazard ratio; base_score > 0
enters as its logarithm; the metric cox-nloglik (default, unweighted, nan for a
set without an event) goes with this objective only. With several ranks every
rank's rows are a stratum with risk sets of their own. survival:aft takes a
row's interval [lower, upper] from ``<path>.label_lower_bound`` and
``<path>.label_upper_bound`` beside data, test:data (task=eval) and every
eval[name] path (task=pred needs none): one number per line, ``inf`` allowed in
the upper file, lower finite and >= 0, upper > 0, lower <= upper; equal bounds
are an uncensored row; the libsvm label column is ignored. Missing files for a
set the objective trains on or its metrics are evaluated on, a wrong count or
a value outside those rules end the run with an error that names the file.
aft_loss_distribution=normal (default) | logistic | extreme and
aft_loss_distribution_scale=sigma > 0 (default 1) are not stored in the
model: task=eval takes them from the command line. The prediction is
exp(margin), the survival time; the metrics aft-nloglik (default; the weighted
mean of -ln max(likelihood, 1e-12)) and interval-regression-accuracy (the
unweighted share of rows with lower <= prediction <= upper) go with this
objective only (docs/bsp_apps.md "Survival").

Learning to rank: the rank: objectives and the metrics ndcg, ndcg@k, map,
map@k (each optionally with a trailing ``-``: a group without a relevant row
scores 0 instead of 1; allowed with any single-output objective) need the
rows' query groups. They come from ``<path>.group`` beside a data path (for
``data#cache`` the path before ``#``): one non-negative integer per line, a
group's row count, in file order; the counts must sum to the rows of the
data. It is looked for beside data, test:data and every eval[name] path
(task=pred needs none); the data path must then be a single file. With
several ranks a group cut by a rank boundary counts as two groups (docs/
bsp_apps.md "Ranking"). Instance weights are refused with a rank: objective.
Output: ``[r]\\t<set>-<metric>:<value>`` lines per round.
"""
import os
import sys

import torch

from .ps_app import _device
from ..utils.fs import open_uri  # noqa: E402


def _strip(v):
    v = v.strip()
    if len(v) >= 2 and v[0] == v[-1] and v[0] in "\"'":
        return v[1:-1]
    return v


def parse_args(argv):
    from .. import _native
    items = []
    if argv and argv[0] != "none" and "=" not in argv[0]:
        for key, kind, val in _native.host().parse_conf(open_uri(argv[0]).read()):
            if kind == "m":
                raise ValueError("nested messages are not valid in an xgboost conf")
            items.append((key, val))
        argv = argv[1:]
    for a in argv:
        if "=" not in a:
            raise ValueError("expected name=value, got %r" % a)
        k, v = a.split("=", 1)
        items.append((k.strip(), _strip(v)))
    return items


def main(argv):
    from .. import _native
    from ..models import gbdt as G
    from ..parallel.bsp import BSP, fault_point

    dev = _device()
    bsp = BSP(dev, job="xgboost")
    if not argv:
        bsp.tracker_print("Usage: xgboost.dmlc <conf> [name=value ...]")
        return 0
    param = G.GBDTParam()
    task, data, test_data = "train", None, None
    model_in, model_out, model_dir = None, None, "./"
    num_round, save_period, eval_train = 10, 0, 0
    fmap, name_dump, name_pred, dump_stats = None, "dump.txt", "pred.txt", 0
    num_feature = 0
    dsparse = None  # dsparse=1|0: keep the data CSR / dense (default: by width)
    ntree_limit, pred_margin, pred_leaf = 0, False, False
    pred_contribs, approx_contribs, pred_interactions = False, False, False
    evals = []
    for k, v in parse_args(argv):
        if param.set(k, v):
            continue
        if k == "task":
            task = v
        elif k == "data":
            data = v
        elif k == "test:data":
            test_data = v
        elif k.startswith("eval[") and k.endswith("]"):
            # a later setting of the same eval set (command line after the
            # conf) replaces the earlier one, like any other parameter
            evals = [(n, p) for n, p in evals if n != k[5:-1]] + [(k[5:-1], v)]
        elif k == "model_in":
            model_in = None if v == "NULL" else v
        elif k == "model_out":
            model_out = v
        elif k == "model_dir":
            model_dir = v
        elif k == "num_round":
            num_round = int(v)
        elif k == "save_period":
            save_period = int(v)
        elif k == "eval_train":
            eval_train = int(v)
        elif k == "fmap":
            fmap = v
        elif k == "name_dump":
            name_dump = v
        elif k == "name_pred":
            name_pred = v
        elif k in ("dump_stats", "with_stats"):
            dump_stats = int(v)
        elif k == "num_feature":
            num_feature = int(v)
        elif k == "dsparse":
            dsparse = bool(int(v))
        elif k == "ntree_limit":
            ntree_limit = int(v)
        elif k == "pred_margin":
            pred_margin = bool(int(v))
        elif k == "pred_leaf":
            pred_leaf = bool(int(v))
        elif k == "pred_contribs":
            pred_contribs = bool(int(v))
        elif k == "approx_contribs":
            approx_contribs = bool(int(v))
        elif k == "pred_interactions":
            pred_interactions = bool(int(v))
        elif k in ("dsplit",):
            if v not in ("row", "auto"):
                raise SystemExit("only dsplit=row is supported")
        elif k in ("nthread", "tree_method", "updater", "silent", "use_buffer"):
            pass
        else:
            bsp.tracker_print("Warning: unknown parameter %s=%s ignored" % (k, v))
    if ntree_limit < 0:
        raise SystemExit("ntree_limit must not be negative")
    if pred_leaf and pred_margin:
        raise SystemExit("pred_leaf=1 and pred_margin=1 exclude each other")
    pred_contribs = pred_contribs or approx_contribs
    if pred_contribs and (pred_leaf or pred_margin):
        raise SystemExit("pred_contribs=1 / approx_contribs=1 and pred_%s=1 exclude each other"
                         % ("leaf" if pred_leaf else "margin"))
    if pred_interactions:
        for name, on in (("pred_margin", pred_margin), ("pred_leaf", pred_leaf),
                         ("approx_contribs", approx_contribs), ("pred_contribs", pred_contribs)):
            if on:
                raise SystemExit("pred_interactions=1 and %s=1 exclude each other" % name)
    host = _native.host()

    def load(path):
        # xgboost external-memory syntax "data#name.cache": the first run parses
        # the text split and writes this rank's rows as a binary CRB page
        # (RecordIO + LZ4, the reference's compressed row block) next to the
        # cache name; later runs load the page instead of re-parsing. The
        # matrix itself is then binned into HBM (288 GB per GPU holds any
        # split this tool is pointed at).
        cache = None
        if "#" in path:
            path, cache = path.split("#", 1)
        if cache:
            cpath = "%s.r%dof%d.crb" % (cache, bsp.rank, bsp.world)
            if host.file_size(cpath) > 0:
                return host.load_split(cpath, 0, 1, "crb")
        blk = host.load_split(path, bsp.rank, bsp.world, "libsvm")
        if cache:
            keys, off, val, lab, wt = blk
            w = host.RecordIOWriter(cpath)
            n = lab.numel()
            for r0 in range(0, max(n, 1), 1 << 18):  # records stay far below 2^29 bytes
                r1 = min(n, r0 + (1 << 18))
                a, b = int(off[r0]), int(off[r1])
                w.write(host.crb_encode(keys[a:b].contiguous(), (off[r0:r1 + 1] - a).contiguous(),
                                        val[a:b].contiguous() if val is not None and val.numel() else None,
                                        lab[r0:r1].contiguous(),
                                        wt[r0:r1].contiguous() if wt is not None and wt.numel() else None))
            w.close()
        return blk

    def load_group(path, nlocal):
        """The query groups of this rank's nlocal rows of ``path`` from
        ``<path>.group`` (group sizes, one per line) -> local offsets
        [Q + 1] (int64), or None when there is no such file. Every rank holds
        a contiguous range of the file's rows, in rank order: its first
        global row comes from one allgather of the row counts, and the
        groups are intersected with its range (a group cut by the boundary
        becomes two groups, one on each rank)."""
        base = path.split("#", 1)[0]
        gpath = base + ".group"
        if host.file_size(gpath) <= 0:
            return None
        # (a data path is one file here: load() reads `path` itself, never a
        # directory or a pattern, so the sizes describe exactly its rows)
        try:
            sizes = torch.tensor([int(t) for t in open_uri(gpath).read().split()],
                                 dtype=torch.int64)
        except ValueError as e:
            raise SystemExit("%s: %s" % (gpath, e))
        if bool((sizes < 0).any()):
            raise SystemExit("%s: a negative group size" % gpath)
        counts = bsp.comm.allgather_object(int(nlocal))
        first, total = sum(counts[:bsp.rank]), sum(counts)
        if int(sizes.sum()) != total:
            raise SystemExit("%s: the group sizes sum to %d, the data has %d rows"
                             % (gpath, int(sizes.sum()), total))
        ends = (sizes.cumsum(0) - first).clamp(0, int(nlocal))
        local = torch.diff(ends, prepend=torch.zeros(1, dtype=torch.int64))
        local = local[local > 0]
        return torch.cat([torch.zeros(1, dtype=torch.int64), local.cumsum(0)])

    def load_bounds(path, nlocal):
        """survival:aft's intervals of this rank's nlocal rows of ``path``
        from ``<path>.label_lower_bound`` and ``<path>.label_upper_bound``
        (one number per line, in file order; ``inf`` is allowed in the upper
        file) -> (lower, upper) float32 [nlocal], or None when neither file
        is there. Read only where the objective is survival:aft (its metrics
        go with no other). The rank takes its slice as load_group does. A file
        without its pair, a wrong count, a NaN, a lower bound that is
        negative or not finite, an upper bound <= 0 or below its lower bound
        end the run with an error that names the file (the flag is allreduced
        before anyone raises)."""
        base = path.split("#", 1)[0]
        paths = [base + ".label_lower_bound", base + ".label_upper_bound"]
        have = [host.file_size(q) > 0 for q in paths]
        if not any(have):
            return None
        counts = bsp.comm.allgather_object(int(nlocal))
        first, total = sum(counts[:bsp.rank]), sum(counts)
        err, vals = None, []
        for q, there in zip(paths, have):
            if not there:
                err = "%s: the file is missing (the other bound file is there)" % q
                break
            try:
                v = torch.tensor([float(t) for t in open_uri(q).read().split()],
                                 dtype=torch.float64).float()
            except ValueError as e:
                err = "%s: %s" % (q, e)
                break
            if v.numel() != total:
                err = "%s: %d bounds, the data has %d rows" % (q, v.numel(), total)
                break
            if bool(torch.isnan(v).any()):
                err = "%s: a bound is NaN" % q
                break
            vals.append(v)
        if err is None:
            lo, up = vals
            if bool(((lo < 0) | ~torch.isfinite(lo)).any()):
                err = "%s: a lower bound must be finite and not negative" % paths[0]
            elif bool((up <= 0).any()):
                err = "%s: an upper bound must be positive" % paths[1]
            elif bool((lo > up).any()):
                err = "%s: an upper bound lies below its lower bound" % paths[1]
        if bsp.allreduce_scalar(1.0 if err else 0.0, "max") > 0:
            raise SystemExit(err or "a bound file was refused on another rank")
        return lo[first:first + nlocal].contiguous(), up[first:first + nlocal].contiguous()

    def check_aft_data(obj, metrics, sets):
        """What survival:aft asks of the data: sets as check_rank_data's. A
        set the objective trains on, or aft-nloglik /
        interval-regression-accuracy is evaluated on, needs its bound files."""
        want = [m for m in metrics if m in ("aft-nloglik", "interval-regression-accuracy")]
        for name, path, d, trains, evaluated in sets:
            for who, needs in (("objective " + obj.name, obj.aft and trains),
                               ("eval_metric " + (want or [""])[0], bool(want) and evaluated)):
                if needs and d.lower is None:
                    raise SystemExit("%s needs the rows' bounds: there is no %s.label_lower_bound "
                                     "(the %s data)" % (who, path.split("#", 1)[0], name))

    def check_rank_data(obj, metrics, sets):
        """What ranking asks of the data: sets = [(name, path, matrix,
        trains, evaluated)]. A set the rank objective trains on, or a rank
        metric is evaluated on, needs its group file (the same answer on
        every rank); a rank objective refuses instance weights (the flag is
        allreduced before anyone raises, so no rank is left waiting in a
        collective)."""
        want = [m for m in metrics if G.parse_rank_metric(m)]
        for name, path, d, trains, evaluated in sets:
            for who, needs in (("objective " + obj.name, obj.rank and trains),
                               ("eval_metric " + (want or [""])[0], bool(want) and evaluated)):
                if needs and d.group is None:
                    raise SystemExit("%s needs query groups: there is no %s.group (the %s data)"
                                     % (who, path.split("#", 1)[0], name))
            if obj.rank and trains and bsp.allreduce_scalar(
                    1.0 if d.weight is not None else 0.0, "max") > 0:
                raise ValueError("instance weights are not defined for objective " + obj.name)

    if task == "dump":
        if bsp.rank == 0:
            b = G.Booster.load(model_in, param)
            fm = G.load_fmap(fmap) if fmap else None
            with open_uri(name_dump, "w") as f:
                f.write(b.dump(fm, bool(dump_stats)))
        bsp.finalize()
        return 0

    if task in ("pred", "eval"):
        b = G.Booster.load(model_in, param)
        path = test_data or data
        raw = load(path)
        group = load_group(path, raw[3].numel()) if task == "eval" else None
        bounds = load_bounds(path, raw[3].numel()) if task == "eval" and b.obj.aft else None
        dm = G.make_dmatrix(*raw, ncol=b.num_feature, device=dev, sparse=dsparse, group=group,
                            bounds=bounds)
        # ntree_limit counts boosting rounds (K trees each); 0 or more than
        # the model has: every tree
        limit = ntree_limit * b.obj.n_group
        if task == "eval":
            margin = b.predict_margin(dm, limit)
            metrics = param.eval_metric or [b.obj.default_metric()]
            b.obj.check_metrics(metrics)
            check_rank_data(b.obj, metrics, [("test", path, dm, False, True)])
            check_aft_data(b.obj, metrics, [("test", path, dm, False, True)])
            b.obj.check_labels(dm.label, bsp)
            vals = b.obj.metrics(metrics, margin, dm.label, dm.weight, bsp, dm.rank_groups(),
                                 data=dm)
            s = "".join("\ttest-%s:%f" % (m, v) for m, v in zip(metrics, vals))
            bsp.tracker_print(s.lstrip("\t"))
        else:
            # one value per line: n class ids (multi:softmax), n x K row-major
            # probabilities (multi:softprob), else n predictions; pred_margin:
            # the untransformed margins, n or n x K row-major; pred_leaf: the
            # n x T row-major node ids (the dump's numbering) of the leaves
            fmt = "%d\n" if pred_leaf else "%g\n"
            lines = pred_contribs or pred_interactions
            if pred_interactions:
                fmt = "%s\n"
                pred = _interaction_lines(b, dm, limit)
            elif pred_contribs:
                fmt = "%s\n"
                pred = _contrib_lines(b, dm, limit, approx_contribs)
            elif pred_leaf:
                pred = b.predict_leaf(dm, limit)
            else:
                margin = b.predict_margin(dm, limit)
                if pred_margin:
                    pred = margin if margin.dim() == 1 else margin.t()
                else:
                    pred = b.obj.pred(margin).float()
            if not lines:
                pred = pred.cpu().reshape(-1).tolist()
            parts = bsp.comm.allgather_object(pred)
            if bsp.rank == 0:
                with open_uri(name_pred, "w") as f:
                    for part in parts:
                        f.write("".join(fmt % p for p in part))
        bsp.finalize()
        return 0

    if task != "train":
        raise SystemExit("unknown task " + task)
    if data is None:
        raise SystemExit("need data=<path> for task=train")
    # (the same answer on every rank, before the first collective: the alphas
    # were validated as they were parsed; here their absence and what an
    # adaptive objective refuses)
    if param.objective in G.ADAPTIVE_OBJECTIVES and not model_in:
        G.make_objective(param.objective, 0, param).check_combination(param)
    param.leaf_limits()  # (grow_policy / max_leaves / max_depth: what is refused)
    train_raw = load(data)
    eval_raw = [(name, load(path)) for name, path in evals]
    ncol = max([int(r[0].max().item()) + 1 if r[0].numel() else 0
                for r in [train_raw] + [e[1] for e in eval_raw]] + [num_feature])
    ncol = int(bsp.allreduce_scalar(ncol, "max", torch.int64))
    # (the same answer on every rank, before any further collective)
    param.monotone_vector(ncol)
    param.interaction_vector(ncol)
    dtrain = G.make_dmatrix(*train_raw, ncol=ncol, device=dev, sparse=dsparse,
                            group=load_group(data, train_raw[3].numel()))
    deval = [(name, G.make_dmatrix(*r, ncol=ncol, device=dev, sparse=dsparse,
                                   group=load_group(path, r[3].numel())))
             for (name, r), (_, path) in zip(eval_raw, evals)]
    booster = G.Booster.load(model_in, param) if model_in else G.Booster(param, ncol)
    version, gstate, _ = bsp.load_checkpoint()
    if version > 0:
        booster = _booster_from_state(G, gstate, param)
    obj = booster.obj
    obj.check_combination(param)
    if obj.adaptive:  # (a continued model: as many alphas as it has outputs)
        obj._alphas("training")
    K = obj.n_group  # trees per round: tree t of the flat list belongs to class t % K
    start = len(booster.trees) // K
    if version > 0:
        print("restart from version=%d (round %d)" % (version, start), flush=True)
    metrics = param.eval_metric or [obj.default_metric()]
    obj.check_metrics(metrics)
    sets = [("train", data, dtrain, True, bool(eval_train))] + [
        (name, path, d, False, True) for (name, d), (_, path) in zip(deval, evals)]
    if obj.aft:  # (the objective is known only now: a continued model brings its own)
        for _, path, d, _, _ in sets:
            d.set_bounds(*(load_bounds(path, d.n) or (None, None)))
    check_rank_data(obj, metrics, sets)
    check_aft_data(obj, metrics, sets)
    for d in [dtrain] + [d for _, d in deval]:
        obj.check_labels(d.label, bsp)
    margin = booster.predict_margin(dtrain)
    # hessian-weighted sketch: weights at the starting margin (multi-class:
    # the row's hessians summed over the classes)
    hess = None
    if dtrain.n:
        hess = obj.gpair(margin, dtrain.label, None, dtrain.rank_groups(),
                         pos_weight=False, data=dtrain)[..., 1]
        hess = hess.sum(0) if K > 1 else hess
    cuts = G.Cuts.build(dtrain, param.max_bin, bsp, hess=hess)
    B = cuts.bin(dtrain)
    builder = G.make_builder(param, bsp, dtrain, cuts, B)
    emargins = [booster.predict_margin(d) for _, d in deval]
    dart = None
    if param.booster == "dart":
        dart = G.DartTrainer(booster, builder, dtrain, [(d, em) for (_, d), em in
                                                        zip(deval, emargins)])
        if start:  # (a continued dart model: its kept margins, replayed)
            margin = dart.start_margin()
    gen = torch.Generator().manual_seed(param.seed + 17 * bsp.rank)
    fgen = torch.Generator().manual_seed(param.seed)
    for r in range(start, num_round):
        if dart is not None:  # (appends the trees, updates the eval margins)
            new = dart.round(r, margin, gen, fgen)
        else:
            new = G.boost_round(obj, builder, dtrain, margin, gen, fgen)  # K trees
            booster.trees += new
        msg = "[%d]" % r
        for (name, d), em in zip(deval, emargins):
            if dart is None:
                for k, tree in enumerate(new):
                    d.predict_tree(tree, em[k] if K > 1 else em)
            for m, v in zip(metrics, obj.metrics(metrics, em, d.label, d.weight, bsp,
                                                 d.rank_groups(), data=d)):
                msg += "\t%s-%s:%f" % (name, m, v)
        if eval_train:
            for m, v in zip(metrics, obj.metrics(metrics, margin, dtrain.label, dtrain.weight,
                                                 bsp, dtrain.rank_groups(), data=dtrain)):
                msg += "\ttrain-%s:%f" % (m, v)
        bsp.tracker_print(msg)
        if save_period and (r + 1) % save_period == 0 and bsp.rank == 0:
            booster.save(os.path.join(model_dir, "%04d.model" % (r + 1)))
        v = bsp.checkpoint(_booster_state(booster))
        fault_point(bsp.rank, v)
    if bsp.rank == 0:
        out = model_out or os.path.join(model_dir, "%04d.model" % num_round)
        booster.save(out)
    bsp.finalize()
    return 0


# bytes of a row block's compact contributions [K, rows, U + 1] (fp32)
CONTRIB_BLOCK_BYTES = 256 << 20


def _contrib_lines(b, dm, limit, approx):
    """The pred_contribs lines of a matrix, n x K of them, row-major:
    ``j:%g`` for the non-zero columns, ascending, then ``num_feature:%g``,
    the bias. Computed in row blocks whose compact contributions stay under
    CONTRIB_BLOCK_BYTES."""
    K, F, lines = b.obj.n_group, b.num_feature, []
    ntree = min(limit, len(b.trees)) if limit else len(b.trees)
    U = len({f for t in b.trees[:ntree] for f in t.feat if f >= 0})
    block = max(1, CONTRIB_BLOCK_BYTES // (4 * K * (U + 1)))
    for a in range(0, dm.n, block):
        phi, used = b.predict_contribs(dm, limit, approx=approx, compact=True,
                                       rows=(a, min(dm.n, a + block)))
        phi = (phi if K > 1 else phi[None]).transpose(0, 1).cpu().double().numpy()
        cols = used.tolist()
        for row in phi.reshape(-1, phi.shape[-1]):
            toks = ["%d:%g" % (cols[j], row[j]) for j in row[:-1].nonzero()[0]]
            lines.append(" ".join(toks + ["%d:%g" % (F, row[-1])]))
    return lines


def _interaction_lines(b, dm, limit):
    """The pred_interactions lines of a matrix, n x K of them, row-major:
    ``i:j:%g`` for the non-zero cells with i <= j, ascending by (i, j), then
    ``num_feature:num_feature:%g``, the bias. Computed in row blocks whose
    compact matrices stay under CONTRIB_BLOCK_BYTES."""
    K, F, lines = b.obj.n_group, b.num_feature, []
    ntree = min(limit, len(b.trees)) if limit else len(b.trees)
    U = len({f for t in b.trees[:ntree] for f in t.feat if f >= 0})
    block = max(1, CONTRIB_BLOCK_BYTES // (4 * K * (U + 1) ** 2))
    for a in range(0, dm.n, block):
        phi, used = b.predict_interactions(dm, limit, compact=True,
                                           rows=(a, min(dm.n, a + block)))
        phi = (phi if K > 1 else phi[None]).transpose(0, 1).cpu().double().numpy()
        cols = used.tolist()
        for mat in phi.reshape(-1, U + 1, U + 1):
            toks = ["%d:%d:%g" % (cols[i], cols[j], mat[i, j])
                    for i, j in zip(*mat[:U, :U].nonzero()) if i <= j]
            lines.append(" ".join(toks + ["%d:%d:%g" % (F, F, mat[U, U])]))
    return lines


def _booster_state(b):
    trees = []
    for t in b.trees:
        trees.append({k: torch.tensor(getattr(t, k), dtype=torch.float64)
                      for k in ("feat", "cond", "left", "right", "defl", "leaf", "gain", "cover")})
    state = {"num_feature": b.num_feature, "num_class": b.param.num_class, "trees": trees}
    if b.weighted():  # (booster=dart: the trees' weights; none: all 1)
        state["tree_w"] = torch.tensor(b.weights(), dtype=torch.float64)
    return state


def _booster_from_state(G, s, param):
    param.num_class = int(s.get("num_class", param.num_class))
    b = G.Booster(param, int(s["num_feature"]))
    for d in s["trees"]:
        t = G.RegTree()
        n = d["feat"].numel()
        for k in ("feat", "left", "right", "defl"):
            setattr(t, k, [int(x) for x in d[k].tolist()])
        for k in ("cond", "leaf", "gain", "cover"):
            setattr(t, k, [float(x) for x in d[k].tolist()])
        t.parent = [-1] * n
        t.bin = [0] * n
        t.base_weight = [0.0] * n
        b.trees.append(t)
    if "tree_w" in s:
        b.tree_w = [float(x) for x in s["tree_w"].tolist()]
    return b


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
