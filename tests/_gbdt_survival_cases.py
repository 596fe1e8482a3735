"""Data, fp64 oracles and bounds shared by the survival tests (CPU and GPU).

The oracles are written in fp64 and independently of the package.

survival:cox -- g is ``torch.autograd`` on the Breslow negative partial
log-likelihood L = -sum_{delta_i = 1} (m_i - ln sum_{t_j >= t_i} exp m_j); the
Hessian's diagonal is the closed form h_i = e_i r_i - e_i^2 q_i (a second
autograd pass confirms it at small n, tests/test_gbdt_survival.py). The error
scale is M_g = e r + delta, M_h = e r + e^2 q, the sums of the absolute values
of the formulas' terms. Bound: |err| <= 2^-22 w M. The package keeps e, D, r, q
in fp64 (together below 1e-9 M at these sizes), rounds g and h to fp32 once
(2^-24 M) and multiplies by w in fp32 (2^-24 more); 2^-22 leaves a factor 2.

survival:aft -- ``torch.autograd`` on the loss written in log space
(log_ndtr, logsigmoid, log1p / expm1), then xgboost's clamps. The error scale
M is the sum of the absolute values of the terms of the pair's closed form
(:func:`aft_scale`). Bound: |err| <= 2^-22 w M (``AFT_BOUND``, derived there)."""
import functools
import math

import torch

DISTS = ("normal", "logistic", "extreme")
KINDS = ("uncensored", "right", "left", "interval")
SIGMAS = (0.5, 1.0, 2.0)
COX_BOUND = 2.0 ** -22
MIN_G, MAX_G, MIN_H, MAX_H = -15.0, 15.0, 1e-16, 15.0


# ---------------------------------------------------------------------- cox
def cox_inputs(n, weighted, times=7, events="mixed", seed=0):
    """(margin, label, weight): times drawn from ``times`` distinct values
    (ties everywhere; 0: every row its own time), margins in [-3, 3]."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + weighted)
    margin = torch.rand(n, generator=g) * 6 - 3
    if times:
        t = torch.randint(1, times + 1, (n,), generator=g).float()
    else:
        t = (torch.randperm(n, generator=g) + 1).float() * 0.25
    ev = {"mixed": torch.rand(n, generator=g) < 0.6, "all": torch.ones(n, dtype=torch.bool),
          "none": torch.zeros(n, dtype=torch.bool)}[events]
    label = torch.where(ev, t, -t)
    weight = torch.rand(n, generator=g) * 1.5 + 0.5 if weighted else None
    return margin.float(), label.float(), weight


def cox_oracle(margin, label, weight=None):
    """(gpair [n, 2], scale [n, 2], loss sum, events) in fp64, the weights
    applied: g by autograd on L, h by the closed form."""
    m = margin.double().clone().requires_grad_(True)
    t, ev = label.double().abs(), label > 0
    n = m.numel()
    w = weight.double() if weight is not None else torch.ones(n, dtype=torch.float64)
    if n == 0:
        z = torch.zeros(0, 2, dtype=torch.float64)
        return z, z, 0.0, 0
    u, inv = torch.unique(t, sorted=True, return_inverse=True)
    top = m.max().detach()
    e = torch.exp(m - top)
    per_time = torch.zeros(u.numel(), dtype=torch.float64).index_add(0, inv, e)
    D = torch.flip(torch.cumsum(torch.flip(per_time, [0]), 0), [0])  # t_j >= u
    L = -((m - top - torch.log(D[inv]))[ev]).sum()
    g = torch.autograd.grad(L, m)[0] if bool(ev.any()) else torch.zeros(n, dtype=torch.float64)
    with torch.no_grad():
        nev = torch.zeros(u.numel(), dtype=torch.float64).index_add(0, inv, ev.double())
        r = torch.cumsum(nev / D, 0)[inv]
        q = torch.cumsum(nev / (D * D), 0)[inv]
        er, eeq = e * r, e * e * q
        h = er - eeq
        scale = torch.stack([(er + ev.double()) * w, (er + eeq) * w], 1)
        pair = torch.stack([g * w, h * w], 1)
    return pair, scale.detach(), float(L.detach()), int(ev.sum())


def cox_hess_autograd(margin, label):
    """The Hessian's diagonal by a second autograd pass (small n)."""
    m = margin.double().clone().requires_grad_(True)
    t, ev = label.double().abs(), label > 0
    risk = (t[None, :] >= t[:, None]).double()
    L = -((m - torch.log((risk * torch.exp(m)[None, :]).sum(1)))[ev]).sum()
    g = torch.autograd.grad(L, m, create_graph=True)[0]
    return torch.stack([torch.autograd.grad(g[i], m, retain_graph=True)[0][i]
                        for i in range(m.numel())]).detach()


def cox_xgboost_loop(margin, label, weight=None):
    """xgboost's sequential Cox gradient loop, transcribed in fp64: the rows
    in ascending |y|, the denominator updated only when the time moves
    forward, r and s accumulated row by row -- so a tied row sees only the
    events sorted before it."""
    p, y = margin.double().tolist(), label.double().tolist()
    n = len(p)
    w = weight.double().tolist() if weight is not None else [1.0] * n
    order = sorted(range(n), key=lambda i: abs(y[i]))  # (stable)
    exp_p_sum = sum(math.exp(p[i]) for i in order)
    out = torch.zeros(n, 2, dtype=torch.float64)
    r_k = s_k = last_exp_p = last_abs_y = accumulated = 0.0
    for ind in order:
        exp_p, abs_y = math.exp(p[ind]), abs(y[ind])
        accumulated += last_exp_p
        if last_abs_y < abs_y:
            exp_p_sum -= accumulated
            accumulated = 0.0
        if y[ind] > 0:
            r_k += 1.0 / exp_p_sum
            s_k += 1.0 / (exp_p_sum * exp_p_sum)
        out[ind, 0] = (exp_p * r_k - (1.0 if y[ind] > 0 else 0.0)) * w[ind]
        out[ind, 1] = (exp_p * r_k - exp_p * exp_p * s_k) * w[ind]
        last_abs_y, last_exp_p = abs_y, exp_p
    return out


def cox_tie_inputs(n, spans):
    """n rows, every row its own time except tie runs laid over sorted
    positions [a, b] for (a, b) in spans; the rows are shuffled, so the order
    in memory is not the sorted one. (margin, label, None)."""
    g = torch.Generator().manual_seed(n)
    t = torch.arange(1, n + 1).float()
    for a, b in spans:
        t[a:b + 1] = t[a]
    ev = torch.rand(n, generator=g) < 0.6
    perm = torch.randperm(n, generator=g)
    label = torch.where(ev, t, -t)[perm]
    margin = (torch.rand(n, generator=g) * 4 - 2)
    return margin.float(), label.float(), None


# ---------------------------------------------------------------------- aft
def _log1mexp(x):
    """ln(1 - e^-x) for x > 0, by the branch that keeps its digits (expm1 for
    small x, log1p for large x, where 1 - e^-x rounds to 1)."""
    return torch.where(x <= math.log(2.0), torch.log(-torch.expm1(-x)),
                       torch.log1p(-torch.exp(-x)))


def _log_cdf_diff(dist, zl, zu):
    """ln(F(zu) - F(zl)) for finite zl < zu, in log space, taken in the tail
    that holds the interval's middle."""
    if dist == "extreme":
        wl, wu = torch.exp(zl), torch.exp(zu)
        return -wl + _log1mexp(wu - wl)
    lf = torch.special.log_ndtr if dist == "normal" else torch.nn.functional.logsigmoid
    upper = zl + zu > 0  # F(zu) - F(zl) = F(-zl) - F(-zu) for both symmetric laws
    a = torch.where(upper, -zu, zl)
    b = torch.where(upper, -zl, zu)
    return lf(b) + torch.log1p(-torch.exp(lf(a) - lf(b)))


def _aft_loss(dist, kind, m, yl, yu, sigma):
    zl = (torch.log(yl) - m) / sigma if kind != "left" else None
    zu = (torch.log(yu) - m) / sigma if kind in ("left", "interval") else None
    if kind == "uncensored":
        logf = {"normal": -0.5 * zl * zl - 0.5 * math.log(2 * math.pi),
                "logistic": torch.nn.functional.logsigmoid(zl) + torch.nn.functional.logsigmoid(-zl),
                "extreme": zl - torch.exp(zl)}[dist]
        return -(logf - torch.log(sigma * yl))
    if kind == "right":  # ln(1 - F(zl))
        return -{"normal": torch.special.log_ndtr(-zl),
                 "logistic": torch.nn.functional.logsigmoid(-zl),
                 "extreme": -torch.exp(zl)}[dist]
    if kind == "left":  # ln F(zu)
        return -{"normal": torch.special.log_ndtr(zu),
                 "logistic": torch.nn.functional.logsigmoid(zu),
                 "extreme": _log1mexp(torch.exp(zu))}[dist]
    return -_log_cdf_diff(dist, zl, zu)


def aft_kind(lower, upper):
    return ["uncensored" if a == b else "right" if math.isinf(b) else "left" if a == 0
            else "interval" for a, b in zip(lower.tolist(), upper.tolist())]


def aft_oracle(dist, margin, lower, upper, sigma, weight=None):
    """(gpair [n, 2] clamped, raw [n, 2] unclamped, loss [n]) in fp64 by
    autograd, row kind by row kind; the weights applied to gpair."""
    n = margin.numel()
    raw = torch.zeros(n, 2, dtype=torch.float64)
    loss = torch.zeros(n, dtype=torch.float64)
    kinds = aft_kind(lower, upper)
    for kind in KINDS:
        idx = torch.tensor([i for i, k in enumerate(kinds) if k == kind], dtype=torch.long)
        if not idx.numel():
            continue
        m = margin.double()[idx].clone().requires_grad_(True)
        ell = _aft_loss(dist, kind, m, lower.double()[idx], upper.double()[idx], sigma)
        g = torch.autograd.grad(ell.sum(), m, create_graph=True)[0]
        h = torch.autograd.grad(g.sum(), m)[0]
        raw[idx, 0], raw[idx, 1], loss[idx] = g.detach(), h.detach(), ell.detach()
    pair = torch.stack([raw[:, 0].clamp(MIN_G, MAX_G), raw[:, 1].clamp(MIN_H, MAX_H)], 1)
    if weight is not None:
        pair = pair * weight.double()[:, None]
    return pair, raw, loss


def _aft_density(dist, z):
    """(f, |f'|) of the law at z in fp64 (0 at +-inf)."""
    fin = torch.isfinite(z)
    zz = torch.where(fin, z, torch.zeros_like(z))
    if dist == "normal":
        f = torch.exp(-0.5 * zz * zz) / math.sqrt(2 * math.pi)
        d = zz.abs() * f
    elif dist == "logistic":
        F = torch.sigmoid(zz)
        f = F * torch.sigmoid(-zz)
        d = f * (1 - 2 * F).abs()
    else:
        w = torch.exp(zz)
        f = w * torch.exp(-w)
        d = f * (1 - w).abs()
    zero = torch.zeros_like(z)
    return torch.where(fin, f, zero), torch.where(fin, d, zero)


def aft_scale(dist, margin, lower, upper, sigma, raw, loss, weight=None):
    """The error scale M [n, 2] of the pair: the sum of the absolute values
    of the terms of its closed form, as tests/_gbdt_objective_cases.py
    defines M, in fp64. An uncensored row: normal g = -(ln y - m) / s^2,
    h = 1 / s^2 give (|ln y| + |m|) / s^2 and 1 / s^2; logistic g = (1 - 2 F) / s,
    h = 2 f / s^2 give (1 + 2 F) / s and h; extreme g = (1 - e^z) / s,
    h = e^z / s^2 give (1 + e^z) / s and h. A censored row, any law:
    g = (f_u - f_l) / (s D), h = g^2 - (f'_u - f'_l) / (s^2 D) with
    D = F(z_u) - F(z_l) give (f_u + f_l) / (s D) and g^2 + (|f'_u| + |f'_l|) /
    (s^2 D); D = exp(-loss) comes from the oracle's log-space loss. Where the
    clamped pair is larger than M (a hessian held at 1e-16), it is the scale.
    raw, loss: the oracle's unclamped pair and loss."""
    m, s = margin.double(), sigma
    yl, yu = lower.double(), upper.double()
    unc = yl == yu
    ly = torch.log(torch.where(yl > 0, yl, torch.ones_like(yl)))
    zl = torch.where(yl > 0, (ly - m) / s, torch.full_like(m, -float("inf")))
    zu = (torch.log(yu) - m) / s
    if dist == "normal":
        ug, uh = (ly.abs() + m.abs()) / s ** 2, torch.full_like(m, 1 / s ** 2)
    elif dist == "logistic":
        ug, uh = (1 + 2 * torch.sigmoid(zl)) / s, raw[:, 1].abs()
    else:
        ug, uh = (1 + torch.exp(zl)) / s, raw[:, 1].abs()
    (fl, dl), (fu, du) = _aft_density(dist, zl), _aft_density(dist, zu)
    D = torch.exp(-loss)
    cg = (fu + fl) / (s * D)
    ch = raw[:, 0] ** 2 + (du + dl) / (s ** 2 * D)
    scale = torch.stack([torch.where(unc, ug, cg), torch.where(unc, uh, ch)], 1)
    clamped = torch.stack([raw[:, 0].clamp(MIN_G, MAX_G), raw[:, 1].clamp(MIN_H, MAX_H)], 1)
    scale = torch.maximum(scale, clamped.abs())
    if weight is not None:
        scale = scale * weight.double()[:, None]
    return scale


# The bound of the pair: |err| <= AFT_BOUND w M + AFT_TINY. The package
# evaluates the forms in fp64 from the fp32 inputs (below 1e-12 M), rounds g and
# h to fp32 once (2^-24 M) and multiplies by w in fp32 (2^-24 more): 2^-23, and
# 2^-22 leaves a factor 2. AFT_TINY is fp32's subnormal spacing times the
# largest weight of the cases (2): a pair below it is 0 in fp32.
AFT_BOUND = 2.0 ** -22
AFT_TINY = 2.0 ** -148


def aft_rel_err(got, ref, scale):
    """|err| / (w M) per element, beyond what fp32's underflow takes."""
    return ((got.double() - ref).abs() - AFT_TINY).clamp(min=0.0) / scale


@functools.lru_cache(maxsize=None)
def aft_inputs(dist, kind, sigma, n=257, weighted=False):
    """(margin, lower, upper, weight): |z| <= 6 at both ends, interval rows
    with upper / lower >= 1.5."""
    g = torch.Generator().manual_seed(DISTS.index(dist) * 100 + KINDS.index(kind) * 10
                                      + int(sigma * 4) + weighted)
    yl = torch.exp(torch.rand(n, generator=g) * 4 - 2).float()
    if kind == "uncensored":
        yu = yl.clone()
    elif kind == "right":
        yu = torch.full((n,), float("inf"))
    elif kind == "left":
        yu, yl = yl, torch.zeros(n)
    else:
        yu = (yl * (1.5 + torch.rand(n, generator=g) * 3)).float()
    lo_end = torch.log(yl.double()) if kind != "left" else torch.log(yu.double())
    hi_end = torch.log(yu.double()) if kind in ("left", "interval") else lo_end
    # z in [-6, 6] at both ends: m in [hi_end - 6 sigma, lo_end + 6 sigma]
    a, b = hi_end - 6 * sigma, lo_end + 6 * sigma
    margin = (a + (b - a) * torch.rand(n, generator=g).double()).float()
    # (the fp32 rounding of m may carry an end a hair past 6: pull back in)
    margin = torch.minimum(torch.maximum(margin.double(), a + 1e-4), b - 1e-4).float()
    weight = torch.rand(n, generator=g) * 1.5 + 0.5 if weighted else None
    return margin, yl, yu, weight


def aft_tail_inputs():
    """Rows with |z| up to 40, upper = inf or lower = 0 among them:
    (margin, lower, upper); sigma = 1."""
    z = torch.tensor([-40.0, -25.0, -12.0, -8.0, 8.0, 12.0, 25.0, 40.0])
    rows = []
    for zz in z.tolist():
        y = 2.0
        m = math.log(y) - zz
        rows += [(m, y, y), (m, y, float("inf")), (m, 0.0, y), (m, y, 3.0 * y)]
    t = torch.tensor(rows, dtype=torch.float64)
    return t[:, 0].float(), t[:, 1].float(), t[:, 2].float()


def write_libsvm(path, X, y):
    with open(path, "w") as f:
        for row, lab in zip(X.tolist(), y.tolist()):
            f.write("%g %s\n" % (lab, " ".join("%d:%g" % (j, v) for j, v in enumerate(row))))


def survival_rows(n=400, seed=5):
    """n rows, 4 features, the hazard driven by feature 0: (X, time, event)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, 4, generator=g)
    rate = torch.exp(2.0 * (X[:, 0] - 0.5))
    t = -torch.log(torch.rand(n, generator=g).clamp(min=1e-6)) / rate
    t = (t * 8).ceil() / 8  # (ties)
    event = torch.rand(n, generator=g) < 0.7
    return X, t.float(), event
