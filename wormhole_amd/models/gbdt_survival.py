"""The survival objectives of the GBDT trainer (docs/bsp_apps.md "Survival").

survival:cox -- labels y > 0 are events at time y, y <= 0 rows right-censored
at |y|. The gradient is not row-local: with t = |y|, delta = [y > 0], m* the
largest margin and e = exp(m - m*),

    D(t) = sum_{t_j >= t} e_j
    r_i = sum_{delta_k = 1, t_k <= t_i} 1 / D(t_k),  q_i likewise with 1 / D^2
    g_i = w_i (e_i r_i - delta_i),  h_i = w_i (e_i r_i - e_i^2 q_i)

(the Breslow partial likelihood; tied times share one risk set). A
:class:`CoxPlan` holds what does not change between rounds: the stable
ascending order of t, delta and the weights in that order and the tie runs.
On the GPU four launches per round (``gbdt_gpair_cox``); :func:`cox_gpair_torch`
is the CPU path and the kernels' reference form, fp64 inside.

survival:aft -- a row's interval [lower, upper] (``DMatrix.lower`` /
``upper``), a distribution and its scale sigma; row-local, one launch
(``gbdt_gpair_aft``), with :func:`aft_gpair_torch` the CPU path in the
operation order of csrc/host/gbdt_aft.h: fp64 inside, the pair rounded to fp32.
"""
import math

import torch

from .. import _native

SURVIVAL_OBJECTIVES = ("survival:cox", "survival:aft")
SURVIVAL_METRICS = ("cox-nloglik", "aft-nloglik", "interval-regression-accuracy")
AFT_DISTS = ("normal", "logistic", "extreme")  # GbdtAftDist ids
AFT_MIN_G, AFT_MAX_G, AFT_MIN_H, AFT_MAX_H = -15.0, 15.0, 1e-16, 15.0
AFT_EPS = 1e-12
AFT_MAX_Z = 700.0


def check_aft_params(p):
    """aft_loss_distribution and aft_loss_distribution_scale of ``p``
    (anything that carries them) -> (distribution id, sigma)."""
    dist = getattr(p, "aft_loss_distribution", "normal")
    if dist not in AFT_DISTS:
        raise SystemExit("aft_loss_distribution=%s: must be normal, logistic or extreme" % dist)
    sigma = getattr(p, "aft_loss_distribution_scale", 1.0)
    if not (sigma > 0 and math.isfinite(sigma)):
        raise SystemExit("aft_loss_distribution_scale=%g: must be positive" % sigma)
    return AFT_DISTS.index(dist), float(sigma)


# ---------------------------------------------------------------------- cox
class CoxPlan:
    """What survival:cox keeps of a matrix between rounds (``gbdt_cox_plan``):
    ``order`` (int32 [n]: the rows in stable ascending t), ``t``, ``delta``
    (uint8) and ``weight`` (None without instance weights) in that order,
    ``head`` / ``tail`` (int32 [n]: the first / last position of the
    position's tie run), ``run_events`` (the run's events at its head, 0
    elsewhere), ``events`` and, on the GPU, the kernels' workspace."""

    def __init__(self, label, weight=None):
        p = _native.hip().gbdt_cox_plan(label.float().contiguous(),
                                        weight.float().contiguous() if weight is not None
                                        else None)
        self.n, self.events = p["n"], p["events"]
        self.order, self.t, self.delta = p["order"], p["t"], p["delta"]
        self.weight = p["weight"] if weight is not None else None
        self.head, self.tail, self.run_events = p["head"], p["tail"], p["run_events"]
        self.ws, self.ticket = p["ws"], p["ticket"]


def _cox_scans(margin, plan):
    """fp64, in the plan's order: e, D of every position's run, r, q, m*. (A
    run whose D underflowed to 0 -- margins more than ~745 below m* -- adds
    nothing to r and q, as in the kernels.)"""
    m = margin.double()
    mstar = m.max()
    e = torch.exp(m[plan.order.long()] - mstar)
    S = torch.flip(torch.cumsum(torch.flip(e, [0]), 0), [0])
    D = S[plan.head.long()]
    d = plan.delta.double()
    tail = plan.tail.long()
    c = torch.where(D > 0, d / D, torch.zeros_like(D))
    r = torch.cumsum(c, 0)[tail]
    q = torch.cumsum(torch.where(D > 0, c / D, torch.zeros_like(D)), 0)[tail]
    return e, D, r, q, mstar


def cox_gpair_torch(margin, label, weight, plan=None):
    """The survival:cox pairs [n, 2] (fp32) in plain torch, fp64 inside: the
    CPU path and the reference form of ``gbdt_gpair_cox``. plan: the
    :class:`CoxPlan` of (label, weight), built when None."""
    n = margin.numel()
    if n == 0:
        return torch.zeros(0, 2, dtype=torch.float32, device=margin.device)
    plan = plan if plan is not None else CoxPlan(label, weight)
    e, _, r, q, _ = _cox_scans(margin, plan)
    er = e * r
    g = (er - plan.delta.double()).float()
    h = torch.clamp(er - e * e * q, min=0.0).float()
    if weight is not None:
        w = plan.weight if plan.weight is not None else weight.float()[plan.order.long()]
        g, h = g * w, h * w
    out = torch.empty(n, 2, dtype=torch.float32, device=margin.device)
    out[plan.order.long()] = torch.stack([g, h], 1)
    return out


def cox_eval_torch(margin, label, plan=None):
    """fp64 [2] = {sum over the events of ln D(t_i) - (m_i - m*), the events}
    of one stratum, in plain torch: cox-nloglik is their quotient."""
    out = torch.zeros(2, dtype=torch.float64, device=margin.device)
    if margin.numel() == 0:
        return out
    plan = plan if plan is not None else CoxPlan(label)
    _, D, _, _, mstar = _cox_scans(margin, plan)
    ev = plan.delta.bool()
    m = margin.double()[plan.order.long()]
    out[0] = torch.log(D[ev & (D > 0)]).sum() - (m[ev] - mstar).sum()
    out[1] = float(plan.events)
    return out


def _on_gpu(margin, *others):
    return margin.is_cuda and margin.dtype == torch.float32 and all(
        o is None or o.dtype == torch.float32 for o in others)


def cox_gpair(margin, label, weight, plan=None):
    """The pairs of survival:cox: on the GPU ``gbdt_gpair_cox`` (the root
    statistics ride along as ``_wh_stats``), else :func:`cox_gpair_torch`."""
    plan = plan if plan is not None else CoxPlan(label, weight)
    if _on_gpu(margin) and margin.numel():
        gp, st = _native.hip().gbdt_gpair_cox(
            margin=margin.contiguous(), order=plan.order, delta=plan.delta,
            weight=plan.weight if weight is not None else None, run_events=plan.run_events,
            ws=plan.ws, ticket=plan.ticket)
        gp._wh_stats = st
        return gp
    return cox_gpair_torch(margin.float(), label, weight, plan)


def cox_eval_sums(margin, label, plan=None):
    """{sum loss, events} of this rank's stratum (fp64 [2])."""
    plan = plan if plan is not None else CoxPlan(label)
    if _on_gpu(margin) and margin.numel():
        return _native.hip().gbdt_cox_eval(margin=margin.contiguous(), order=plan.order,
                                           delta=plan.delta, run_events=plan.run_events,
                                           ws=plan.ws, ticket=plan.ticket)
    return cox_eval_torch(margin.float(), label, plan)


# ---------------------------------------------------------------------- aft
def _mills(z):
    """(1 - Phi(z)) / phi(z) for z >= 0, through the scaled complementary
    error function."""
    return 1.2533141373155001 * torch.special.erfcx(z.clamp(min=0.0) * 0.70710678118654752)


def _normal_tail(a, b):
    """The interval in the upper tail, 0 <= a < b <= inf (aft_normal_tail)."""
    Ra, Rb = _mills(a), _mills(b)
    rho = torch.exp(-0.5 * ((b - a) * (b + a)))
    den = Ra - rho * Rb
    brho = torch.where(rho > 0, b * rho, torch.zeros_like(b))
    gs = (rho - 1.0) / den
    return gs, gs * gs - (a - brho) / den


def _aft_censored(dist, zl, zu):
    if dist == 0:
        g1, h1 = _normal_tail(zl, zu)
        g2, h2 = _normal_tail(-zu, -zl)
        c = 0.70710678118654752
        Fl, Qu = 0.5 * torch.erfc(-zl * c), 0.5 * torch.erfc(zu * c)
        den = 1.0 - Fl - Qu
        k = 0.3989422804014327
        pl, pu = k * torch.exp(-0.5 * zl * zl), k * torch.exp(-0.5 * zu * zu)
        zero = torch.zeros_like(zl)
        zpl, zpu = torch.where(pl > 0, zl * pl, zero), torch.where(pu > 0, zu * pu, zero)
        g3 = (pu - pl) / den
        h3 = g3 * g3 - (zpl - zpu) / den
        up, lo = zl >= 0, zu <= 0
        return (torch.where(up, g1, torch.where(lo, -g2, g3)),
                torch.where(up, h1, torch.where(lo, h2, h3)))
    if dist == 1:
        Fl, Sl = torch.sigmoid(zl), torch.sigmoid(-zl)
        Fu, Su = torch.sigmoid(zu), torch.sigmoid(-zu)
        return Su - Fl, Fu * Su + Fl * Sl
    wl, wu = torch.exp(zl.clamp(max=AFT_MAX_Z)), torch.exp(zu.clamp(max=AFT_MAX_Z))
    D = wu - wl
    one = torch.ones_like(D)
    pos = D > 0
    k = torch.where(pos, D / torch.expm1(D), one)
    t = torch.where(pos, D / -torch.expm1(-D), one)
    return k - wl, wl + k * (t - 1.0)


def _aft_uncensored(dist, z):
    if dist == 0:
        return -z, torch.ones_like(z)
    if dist == 1:
        F, S = torch.sigmoid(z), torch.sigmoid(-z)
        return S - F, 2.0 * (F * S)
    w = torch.exp(z.clamp(max=AFT_MAX_Z))
    return 1.0 - w, w


def aft_gpair_torch(margin, lower, upper, weight, dist=0, sigma=1.0):
    """The survival:aft pairs [n, 2] (fp32) in plain torch, in the operation
    order of csrc/host/gbdt_aft.h (fp64 from the fp32 inputs, rounded once):
    the CPU path and the reference of ``gbdt_gpair_aft``. dist: an index of
    ``AFT_DISTS``."""
    m, yl, yu = margin.float().double(), lower.float().double(), upper.float().double()
    s = float(torch.tensor(sigma, dtype=torch.float32))
    zl, zu = (torch.log(yl) - m) / s, (torch.log(yu) - m) / s
    gu, hu = _aft_uncensored(dist, zl)
    gc, hc = _aft_censored(dist, zl, zu)
    unc = yl == yu
    g = torch.where(unc, gu, gc) / s
    h = torch.where(unc, hu, hc) / (s * s)
    # (fmaxf / fminf drop a NaN; clamp would keep it)
    g = torch.nan_to_num(g, nan=AFT_MIN_G).clamp(AFT_MIN_G, AFT_MAX_G).float()
    h = torch.nan_to_num(h, nan=AFT_MIN_H).clamp(AFT_MIN_H, AFT_MAX_H).float()
    if weight is not None:
        w = weight.float()
        g, h = g * w, h * w
    return torch.stack([g, h], 1).contiguous()


def aft_loss_torch(margin, lower, upper, dist=0, sigma=1.0):
    """-ln max(likelihood, 1e-12) per row, fp64 from the inputs (gbdt_aft_loss)."""
    m, yl, yu = margin.double(), lower.double(), upper.double()
    zl, zu = (torch.log(yl) - m) / sigma, (torch.log(yu) - m) / sigma
    if dist == 0:
        c = 0.70710678118654752
        f = 0.3989422804014327 * torch.exp(-0.5 * zl * zl)
        cen = torch.where(zl >= 0, 0.5 * (torch.erfc(zl * c) - torch.erfc(zu * c)),
                          torch.where(zu <= 0, 0.5 * (torch.erfc(-zu * c) - torch.erfc(-zl * c)),
                                      1.0 - 0.5 * torch.erfc(zu * c) - 0.5 * torch.erfc(-zl * c)))
    elif dist == 1:
        f = torch.sigmoid(zl) * torch.sigmoid(-zl)
        cen = torch.sigmoid(zu) * torch.sigmoid(-zl) * -torch.expm1(-(zu - zl))
    else:
        wl, wu = torch.exp(zl), torch.exp(zu)
        zero = torch.zeros_like(wl)
        f = torch.where(wl < 1e300, wl * torch.exp(-wl), zero)
        cen = torch.where(wl < 1e300, torch.exp(-wl) * -torch.expm1(-(wu - wl)), zero)
    lik = torch.where(yl == yu, f / (sigma * yl), cen)
    return -torch.log(torch.nan_to_num(lik, nan=0.0).clamp(min=AFT_EPS))


def aft_eval_torch(margin, lower, upper, weight, dist=0, sigma=1.0):
    """fp64 [4] = {sum w nll, sum w, rows with lower <= exp(m) <= upper, rows}."""
    out = torch.zeros(4, dtype=torch.float64, device=margin.device)
    if margin.numel() == 0:
        return out
    w = weight.double() if weight is not None else torch.ones_like(margin, dtype=torch.float64)
    p = torch.exp(margin.double())
    out[0] = (w * aft_loss_torch(margin, lower, upper, dist, sigma)).sum()
    out[1] = w.sum()
    out[2] = ((lower.double() <= p) & (p <= upper.double())).sum()
    out[3] = margin.numel()
    return out


def aft_gpair(margin, lower, upper, weight, dist=0, sigma=1.0):
    """The pairs of survival:aft: on the GPU ``gbdt_gpair_aft`` (with
    ``_wh_stats``), else :func:`aft_gpair_torch`."""
    if _on_gpu(margin, lower, upper, weight) and margin.numel():
        gp, st = _native.hip().gbdt_gpair_aft(
            margin=margin.contiguous(), lower=lower.contiguous(), upper=upper.contiguous(),
            weight=weight.contiguous() if weight is not None else None, dist=dist, sigma=sigma)
        gp._wh_stats = st
        return gp
    return aft_gpair_torch(margin, lower, upper, weight, dist, sigma)


def aft_eval_sums(margin, lower, upper, weight, dist=0, sigma=1.0):
    if _on_gpu(margin, lower, upper, weight) and margin.numel():
        return _native.hip().gbdt_aft_eval(
            margin=margin.contiguous(), lower=lower.contiguous(), upper=upper.contiguous(),
            weight=weight.contiguous() if weight is not None else None, dist=dist, sigma=sigma)
    return aft_eval_torch(margin, lower, upper, weight, dist, sigma)


class SurvivalData:
    """What both matrices keep for the survival objectives: the AFT bounds
    ``lower`` / ``upper`` (float32 [n] on the matrix's device, or None) and
    the Cox plan of the labels and weights, built once per matrix on first
    use (every eval set has its own)."""

    lower = upper = None
    _cox_plan = None

    def set_bounds(self, lower, upper):
        """lower / upper: [n] tensors (any device) or None."""
        self.lower = self.upper = None
        if lower is not None:
            if lower.numel() != self.n or upper.numel() != self.n:
                raise ValueError("the bounds must have one entry per row")
            self.lower = lower.to(self.device).float().contiguous()
            self.upper = upper.to(self.device).float().contiguous()

    def cox_plan(self):
        if self._cox_plan is None:
            self._cox_plan = CoxPlan(self.label, self.weight)
        return self._cox_plan
