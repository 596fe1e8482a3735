"""Data, fp64 formulas and checks shared by the objective / max_delta_step
tests (CPU and GPU).

The formulas are the table of docs/bsp_apps.md "Objectives and
max_delta_step", written here in fp64 and independently of the package: each
returns the pair per unit of row weight together with M, the sum of the
absolute values of the formula's terms, which is the scale a rounding error is
measured against (a gradient like exp(m) - y may cancel to nearly 0 while
either term carries its own rounding error)."""
import functools

import torch

import _gbdt_monotone_cases as M

OBJECTIVES = ("count:poisson", "reg:gamma", "reg:tweedie", "binary:hinge",
              "reg:pseudohubererror", "reg:squaredlogerror")
FLT_MIN = 1.1754943508222875e-38
# what fp32 makes of the squared-log-error clamp -1 + 1e-6: the gradient
# kernel and the fp32 CPU path both clamp there
SLE_MIN32 = float(torch.tensor(-1.0 + 1e-6, dtype=torch.float32))
RHO, DELTA, POISSON_STEP = 1.5, 1.0, 0.7
METRICS = ("poisson-nloglik", "gamma-nloglik", "gamma-deviance", "tweedie-nloglik@1.5", "mae",
           "mphe", "rmsle")


def labels(name, n, g):
    """n labels that fit the objective (float32), drawn from g."""
    u = torch.rand(n, generator=g)
    if name in ("count:poisson", "reg:tweedie"):
        y = torch.floor(u * 6)  # counts 0..5, zeros included
    elif name == "reg:gamma":
        y = u * 4 + 0.05
    elif name == "binary:hinge":
        y = (u < 0.5).float()
    elif name == "reg:squaredlogerror":
        y = u * 5 - 0.9
    else:
        y = u * 8 - 4
    return y.float()


def pair64(name, m, y, d=POISSON_STEP, rho=RHO, delta=DELTA, sle_min=-1.0 + 1e-6):
    """(g, h, M_g, M_h, final) per unit weight, fp64, from fp64 margins and
    labels. final: rows whose pair the row weight does not multiply (hinge's
    satisfied rows), or None."""
    m, y = m.double(), y.double()
    one = torch.ones_like(m)
    if name == "count:poisson":
        e = torch.exp(m)
        return e - y, torch.exp(m + d), e + y.abs(), torch.exp(m + d), None
    if name == "reg:gamma":
        r = y / torch.exp(m)
        return 1 - r, r, 1 + r.abs(), r.abs(), None
    if name == "reg:tweedie":
        a, b = torch.exp((1 - rho) * m), torch.exp((2 - rho) * m)
        return (-y * a + b, -y * (1 - rho) * a + (2 - rho) * b, (y * a).abs() + b,
                (y * (1 - rho) * a).abs() + (2 - rho) * b, None)
    if name == "binary:hinge":
        ys = 2 * y - 1
        final = ~(m * ys < 1)
        return (torch.where(final, 0 * one, -ys), torch.where(final, FLT_MIN * one, one), one,
                one, final)
    if name == "reg:pseudohubererror":
        z = m - y
        s = torch.sqrt(1 + z * z / delta ** 2)
        h = delta ** 2 / ((delta ** 2 + z * z) * s)
        return z / s, h, (z / s).abs(), h, None
    if name == "reg:squaredlogerror":
        mm = m.clamp(min=sle_min)
        lm, ly, dd = torch.log1p(mm), torch.log1p(y), mm + 1
        h = (1 - lm + ly) / dd ** 2
        return ((lm - ly) / dd, h.clamp(min=1e-6), (lm.abs() + ly.abs()) / dd,
                ((1 + lm.abs() + ly.abs()) / dd ** 2).clamp(min=1e-6), None)
    raise ValueError(name)


def weighted64(name, m, y, w, **kw):
    """(gpair [n, 2], scale [n, 2]) in fp64 with the row weights applied."""
    g, h, mg, mh, final = pair64(name, m, y, **kw)
    w = w.double() if w is not None else torch.ones_like(g)
    gw, hw = g * w, h * w
    if final is not None:
        gw, hw = torch.where(final, g, gw), torch.where(final, h, hw)
    return torch.stack([gw, hw], 1), torch.stack([mg * w, mh * w], 1)


def metric64(name, p, y, w, rho=RHO, delta=DELTA):
    """A metric of METRICS in fp64 from predictions p -> (value, sum w loss,
    sum |w loss|)."""
    p, y = p.double(), y.double()
    w = w.double() if w is not None else torch.ones_like(p)
    base = name.partition("@")[0]
    q = p.clamp(min=1e-16)
    if base == "poisson-nloglik":
        loss = torch.lgamma(y + 1) + q - y * torch.log(q)
    elif base == "gamma-nloglik":
        loss = y / q + torch.log(q)
    elif base == "gamma-deviance":
        loss = torch.log((p + 1e-16) / (y + 1e-16)) + (y + 1e-16) / (p + 1e-16) - 1
    elif base == "tweedie-nloglik":
        loss = -y * p ** (1 - rho) / (1 - rho) + p ** (2 - rho) / (2 - rho)
    elif base == "mae":
        loss = (p - y).abs()
    elif base == "mphe":
        loss = delta ** 2 * (torch.sqrt(1 + (p - y) ** 2 / delta ** 2) - 1)
    elif base == "rmsle":
        loss = (torch.log1p(y) - torch.log1p(p)) ** 2
    else:
        raise ValueError(name)
    s, den = float((w * loss).sum()), float(w.sum())
    mean = s / den if den > 0 else 0.0
    val = 2 * mean if base == "gamma-deviance" else (mean ** 0.5 if base == "rmsle" else mean)
    return val, s, float((w * loss).abs().sum())


# ------------------------------------------------------------ max_delta_step
STEP = 0.5


@functools.lru_cache(maxsize=None)
def outlier_data(n=2000, f=6):
    """The monotone cases' rows with every 37th label moved by +-10: an
    unbounded tree answers an outlier with a leaf far beyond 0.5."""
    X, y = M.data(n, f)
    y = y.clone()
    y[::37] += 10.0
    y[18::37] -= 10.0
    return X, y


def largest_leaf(trees):
    return max(abs(v) for t in trees for i, v in enumerate(t.leaf) if t.feat[i] < 0)


def leaves_bounded(trees, bound):
    """Every leaf within [-bound, bound] (1e-6 relative: a leaf read back
    from a model file is the fp32 rounding of eta x the clamped weight)."""
    return largest_leaf(trees) <= bound * (1 + 1e-6)


def same_structure(a, b):
    assert a.feat == b.feat and a.cond == b.cond and a.defl == b.defl
    assert a.left == b.left and a.right == b.right


def write_libsvm(path, X, y, weight=None):
    """Rows as ``label[:weight] j:value ...`` (NaN cells left out)."""
    with open(path, "w") as f:
        for i, (row, lab) in enumerate(zip(X.tolist(), y.tolist())):
            head = "%r" % lab if weight is None else "%r:%r" % (lab, float(weight[i]))
            f.write("%s %s\n" % (head, " ".join("%d:%g" % (j, v) for j, v in enumerate(row)
                                                if v == v)))
