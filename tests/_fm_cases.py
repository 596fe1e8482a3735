"""Inputs, float64 references and derived error bounds for the FM / linear
forward and backward kernels (csrc/hip/fm.hip), shared by
test_fm_reference.py (CPU), test_fm_kernels_gpu.py and _fm_det_check.py.

The references follow ops/ref.py:fm_forward / fm_backward term by term in
float64 and return, with every value, the standard summation bound
gamma_n * sum|terms| (u = 2**-24), which holds for ANY order of an fp32
sum of those terms (atomics, butterflies, FMA contraction):

  forward, row with n non-zeros:
    W = sum|x_i w_i|, A_d = sum|x_i V_id|, Q_d = sum x_i^2 V_id^2
    bound_xv[d] = (n + 8) u A_d
    bound_py    = (n + 16) u (W + sum_d (A_d^2 + Q_d))
  backward, key with c occurrences, dx_j = dual_r x_j:
    bound_gw    = (c + 8) u sum|dx_j|
    bound_gV[d] = (c + 8) u (sum|dx_j xv_rd| + sum|dx_j x_j| |V_kd|)

A result passes when |got - ref64| <= 2 * bound (the factor covers the extra
roundings of the tree / shuffle stages); where the bound is 0 (an empty row,
a row without an embedded id, a padding column) it must match exactly.

Underflow: gamma_n * sum|terms| assumes that no product underflows. A
saturated logit dual is ~1e-38 and smaller, and dual * x * xv is then
subnormal: fp32 rounds it to a multiple of 2**-149, or flushes it to zero
where an instruction does not keep subnormals (float atomics), so each
operation may err by up to the smallest normal number 2**-126 however small
its terms are. (Measured: gV entries of 1e-40..1e-41 off by 1..9 units of
2**-149, 2.5..65 times the relative bound.) Every non-zero bound therefore
carries the absolute term (n + 8) * 2**-126 (~1e-37 per term).

Importable without a GPU: the GPU drivers below take the loaded native
module and the device as arguments.
"""
import types

import numpy as np
import torch

from wormhole_amd.ops import ref

U24 = 2.0 ** -24
TINY = 2.0 ** -126  # smallest normal fp32: the most one underflowing operation can lose
FACTOR = 2.0
SPECIAL_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 500)
N_SPECIAL = 20  # rows of each special length
EMPTY_RUN = (1000, 1070)  # more than one whole 64-row block of empty rows
DEEP_ROWS = 45000
EDGE_ROWS = 3000
# persistent grids: at most 2048 blocks of 4 waves, one row / chunk at a time
MAX_WAVES = 2048 * 4
BUCKET_BYTES = 2 << 20  # fm_backward buckets its V chunks above this much xv

_ID_HOT_A, _ID_HOT_B = 500_000, 500_001
_ID_SCALAR_ROW, _ID_EMBED_ROW = 600_000, 700_000

# largest |err| / bound seen per checked quantity (reported by the tests)
RATIOS = {}


def _key_of(ids):
    """Feature id -> int64 key (the mapping of test_kernels_gpu._rand_batch)."""
    k = np.atleast_1d(np.asarray(ids, dtype=np.uint64)) * np.uint64(0x9E3779B97F4A7C15)
    return ((k & np.uint64((1 << 62) - 1)) + np.uint64(7)).astype(np.int64)


def make_batch(nrows, seed, with_val, base_max=7):
    """A CSR minibatch with empty rows, long rows and two planted hot keys.

    Row lengths: uniform 1..base_max, 5 % empty, rows 0, 1000..1069 and the
    last one empty, N_SPECIAL rows of every length in SPECIAL_LENS at random
    positions. Ids: 75 % uniform over 400 000 keys, 25 % power-law over 2000,
    then ~8 % of all non-zeros each replaced by hot key A and hot key B. One
    row of 128 ids and one of 129 get ids of their own, so that a model can
    give the first no embedding at all and the second one for every id."""
    g = np.random.default_rng(seed)
    lens = g.integers(1, base_max + 1, nrows)
    lens[g.random(nrows) < 0.05] = 0
    forced = np.r_[0, np.arange(*EMPTY_RUN), nrows - 1]
    free = np.setdiff1d(np.arange(nrows), forced)
    pos = g.choice(free, N_SPECIAL * len(SPECIAL_LENS), replace=False)
    for i, n in enumerate(SPECIAL_LENS):
        lens[pos[i * N_SPECIAL:(i + 1) * N_SPECIAL]] = n
    lens[forced] = 0
    scalar_row = int(pos[SPECIAL_LENS.index(128) * N_SPECIAL])
    embed_row = int(pos[SPECIAL_LENS.index(129) * N_SPECIAL])
    off = np.zeros(nrows + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    nnz = int(off[-1])
    ids = g.integers(0, 400_000, nnz)
    kind = g.random(nnz)
    power = np.floor(np.exp(g.random(nnz) * np.log(2000.0)) - 1).astype(np.int64)
    ids = np.where(kind < 0.25, 400_000 + power, ids)
    ids = np.where((kind >= 0.25) & (kind < 0.33), _ID_HOT_A, ids)
    ids = np.where((kind >= 0.33) & (kind < 0.41), _ID_HOT_B, ids)
    ids[off[scalar_row]:off[scalar_row + 1]] = _ID_SCALAR_ROW + np.arange(lens[scalar_row])
    ids[off[embed_row]:off[embed_row + 1]] = _ID_EMBED_ROW + np.arange(lens[embed_row])
    val = None
    if with_val:  # both signs, so |x|, x and x*x all differ
        val = (g.random(nnz) + 0.5) * np.where(g.random(nnz) < 0.25, -1.0, 1.0)
        val = torch.from_numpy(val.astype(np.float32))
    label = torch.from_numpy((g.random(nrows) < 0.3).astype(np.float32))
    b = types.SimpleNamespace()
    b.nrows, b.nnz = nrows, nnz
    b.keys = torch.from_numpy(_key_of(ids))
    b.off = torch.from_numpy(off)
    b.lens = torch.from_numpy(lens.astype(np.int64))
    b.val, b.label = val, label
    b.hot_a, b.hot_b = int(_key_of(_ID_HOT_A)[0]), int(_key_of(_ID_HOT_B)[0])
    b.scalar_row, b.embed_row = scalar_row, embed_row
    b.embed_keys = torch.from_numpy(
        np.r_[_key_of(_ID_HOT_A), _key_of(_ID_EMBED_ROW + np.arange(lens[embed_row]))])
    b.scalar_keys = torch.from_numpy(
        np.r_[_key_of(_ID_HOT_B), _key_of(_ID_SCALAR_ROW + np.arange(lens[scalar_row]))])
    return b


_BATCHES = {}


def deep_batch(with_val, base_max=7):
    """45 000 rows: every persistent wave gets >= 5 rows (forward) and, with
    m >= 40960 embedded keys, >= 5 chunks (backward), on any device."""
    k = ("deep", bool(with_val), base_max)
    if k not in _BATCHES:
        _BATCHES[k] = make_batch(DEEP_ROWS, 17, with_val, base_max)
    return _BATCHES[k]


def edge_batch(with_val):
    """3000 rows: one wave runs one row (the non-rotating path)."""
    k = ("edge", bool(with_val))
    if k not in _BATCHES:
        _BATCHES[k] = make_batch(EDGE_ROWS, 23, with_val)
    return _BATCHES[k]


def make_model(batch, uniq, vstride, seed, w_scale=1.0):
    """test_kernels_gpu._pulled's shape for the keys `uniq` of `batch`: random
    w, 60 % of the keys with an embedding row, shuffled vidx, 7 spare rows;
    hot A and the all-embedded row forced to have one, hot B and the
    all-scalar row to have none. The last column is padding (dim = vstride-1).
    vstride 0: a flat w."""
    uniq = uniq.cpu()
    U = uniq.numel()
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(U, generator=g) * 0.3 * w_scale
    if vstride == 0:
        return w, None
    flag = torch.rand(U, generator=g) < 0.6
    flag[torch.isin(uniq, batch.embed_keys)] = True
    flag[torch.isin(uniq, batch.scalar_keys)] = False
    m = int(flag.sum())
    vidx = torch.full((U,), -1, dtype=torch.int64)
    vidx[flag] = torch.randperm(m, generator=g)
    vc = torch.randn(m + 7, vstride, generator=g) * 0.2
    vc[:, vstride - 1:] = 0
    return ref.make_hdr(w, vidx), vc


def local_id(uniq, key):
    hit = (uniq.cpu() == key).nonzero()
    assert hit.numel() == 1, "key not (uniquely) in the minibatch"
    return int(hit)


# ------------------------------------------------------------ fp64 references
def _with_underflow(bound, n):
    """bound + (n + 8) * TINY where the bound is not 0 (module docstring)."""
    return bound + (bound > 0) * ((torch.as_tensor(n).double() + 8) * TINY)


def fm_forward_ref64(off, lid, val, w_or_hdr, vc, vstride, block=8192):
    """float64 ops/ref.py:fm_forward without the loss, in blocks of rows.
    Returns py, wsum, xv [nrows, vstride] and bound_py, bound_w, bound_xv."""
    off = off.cpu()
    lid = lid.cpu().long()
    nrows = off.numel() - 1
    lens = off[1:] - off[:-1]
    f64 = torch.float64
    if vstride == 0:
        w = w_or_hdr.cpu().reshape(-1).double()
    else:
        w_or_hdr = w_or_hdr.cpu()
        w = w_or_hdr[:, 0].double()
        vid = ref.hdr_vidx(w_or_hdr).long()
        vc = vc.cpu()
    wsum = torch.zeros(nrows, dtype=f64)
    W = torch.zeros(nrows, dtype=f64)
    xv = torch.zeros(nrows, vstride, dtype=f64)
    A = torch.zeros(nrows, vstride, dtype=f64)
    Q = torch.zeros(nrows, vstride, dtype=f64)
    for r0 in range(0, nrows, block):
        r1 = min(r0 + block, nrows)
        j0, j1 = int(off[r0]), int(off[r1])
        if j1 == j0:
            continue
        li = lid[j0:j1]
        x = (val[j0:j1].double() if val is not None and val.numel()
             else torch.ones(j1 - j0, dtype=f64))
        rows = torch.repeat_interleave(torch.arange(r1 - r0), lens[r0:r1])
        t = x * w[li]
        wsum[r0:r1].index_add_(0, rows, t)
        W[r0:r1].index_add_(0, rows, t.abs())
        if vstride:
            v = vid[li]
            has = v >= 0
            rh = rows[has]
            xV = x[has, None] * vc[v[has]].double()
            xv[r0:r1].index_add_(0, rh, xV)
            A[r0:r1].index_add_(0, rh, xV.abs())
            Q[r0:r1].index_add_(0, rh, xV * xV)
    n = lens.double()
    o = types.SimpleNamespace()
    o.wsum, o.xv, o.n = wsum, xv, lens
    o.py = wsum + 0.5 * (xv * xv - Q).sum(1)
    o.bound_w = _with_underflow((n + 16) * U24 * W, n)
    o.bound_py = _with_underflow((n + 16) * U24 * (W + (A * A + Q).sum(1)), n)
    o.bound_xv = _with_underflow((n + 8)[:, None] * U24 * A, n[:, None])
    return o


def fm_backward_ref64(csc_off, csc_row, csc_val, dual, xv, w_or_hdr, vc, vstride, block=8192):
    """float64 ops/ref.py:fm_backward on the given (fp32) dual and xv, in
    blocks of keys. Returns gw, bound_gw and, for vstride > 0, gvc, bound_gvc
    [rows of vc, vstride] (rows no header points to stay 0)."""
    csc_off = csc_off.cpu()
    U = csc_off.numel() - 1
    f64 = torch.float64
    cnt = csc_off[1:] - csc_off[:-1]
    rows = csc_row.cpu().long()
    x = (csc_val.cpu().double() if csc_val is not None and csc_val.numel()
         else torch.ones(rows.numel(), dtype=f64))
    dx = dual.cpu().double()[rows] * x
    key = torch.repeat_interleave(torch.arange(U), cnt)
    o = types.SimpleNamespace()
    o.cnt = cnt
    o.gw = torch.zeros(U, dtype=f64).index_add_(0, key, dx)
    o.bound_gw = _with_underflow(
        (cnt + 8).double() * U24 * torch.zeros(U, dtype=f64).index_add_(0, key, dx.abs()), cnt)
    if vstride == 0:
        return o
    w_or_hdr, vc = w_or_hdr.cpu(), vc.cpu()
    vid = ref.hdr_vidx(w_or_hdr).long()
    has = vid >= 0
    xvr = xv.cpu().reshape(-1, vstride)
    o.gvc = torch.zeros(vc.shape[0], vstride, dtype=f64)
    o.bound_gvc = torch.zeros(vc.shape[0], vstride, dtype=f64)
    o.xxp = torch.zeros(U, dtype=f64).index_add_(0, key, dx * x)
    for k0 in range(0, U, block):
        k1 = min(k0 + block, U)
        p0, p1 = int(csc_off[k0]), int(csc_off[k1])
        hb = has[k0:k1]
        kl = key[p0:p1] - k0
        sel = hb[kl]
        kl, r, d, xx = kl[sel], rows[p0:p1][sel], dx[p0:p1][sel], x[p0:p1][sel]
        t = d[:, None] * xvr[r].double()
        acc = torch.zeros(k1 - k0, vstride, dtype=f64).index_add_(0, kl, t)
        aabs = torch.zeros(k1 - k0, vstride, dtype=f64).index_add_(0, kl, t.abs())
        xxa = torch.zeros(k1 - k0, dtype=f64).index_add_(0, kl, (d * xx).abs())
        vv = vid[k0:k1][hb]
        V = vc[vv].double()
        o.gvc[vv] = acc[hb] - o.xxp[k0:k1][hb, None] * V
        o.bound_gvc[vv] = _with_underflow((cnt[k0:k1][hb] + 8).double()[:, None] * U24 * (
            aabs[hb] + xxa[hb, None] * V.abs()), cnt[k0:k1][hb][:, None])
    return o


def loss64(loss, label, py):
    """(objv, dual) of ops/ref.py:_loss in float64, stable at any |py|."""
    label, py = label.cpu().double(), py.cpu().double()
    if loss == ref.LOSS_SQUARE:
        d = py - label
        return 0.5 * d * d, d
    y = torch.where(label > 0, 1.0, -1.0).double()
    if loss == ref.LOSS_SQUARE_HINGE:
        t = torch.clamp(1 - y * py, min=0)
        return t * t, -2 * y * t
    return torch.nn.functional.softplus(-y * py, threshold=700.0), -y * torch.sigmoid(-y * py)


# --------------------------------------------------------------------- checks
def err_ratio(got, ref64, bound):
    """(largest |err| / bound over bound > 0, entries with bound 0 that differ,
    flat index of the worst entry)."""
    err = (got.cpu().double() - ref64).abs().reshape(-1)
    bound = bound.reshape(-1)
    zero = bound == 0
    inexact = int((zero & (err != 0)).sum())
    ratio = torch.where(zero, torch.zeros_like(err), err / torch.where(zero, 1.0, bound))
    if ratio.numel() == 0:
        return 0.0, inexact, -1
    worst = int(ratio.argmax())
    return float(ratio[worst]), inexact, worst


def assert_within(name, got, ref64, bound, factor=FACTOR, where=None):
    """|got - ref64| <= factor * bound, exact where the bound is 0. Returns
    the largest |err| / bound and records it in RATIOS[name]. `where` turns
    the flat index of the worst entry into a description for the message."""
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    ratio, inexact, worst = err_ratio(got, ref64, bound)
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    if inexact or ratio > factor:
        g, r, b = (t.reshape(-1)[worst].item() for t in (got, ref64, bound))
        raise AssertionError(
            "%s: largest |err|/bound = %.3f (limit %g) at flat index %d%s: got %.9g, reference "
            "%.17g, bound %.3g; %d entries with bound 0 differ from the reference" % (
                name, ratio, factor, worst, " (%s)" % where(worst) if where else "", g, r, b,
                inexact))
    return ratio


def check_forward(tag, fr, label, loss, py, dual, xv, met, vstride):
    """Kernel outputs of one forward against the float64 reference `fr`
    (fm_forward_ref64): py / xv by bound, loss, dual and metrics against the
    float64 loss at the kernel's own py."""
    nrows = label.numel()
    py, dual, met = py.cpu(), dual.cpu(), met.cpu()
    kern = "k_fm_fwd" if vstride else "k_lin_fwd"
    assert_within("%s%s py" % (tag, kern), py, fr.py, fr.bound_py,
                  where=lambda i: "row %d of %d non-zeros" % (i, int(fr.n[i])))
    if vstride:
        assert_within("%s%s xv" % (tag, kern), xv.cpu().reshape(nrows, vstride), fr.xv,
                      fr.bound_xv, where=lambda i: "row %d of %d non-zeros, column %d" % (
                          i // vstride, int(fr.n[i // vstride]), i % vstride))
    objv, d64 = loss64(loss, label, py)
    assert bool(torch.isfinite(dual).all()), "non-finite dual"
    assert torch.allclose(dual.double(), d64, atol=1e-5, rtol=1e-4), (
        "dual: max abs diff %.3g" % float((dual.double() - d64).abs().max()))
    exp0 = float(objv.sum())
    assert abs(float(met[0]) - exp0) <= 1e-5 * abs(exp0), ("met[0]", float(met[0]), exp0)
    # met[1]: the loss of the linear part alone; the kernel's fp32 wsum is
    # within 2 * bound_w of the float64 one, so its loss is within
    # |dual| e + e^2 (all three losses have |loss''| <= 2)
    objw, dw = loss64(loss, label, fr.wsum)
    e = FACTOR * fr.bound_w
    exp1 = float(objw.sum())
    tol1 = 1e-5 * abs(exp1) + float((dw.abs() * e + e * e).sum())
    assert abs(float(met[1]) - exp1) <= tol1, ("met[1]", float(met[1]), exp1, tol1)
    lab = label.cpu()
    correct = float((((lab > 0) & (py > 0)) | ((lab <= 0) & (py <= 0))).sum())
    assert float(met[2]) == correct, ("met[2]", float(met[2]), correct)
    assert float(met[3]) == float(nrows), ("met[3]", float(met[3]), nrows)
    if met.numel() >= 5:
        acc = correct / float(nrows)
        assert float(met[4]) == (acc if acc > 0.5 else 1.0 - acc), ("met[4]", float(met[4]), acc)


def live_rows(hdr):
    v = ref.hdr_vidx(hdr.cpu()).long()
    return v[v >= 0]


def check_backward(tag, br, hdr, gw, gvc, vstride):
    """gw by the kernel that wrote it (keys without an embedding row:
    k_bwd_scalar, with one: k_bwd_v) and the live rows of gvc."""
    gw = gw.cpu()
    has = ref.hdr_vidx(hdr.cpu()) >= 0 if vstride else torch.zeros(gw.numel(), dtype=torch.bool)
    for kern, sel in (("k_bwd_scalar", ~has), ("k_bwd_v", has)):
        keys = sel.nonzero().reshape(-1)
        assert_within("%s%s gw" % (tag, kern), gw[keys], br.gw[keys], br.bound_gw[keys],
                      where=lambda i: "key %d of %d occurrences" % (
                          int(keys[i]), int(br.cnt[keys[i]])))
    if vstride:
        live = live_rows(hdr)  # in key order
        keys = has.nonzero().reshape(-1)

        def where(i):
            k = int(keys[i // vstride])
            return "key %d of %d occurrences, column %d, xxp %.3g" % (
                k, int(br.cnt[k]), i % vstride, float(br.xxp[k]))
        assert_within(tag + "k_bwd_v gV", gvc.cpu()[live], br.gvc[live], br.bound_gvc[live],
                      where=where)


def check_localize(batch, out):
    """hip.localize's first seven outputs against ops/ref.py:localize (one
    shard): key set and counts, uniq[lid] == keys, and the (key, row[, val])
    multiset of the CSC."""
    uniq, ucnt, owner_cnt, lid, csc_off, csc_row, csc_val = [
        t.cpu() if torch.is_tensor(t) else t for t in out[:7]]
    ru, rcnt = ref.localize(batch.keys, batch.off, batch.val, 1)[:2]
    assert uniq.numel() == ru.numel()
    order = torch.argsort(uniq)
    assert torch.equal(uniq[order], ru)
    assert torch.equal(ucnt[order].long(), rcnt.long())
    assert int(owner_cnt.sum()) == uniq.numel()
    assert lid.numel() == batch.nnz and csc_row.numel() == batch.nnz
    assert torch.equal(uniq[lid.long()], batch.keys)
    cnt = torch.bincount(lid.long(), minlength=uniq.numel())
    assert int(csc_off[0]) == 0 and torch.equal(csc_off[1:] - csc_off[:-1], cnt)
    rows = torch.repeat_interleave(torch.arange(batch.nrows), batch.lens)
    keyof = torch.repeat_interleave(torch.arange(uniq.numel()), cnt)
    cr = csc_row.long()
    assert int(cr.min()) >= 0 and int(cr.max()) < batch.nrows
    if batch.val is None:
        got = torch.sort(keyof * batch.nrows + cr).values
        exp = torch.sort(lid.long() * batch.nrows + rows).values
        assert torch.equal(got, exp)
    else:  # values follow their non-zeros (bit for bit)
        g = np.lexsort((csc_val.numpy(), cr.numpy(), keyof.numpy()))
        e = np.lexsort((batch.val.numpy(), rows.numpy(), lid.numpy()))
        assert np.array_equal(keyof.numpy()[g], lid.long().numpy()[e])
        assert np.array_equal(cr.numpy()[g], rows.numpy()[e])
        assert np.array_equal(csc_val.numpy()[g], batch.val.numpy()[e])


def check_structure(batch, uniq, csc_off, hdr, deep):
    """The conditions the GPU tests rely on (not measurements)."""
    lens = batch.lens
    for n in SPECIAL_LENS:
        assert int((lens == n).sum()) >= N_SPECIAL, "no rows of length %d" % n
    empty = [0, batch.nrows - 1] + list(range(*EMPTY_RUN))
    assert int(lens[empty].sum()) == 0
    assert int(lens[batch.scalar_row]) >= 64 and int(lens[batch.embed_row]) >= 65
    cnt = (csc_off[1:] - csc_off[:-1]).cpu()
    vid = ref.hdr_vidx(hdr.cpu()).long()
    ka, kb = local_id(uniq, batch.hot_a), local_id(uniq, batch.hot_b)
    assert int(vid[ka]) >= 0 and int(vid[kb]) < 0
    m = int((vid >= 0).sum())
    if deep:
        # a second round of the planner's 64-chunks-per-round expansion
        assert int(cnt[ka]) > 4096 and int(cnt[kb]) > 4096, (int(cnt[ka]), int(cnt[kb]))
        assert batch.nrows >= 5 * MAX_WAVES and m >= 5 * MAX_WAVES, (batch.nrows, m)
    else:
        assert batch.nrows <= MAX_WAVES
    return m


def grad_post_ref64(gvc, m, dim, clip, dropout, seed, normalize):
    """float64 mirror of fm.hip k_grad_post / k_grad_scale on gvc[:m, :dim]:
    clip, dropout by the host mirror of wh::uhash01 (compared in fp32, as the
    kernel does), normalisation. Returns (expected, mask of dropped entries)."""
    from wormhole_amd.kv.cpu_store import uhash01
    v = gvc[:m, :dim].double().clone()
    if clip > 0:
        c = float(np.float32(clip))
        v.clamp_(-c, c)
    zeroed = torch.zeros(m, dim, dtype=torch.bool)
    if dropout > 0:
        r = np.arange(m, dtype=np.uint64)[:, None]
        c = np.arange(dim, dtype=np.uint64)[None, :]
        zeroed = torch.from_numpy(uhash01(seed, r, c) > np.float32(1) - np.float32(dropout))
        v[zeroed] = 0
    if normalize:
        n2 = float((v * v).sum())
        if n2 >= 1e-10:
            v /= n2 ** 0.5
    return v, zeroed


# ---------------------------------------------------------------- GPU drivers
def _dev(t, dev):
    return t.to(dev) if t is not None else None


def localize_checked(hip, dev, batch):
    """hip.localize on the batch at hint 0 and at hint U (both checked against
    the reference); returns the first call's outputs."""
    k, o, v = batch.keys.to(dev), batch.off.to(dev), _dev(batch.val, dev)
    first = hip.localize(k, o, v, 1, 0)[:7]
    check_localize(batch, first)
    again = hip.localize(k, o, v, 1, int(first[0].numel()))[:7]
    check_localize(batch, again)
    return first


def run_fm_case(hip, dev, batch, loc, vstride, loss, w_scale=1.0, deep=False, tag="",
                repeat_bitwise=False, two_pass=False):
    """Forward (met of 4 and of 5 slots), one-call backward and the
    plan-on-a-side-stream + run backward of one model on a localized batch,
    all against the float64 references. two_pass: the plan comes from the
    count -> scan -> fill planner (and the linear model is planned and run
    too). Returns the forward reference."""
    uniq, ucnt, oc, lid, csc_off, csc_row, csc_val = loc
    with_val = batch.val is not None
    hdr, vc = make_model(batch, uniq, vstride, 5, w_scale)
    if vstride:
        check_structure(batch, uniq, csc_off, hdr, deep)
    off_d, val_d, lab_d = batch.off.to(dev), _dev(batch.val, dev), batch.label.to(dev)
    hdr_d, vc_d = hdr.to(dev), _dev(vc, dev)
    fr = fm_forward_ref64(batch.off, lid, batch.val, hdr, vc, vstride)
    for slots in (4, 5):
        met = torch.zeros(slots, dtype=torch.float64, device=dev)
        py, dual, xv = hip.fm_forward(off_d, lid, val_d, hdr_d, vc_d, vstride, lab_d, loss, met)
        check_forward(tag, fr, batch.label, loss, py, dual, xv, met, vstride)
    cv = csc_val if with_val else None
    xv_in = xv if vstride else None
    br = fm_backward_ref64(csc_off, csc_row, cv, dual, xv_in, hdr, vc, vstride)
    gw, gvc = hip.fm_backward(csc_off, csc_row, cv, dual, xv_in, hdr_d, vc_d, vstride)
    check_backward(tag, br, hdr, gw, gvc, vstride)
    if repeat_bitwise:
        gw_a, gvc_a = gw.clone(), gvc.clone()
        gw_b, gvc_b = hip.fm_backward(csc_off, csc_row, cv, dual, xv_in, hdr_d, vc_d, vstride)
        live = live_rows(hdr).to(dev)
        assert torch.equal(gw_a, gw_b), "gw differs between two deterministic backward calls"
        assert torch.equal(gvc_a[live], gvc_b[live]), "gV differs between two deterministic calls"
    if vstride or two_pass:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            plan = hip.fm_backward_plan(csc_off, csc_row, hdr_d, vc.shape[0] if vstride else 0,
                                        batch.nrows, vstride, two_pass=two_pass)
        torch.cuda.current_stream(dev).wait_stream(side)
        gw2, gvc2 = hip.fm_backward_run(plan, csc_off, csc_row, cv, dual, xv_in, hdr_d, vc_d,
                                        vstride)
        del plan  # fm_backward_run has recorded this stream on the side stream's memory
        check_backward(tag, br, hdr, gw2, gvc2, vstride)
    return fr


def run_depth_case(hip, dev, vstride, with_val, localized, deterministic=False, tag="",
                   two_pass=False):
    """Section "deep batch" of the FM kernel tests; `localized` caches the
    checked hip.localize outputs per batch."""
    batch = deep_batch(with_val)
    key = id(batch)
    if key not in localized:
        localized[key] = localize_checked(hip, dev, batch)
    # which chunk order the backward takes (fm.hip:fm_backward `bucket`)
    bucketed = batch.nrows * vstride * 4 > BUCKET_BYTES and not deterministic
    assert bucketed == (vstride >= 16 and not deterministic)
    run_fm_case(hip, dev, batch, localized[key], vstride, ref.LOSS_LOGIT, deep=True, tag=tag,
                repeat_bitwise=deterministic, two_pass=two_pass)
