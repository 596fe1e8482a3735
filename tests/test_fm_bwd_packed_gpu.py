"""The packed iterations of the FM backward (fm.hip k_bwd_v): a wave takes
SUB = 256 / vstride consecutive V chunks and, when every one of them is small
(a single-chunk key of at most TI = min(vstride / 4, 4) occurrences), runs
them in one iteration, one lane group per key; the bucket sort (digit = row
window x 2 + class) puts the small chunks of a row window side by side.

Op level (hip.fm_backward on hand-built CSCs): planted per-key counts 1..TI,
TI + 1, 63, 64, 65 and 200, the number of small chunks in every residue mod
SUB, all-small and none-small lists, with and without csc_val, vstride 4, 16,
64, 128 and 256 (which packs nothing), key-major lists (mixed groups, partial
last group) and bucketed ones. Both settings of the switch
(hip.set_fm_bwd_pack, WH_FM_BWD_PACK) stay within the float64 bounds of
_fm_cases.py, and every single-chunk key's gw and gV row is the same bits
with packing on and off; multi-chunk keys (float atomics, any order) to
float tolerance.

Fused: run as a script in a fresh process with WH_DETERMINISTIC=1, this file
trains the native DiFacto step (the minibatches of _difacto_fused_check.py)
with packing on and off, for both fused_v settings, and compares every model
tensor bit for bit. Prints OK."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

import pytest  # noqa: E402

import _difacto_fused_check as fz  # noqa: E402
import _fm_cases as fc  # noqa: E402
from wormhole_amd.ops import ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROWS = 300
VSTRIDES = (4, 16, 64, 128, 256)


def shape_of(vstride):
    """(SUB, TI) of fm.hip Shape<vstride / 4>."""
    g = vstride // 4
    return 64 // g, min(g, 4)


def base_small(sub):
    """A multiple of SUB near 150: with the other keys, about 200 keys."""
    return 150 // sub * sub


def make_case(vstride, n_small, kind, with_val, rows=ROWS, seed=0):
    """A CSC of ~200 keys over `rows` rows. Embedded keys: n_small small ones
    (counts cycling 1..TI) and, unless kind == "all_small", the planted counts
    TI + 1, 63, 64, 65, 200 and a spread of others; ~20 keys without an
    embedding row. kind == "none_small": no small key at all. The key order
    (= the key-major chunk order) is shuffled, so small and other chunks mix."""
    sub, ti = shape_of(vstride)
    g = np.random.default_rng([7, vstride, n_small, seed, int(with_val)])
    small = [1 + i % ti for i in range(n_small)] if kind != "none_small" else []
    other = []
    if kind != "all_small":
        other = [ti + 1, 63, 64, 65, 200] + [int(c) for c in g.integers(ti + 1, 41, 14)]
    scalar = [int(c) for c in g.integers(1, 41, 20)]
    cnt = np.array(small + other + scalar, dtype=np.int64)
    emb = np.r_[np.ones(len(small) + len(other), bool), np.zeros(len(scalar), bool)]
    order = g.permutation(cnt.size)
    cnt, emb = cnt[order], emb[order]
    U = cnt.size
    csc_off = np.zeros(U + 1, dtype=np.int64)
    csc_off[1:] = np.cumsum(cnt)
    csc_row = np.concatenate([np.sort(g.choice(rows, int(c), replace=False)) for c in cnt])
    nnz = int(csc_off[-1])
    m = int(emb.sum())
    vidx = np.full(U, -1, dtype=np.int64)
    vidx[emb] = g.permutation(m)
    c = types.SimpleNamespace()
    c.vstride, c.rows, c.U, c.m, c.sub, c.ti = vstride, rows, U, m, sub, ti
    c.cnt = torch.from_numpy(cnt)
    c.emb = torch.from_numpy(emb)
    c.vidx = torch.from_numpy(vidx)
    c.n_small = int(((cnt <= ti) & emb).sum())
    c.csc_off = torch.from_numpy(csc_off)
    c.csc_row = torch.from_numpy(csc_row.astype(np.int32))
    c.csc_val = None
    if with_val:
        v = (g.random(nnz) + 0.5) * np.where(g.random(nnz) < 0.25, -1.0, 1.0)
        c.csc_val = torch.from_numpy(v.astype(np.float32))
    c.dual = torch.from_numpy((g.standard_normal(rows) * 0.5).astype(np.float32))
    c.xv = torch.from_numpy((g.standard_normal((rows, vstride)) * 0.3).astype(np.float32))
    c.hdr = ref.make_hdr(torch.from_numpy((g.standard_normal(U) * 0.3).astype(np.float32)),
                         c.vidx)
    c.vc = torch.from_numpy((g.standard_normal((m + 3, vstride)) * 0.2).astype(np.float32))
    return c


@pytest.fixture(scope="module")
def hip():
    from wormhole_amd import _native
    h = _native.hip()
    default = h.fm_bwd_pack()
    assert default == (os.environ.get("WH_FM_BWD_PACK") != "0"), "packing is the default"
    yield h
    h.set_fm_bwd_pack(default)


def run_both(hip, c, tag):
    """The backward with packing off and on against the float64 reference,
    then single-chunk keys bit for bit and multi-chunk keys to tolerance."""
    d = lambda t: t.to(DEV) if t is not None else None  # noqa: E731
    args = (d(c.csc_off), d(c.csc_row), d(c.csc_val), d(c.dual), d(c.xv), d(c.hdr), d(c.vc),
            c.vstride)
    br = fc.fm_backward_ref64(c.csc_off, c.csc_row, c.csc_val, c.dual, c.xv, c.hdr, c.vc,
                              c.vstride)
    out = {}
    default = hip.fm_bwd_pack()
    try:
        for on in (False, True):
            hip.set_fm_bwd_pack(on)
            gw, gvc = hip.fm_backward(*args)
            fc.check_backward("%s pack %d " % (tag, on), br, c.hdr, gw, gvc, c.vstride)
            out[on] = (gw.cpu(), gvc.cpu())
    finally:
        hip.set_fm_bwd_pack(default)
    (gw0, gv0), (gw1, gv1) = out[False], out[True]
    single = torch.where(c.emb, c.cnt <= 64, c.cnt <= 32)
    assert torch.equal(fz.bits(gw0)[single], fz.bits(gw1)[single]), (
        "%s: gw of %d single-chunk keys differs with packing" % (
            tag, int((fz.bits(gw0)[single] != fz.bits(gw1)[single]).sum())))
    live = c.vidx[single & c.emb]
    if live.numel():
        diff = (fz.bits(gv0[live]) != fz.bits(gv1[live])).any(1)
        assert not bool(diff.any()), "%s: gV rows of %d single-chunk keys differ with packing" % (
            tag, int(diff.sum()))
    multi = ~single
    assert torch.allclose(gw0[multi], gw1[multi], rtol=1e-4, atol=1e-5)
    rows = c.vidx[multi & c.emb]
    assert torch.allclose(gv0[rows], gv1[rows], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("with_val", [False, True])
@pytest.mark.parametrize("vstride", VSTRIDES)
def test_every_residue_of_small_chunks(hip, vstride, with_val):
    """Key-major lists (xv far below the bucketing size): the planted counts,
    mixed groups, and n_small = k SUB + r for every r in 0..SUB-1."""
    sub, ti = shape_of(vstride)
    base = base_small(sub)
    for r in range(sub):
        c = make_case(vstride, base + r, "mixed", with_val)
        assert c.n_small == base + r and c.n_small % sub == r
        planted = set(c.cnt[c.emb].tolist())
        assert set(range(1, ti + 2)) | {63, 64, 65, 200} <= planted
        assert c.rows * vstride * 4 <= fc.BUCKET_BYTES
        run_both(hip, c, "vstride %d r %d" % (vstride, r))


@pytest.mark.parametrize("kind", ["all_small", "none_small"])
@pytest.mark.parametrize("vstride", VSTRIDES)
def test_all_small_and_none_small(hip, vstride, kind):
    sub, ti = shape_of(vstride)
    for n_small in (base_small(sub), base_small(sub) + max(sub - 1, 1)):
        c = make_case(vstride, n_small, kind, with_val=True)
        assert c.n_small == (n_small if kind == "all_small" else 0)
        if kind == "all_small":
            assert int(c.cnt[c.emb].max()) <= ti
        run_both(hip, c, "vstride %d %s" % (vstride, kind))


@pytest.mark.parametrize("vstride,rows", [(64, 8200), (128, 4200)])
def test_bucketed_list(hip, vstride, rows):
    """rows * vstride * 4 > 2 MiB: the bucket sort with the class digit runs
    (few non-zeros over many rows: every row window gets small and other
    chunks), for two residues of the small count."""
    assert rows * vstride * 4 > fc.BUCKET_BYTES
    sub, _ = shape_of(vstride)
    for r in (0, sub - 1):
        c = make_case(vstride, 40 * sub + r, "mixed", with_val=True, rows=rows, seed=r)
        assert c.n_small % sub == r
        run_both(hip, c, "bucketed vstride %d r %d" % (vstride, r))


def test_fused_bit_for_bit_deterministic():
    env = dict(os.environ, WH_DETERMINISTIC="1")
    env.pop("WH_FM_BWD_PACK", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert any(l.strip() == "OK" for l in r.stdout.splitlines()), r.stdout[-2000:] + r.stderr[-3000:]


def main():
    """Child process: packing on and off, fused_v on and off, dim 8 and 64
    (vstride 64: four keys to a packed iteration); every model tensor the
    same bits."""
    assert os.environ.get("WH_DETERMINISTIC") == "1", "run with WH_DETERMINISTIC=1"
    from wormhole_amd import _native
    hip = _native.hip()
    dev = torch.device("cuda", 0)
    batches = fz.five_steps()
    for b in batches[::2]:
        fz.check_structure(b)
    for dim in (8, 64):
        for fused in (True, False):
            models = {}
            for on in (True, False):
                hip.set_fm_bwd_pack(on)
                models[on] = fz.model_by_key(fz.train(fused, batches, dim, dev))
            ma, mb = models[True], models[False]
            fz.check_rows(ma, batches[0])
            assert torch.equal(ma.keys, mb.keys), "key sets differ"
            assert torch.equal(ma.cnt, mb.cnt) and torch.equal(ma.has, mb.has)
            for name in ("w", "z", "sq", "V", "VG"):
                a, c = fz.bits(getattr(ma, name)), fz.bits(getattr(mb, name))
                diff = (a != c).reshape(a.shape[0], -1).any(1)
                print("  dim %d fused %d %-2s keys that differ: %d of %d" % (
                    dim, fused, name, int(diff.sum()), a.shape[0]))
                assert not bool(diff.any()), "%s differs, first at key %d" % (
                    name, int(ma.keys[int(diff.nonzero()[0])]))
            assert float(ma.VG.abs().sum()) > 0 and int(ma.has.sum()) > 500
    print("OK")


if __name__ == "__main__":
    main()
