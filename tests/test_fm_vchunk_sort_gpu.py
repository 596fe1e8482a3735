"""The bucket sort of the FM backward's V chunks (fm.hip k_vchunk_hist ->
k_vchunk_scan -> k_vchunk_scatter: 128 block histograms, a scan that a few
blocks share by digit slices, the digit totals scanned by every scatter
block): every chunk must land in the sorted list exactly once, whatever the
histograms look like. Checked through the backward's results against
fm_backward_ref64 on hand-built CSCs whose xv is large enough to bucket
(more than 2 MiB):

  fewer V chunks than the sort has blocks (most block histograms empty),
  exactly one V chunk, all chunks in one row window, all chunks small, no
  chunk small, and more than 128 x 256 x 8 chunks (a block's loop takes a
  second step).

Each with packing on (digit = row window x 2 + class, 512 digits) and off
(256 digits) through hip.set_fm_bwd_pack, and once more in a fresh process
with WH_FM_BWD_PACK=0 (this file run as a script; prints OK)."""
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

import _fm_cases as fc  # noqa: E402
from wormhole_amd.ops import ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SORT_BLOCKS, SORT_THREADS, SORT_UNROLL = 128, 256, 8  # fm.hip kBucketBlocks, kThreads, kBucketU
CHUNK_V = 64  # occurrences per V chunk
SMALL = 4  # a small chunk: one chunk of at most min(vstride / 4, 4) occurrences


def make_case(vstride, rows, cnt_emb, n_scalar, row_lo, row_hi, seed):
    """A CSC over `rows` rows: one embedded key per entry of cnt_emb (its
    occurrence count), n_scalar keys without an embedding row, key order
    shuffled, every occurrence in a row of [row_lo, row_hi), ascending per key."""
    g = np.random.default_rng([13, vstride, seed])
    cnt = np.r_[np.asarray(cnt_emb, dtype=np.int64), g.integers(1, 30, n_scalar)]
    emb = np.r_[np.ones(len(cnt_emb), bool), np.zeros(n_scalar, bool)]
    order = g.permutation(cnt.size)
    cnt, emb = cnt[order], emb[order]
    U = cnt.size
    csc_off = np.zeros(U + 1, dtype=np.int64)
    csc_off[1:] = np.cumsum(cnt)
    nnz = int(csc_off[-1])
    key = np.repeat(np.arange(U), cnt)
    row = g.integers(row_lo, row_hi, nnz)
    row = row[np.lexsort((row, key))]
    m = int(emb.sum())
    vidx = np.full(U, -1, dtype=np.int64)
    vidx[emb] = g.permutation(m)
    c = types.SimpleNamespace()
    c.vstride, c.rows, c.U, c.m = vstride, rows, U, m
    c.chunks = int(((cnt[emb] + CHUNK_V - 1) // CHUNK_V).sum())
    c.small = int((cnt[emb] <= SMALL).sum())
    c.csc_off = torch.from_numpy(csc_off)
    c.csc_row = torch.from_numpy(row.astype(np.int32))
    v = (g.random(nnz) + 0.5) * np.where(g.random(nnz) < 0.25, -1.0, 1.0)
    c.csc_val = torch.from_numpy(v.astype(np.float32))
    c.dual = torch.from_numpy((g.standard_normal(rows) * 0.5).astype(np.float32))
    c.xv = torch.from_numpy((g.standard_normal((rows, vstride)) * 0.3).astype(np.float32))
    c.hdr = ref.make_hdr(torch.from_numpy((g.standard_normal(U) * 0.3).astype(np.float32)),
                         torch.from_numpy(vidx))
    c.vc = torch.from_numpy((g.standard_normal((m + 3, vstride)) * 0.2).astype(np.float32))
    assert rows * vstride * 4 > fc.BUCKET_BYTES, "the backward must bucket this batch"
    return c


def _mixed(g, n):
    """n counts: small ones, a chunk's worth and multi-chunk keys."""
    return np.r_[g.integers(1, SMALL + 1, n // 2), g.integers(SMALL + 1, 64, n - n // 2 - 3),
                 [64, 65, 200]]


def build(name):
    g = np.random.default_rng(5)
    if name == "fewer_chunks_than_blocks":
        c = make_case(64, 8200, _mixed(g, 40), 20, 0, 8200, 1)
        assert 1 < c.chunks < SORT_BLOCKS
    elif name == "one_chunk":
        c = make_case(64, 8200, [7], 20, 0, 8200, 2)
        assert c.chunks == 1
    elif name == "one_row_window":
        # 8200 rows: row windows of 64 rows; every occurrence in the 100th
        c = make_case(64, 8200, _mixed(g, 900), 50, 100 * 64, 101 * 64, 3)
        assert c.chunks > SORT_BLOCKS
    elif name == "all_small":
        c = make_case(64, 8200, g.integers(1, SMALL + 1, 3000), 50, 0, 8200, 4)
        assert c.small == c.m == c.chunks
    elif name == "none_small":
        c = make_case(64, 8200, np.r_[g.integers(SMALL + 1, 64, 1500), [64, 65, 200, 700]], 50,
                      0, 8200, 5)
        assert c.small == 0
    elif name == "second_step":
        n = SORT_BLOCKS * SORT_THREADS * SORT_UNROLL + 3000
        cnt = np.where(g.random(n) < 0.8, 1, g.integers(1, 8, n))
        c = make_case(16, 33000, cnt, 1000, 0, 33000, 6)
        assert c.chunks > SORT_BLOCKS * SORT_THREADS * SORT_UNROLL
    else:
        raise KeyError(name)
    return c


CASES = ("fewer_chunks_than_blocks", "one_chunk", "one_row_window", "all_small", "none_small",
         "second_step")


def run_case(hip, name, settings, dev=DEV):
    c = build(name)
    d = lambda t: t.to(dev)  # noqa: E731
    br = fc.fm_backward_ref64(c.csc_off, c.csc_row, c.csc_val, c.dual, c.xv, c.hdr, c.vc,
                              c.vstride)
    args = (d(c.csc_off), d(c.csc_row), d(c.csc_val), d(c.dual), d(c.xv), d(c.hdr), d(c.vc),
            c.vstride)
    default = hip.fm_bwd_pack()
    try:
        for on in settings:
            hip.set_fm_bwd_pack(on)
            gw, gvc = hip.fm_backward(*args)
            fc.check_backward("%s pack %d " % (name, on), br, c.hdr, gw, gvc, c.vstride)
    finally:
        hip.set_fm_bwd_pack(default)


@pytest.fixture(scope="module")
def hip():
    from wormhole_amd import _native
    return _native.hip()


@pytest.mark.parametrize("name", CASES)
def test_sorted_backward_matches_reference(hip, name):
    run_case(hip, name, (True, False))


def test_unpacked_in_a_fresh_process():
    env = dict(os.environ, WH_FM_BWD_PACK="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert any(l.strip() == "OK" for l in r.stdout.splitlines()), r.stdout[-2000:] + r.stderr[-3000:]


def main():
    """Child process: WH_FM_BWD_PACK=0 from the environment, every case."""
    from wormhole_amd import _native
    hip = _native.hip()
    assert os.environ.get("WH_FM_BWD_PACK") == "0" and not hip.fm_bwd_pack()
    for name in CASES:
        run_case(hip, name, (False,))
    print("OK")


if __name__ == "__main__":
    main()
