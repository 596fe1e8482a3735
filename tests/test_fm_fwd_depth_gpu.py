"""The gather depth of the FM forward (fm.hip k_fm_fwd): a wave issues the
gathers of SUB x depth compacted slots (SUB = 256 / vstride rows per
instruction) before it uses the first. The default depth is
min(vstride / 4, 4); WH_FM_FWD_DEPTH=10 / hip.set_fm_fwd_depth(10) selects the
deep schedule: 10 at vstride 64 (40 slots, a whole headline row), unchanged
elsewhere.

Rows are built directly (off, lid, hdr, vc), with an exact number of
EMBEDDED ids per row and ids without an embedding row between them, so the
LDS compaction is exercised: embedded counts 0, 1, 3, 4, 5, 16, 17, 39, 40,
41, 63, 64 and each shape's batch capacity - 1, capacity, capacity + 1 (both
depths) inside one 64-id pass; rows of 65, 104, 105 and 193 ids (the second
batch of a pass, later passes); with and without val; batches of 1 and 7
rows, a few blocks, and at vstride 64 enough rows that every persistent wave
runs at least 5. vc holds NaN in row 0 and in every row no live id points
to: a dead gather slot must not multiply table data by zero. Both depths stay
within the float64 bounds of _fm_cases.py.

Bitwise: run as a script in a fresh process (WH_FM_FWD_DEPTH=10, and the
default depth 4), this file runs the same inputs and saves py, dual, xv and
met; the test compares the two files bit for bit."""
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
VSTRIDES = (4, 32, 64, 128, 256)
BASE_COUNTS = (0, 1, 3, 4, 5, 16, 17, 39, 40, 41, 63, 64)
LONG_ROWS = (65, 104, 105, 193)
DEEP_DEPTH = {16: 10}  # lane-group width G -> fm.hip FwdDepth<G>::kDeep, where it is not TI
N_EMB, N_SCALAR = 3000, 500
DEEP_ROWS = 5 * fc.MAX_WAVES + 40  # every persistent wave runs at least 5 rows
BLOCK_ROWS = 600  # 150 blocks of four one-row waves


def capacities(vstride):
    """Slots per gather batch of fm.hip at this vstride: {default, deep}."""
    g = vstride // 4
    sub, ti = 64 // g, min(g, 4)
    return {sub * ti, sub * DEEP_DEPTH.get(g, ti)}


def row_specs(vstride):
    """(embedded ids, other ids) of every row kind: one-pass rows (at most 64
    ids), then the long rows, all embedded and with every fifth id not."""
    counts = set(BASE_COUNTS)
    for cap in capacities(vstride):
        counts |= {cap - 1, cap, cap + 1}
    specs = []
    for i, e in enumerate(sorted(c for c in counts if 0 <= c <= 64)):
        specs.append((e, min(64 - e, (3, 0, 11, 1)[i % 4])))
    for n in LONG_ROWS:
        specs.append((n, 0))
        specs.append((n - n // 5, n // 5))
    return specs


def make_case(vstride, specs, with_val, seed):
    """A minibatch whose row i has specs[i] = (embedded, other) ids, the others
    spread between the embedded ones; a model of N_EMB keys with an embedding
    row and N_SCALAR without; NaN in every row of vc that no id of the batch
    points to, row 0 among them."""
    g = np.random.default_rng([11, vstride, seed, int(with_val)])
    lens = np.array([e + o for e, o in specs], dtype=np.int64)
    off = np.zeros(len(specs) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    nnz = int(off[-1])
    is_emb = np.zeros(nnz, dtype=bool)
    for i, (e, o) in enumerate(specs):
        if e:
            is_emb[off[i] + g.choice(e + o, e, replace=False)] = True
    lid = np.where(is_emb, g.integers(0, N_EMB, nnz), N_EMB + g.integers(0, N_SCALAR, nnz))
    vidx = np.full(N_EMB + N_SCALAR, -1, dtype=np.int64)
    vidx[:N_EMB] = 1 + g.permutation(N_EMB)  # no key owns row 0
    # (scaled so that a row of 193 ids alone keeps |py| of order 1..10: a
    # batch of one row must not put its whole loss below fp32's range)
    vc = (g.standard_normal((N_EMB + 8, vstride)) * 0.5 / np.sqrt(vstride)).astype(np.float32)
    vc[:, vstride - 1:] = 0  # the padding column
    used = np.zeros(N_EMB + 8, dtype=bool)
    used[vidx[lid[is_emb]]] = True
    vc[~used] = np.nan
    c = types.SimpleNamespace()
    c.vstride, c.nrows, c.nnz = vstride, len(specs), nnz
    c.off = torch.from_numpy(off)
    c.lid = torch.from_numpy(lid.astype(np.int32))
    c.val = None
    if with_val:  # both signs
        v = (g.random(nnz) + 0.5) * np.where(g.random(nnz) < 0.25, -1.0, 1.0)
        c.val = torch.from_numpy(v.astype(np.float32))
    c.label = torch.from_numpy((g.random(len(specs)) < 0.3).astype(np.float32))
    c.hdr = ref.make_hdr(torch.from_numpy((g.standard_normal(N_EMB + N_SCALAR) * 0.3)
                                          .astype(np.float32)), torch.from_numpy(vidx))
    c.vc = torch.from_numpy(vc)
    assert bool(torch.isnan(c.vc[0]).all()) and int(used.sum()) <= N_EMB
    c.embedded = np.zeros(len(specs), dtype=np.int64)
    np.add.at(c.embedded, np.repeat(np.arange(len(specs)), lens), is_emb.astype(np.int64))
    assert c.embedded.tolist() == [e for e, _ in specs], "embedded ids per row are exact"
    return c


def cases(vstride, with_val, deep):
    """(tag, case) of one vstride: every row kind alone, in batches of 7,
    BLOCK_ROWS rows cycling through the kinds and, deep, DEEP_ROWS rows of the
    one-pass kinds with a long row every 500."""
    specs = row_specs(vstride)
    out = []
    for i, s in enumerate(specs):
        out.append(("row %d+%d" % s, make_case(vstride, [s], with_val, i)))
    for k in range(0, len(specs), 7):
        seven = [specs[(k + j) % len(specs)] for j in range(7)]
        out.append(("seven from %d" % k, make_case(vstride, seven, with_val, 100 + k)))
    cyc = [specs[i % len(specs)] for i in range(BLOCK_ROWS)]
    out.append(("%d rows" % BLOCK_ROWS, make_case(vstride, cyc, with_val, 200)))
    if deep:
        short = [s for s in specs if sum(s) <= 64]
        many = [specs[len(short) + (i // 500) % (len(specs) - len(short))] if i % 500 == 499
                else short[i % len(short)] for i in range(DEEP_ROWS)]
        out.append(("%d rows" % DEEP_ROWS, make_case(vstride, many, with_val, 300)))
    return out


def forward(hip, c, dev=DEV):
    d = lambda t: t.to(dev) if t is not None else None  # noqa: E731
    met = torch.zeros(5, dtype=torch.float64, device=dev)
    py, dual, xv = hip.fm_forward(d(c.off), d(c.lid), d(c.val), d(c.hdr), d(c.vc), c.vstride,
                                  d(c.label), ref.LOSS_LOGIT, met)
    return py, dual, xv, met


@pytest.fixture(scope="module")
def hip():
    from wormhole_amd import _native
    h = _native.hip()
    default = h.fm_fwd_depth()
    assert default == (10 if os.environ.get("WH_FM_FWD_DEPTH") == "10" else 4), (
        "batches of 4 are the default")
    yield h
    h.set_fm_fwd_depth(default)


def test_switch(hip):
    default = hip.fm_fwd_depth()
    try:
        hip.set_fm_fwd_depth(10)
        assert hip.fm_fwd_depth() == 10
        hip.set_fm_fwd_depth(4)
        assert hip.fm_fwd_depth() == 4
    finally:
        hip.set_fm_fwd_depth(default)


def test_row_kinds_cover_the_batch_edges():
    for vstride in VSTRIDES:
        emb = {e for e, _ in row_specs(vstride)}
        assert set(BASE_COUNTS) | set(LONG_ROWS) <= emb
        for cap in capacities(vstride):
            assert {cap - 1, cap, cap + 1} <= emb, (vstride, cap)
        assert any(o and e for e, o in row_specs(vstride))
    assert capacities(64) == {16, 40} and capacities(256) == {4} and capacities(4) == {64}
    assert DEEP_ROWS >= 5 * fc.MAX_WAVES


@pytest.mark.parametrize("with_val", [False, True])
@pytest.mark.parametrize("vstride", VSTRIDES)
def test_within_bounds_both_depths(hip, vstride, with_val):
    """Finite (NaN rows never reach a sum) and within the float64 bounds, at
    depth 4 and at the deep schedule; and the two the same bits."""
    default = hip.fm_fwd_depth()
    for tag, c in cases(vstride, with_val, deep=vstride == 64):
        fr = fc.fm_forward_ref64(c.off, c.lid, c.val, c.hdr, c.vc, vstride)
        outs = {}
        try:
            for depth in (4, 10):
                hip.set_fm_fwd_depth(depth)
                py, dual, xv, met = forward(hip, c)
                name = "vstride %d %s depth %d " % (vstride, tag, depth)
                assert bool(torch.isfinite(xv).all()) and bool(torch.isfinite(py).all()), name
                fc.check_forward(name, fr, c.label, ref.LOSS_LOGIT, py, dual, xv, met, vstride)
                outs[depth] = [t.cpu() for t in (py, dual, xv, met)]
        finally:
            hip.set_fm_fwd_depth(default)
        for a, b, what in zip(outs[4], outs[10], ("py", "dual", "xv", "met")):
            assert torch.equal(bits(a), bits(b)), "vstride %d %s: %s differs between depths" % (
                vstride, tag, what)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def test_depths_bit_for_bit_in_fresh_processes(tmp_path):
    """WH_FM_FWD_DEPTH=10 against the default depth (4), each in a process of
    its own (the switch is read once per process)."""
    procs = []
    for name, depth in (("deep", "10"), ("four", None)):
        env = dict(os.environ)
        env.pop("WH_FM_FWD_DEPTH", None)
        if depth:
            env["WH_FM_FWD_DEPTH"] = depth
        path = str(tmp_path / (name + ".pt"))
        procs.append((path, depth, subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), path], env=env, stdout=subprocess.PIPE,
            stderr=subprocess.PIPE, text=True)))
    saved = []
    for path, depth, p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, out[-2000:] + err[-3000:]
        assert ("OK depth %d" % (10 if depth else 4)) in out, out[-2000:] + err[-3000:]
        saved.append(torch.load(path))
    a, b = saved
    assert a.keys() == b.keys() and len(a) > 100
    for k in a:
        for x, y, what in zip(a[k], b[k], ("py", "dual", "xv", "met")):
            assert torch.equal(bits(x), bits(y)), "%s: %s differs between the depths" % (k, what)
            assert bool(torch.isfinite(x).all()), "%s: non-finite %s" % (k, what)


def main(path):
    """Child process: every case of the bounds test at this process's depth."""
    from wormhole_amd import _native
    hip = _native.hip()
    out = {}
    for vstride in VSTRIDES:
        for with_val in (False, True):
            for tag, c in cases(vstride, with_val, deep=vstride == 64 and with_val):
                out["vstride %d val %d %s" % (vstride, with_val, tag)] = [
                    t.cpu() for t in forward(hip, c)]
    torch.save(out, path)
    print("OK depth %d" % hip.fm_fwd_depth())


if __name__ == "__main__":
    main(sys.argv[1])
