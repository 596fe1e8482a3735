"""The two fusions of the native DiFacto step (csrc/bind/fm_ops.cc).

The backward's chunk plan emitted by the open (kvstore.hip
k_difacto_open_pull with a plan argument, wh_chunk_plan.h emit_key) against
the plan of fm.hip's own planner on the same localize output: both backward
results within the float64 bounds of _fm_cases.py, equal chunk totals, and
the single-chunk keys bit for bit (the same kernel on the same lists).

The fused V update (fused_v): keys whose occurrences fit one V chunk of the backward get their
AdaGrad step from the backward wave itself (fm.hip k_bwd_v<G, true>), the push
skips them (kvstore.hip k_difacto_push with the minibatch counts). Against the
same step with WH_DIFACTO_FUSED_V=0 (every row through gvc and the push):
bit for bit in deterministic mode (a child process, _difacto_fused_check.py),
to float tolerance in the default mode, where the hot keys' float atomics
land in a different order from run to run."""
import os
import subprocess
import sys

import pytest
import torch

import _difacto_fused_check as fz
from test_difacto_native import _same

import _fm_cases as fc
from wormhole_amd.ops import ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda", 0)
HP = [0.1, 1.0, 0.3, 0.0, 0.1, 1.0, 0.0, 0.01]  # (lambda_l1 0.3: some w stay 0 after a push)


@pytest.fixture(scope="module")
def hip():
    from wormhole_amd import _native
    return _native.hip()


def _localized(hip, b):
    out = hip.localize(b.keys.to(DEV), b.off.to(DEV), None, 1, 0)[:7]
    return out[0], out[1], out[4], out[5]  # uniq, ucnt, csc_off, csc_row


def _open_store(hip, l1_shrk):
    """A store that has seen one big minibatch twice: counts, embedding rows
    for keys above the threshold (allocated by an open or, under l1_shrk, by
    the push that moves w off 0), and w == 0 for the keys FTRL's l1 holds or
    brings back there -- some of them with a row, which l1_shrk then masks.
    The planted keys get a gradient of one sign, so their w is not 0."""
    gs = hip.KVStore(1 << 16, 1 << 14, 16, 0)
    b = fz.make_batch(1)
    uniq, ucnt, _, _ = _localized(hip, b)
    planted = torch.from_numpy(b.small_keys).tolist() + [b.key_all, b.key_64, b.key_65]
    planted = torch.isin(uniq.cpu(), torch.tensor(planted))
    g = torch.Generator().manual_seed(3)
    for _ in range(2):
        slot, hdr, vc, vpos = gs.difacto_open_pull(uniq, True, ucnt, HP, fz.THRESHOLD, l1_shrk, 5)
        gw = torch.randn(uniq.numel(), generator=g)
        gw[planted] = 3.0
        gvc = torch.zeros(max(int(vpos[-1]), 1), gs.V.shape[1], device=DEV)
        gs.difacto_push(slot, hdr, gw.to(DEV), gvc, HP, fz.THRESHOLD, l1_shrk, 5)
    return gs


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("l1_shrk", [False, True])
@pytest.mark.parametrize("which", ["big", "small"])
def test_plan_from_the_open(hip, which, l1_shrk, direct):
    b = fz.make_batch(0) if which == "big" else fz.small_batch(0)
    gs = _open_store(hip, l1_shrk)
    vstride = gs.V.shape[1]
    uniq, ucnt, csc_off, csc_row = _localized(hip, b)
    U, nnz = uniq.numel(), csc_row.numel()
    if which == "big":
        assert fz.check_structure(b) == U
    else:
        assert 0 < U < 1024
    rows_before = int(gs.vnext[0])
    slot, hdr, vc, vpos, plan = hip.difacto_open_pull_plan(
        gs, uniq, True, ucnt, HP, fz.THRESHOLD, l1_shrk, 5, direct, csc_off, csc_row, b.rows)
    assert len(plan) == 3, "the open fell back"
    vid = ref.hdr_vidx(hdr.cpu()).long()
    cnt = (csc_off[1:] - csc_off[:-1]).cpu()
    assert torch.equal(cnt, ucnt.cpu().long())
    # the structure the case relies on: keys with and without a row, rows
    # allocated by this very open, rows masked by l1_shrk
    assert int((vid >= 0).sum()) > 0 and int((vid < 0).sum()) > 0
    vrow = gs.vrow[slot.long()].cpu()
    if which == "big":
        if l1_shrk:
            assert int(((vrow >= 0) & (vid < 0)).sum()) > 0, "no row masked by l1_shrk"
        else:
            assert int(gs.vnext[0]) > rows_before, "no row allocated by this open"
        assert int(((vid >= 0) & (cnt > 64)).sum()) >= 2 and int(((vid >= 0) & (cnt <= 4)).sum()) > 0
    if direct:
        assert vc.data_ptr() == gs.V.data_ptr() and torch.equal(vid[vid >= 0], vrow[vid >= 0].long())
    g = torch.Generator().manual_seed(9)
    dual = (torch.randn(b.rows, generator=g) * 0.5).to(DEV)
    xv = (torch.randn(b.rows, vstride, generator=g) * 0.3).to(DEV)
    gw1, gvc1 = hip.fm_backward_run(plan, csc_off, csc_row, None, dual, xv, hdr, vc, vstride)
    plan2 = hip.fm_backward_plan(csc_off, csc_row, hdr, vc.shape[0], b.rows, vstride)
    gw2, gvc2 = hip.fm_backward_run(plan2, csc_off, csc_row, None, dual, xv, hdr, vc, vstride)
    tot1 = hip.fm_backward_plan_totals(plan, csc_off, nnz, vstride).cpu()
    tot2 = hip.fm_backward_plan_totals(plan2, csc_off, nnz, vstride).cpu()
    exp_v = int(((cnt[vid >= 0] + 63) // 64).sum())
    exp_s = int(((cnt[vid < 0] + 31) // 32).sum())
    assert tot1.tolist() == tot2.tolist() == [exp_s, exp_v]
    br = fc.fm_backward_ref64(csc_off, csc_row, None, dual, xv, hdr, vc, vstride)
    fc.check_backward("open plan ", br, hdr, gw1, gvc1, vstride)
    fc.check_backward("fm plan ", br, hdr, gw2, gvc2, vstride)
    single = torch.where(vid >= 0, cnt <= 64, cnt <= 32)
    bits = fz.bits
    assert torch.equal(bits(gw1.cpu())[single], bits(gw2.cpu())[single])
    live = vid[single & (vid >= 0)]
    assert live.numel() > 0
    assert torch.equal(bits(gvc1.cpu()[live]), bits(gvc2.cpu()[live]))


def test_plan_from_the_open_no_keys(hip):
    """U = 0: nothing to open, no plan (the step then skips the backward)."""
    gs = _open_store(hip, False)
    e64 = torch.zeros(0, dtype=torch.int64, device=DEV)
    e32 = torch.zeros(0, dtype=torch.int32, device=DEV)
    slot, hdr, vc, vpos, plan = hip.difacto_open_pull_plan(
        gs, e64, True, e32, HP, fz.THRESHOLD, False, 5, True,
        torch.zeros(1, dtype=torch.int64, device=DEV), e32, 8)
    assert len(plan) == 0 and slot.numel() == 0 and hdr.numel() == 0 and vpos.cpu().tolist() == [0]


def test_fused_update_bit_for_bit_deterministic():
    env = dict(os.environ, WH_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_difacto_fused_check.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert any(l.strip() == "OK" for l in r.stdout.splitlines()), r.stdout[-2000:] + r.stderr[-3000:]


# dim 8: the batches as they are (key-major V chunks); dim 64, twice the rows:
# the headline's row width, and enough xv for the backward to bucket its V
# chunks by row window (fm.hip fm_backward `bucket`: rows * vstride * 4 > 2 MiB)
@pytest.mark.parametrize("dim,rows", [(8, fz.ROWS), (64, 2 * fz.ROWS)])
def test_fused_update_default_mode(dim, rows, monkeypatch):
    monkeypatch.delenv("WH_DETERMINISTIC", raising=False)
    dev = torch.device("cuda", 0)
    batches = [fz.make_batch(0, rows), fz.small_batch(0), fz.make_batch(1, rows),
               fz.small_batch(1), fz.make_batch(2, rows)]
    for b in batches[::2]:
        fz.check_structure(b)
    if dim == 64:
        assert rows * 64 * 4 > 2 << 20
    for name in ("WH_DIFACTO_NATIVE", "WH_DIFACTO_FUSED_V"):  # (train() sets them)
        monkeypatch.setenv(name, "1")
    la, lb = (fz.train(f, batches, dim, dev) for f in (True, False))
    _same(la, lb)  # keys, cnt and row allocation exactly; w and V to 1e-4
    ma, mb = fz.model_by_key(la), fz.model_by_key(lb)
    fz.check_rows(ma, batches[0])
    assert torch.equal(ma.keys, mb.keys) and torch.equal(ma.cnt, mb.cnt)
    assert torch.equal(ma.has, mb.has)
    for name in ("z", "sq", "VG"):
        a, c = getattr(ma, name), getattr(mb, name)
        far = ~torch.isclose(a, c, atol=1e-4, rtol=1e-4)
        far = far.reshape(a.shape[0], -1).any(1)
        assert int(far.sum()) <= a.shape[0] // 1000, (name, int(far.sum()))
