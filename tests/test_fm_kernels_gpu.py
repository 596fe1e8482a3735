"""The FM / linear forward and backward kernels of csrc/hip/fm.hip against
float64 references with derived error bounds (tests/_fm_cases.py): software
pipeline depth (every persistent wave runs >= 5 rows / chunks), rows of 0, 1,
63..65, 127..129, 191..193 and 500 non-zeros, runs of empty rows, all seven
lane-group shapes (vstride 4..256), valued data, hot keys of more than 64
chunks (embedded and scalar), both chunk orders of the backward, all three
losses, the 5-slot metrics, saturated margins, the deterministic mode, the
two-pass chunk planner, a plan run against a CSC of another size, and
k_grad_post past one step of its capped grid with dropout.
"""
import os
import subprocess
import sys

import pytest
import torch

import _fm_cases as fc
from wormhole_amd.ops import ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hip():
    from wormhole_amd import _native
    yield _native.hip()
    print("\nlargest |err|/bound per checked quantity:")
    for name in sorted(fc.RATIOS):
        print("  RATIO %-12s %.3f" % (name, fc.RATIOS[name]))


@pytest.fixture(scope="module")
def localized():
    """hip.localize outputs (checked against ops/ref.py) per batch."""
    return {}


@pytest.mark.parametrize("with_val", [False, True])
@pytest.mark.parametrize("vstride", [4, 8, 16, 32, 64, 128, 256])
def test_fm_pipeline_depth(hip, localized, vstride, with_val):
    fc.run_depth_case(hip, DEV, vstride, with_val, localized)


@pytest.mark.parametrize("with_val", [False, True])
@pytest.mark.parametrize("loss", [1, 2, 4])
@pytest.mark.parametrize("vstride", [0, 4, 8, 16, 32, 64, 128, 256])
def test_fm_row_edges(hip, localized, vstride, loss, with_val):
    batch = fc.edge_batch(with_val)
    assert bool((batch.label == 0.0).any()) and bool((batch.label == 1.0).any())
    if id(batch) not in localized:
        localized[id(batch)] = fc.localize_checked(hip, DEV, batch)
    loc = localized[id(batch)]
    fc.run_fm_case(hip, DEV, batch, loc, vstride, loss)
    # |py| past 100: softplus and __expf saturate, the dual stays finite
    fr = fc.run_fm_case(hip, DEV, batch, loc, vstride, loss, w_scale=200.0, tag="sat ")
    assert float(fr.py.abs().max()) > 100.0
    if not with_val:
        _all_rows_empty(hip, vstride, loss)


def _all_rows_empty(hip, vstride, loss):
    """A minibatch of 3000 empty rows: py == 0, xv == 0, metrics count them."""
    n = fc.EDGE_ROWS
    g = torch.Generator().manual_seed(3)
    label = (torch.rand(n, generator=g) < 0.3).float()
    off = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    lid = torch.empty(0, dtype=torch.int32, device=DEV)
    w = torch.randn(10, generator=g)
    if vstride:
        hdr = ref.make_hdr(w, torch.arange(10) - 3).to(DEV)
        vc = torch.randn(7, vstride, generator=g).to(DEV)
    else:
        hdr, vc = w.to(DEV), None
    met = torch.zeros(5, dtype=torch.float64, device=DEV)
    py, dual, xv = hip.fm_forward(off, lid, None, hdr, vc, vstride, label.to(DEV), loss, met)
    zero = torch.zeros(n)
    assert torch.equal(py.cpu(), zero)
    assert xv.numel() == n * vstride and torch.equal(xv.cpu(), torch.zeros(n * vstride))
    objv, d64 = fc.loss64(loss, label, zero)
    assert torch.allclose(dual.cpu().double(), d64, atol=1e-5, rtol=1e-4)
    met = met.cpu()
    assert float(met[0]) == pytest.approx(float(objv.sum()), rel=1e-5)
    assert float(met[1]) == pytest.approx(float(objv.sum()), rel=1e-5)
    correct = float((label <= 0).sum())  # py == 0 counts as a negative prediction
    acc = correct / n
    assert float(met[2]) == correct and float(met[3]) == float(n)
    assert float(met[4]) == (acc if acc > 0.5 else 1.0 - acc)


@pytest.mark.parametrize("vstride", [0, 16, 64])
def test_fm_two_pass_plan_deep(hip, localized, vstride):
    """fm_backward_plan(two_pass=True): k_chunk_count -> scans -> k_chunk_fill,
    the planner of minibatches with more unique keys than the look-back scan
    has tiles. The deep batch's planted keys (~16 000 occurrences: about 250 V
    chunks or 500 scalar chunks) take the whole-wave expansion through more
    than one round of 64; vstride 0 plans and runs the linear model."""
    fc.run_depth_case(hip, DEV, vstride, False, localized, two_pass=True, tag="two-pass ")


def test_fm_two_pass_plan_edges(hip, localized):
    batch = fc.edge_batch(False)
    if id(batch) not in localized:
        localized[id(batch)] = fc.localize_checked(hip, DEV, batch)
    fc.run_fm_case(hip, DEV, batch, localized[id(batch)], 4, ref.LOSS_LOGIT, two_pass=True,
                   tag="two-pass ")


@pytest.mark.parametrize("vstride", [0, 4])
def test_fm_backward_run_rejects_a_plan_of_another_size(hip, vstride):
    """A plan holds chunk lists sized for its CSC's non-zeros: run with a CSC
    of the same U and 40 times the non-zeros (or the reverse) it must raise
    before any kernel indexes the lists."""
    U, nrows = 1000, 64
    w = torch.zeros(U)
    hdr = (ref.make_hdr(w, torch.arange(U)) if vstride else w).to(DEV)
    vc = torch.zeros(U, vstride, device=DEV) if vstride else None
    dual = torch.zeros(nrows, device=DEV)
    xv = torch.zeros(nrows * vstride, device=DEV) if vstride else None

    def csc(per):
        off = torch.arange(U + 1, dtype=torch.int64, device=DEV) * per
        row = (torch.arange(U * per, device=DEV) % nrows).to(torch.int32)
        return off, row

    small, big = csc(1), csc(40)
    for a, b in ((small, big), (big, small)):
        plan = hip.fm_backward_plan(a[0], a[1], hdr, U if vstride else 0, nrows, vstride)
        with pytest.raises(RuntimeError, match="CSC of another size"):
            hip.fm_backward_run(plan, b[0], b[1], None, dual, xv, hdr, vc, vstride)
        gw, gvc = hip.fm_backward_run(plan, a[0], a[1], None, dual, xv, hdr, vc, vstride)
        assert torch.equal(gw.cpu(), torch.zeros(U))  # the plan itself is intact
    with pytest.raises(RuntimeError, match="not a backward plan"):
        hip.fm_backward_run(plan[:2], big[0], big[1], None, dual, xv, hdr, vc, vstride)


def test_fm_deterministic_matches_reference():
    """WH_DETERMINISTIC=1 is read once per process: the deep-batch checks at
    vstride 16 and 64 (ordered partial sums, k_bwd_reduce_s / _v) and the
    bitwise repeat of the backward run in a fresh child."""
    env = dict(os.environ, WH_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_fm_det_check.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert any(l.strip() == "OK" for l in r.stdout.splitlines()), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("clip,dropout,normalize", [(1.0, 0.0, False), (0.0, 0.3, False),
                                                    (1.5, 0.3, True)])
def test_fm_grad_post_large(hip, clip, dropout, normalize):
    """320 000 live floats: more than the 1024 x 256 threads of the capped
    grid, so the grid-stride loop takes a second step."""
    rows, vs, m, dim, seed = 6000, 64, 5000, 50, 0x1234567
    assert m * vs > 1024 * 256
    gvc = torch.randn(rows, vs, generator=torch.Generator().manual_seed(8)) * 3
    a = gvc.clone().to(DEV)
    hip.fm_grad_post(a, torch.tensor([m], dtype=torch.int64, device=DEV), dim, clip, dropout,
                     seed, normalize)
    a = a.cpu()
    exp, zeroed = fc.grad_post_ref64(gvc, m, dim, clip, dropout, seed, normalize)
    got = a[:m, :dim]
    assert torch.equal(got == 0, zeroed), "dropped set differs from the host mirror of uhash01"
    if dropout > 0:
        assert 0.25 < float(zeroed.double().mean()) < 0.35
    assert torch.allclose(got.double(), exp, atol=1e-6, rtol=0)
    if not normalize:  # clip and dropout alone are exact
        assert torch.equal(got.double(), exp)
    assert torch.equal(a[m:], gvc[m:]) and torch.equal(a[:, dim:], gvc[:, dim:])
