"""CPU half of the LayerNorm / pooling / return-scan limits tests (the device half is
tests/test_ln_pool_scan_limits_gpu.py):

- the float32 restatement of LayerNorm in the header's lane layout and summation order (tests/ln_ref.py) stays within the
  first-order bounds of DESIGN.md 22 of the float64 restatement, at every shape the device half runs;
- on those same inputs the restatement tells the stated order from the nearest wrong ones -- a left-to-right sum over the
  row, a butterfly as wide as the wave where LPR is 8 or 16 (it adds up the rows that share the wave), and, where a lane
  holds three live float4s or more, the slots taken last first -- so a kernel that summed in one of these orders could not
  pass the device half's bit-for-bit comparison;
- the shapes of the device half take the trips and cross the thresholds they were chosen for (pure arithmetic on the
  restated launch shapes).

A single row (rows = 1) is left out of the order assertions: beside it a wave holds only dead row slots, so the wide
butterfly adds zeros, and one short row can round the same way in two orders by chance."""
import numpy as np
import pytest

import ln_ref as lr
import pqn_ref as pr
from ln_ref import EPS, LN_ROWS, LN_SECOND_TRIP, LN_WIDTHS

SHAPES = [(r, w) for w in LN_WIDTHS for r in LN_ROWS] + list(LN_SECOND_TRIP)
_ids = lambda s: "%dx%d" % s                                    # noqa: E731


def _run32(rows, width, **order):
    """Forward and unmasked backward of one case in fp32 -> dict of arrays."""
    z, gamma, beta, dy = lr.ln_case(rows, width)
    y, stats = lr.ln_relu_fwd32(z, gamma, beta, EPS, **order)
    dz, part_g, part_b = lr.ln_relu_bwd32(dy, y, z, stats, gamma, False, **order)
    return dict(y=y, stats=stats, dz=dz, part_g=part_g, part_b=part_b)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_fp32_restatement_is_within_the_derived_bounds_of_float64(shape):
    rows, width = shape
    z, gamma, beta, dy = lr.ln_case(rows, width)
    out = _run32(rows, width)
    y64, mean64, rstd64 = pr.ln_relu_fwd64(z, gamma, beta, EPS)
    e_y, e_mean, e_rstd = pr.ln_fwd_bound(z, gamma, beta, EPS)
    mask = out["y"] > 0
    assert mask.any() and not mask.all()
    dz64, dg64, db64 = pr.ln_relu_bwd64(dy, mask, z, gamma, EPS)
    e_dz, e_dg, e_db = pr.ln_bwd_bound(dy, mask, z, gamma, EPS)
    st = out["stats"].astype(np.float64)
    ratios = dict(y=(np.abs(out["y"] - y64) / e_y).max(), mean=(np.abs(st[:, 0] - mean64) / e_mean).max(),
                  rstd=(np.abs(st[:, 1] - rstd64) / e_rstd).max(),
                  dz=(np.abs(out["dz"] - dz64) / np.maximum(e_dz, 1e-300)).max(),
                  dgamma=(np.abs(lr.ln_fold32(out["part_g"]) - dg64) / np.maximum(e_dg, 1e-300)).max(),
                  dbeta=(np.abs(lr.ln_fold32(out["part_b"]) - db64) / np.maximum(e_db, 1e-300)).max())
    print("ln32 rows %5d width %4d error / bound: %s" % (rows, width, " ".join("%s %.3f" % kv for kv in ratios.items())))
    for k, v in ratios.items():
        assert v <= 1.0, (k, rows, width, v)
    if rows >= 3:                                               # the constant row: xhat = 0 exactly
        assert lr.bits(out["y"][-1]).tobytes() == lr.bits(np.maximum(beta, 0)).tobytes()
        assert st[-1, 0] == 0.75 and out["stats"][-1, 1] == np.float32(1) / np.sqrt(np.float32(0) + np.float32(EPS))


def _differs(a, b):
    """At least one bit of the row statistics or of dz differs."""
    return any(lr.bits(a[k]).tobytes() != lr.bits(b[k]).tobytes() for k in ("stats", "dz"))


ORDER_SHAPES = [s for s in SHAPES if s[0] >= 3]


@pytest.mark.parametrize("shape", ORDER_SHAPES, ids=_ids)
def test_restatement_rejects_a_plain_left_to_right_row_sum(shape):
    own, wrong = _run32(*shape), _run32(*shape, plain=True)
    assert _differs(own, wrong)


@pytest.mark.parametrize("shape", [s for s in ORDER_SHAPES if pr.ln_shape(*s)[0] < 64], ids=_ids)
def test_restatement_rejects_a_butterfly_of_the_waves_width(shape):
    """Width 64 where LPR is 8 or 16: the sums of the 8 or 4 rows of a wave run together."""
    own, wrong = _run32(*shape), _run32(*shape, butterfly=64)
    assert _differs(own, wrong)


@pytest.mark.parametrize("shape", [s for s in ORDER_SHAPES if s[1] in (768, 1020)], ids=_ids)
def test_restatement_rejects_the_float4_slots_taken_last_first(shape):
    """Only where three slots of most lanes are live: with two (V = 2; width 516, but for one lane) the swapped order is
    the same sum, addition being commutative."""
    assert _differs(_run32(*shape), _run32(*shape, v_descending=True))


def test_the_restated_orders_agree_where_they_must():
    """One float4 per lane and the butterfly of the row's own width written out: the keyword arguments change nothing."""
    for rows, width in ((65, 36), (65, 68), (3, 256)):
        own = _run32(rows, width)
        same = _run32(rows, width, butterfly=pr.ln_shape(rows, width)[0], v_descending=True)
        assert not _differs(own, same)


def test_row_sum_layout_on_a_hand_checked_row():
    """Width 36 (LPR 16, nine live lanes): the butterfly's tree written out by hand."""
    e = (np.arange(36, dtype=np.float32) * np.float32(1.1) + np.float32(1e4) * (np.arange(36) % 5 == 0)).reshape(1, 36)
    q = [np.float32(0)] * 16
    for lane in range(9):
        x = e[0, 4 * lane:4 * lane + 4]
        q[lane] = ((x[0] + x[1]) + x[2]) + x[3]
    for off in (8, 4, 2, 1):
        q = [q[lane] + q[lane ^ off] for lane in range(16)]
    assert lr.row_sums32(e)[0] == q[0] and all(v == q[0] for v in q)


def test_the_limit_shapes_take_the_trips_they_were_chosen_for():
    for rows, width in LN_SECOND_TRIP:
        lpr = pr.ln_shape(rows, width)[0]
        grid, iters = lr.ln_fwd_grid(rows, width)
        assert (grid, iters) == (2048, 2) and rows % (256 // lpr) != 0          # a second, ragged forward trip
        assert pr.ln_shape(rows, width)[2:4] == (256, 9)                        # nine backward trips of 256 blocks
        assert lr.ln_fwd_grid(rows - (256 // lpr) - 1, width)[1] == 1           # and none a block earlier
    assert [pr.ln_shape(3, w)[:2] for w in LN_WIDTHS] == [(8, 1), (16, 1), (64, 1), (64, 1), (64, 2), (64, 4), (64, 4),
                                                          (64, 4)]
    assert pr.ln_shape(1031, 1024)[2] == 256 and 2 * 256 * 1024 * 4 == 2 * 1024 * 1024      # the workspace's last float
