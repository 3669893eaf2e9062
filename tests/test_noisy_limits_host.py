"""CPU half of the noisy-layer limits tests (csrc/noisy.hip; the device half is tests/test_noisy_limits_gpu.py):

- the float32 restatements of tests/noisy_ref.py stay within the float64 bounds derived there;
- the restatements and the input builders the device tests reuse can tell the stated order from the nearest wrong one
  (the other fold width, a sequential sum, a tree of rows, the other association of the dueling data gradient, a fused
  multiply-add) -- so a device kernel that summed in another order could not pass the bit-for-bit comparisons;
- every refusal of the noisy entry points that needs no device, with its exact code."""
import ctypes

import numpy as np
import pytest

import noisy_ref as R

ARG, RANGE, ALIGN = -1, -2, -3
HOST_SPLITS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 1000, 4096]


# ---------------------------------------------------------------------------------------------- bounds

def test_fold_f32_is_within_its_float64_bound():
    worst = 0.
    for splits in HOST_SPLITS:
        part = R.fold_parts(splits, splits, 35)
        bias = (R._randn(splits + 1, 35) * 0.1).astype(np.float32)
        for zgn in (16, 64):                              # either width is a valid order of the same sum
            want, bound = R.fold_f64(part, splits, zgn, bias)
            r = R.ratio(R.fold_f32(part, splits, zgn, bias), want, bound)
            assert r <= 1, (splits, zgn, r)
            worst = max(worst, r)
    print("fold_f32: largest error / bound = %.4f" % worst)
    part = R.fold_parts(3, 0, 35)
    assert R.fold_f32(part, 0, 16, np.ones(35, np.float32)).tobytes() == part[0].tobytes()     # finished: unchanged


def test_combine_and_prep_restatements_are_within_their_bounds():
    worst = 0.
    for rows, units in R.FOLD_SHAPES:
        for k, (sw, ss) in enumerate(R.fold_cases(rows, units)):
            pw, ps = R.fold_parts(R.fold_seed(rows, units, 0, sw), sw, rows * units), \
                R.fold_parts(R.fold_seed(rows, units, 1, ss), ss, rows * units)
            bias, bs = (R._randn(k + 5, units) * 0.1).astype(np.float32), (R._randn(k + 6, units) * 0.1).astype(np.float32)
            feout, fnext = R.fe_like(k + 7, rows, units), R.fe_like(k + 8, rows, units)
            y, xs = R.combine_f32(pw, sw, ps, ss, bias, bs, feout, rows, units, k % 2, fnext)
            y64, by, xs64, bxs = R.combine_f64(pw, sw, ps, ss, bias, bs, feout, rows, units, k % 2, fnext)
            worst = max(worst, R.ratio(y, y64, by), R.ratio(xs, xs64, bxs))
    assert worst <= 1, worst
    print("combine_f32: largest error / bound = %.4f" % worst)
    worst = 0.
    for rows, units in R.PREP_SHAPES:
        g, feout = R.bwd_prep_case(rows + units, rows, units)
        g2, db, dbs = R.bwd_prep_f32(g, feout)
        g64, db64, b_db, dbs64, b_dbs = R.bwd_prep_f64(g, feout)
        assert R.ratio(g2, g64, R.EPS * np.abs(g64)) <= 1
        worst = max(worst, R.ratio(db, db64, b_db), R.ratio(dbs, dbs64, b_dbs))
    assert worst <= 1, worst
    print("bwd_prep_f32: largest error / bound = %.4f" % worst)


# ------------------------------------------------------------------------------ the restatements tell orders apart

def _differs(a, b):
    return a.tobytes() != b.tobytes()


@pytest.mark.parametrize("splits", [s for s in HOST_SPLITS if s >= 17])
def test_fold_restatement_rejects_the_other_width_and_a_sequential_sum(splits):
    part = R.fold_parts(splits, splits, 35)
    zgn = R.zgn_of(splits)
    own = R.fold_f32(part, splits, zgn)
    assert _differs(own, R.fold_f32(part, splits, 80 - zgn))
    assert _differs(own, R.sequential_f32(part, splits))


def test_device_fold_inputs_tell_the_orders_apart():
    """Every partial-sum array the device tests fold with 17 or more splits (tests/test_noisy_limits_gpu.py builds them
    with these same calls) gives another value under the other width and under a sequential sum."""
    seen = 0
    items = []
    for rows, units in R.FOLD_SHAPES:
        for sw, ss in R.fold_cases(rows, units):
            items += [(R.fold_seed(rows, units, 0, sw), sw, rows * units), (R.fold_seed(rows, units, 1, ss), ss, rows * units)]
    for units, split in R.DUEL_SHAPES:
        for rows in R.duel_rows(units):
            for sw, sl, sh in R.duel_cases(rows, units, split):
                items += [(R.fold_seed(rows, units, 0, sw), sw, rows * units), (R.fold_seed(rows, units, 1, sl), sl, rows * split),
                          (R.fold_seed(rows, units, 2, sh), sh, rows * (units - split))]
    for wide_from, splits in ((20, 19), (20, 20)):                                  # the moved threshold's two sides
        items.append((R.fold_seed(5, 7, 0, splits), splits, 35))
    for seed, splits, n in items:
        if splits < 17:
            continue
        part = R.fold_parts(seed, splits, n)
        own = R.fold_f32(part, splits, R.zgn_of(splits))
        assert _differs(own, R.fold_f32(part, splits, 80 - R.zgn_of(splits))), (seed, splits, n)
        assert _differs(own, R.sequential_f32(part, splits)), (seed, splits, n)
        seen += 1
    assert seen > 40
    run = [c for u, s in R.DUEL_SHAPES for r in R.duel_rows(u) for c in R.duel_cases(r, u, s)]
    assert (17, 0, 129) in run and (128, 16, 16) in run
    assert all(c in R.fold_cases(5, 7) for c in R.FOLD_SPLITS)                      # every pair runs somewhere


def test_bwd_dx_inputs_tell_the_associations_apart():
    for rows, fan_in in R.DX_SHAPES:
        a, p, e, q, h = R.bwd_dx_case(rows * fan_in, rows, fan_in)
        assert _differs(R.duel_bwd_dx_f32(a, p, e, q, h), R.duel_bwd_dx_other_f32(a, p, e, q, h)), (rows, fan_in)
        assert _differs(R.bwd_dx_f32(a, p, e), R.bwd_dx_fused(a, p, e)), (rows, fan_in)            # -ffp-contract=off
        assert R.bwd_dx_f32(a, p, e)[0, 1] == 0 and R.duel_bwd_dx_f32(a, p, e, q, h)[0, 1] == 0


def test_bwd_prep_inputs_tell_a_tree_from_the_row_order():
    """(Two rows or fewer have one order only: a + b.)"""
    cases = [(rows, units) for rows, units in R.PREP_SHAPES] + \
        [(rows, units) for units, _ in R.DUEL_PREP_SHAPES for rows in R.DUEL_PREP_ROWS]
    seen = 0
    for rows, units in cases:
        if rows < 3:
            continue
        g, feout = R.bwd_prep_case(rows + units, rows, units)
        g2, db, dbs = R.bwd_prep_f32(g, feout)
        assert _differs(db, R.pairwise_f32(g)), (rows, units)
        assert _differs(dbs, R.pairwise_f32(g2)), (rows, units)
        seen += 1
    assert seen >= 9


# ---------------------------------------------------------------------------------------------- refusals

@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


OK, ODD = ctypes.c_void_p(16), ctypes.c_void_p(20)       # never dereferenced: every call below is refused first


def _refused(lib, rc, code, text):
    assert rc == code, (rc, lib.arl_last_error())
    assert text.encode() in lib.arl_last_error(), lib.arl_last_error()


def _noise(lib, n_layers=1, rows=4, **kw):
    from accel_rl_amd import _lib
    layers = (_lib.ArlNoisyLayer * n_layers)()
    for it in layers:
        it.fein, it.feout, it.x, it.xs = 16, 16, None, None
        it.fan_in, it.units, it.out_stride, it.layer = 8, 3, 4, 0
        for k, v in kw.items():
            setattr(it, k, v)
    return lib.arl_noisy_noise(OK, layers, n_layers, rows, 1, None)


def test_noise_refusals(lib):
    _refused(lib, _noise(lib, n_layers=9), RANGE, "ARL_NOISY_MAX_LAYERS")
    _refused(lib, _noise(lib, fan_in=6), RANGE, "multiples of 4")
    _refused(lib, _noise(lib, out_stride=6), RANGE, "multiples of 4")
    _refused(lib, _noise(lib, units=5), ARG, "layer sizes")                     # out_stride 4 < units
    _refused(lib, _noise(lib, x=16), ARG, "null pointer in a layer")            # x without xs
    _refused(lib, _noise(lib, layer=-1), ARG, "layer index")
    _refused(lib, _noise(lib, fein=20), ALIGN, "alignment")
    _refused(lib, _noise(lib, feout=20), ALIGN, "alignment")
    _refused(lib, _noise(lib, x=16, xs=20), ALIGN, "alignment")


def test_noise_refuses_what_its_siblings_refuse(lib):
    """arl_noisy_normals and arl_noisy_draws refuse layer >= 2^30 (2 layer + which would overflow an int) and more than
    2^40 elements; arl_noisy_noise makes the same streams and refuses the same."""
    _refused(lib, _noise(lib, layer=2 ** 30), ARG, "layer index")
    _refused(lib, _noise(lib, layer=2 ** 31 - 1), ARG, "layer index")
    _refused(lib, _noise(lib, rows=2 ** 40 // 8 + 1), RANGE, "too large")                     # rows x fan_in
    _refused(lib, _noise(lib, rows=2 ** 40 // 16 + 1, fan_in=4, out_stride=16), RANGE, "too large")    # rows x out_stride
    _refused(lib, lib.arl_noisy_normals(1, 0, 2 ** 30, 0, 4, 8, 1, OK, None, None, None), ARG, "layer")
    _refused(lib, lib.arl_noisy_normals(1, 0, 0, 0, 2 ** 40 // 8 + 1, 8, 1, OK, None, None, None), RANGE, "too large")


def _draws(lib, n_draws=1, rows=4, **kw):
    from accel_rl_amd import _lib
    draws = (_lib.ArlNoisyDraw * n_draws)()
    for it in draws:
        it.f, it.x, it.xs, it.width, it.pitch, it.layer, it.which = 16, None, None, 8, 8, 0, 0
        for k, v in kw.items():
            setattr(it, k, v)
    return lib.arl_noisy_draws(OK, draws, n_draws, rows, 1, None)


def test_draws_refusals(lib):
    _refused(lib, _draws(lib, n_draws=17), RANGE, "ARL_NOISY_MAX_DRAWS")
    _refused(lib, _draws(lib, pitch=4), ARG, "draw sizes")
    _refused(lib, _draws(lib, x=16, xs=16, which=1), ARG, "e_out draw")
    _refused(lib, _draws(lib, x=16), ARG, "null pointer in a draw")
    _refused(lib, _draws(lib, width=6), RANGE, "multiples of 4")
    _refused(lib, _draws(lib, pitch=10), RANGE, "multiples of 4")
    _refused(lib, _draws(lib, f=20), ALIGN, "alignment")
    _refused(lib, _draws(lib, x=20, xs=16), ALIGN, "alignment")
    _refused(lib, _draws(lib, layer=2 ** 30), ARG, "layer")
    _refused(lib, _draws(lib, which=2), ARG, "which")
    _refused(lib, _draws(lib, rows=2 ** 40 // 8 + 1), RANGE, "too large")


def _item(total, splits=2, part=16):
    from accel_rl_amd import _lib
    return ctypes.byref(_lib.ArlFoldItem(part, None, total, splits, 0))


def test_combine_refusals(lib):
    rows, units, split = 4, 8, 3

    def dense(w=_item(32), s=_item(32), fnext=None, xs=None):
        return lib.arl_noisy_dense_combine(w, None, s, None, OK, rows, units, 1, OK, fnext, xs, None, None)

    def duel(w=_item(32), lo=_item(12), hi=_item(20), fnext=None, xs=None):
        return lib.arl_noisy_duel_combine(w, None, lo, hi, None, OK, rows, units, split, 1, OK, fnext, xs, None, None)
    for call in (dense, duel):
        _refused(lib, call(fnext=OK), ARG, "both or neither")
        _refused(lib, call(xs=OK), ARG, "both or neither")
        _refused(lib, call(w=_item(32, splits=-1)), ARG, "fold items")
        _refused(lib, call(w=_item(32, splits=4097)), ARG, "fold items")
        _refused(lib, call(w=_item(28)), ARG, "fold items")                     # total != rows x units
        _refused(lib, call(w=_item(32, part=None)), ARG, "fold items")
    _refused(lib, dense(s=_item(36)), ARG, "fold items")
    _refused(lib, dense(s=_item(32, splits=4097)), ARG, "fold items")
    _refused(lib, duel(lo=_item(20)), ARG, "fold items")                        # total != rows x split
    _refused(lib, duel(hi=_item(12)), ARG, "fold items")                        # total != rows x (units - split)
    _refused(lib, duel(lo=_item(12, splits=-1)), ARG, "fold items")
    _refused(lib, duel(hi=_item(20, splits=4097)), ARG, "fold items")
    for bad in (0, units):
        assert lib.arl_noisy_duel_combine(_item(32), None, _item(12), _item(20), None, OK, rows, units, bad, 1, OK, None,
                                          None, None, None) == ARG


def test_bwd_dx_refusals(lib):
    _refused(lib, lib.arl_noisy_dense_bwd_dx(OK, OK, OK, 4, 6, OK, None), RANGE, "multiple of 4")
    _refused(lib, lib.arl_noisy_duel_bwd_dx(OK, OK, OK, OK, OK, 4, 6, OK, None), RANGE, "multiple of 4")
    for k in range(4):
        p = [OK] * 4
        p[k] = ODD
        _refused(lib, lib.arl_noisy_dense_bwd_dx(p[0], p[1], p[2], 4, 8, p[3], None), ALIGN, "alignment")
    for k in range(6):
        p = [OK] * 6
        p[k] = ODD
        _refused(lib, lib.arl_noisy_duel_bwd_dx(p[0], p[1], p[2], p[3], p[4], 4, 8, p[5], None), ALIGN, "alignment")
    assert lib.arl_noisy_duel_bwd_prep(OK, OK, 4, 8, 0, OK, OK, OK, OK, None) == ARG
    assert lib.arl_noisy_duel_bwd_prep(OK, OK, 4, 8, 8, OK, OK, OK, OK, None) == ARG
