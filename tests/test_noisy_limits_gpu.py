"""The noisy-layer kernels (csrc/noisy.hip) at the edges of what their entry points accept, driven directly and compared
BIT FOR BIT with the NumPy float32 restatements of tests/noisy_ref.py (the file is compiled with -ffp-contract=off and
is fp32 element-wise arithmetic in a stated order), and with the float64 versions within the bounds derived there.

a. arl_noisy_noise against arl_noisy_normals (the same device function through another launch) and the generator's
   NumPy statement: one, three and ARL_NOISY_MAX_LAYERS layers, row groups with a short last group, a workgroup that
   spans many segments and segment boundaries inside workgroups, counters up to 2^63 - 1, zero columns past `units`.
b. arl_noisy_draws into column slices of wider buffers, 1 and ARL_NOISY_MAX_DRAWS draws, and two refused calls.
c. arl_noisy_dense_combine: both folds in both widths, around the threshold (also moved), totals that are no multiple
   of 4, 4096 splits; every option; tied to arl_fold_many.
d. arl_noisy_duel_combine, also against arl_noisy_dense_combine on the concatenated sigma parts.
e. arl_noisy_dense_bwd_prep / arl_noisy_duel_bwd_prep: rows summed in order.
f. arl_noisy_dense_bwd_dx / arl_noisy_duel_bwd_dx: the stated association, in place and out of place.
g. Two launches of every entry point give the same bits.

tests/test_noisy_limits_host.py shows on the CPU that the inputs built here (same builders, same seeds) give other
bits under the nearest wrong order, so the comparisons below cannot pass by accident.

Every output is carved from one NaN-poisoned buffer at a 16-byte-aligned offset with at least 64 poisoned floats on
either side, and every test ends by checking that nothing outside the outputs was written."""
import numpy as np
import pytest
import torch

import noisy_ref as R
from noisy_ref import noisy_words_normals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
WORST = {}                      # section -> largest error / bound seen (printed by each test: run with -s)


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


class Arena(object):
    """One NaN-poisoned float buffer; carve() hands out the outputs in order, check() proves the rest untouched."""

    def __init__(self, *sizes):
        total = GUARD + sum((n + 3) // 4 * 4 + GUARD + 4 for n in sizes)
        self.buf = torch.full((total,), float("nan"), dtype=torch.float32, device=DEV)
        self.poison = int(self.buf[:1].view(torch.int32).item())
        self.used = np.zeros(total, bool)
        self.pos = GUARD

    def carve(self, n, shift=0):
        """n floats starting `shift` floats past a 16-byte boundary."""
        start = (self.pos + 3) // 4 * 4 + shift
        assert start - GUARD >= 0 and not self.used[start - GUARD:start].any()
        assert start + n + GUARD <= self.buf.numel(), "arena too small"
        self.used[start:start + n] = True
        self.pos = start + n + GUARD
        out = self.buf[start:start + n]
        assert (out.data_ptr() - 4 * shift) % 16 == 0
        return out

    def release(self, t, keep):
        """Of a carved [rows][pitch] block only the columns in `keep` (bool[pitch]) are outputs: the rest is guard."""
        start = (t.data_ptr() - self.buf.data_ptr()) // 4
        self.used[start:start + t.numel()] = np.tile(keep, t.numel() // len(keep))

    def check(self):
        torch.cuda.synchronize()
        bits = self.buf.view(torch.int32).cpu().numpy()
        assert (bits[~self.used] == self.poison).all(), "a launch wrote outside its outputs"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.contiguous().cpu().numpy()


def _bits(a):
    a = _host(a) if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def _same_bits(got, want, what=""):
    got, want = _bits(got).reshape(-1), _bits(want).reshape(-1)
    np.testing.assert_array_equal(got, want, err_msg=str(what))


def _state(seed, counter):
    """-> (int64[4] = guard, seed, counter, guard; its middle two as the entry points' state)."""
    t = torch.tensor([-11, seed, counter, -13], dtype=torch.int64, device=DEV)
    return t, t[1:3]


def _note(section, r):
    WORST[section] = max(WORST.get(section, 0.), r)
    assert r <= 1, (section, r)


# ---------------------------------------------------------------------------------------------- a. arl_noisy_noise

ROWS_RPD = [(1, 1), (5, 1), (5, 5), (7, 3), (64, 32), (257, 1)]
SEEDS = [(1234, 0), (-7, 2 ** 32 - 1), (2 ** 40 + 3, 2 ** 32), (99, 2 ** 33 + 7), (5, 2 ** 63 - 1)]
# every (rows, rows_per_draw) and every (seed, counter) at least once; the large counters at both ends of the row sizes
NOISE_COVER = [(ROWS_RPD[i], SEEDS[j]) for i, j in ((0, 0), (0, 4), (1, 1), (2, 2), (3, 3), (3, 1), (4, 4), (4, 2),
                                                     (5, 0), (5, 3))]
# (fan_in, units, out_stride, layer, x given)
LAYER_LISTS = {
    "one": [(4, 1, 4, 0, False)],
    "three": [(8, 3, 4, 0, True), (52, 6, 32, 5, False), (260, 7, 16, 2 ** 30 - 1, False)],
    "eight": [(4, 1, 4, 0, True), (8, 3, 4, 1, False), (12, 5, 8, 2, False), (20, 8, 8, 3, True), (36, 9, 12, 7, False),
              (52, 13, 16, 100, False), (68, 30, 32, 2 ** 20, False), (100, 33, 36, 2 ** 30 - 1, True)],
}


def _noise_x(seed, rows, fan_in):
    """Zeros, negatives and magnitudes up to 1e30 (|f| <= 2.43: the product stays finite)."""
    x = R._randn(seed, rows, fan_in)
    flat = x.reshape(-1)
    flat[1::7] *= np.float32(2.5e29)
    np.clip(flat, -1e30, 1e30, out=flat)
    flat[::5] = 0
    flat[1] = -1e30
    return x


def _run_noise(L, layers, rows, rpd, seed, counter):
    """One arl_noisy_noise launch on carved outputs -> per layer (fein, feout, x or None, xs or None) on the host."""
    sizes = []
    for fan_in, units, stride, layer, has_x in layers:
        sizes += [rows * fan_in, rows * stride] + ([rows * fan_in] if has_x else [])
    arena = Arena(*sizes)
    full, state = _state(seed, counter)
    args, keep = [], []
    for k, (fan_in, units, stride, layer, has_x) in enumerate(layers):
        fein, feout = arena.carve(rows * fan_in).view(rows, fan_in), arena.carve(rows * stride).view(rows, stride)
        x = _dev(_noise_x(31 * k + rows, rows, fan_in)) if has_x else None
        xs = arena.carve(rows * fan_in).view(rows, fan_in) if has_x else None
        args.append((fein, feout, x, xs, fan_in, units, stride, layer))
        keep.append((fein, feout, x, xs))
    L.noisy_noise(state, args, rows, rpd)
    arena.check()
    assert full.cpu().tolist() == [-11, seed, counter, -13]                  # this launch does not advance the counter
    return [tuple(None if t is None else _host(t) for t in ts) for ts in keep]


def _normals(L, seed, counter, layer, which, rows, width, rpd):
    """arl_noisy_normals -> (words, e, f) on the host."""
    e = torch.empty((rows, width), dtype=torch.float32, device=DEV)
    f = torch.empty_like(e)
    w = torch.empty((rows, width), dtype=torch.int32, device=DEV)
    L.noisy_normals(seed, counter, layer, which, rows, width, rpd, e=e, f=f, words=w)
    return _host(w).view(np.uint32), _host(e), _host(f)


def _check_draw(L, got, seed, counter, layer, which, rows, width, rpd, what):
    """got f32[rows][width] is the (layer, which) draw: arl_noisy_normals' bits; that launch against the NumPy statement
    within test_device_generator_equals_numpy_statement's tolerances; groups; range."""
    words, e, f = _normals(L, seed, counter, layer, which, rows, width, rpd)
    _same_bits(got, f, what)
    w_np, e_np, f_np = noisy_words_normals(seed, counter, layer, which, rows, width, rpd)
    np.testing.assert_array_equal(words, w_np, err_msg=str(what))
    assert (np.abs(e - e_np) <= 1e-6 * np.maximum(1, np.abs(e_np))).all(), what
    np.testing.assert_allclose(f, f_np, rtol=1e-6, atol=1e-6, err_msg=str(what))
    assert np.isfinite(got).all() and (np.abs(got) <= np.sqrt(5.9)).all(), what     # u1 >= 2^-25: |e| <= sqrt(50 ln 2)
    first = (np.arange(rows) // rpd) * rpd
    _same_bits(got, got[first], what)                                               # a group shares its draw
    heads = got[::rpd]
    for a, b in zip(heads[:-1], heads[1:]):
        assert a.tobytes() != b.tobytes(), what                                     # consecutive groups do not
    return f


@pytest.mark.parametrize("name", list(LAYER_LISTS))
def test_noise_launch_equals_the_generator(L, name):
    layers = LAYER_LISTS[name]
    seg = [w // 4 for fan_in, _, stride, _, _ in layers for w in (fan_in, stride)]          # threads per row, per segment
    if name == "eight":
        assert len(layers) == L.NOISY_MAX_LAYERS and sum(seg) < 256                         # rows 1: one workgroup, 16 segments
        starts = np.cumsum([257 * s for s in seg])[:-1]
        assert (starts % 256 != 0).all()                                                    # rows 257: every boundary inside one
    if name == "three":
        assert sum(seg) < 256                                                               # rows 1: six segments, one workgroup
    for (rows, rpd), (seed, counter) in NOISE_COVER:
        out = _run_noise(L, layers, rows, rpd, seed, counter)
        for (fan_in, units, stride, layer, has_x), (fein, feout, x, xs) in zip(layers, out):
            what = (name, rows, rpd, seed, counter, layer)
            _check_draw(L, fein, seed, counter, layer, 0, rows, fan_in, rpd, what)
            _check_draw(L, feout[:, :units], seed, counter, layer, 1, rows, units, rpd, what)
            assert (_bits(feout[:, units:]) == 0).all(), what                               # +0.0, by its bits
            if has_x:
                assert (x == 0).any() and (x < 0).any() and np.abs(x).max() >= 1e29
                _same_bits(xs, x * fein, what)


# ---------------------------------------------------------------------------------------------- b. arl_noisy_draws

# buffers: name -> pitch; draws: (buffer, c0, width, layer, which, x given).  c0 in {0, 4, 36}, pitch in {width, width + 4,
# 2 width + 8}; (D, D), (G, H) repeat a (layer, which); (E, F), (J, K), (I, I) are which 0 / 1 twins.
DRAW_PITCH = dict(A=8, B=16, C=88, D=64, E=4, F=8, G=260, H=264, I=112, J=16, K=16, M=12, N=72)
DRAWS_16 = [("A", 0, 8, 0, 0, True), ("B", 4, 12, 0, 1, False), ("C", 0, 36, 1, 0, True), ("C", 36, 40, 2, 0, True),
            ("D", 36, 28, 1, 1, False), ("D", 4, 28, 1, 1, False), ("E", 0, 4, 2 ** 30 - 1, 0, False),
            ("F", 4, 4, 2 ** 30 - 1, 1, False), ("G", 0, 260, 5, 0, True), ("H", 4, 260, 5, 0, False),
            ("I", 36, 52, 7, 1, False), ("I", 0, 36, 7, 0, False), ("J", 0, 16, 8, 0, False), ("K", 0, 16, 8, 1, False),
            ("M", 4, 8, 9, 0, True), ("N", 36, 32, 9, 1, False)]
DRAWS_1 = [("D", 36, 28, 3, 0, True)]
DRAW_RUNS = [(1, 1, SEEDS[1]), (7, 3, SEEDS[2]), (33, 33, SEEDS[3]), (257, 1, SEEDS[4])]


def _run_draws(L, plan, rows, rpd, seed, counter):
    """One arl_noisy_draws launch -> [(f slice, x slice or None, xs slice or None)] on the host, in plan order."""
    names = sorted({d[0] for d in plan})
    with_x = sorted({d[0] for d in plan if d[5]})
    arena = Arena(*([rows * DRAW_PITCH[n] for n in names] + [rows * DRAW_PITCH[n] for n in with_x]))
    fbuf = {n: arena.carve(rows * DRAW_PITCH[n]).view(rows, DRAW_PITCH[n]) for n in names}
    xsbuf = {n: arena.carve(rows * DRAW_PITCH[n]).view(rows, DRAW_PITCH[n]) for n in with_x}
    xbuf = {n: _dev(_noise_x(ord(n) + rows, rows, DRAW_PITCH[n])) for n in with_x}
    written = {n: np.zeros(DRAW_PITCH[n], bool) for n in names}
    written_xs = {n: np.zeros(DRAW_PITCH[n], bool) for n in with_x}
    args = []
    for n, c0, width, layer, which, has_x in plan:
        assert c0 + width <= DRAW_PITCH[n] and not written[n][c0:c0 + width].any()
        written[n][c0:c0 + width] = True
        if has_x:
            written_xs[n][c0:c0 + width] = True
        cols = slice(c0, c0 + width)
        args.append((fbuf[n][:, cols], xbuf[n][:, cols] if has_x else None, xsbuf[n][:, cols] if has_x else None, width,
                     DRAW_PITCH[n], layer, which))
    for n in names:
        arena.release(fbuf[n], written[n])
    for n in with_x:
        arena.release(xsbuf[n], written_xs[n])
    full, state = _state(seed, counter)
    L.noisy_draws(state, args, rows, rpd)
    arena.check()                                                            # columns outside the slices: still poison
    assert full.cpu().tolist() == [-11, seed, counter, -13]
    return [tuple(None if t is None else _host(t) for t in a[:3]) for a in args]


@pytest.mark.parametrize("plan", [DRAWS_1, DRAWS_16], ids=["1", "16"])
def test_draws_into_column_slices(L, plan):
    assert len(plan) in (1, L.NOISY_MAX_DRAWS)
    for rows, rpd, (seed, counter) in DRAW_RUNS:
        out = _run_draws(L, plan, rows, rpd, seed, counter)
        by_key = {}
        for (n, c0, width, layer, which, has_x), (f, x, xs) in zip(plan, out):
            what = (rows, rpd, seed, counter, n, c0, layer, which)
            _check_draw(L, f, seed, counter, layer, which, rows, width, rpd, what)
            if has_x:
                _same_bits(xs, x * f, what)
            by_key.setdefault((layer, which), []).append(f)
        for (layer, which), fs in by_key.items():
            for f in fs[1:]:
                _same_bits(f, fs[0], (layer, which))                         # one stream, two places: the same bits
            twin = by_key.get((layer, 1 - which))
            if twin is not None:
                w = min(fs[0].shape[1], twin[0].shape[1])
                assert (fs[0][:, :w] == twin[0][:, :w]).mean() < 0.5, (layer, which)
        if len(plan) > 1:
            assert sum(len(v) > 1 for v in by_key.values()) >= 2 and sum((k[0], 1 - k[1]) in by_key for k in by_key) >= 6


@pytest.mark.parametrize("bad", ["17 draws", "misaligned f"])
def test_refused_draws_write_nothing(L, bad):
    rows, width = 5, 8
    arena = Arena(rows * width + 4)
    f = arena.carve(rows * width + 4)
    arena.used[:] = False                                                    # a refused call has no outputs
    full, state = _state(77, 5)
    n = 17 if bad == "17 draws" else 1
    draws = (L.ArlNoisyDraw * n)()
    for it in draws:
        it.f, it.x, it.xs = f.data_ptr() + (4 if bad == "misaligned f" else 0), None, None
        it.width, it.pitch, it.layer, it.which = width, width, 0, 0
    with pytest.raises(RuntimeError, match="code -2" if n == 17 else "code -3"):
        L._check(L.load().arl_noisy_draws(state.data_ptr(), draws, n, rows, 1, L.stream_ptr()), "arl_noisy_draws")
    arena.check()
    assert full.cpu().tolist() == [-11, 77, 5, -13]


# ------------------------------------------------------------------------------------- c. arl_noisy_dense_combine

def _item(L, part, splits, total, out=None):
    assert part.numel() == max(splits, 1) * total and part.is_contiguous()
    return L.ArlFoldItem(part.data_ptr(), None if out is None else out.data_ptr(), total, splits, 0)


def _vec(seed, units, given):
    return (R._randn(seed, units) * 0.1).astype(np.float32) if given else None


def _opt_dev(a, shift=0):
    """Device copy of an input (None stays None), `shift` floats past a 16-byte boundary."""
    if a is None:
        return None
    t = torch.empty(a.size + shift, dtype=torch.float32, device=DEV)
    t[shift:] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    return t[shift:]


def _options(k):
    """The k-th case of a shape: which optional arguments it passes; case 2 misaligns every pointer the header leaves
    free (y, xs_next, feout, fein_next) by one float."""
    return dict(bias=k % 2 == 0, bsig=k % 3 != 0, relu=(k // 2) % 2, nxt=k % 4 != 1, state=k % 3 != 1, shift=int(k == 2))


def _run_combine(L, rows, units, sw, ss, bias, bsig, relu, nxt, state, shift, duel=None):
    """One combine launch (dueling: duel = (split, lo splits, hi splits), ss unused) on carved outputs ->
    (y, xs_next or None, inputs for the restatement)."""
    n = rows * units
    pw = R.fold_parts(R.fold_seed(rows, units, 0, sw), sw, n)
    if duel is None:
        sig = [(R.fold_parts(R.fold_seed(rows, units, 1, ss), ss, n), ss, n)]
    else:
        split, sl, sh = duel
        sig = [(R.fold_parts(R.fold_seed(rows, units, 1, sl), sl, rows * split), sl, rows * split),
               (R.fold_parts(R.fold_seed(rows, units, 2, sh), sh, rows * (units - split)), sh, rows * (units - split))]
    b, bs = _vec(rows + 1, units, bias), _vec(rows + 2, units, bsig)
    feout = R.fe_like(rows + units, rows, units)
    fnext = R.fe_like(rows + units + 1, rows, units) if nxt else None
    arena = Arena(*([n + shift] * (2 if nxt else 1)))
    y = arena.carve(n, shift)
    xs = arena.carve(n, shift) if nxt else None
    full, st = _state(321, 2 ** 32 - 1)
    d_pw, d_sig = _dev(pw), [_dev(p) for p, _, _ in sig]
    it_w = _item(L, d_pw, sw, n)
    it_s = [_item(L, d, s, tot) for d, (_, s, tot) in zip(d_sig, sig)]
    d_b, d_bs, d_fe, d_fn = _opt_dev(b), _opt_dev(bs), _opt_dev(feout, shift), _opt_dev(fnext, shift)
    if duel is None:
        L.noisy_dense_combine(it_w, d_b, it_s[0], d_bs, d_fe, y.view(rows, units), relu, fein_next=d_fn, xs_next=xs,
                              state=st if state else None)
    else:
        L.noisy_duel_combine(it_w, d_b, it_s[0], it_s[1], d_bs, d_fe, y.view(rows, units), duel[0], relu, fein_next=d_fn,
                             xs_next=xs, state=st if state else None)
    arena.check()
    # state[1] += 1 exactly once whatever the grid size; without state nothing moves
    assert full.cpu().tolist() == [-11, 321, 2 ** 32 - 1 + int(bool(state)), -13]
    return _host(y), None if xs is None else _host(xs), dict(pw=pw, sig=sig, bias=b, b_sigma=bs, feout=feout, fnext=fnext)


def _check_combine(section, got_y, got_xs, inp, rows, units, sw, relu, wide_from=R.WIDE_FROM, split=None, what=""):
    if split is None:
        (ps, ss, _), = inp["sig"]
        args = (inp["pw"], sw, ps, ss, inp["bias"], inp["b_sigma"], inp["feout"], rows, units, relu, inp["fnext"], wide_from)
        f32, f64 = R.combine_f32, R.combine_f64
    else:
        (lo, sl, _), (hi, sh, _) = inp["sig"]
        args = (inp["pw"], sw, lo, sl, hi, sh, inp["bias"], inp["b_sigma"], inp["feout"], rows, units, split, relu,
                inp["fnext"], wide_from)
        f32, f64 = R.duel_combine_f32, R.duel_combine_f64
    y, xs = f32(*args)
    _same_bits(got_y, y, what)
    y64, b_y, xs64, b_xs = f64(*args)
    _note(section, R.ratio(got_y, y64, b_y))
    if xs is not None:
        _same_bits(got_xs, xs, what)
        _note(section, R.ratio(got_xs, xs64, b_xs))
    return y, xs


@pytest.mark.parametrize("rows,units", R.FOLD_SHAPES)
def test_dense_combine_equals_the_restatement(L, rows, units):
    cases = R.fold_cases(rows, units)
    assert len(cases) >= 8
    for k, (sw, ss) in enumerate(cases):
        o = _options(k)
        y, xs, inp = _run_combine(L, rows, units, sw, ss, **o)
        _check_combine("c", y, xs, inp, rows, units, sw, o["relu"], what=(rows, units, sw, ss, o))
    print("dense combine %s: largest error / bound so far %.4f" % ((rows, units), WORST["c"]))


def test_fold_threshold_moves_with_the_dev_switch(L):
    rows, units = 5, 7
    o = dict(bias=True, bsig=True, relu=0, nxt=True, state=True, shift=0)
    try:
        L.load().arl_dev_fold_wide_from(20)
        y, xs, inp = _run_combine(L, rows, units, 19, 20, **o)
    finally:
        L.load().arl_dev_fold_wide_from(0)
    want, _ = _check_combine("c", y, xs, inp, rows, units, 19, 0, wide_from=20)       # 19: 16-way, 20: 64-way
    for other in (19, 21):                                                           # ... and not on either other side
        assert R.combine_f32(inp["pw"], 19, inp["sig"][0][0], 20, inp["bias"], inp["b_sigma"], inp["feout"], rows, units, 0,
                             inp["fnext"], other)[0].tobytes() != want.tobytes()
    y, xs, inp = _run_combine(L, rows, units, 19, 20, **o)                            # restored: both 16-way again
    _check_combine("c", y, xs, inp, rows, units, 19, 0)


@pytest.mark.parametrize("rows,units", [s for s in R.FOLD_SHAPES if s[0] * s[1] % 4 == 0])
def test_combine_folds_as_fold_many_does(L, rows, units):
    """arl_fold_many's sum of the W product, plus the bias in float32, is what a combine with a finished all-zero sigma
    product and a finite f(e_out) gives."""
    n = rows * units
    bias = _vec(3, units, True)
    feout, zeros = _dev(R.fe_like(9, rows, units)), torch.zeros(n, device=DEV)
    for sw, _ in R.fold_cases(rows, units):
        if sw == 0:
            continue
        part = _dev(R.fold_parts(R.fold_seed(rows, units, 0, sw), sw, n))
        arena = Arena(n, n)
        out, y = arena.carve(n), arena.carve(n)
        items = (L.ArlFoldItem * 1)(_item(L, part, sw, n, out))
        L._check(L.load().arl_fold_many(items, 1, L.stream_ptr()), "arl_fold_many")
        L.noisy_dense_combine(items[0], _dev(bias), _item(L, zeros, 0, n), None, feout, y.view(rows, units), 0)
        arena.check()
        want = torch.from_numpy(_host(out).reshape(rows, units) + bias).reshape(-1)
        # values, not bits: a + f(e_out) * 0 turns a sum of -0.f into +0.f
        assert torch.equal(y.cpu(), want), (rows, units, sw)


# -------------------------------------------------------------------------------------- d. arl_noisy_duel_combine

@pytest.mark.parametrize("units,split", R.DUEL_SHAPES)
def test_duel_combine_equals_the_restatement_and_the_dense_combine(L, units, split):
    k = 0
    for rows in R.duel_rows(units):
        cases = R.duel_cases(rows, units, split)
        assert len(cases) >= 4
        for sw, sl, sh in cases:
            o = _options(k)
            k += 1
            what = (rows, units, split, sw, sl, sh, o)
            y, xs, inp = _run_combine(L, rows, units, sw, None, duel=(split, sl, sh), **o)
            _check_combine("d", y, xs, inp, rows, units, sw, o["relu"], split=split, what=what)
            if sl != sh:
                continue
            # equal split counts: one sigma product over all units, the streams' parts side by side
            (lo, _, _), (hi, _, _) = inp["sig"]
            cat = np.concatenate([lo.reshape(-1, rows, split), hi.reshape(-1, rows, units - split)], axis=2)
            n = rows * units
            arena = Arena(n, n)
            y2, xs2 = arena.carve(n), arena.carve(n) if o["nxt"] else None
            d_pw, d_cat = _dev(inp["pw"]), _dev(cat.reshape(-1, n))
            L.noisy_dense_combine(_item(L, d_pw, sw, n), _opt_dev(inp["bias"]), _item(L, d_cat, sl, n),
                                  _opt_dev(inp["b_sigma"]), _dev(inp["feout"]), y2.view(rows, units), o["relu"],
                                  fein_next=_opt_dev(inp["fnext"]), xs_next=xs2)
            arena.check()
            _same_bits(y2, y, what)
            if xs2 is not None:
                _same_bits(xs2, xs, what)
    print("duel combine %s: largest error / bound so far %.4f" % ((units, split), WORST["d"]))


# ------------------------------------------------------------- e. arl_noisy_dense_bwd_prep / arl_noisy_duel_bwd_prep

def _run_prep(L, rows, units, split=None):
    """-> (g2 or (g2_lo, g2_hi), db, db_sigma) on the host, and the inputs."""
    g, feout = R.bwd_prep_case(rows + units, rows, units)
    d_g, d_fe = _dev(g), _dev(feout)
    if split is None:
        arena = Arena(rows * units, units, units)
        g2 = arena.carve(rows * units).view(rows, units)
        db, dbs = arena.carve(units), arena.carve(units)
        L.noisy_dense_bwd_prep(d_g, d_fe, g2, db, dbs)
        out = _host(g2)
    else:
        arena = Arena(rows * split, rows * (units - split), units, units)
        lo, hi = arena.carve(rows * split).view(rows, split), arena.carve(rows * (units - split)).view(rows, units - split)
        db, dbs = arena.carve(units), arena.carve(units)
        L.noisy_duel_bwd_prep(d_g, d_fe, split, lo, hi, db, dbs)
        out = (_host(lo), _host(hi))
    arena.check()                                                            # (the guards between g2_lo and g2_hi too)
    _same_bits(d_g, g)
    _same_bits(d_fe, feout)
    return out, _host(db), _host(dbs), g, feout


@pytest.mark.parametrize("rows,units", R.PREP_SHAPES)
def test_bwd_prep_sums_rows_in_order(L, rows, units):
    g2, db, dbs, g, feout = _run_prep(L, rows, units)
    want_g2, want_db, want_dbs = R.bwd_prep_f32(g, feout)
    _same_bits(g2, want_g2)
    _same_bits(db, want_db)
    _same_bits(dbs, want_dbs)
    _, db64, b_db, dbs64, b_dbs = R.bwd_prep_f64(g, feout)
    _note("e", R.ratio(db, db64, b_db))
    _note("e", R.ratio(dbs, dbs64, b_dbs))
    print("bwd_prep %s: largest error / bound so far %.4f" % ((rows, units), WORST["e"]))


@pytest.mark.parametrize("units,split", R.DUEL_PREP_SHAPES)
def test_duel_bwd_prep_is_the_plain_kernel_in_two_blocks(L, units, split):
    for rows in R.DUEL_PREP_ROWS:
        (lo, hi), db, dbs, g, feout = _run_prep(L, rows, units, split)
        want_lo, want_hi, want_db, want_dbs = R.duel_bwd_prep_f32(g, feout, split)
        for got, want in ((lo, want_lo), (hi, want_hi), (db, want_db), (dbs, want_dbs)):
            _same_bits(got, want, (rows, units, split))
        _, db64, b_db, dbs64, b_dbs = R.bwd_prep_f64(g, feout)
        _note("e", R.ratio(db, db64, b_db))
        _note("e", R.ratio(dbs, dbs64, b_dbs))
        g2, p_db, p_dbs, _, _ = _run_prep(L, rows, units)                    # the plain kernel on the same input
        _same_bits(db, p_db)
        _same_bits(dbs, p_dbs)
        _same_bits(lo, g2[:, :split])
        _same_bits(hi, g2[:, split:])


# ------------------------------------------------------------------ f. arl_noisy_dense_bwd_dx / arl_noisy_duel_bwd_dx

def _run_dx(L, rows, fan_in, duel, alias):
    """-> dx on the host and the restatement's inputs; checks that inputs that are not the output stay as they were."""
    case = R.bwd_dx_case(rows * fan_in, rows, fan_in)
    a, p, e, q, h = case
    n = rows * fan_in
    arena = Arena(n)
    dx = arena.carve(n).view(rows, fan_in)
    if alias:
        dx.copy_(_dev(a))
        d_a = dx
    else:
        d_a = _dev(a)
    d_p, d_e, d_q, d_h = (_dev(t) for t in (p, e, q, h))
    if duel:
        L.noisy_duel_bwd_dx(d_a, d_p, d_e, d_q, d_h, dx)
    else:
        L.noisy_dense_bwd_dx(d_a, d_p, d_e, dx)
    arena.check()
    for t, src in ((d_p, p), (d_e, e), (d_q, q), (d_h, h)) + (() if alias else ((d_a, a),)):
        _same_bits(t, src)
    return _host(dx), case


@pytest.mark.parametrize("duel", [False, True], ids=["dense", "duel"])
@pytest.mark.parametrize("rows,fan_in", R.DX_SHAPES)
def test_bwd_dx_association_in_place_and_out_of_place(L, rows, fan_in, duel):
    apart, (a, p, e, q, h) = _run_dx(L, rows, fan_in, duel, alias=False)
    inplace, _ = _run_dx(L, rows, fan_in, duel, alias=True)
    want = R.duel_bwd_dx_f32(a, p, e, q, h) if duel else R.bwd_dx_f32(a, p, e)
    _same_bits(apart, want)
    _same_bits(inplace, want)
    if duel:
        assert want.tobytes() != R.duel_bwd_dx_other_f32(a, p, e, q, h).tobytes()


# ---------------------------------------------------------------------------------------------- g. determinism

def test_two_launches_give_the_same_bits(L):
    def flat(out):
        if isinstance(out, np.ndarray):
            return [out]
        if out is None or isinstance(out, dict):
            return []
        return [a for o in out for a in flat(o)]

    full = dict(bias=True, bsig=True, relu=1, nxt=True, state=True, shift=0)
    runs = {
        "arl_noisy_noise": lambda: _run_noise(L, LAYER_LISTS["eight"], 257, 1, *SEEDS[3]),
        "arl_noisy_draws": lambda: _run_draws(L, DRAWS_16, 257, 1, *SEEDS[4]),
        "arl_noisy_dense_combine": lambda: _run_combine(L, 257, 6, 64, 65, **full)[:2],
        "arl_noisy_duel_combine": lambda: _run_combine(L, 5, 1024, 5, None, duel=(512, 20, 20), **full)[:2],
        "arl_noisy_dense_bwd_prep": lambda: _run_prep(L, 1000, 256)[:3],
        "arl_noisy_duel_bwd_prep": lambda: _run_prep(L, 33, 600, 300)[:3],
        "arl_noisy_dense_bwd_dx": lambda: _run_dx(L, 257, 260, False, False)[0],
        "arl_noisy_duel_bwd_dx": lambda: _run_dx(L, 257, 260, True, False)[0],
    }
    assert len(runs) == 8
    for name, run in runs.items():
        first, second = flat(run()), flat(run())
        assert len(first) == len(second) > 0
        for a, b in zip(first, second):
            _same_bits(a, b, name)
