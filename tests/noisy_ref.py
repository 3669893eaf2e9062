"""Shared by tests/test_noisy_limits_host.py and tests/test_noisy_limits_gpu.py: NumPy float32 restatements of what
csrc/noisy.hip computes between the matrix products, in the order include/accel_rl_hip.h states, their float64
versions with derived error bounds, and the input builders and case lists of both files.

csrc/noisy.hip is compiled with -ffp-contract=off and is fp32 element-wise arithmetic in a stated order, so the
float32 restatements are compared with the device BIT FOR BIT.  NumPy float32 array arithmetic rounds every operation
to float32 (round to nearest even), which is what the device does with contraction off; nothing below ever lets two
operations share one rounding.

The order of a fold (arl_fold_many, csrc/mfma_conv.hip fold_sum; repeated by csrc/noisy.hip folded()):
  zgn = 64 if splits >= wide_from (128 unless arl_dev_fold_wide_from moved it) else 16;
  s_k = ((0.f + part[k]) + part[k + zgn]) + part[k + 2 zgn] + ...     for k = 0 .. zgn-1 (an empty group is 0.f);
  out = (((s_0 + s_1) + s_2) + ... + s_{zgn-1}) + bias.
splits == 0 means "finished": the value is part[0], no bias added.

Bounds (EPS = 2^-24, the relative error of one float32 rounding; |.| element-wise).
  fold.  An element's value passes through at most ceil(S / zgn) additions inside its group, at most zgn more across
    the groups (the first, s_0 + s_1, included; 0.f + x is exact but counted) and one for the bias.  Every
    intermediate sum is at most T = sum_z |part_z| + |bias| in magnitude (to first order), so
      |fold_f32 - fold_f64| <= (ceil(S / zgn) + zgn + 1) EPS T.           A finished item (S == 0) has bound 0.
  combine.  y = relu?(a + feout s): the errors of the two folds enter as B_a + |feout| B_s; the product feout s is
    rounded once, EPS |feout s|, and the sum once, EPS |y|; relu is 1-Lipschitz:
      B_y = B_a + |feout| B_s + EPS (|feout s| + |a + feout s|).
    (Where the sigma item has splits, |feout| B_s >= 18 EPS |feout s| already covers the product's rounding; where it is
    finished but the W item has splits, |feout s| <= |a| + |y| and B_a >= 18 EPS |a| does.  With BOTH finished nothing
    else covers it, and under cancellation |feout s| exceeds |y| by any factor: the term has to be there.)
    First order in EPS: the roundings are relative to the computed values, which differ from the exact ones by terms
    of the bound's own size times EPS; B_y is multiplied by 1 + 2^-20 for them.
    xs_next = y fein_next: B_xs = |fein_next| B_y + EPS |xs_next|.
  db = sum_rows g: rows - 1 roundings of sums of magnitude <= G = sum_r |g_r|:  rows EPS G.
  db_sigma = sum_rows (g feout): each term rounded once more: (rows + 1) EPS sum_r |g_r feout_r|.
These are worst cases: a CPU trial of fold_f32 on random parts with a planted +-3e4 cancelling column at splits
1 .. 4096 stayed below 0.1 of the fold bound.  A value outside its bound is a wrong operation, not noise."""
import numpy as np
import torch

from test_noisy_net_host import noisy_words_normals          # noqa: F401  (the generator's statement, shared)

EPS = 2.0 ** -24
F32 = np.float32
WIDE_FROM = 128                 # csrc/mfma_conv.hip FOLD_WIDE: arl_dev_fold_wide_from(0) restores it
MAX_SPLITS = 4096               # fold_item_ok in csrc/noisy.hip
MAX_PART_FLOATS = 4096 * 35     # the largest partial-sum buffer a test builds


def zgn_of(splits, wide_from=WIDE_FROM):
    return 64 if splits >= wide_from else 16


# ---- float32 restatements -------------------------------------------------------------------------------------------

def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def fold_f32(part, splits, zgn, bias=None):
    """part f32[max(splits, 1)][n], bias f32[n] (per element) or None -> f32[n]."""
    part = _f32(part)
    if splits == 0:
        return part[0].copy()
    s = None
    for k in range(zgn):
        sk = np.zeros(part.shape[1], F32)
        for z in range(k, splits, zgn):
            sk = sk + part[z]
        s = sk if k == 0 else s + sk
    if bias is not None:
        s = s + _f32(bias)
    return s


def sequential_f32(part, splits, bias=None):
    """The nearest wrong order: part[0] + part[1] + ... in split order."""
    s = np.zeros(part.shape[1], F32)
    for z in range(splits):
        s = s + _f32(part[z])
    return s if bias is None else s + _f32(bias)


def _per_element(vec, rows):
    return None if vec is None else np.tile(_f32(vec), rows)


def _finish_f32(a, s, feout, relu, fein_next):
    p = _f32(feout).reshape(-1) * s             # rounded
    v = a + p                                   # rounded
    if relu:
        v = np.where(v > 0, v, F32(0))          # fmaxf(v, 0.f); a -0.f comes out +0.f either way
    xs = None if fein_next is None else v * _f32(fein_next).reshape(-1)
    return v, xs


def combine_f32(pw, sw, ps, ss, bias, b_sigma, feout, rows, units, relu, fein_next=None, wide_from=WIDE_FROM):
    """arl_noisy_dense_combine -> (y f32[rows * units], xs_next or None)."""
    a = fold_f32(pw, sw, zgn_of(sw, wide_from), _per_element(bias, rows))
    s = fold_f32(ps, ss, zgn_of(ss, wide_from), _per_element(b_sigma, rows))
    return _finish_f32(a, s, feout, relu, fein_next)


def _duel_sigma(fold, lo, s_lo, hi, s_hi, b_sigma, rows, units, split, wide_from):
    """Both streams' sigma sums in the stacked layout [rows][units]: fold(part, splits, zgn, bias) per stream."""
    b_lo = None if b_sigma is None else np.tile(b_sigma[:split], rows)
    b_hi = None if b_sigma is None else np.tile(b_sigma[split:], rows)
    return fold(lo, s_lo, zgn_of(s_lo, wide_from), b_lo), fold(hi, s_hi, zgn_of(s_hi, wide_from), b_hi)


def _stack(v_lo, v_hi, rows, units, split):
    return np.concatenate([v_lo.reshape(rows, split), v_hi.reshape(rows, units - split)], axis=1).reshape(-1)


def duel_combine_f32(pw, sw, lo, s_lo, hi, s_hi, bias, b_sigma, feout, rows, units, split, relu, fein_next=None,
                     wide_from=WIDE_FROM):
    """arl_noisy_duel_combine: the sigma sum of unit u < split is lo[r * split + u], else
    hi[r * (units - split) + (u - split)]; b_sigma by the global u."""
    a = fold_f32(pw, sw, zgn_of(sw, wide_from), _per_element(bias, rows))
    v_lo, v_hi = _duel_sigma(fold_f32, lo, s_lo, hi, s_hi, b_sigma, rows, units, split, wide_from)
    return _finish_f32(a, _stack(v_lo, v_hi, rows, units, split), feout, relu, fein_next)


def bwd_prep_f32(g, feout):
    """arl_noisy_dense_bwd_prep, g / feout f32[rows][units] -> (g2, db, db_sigma); the sums row by row from 0.f."""
    g, feout = _f32(g), _f32(feout)
    g2 = g * feout
    db, dbs = np.zeros(g.shape[1], F32), np.zeros(g.shape[1], F32)
    for r in range(g.shape[0]):
        db = db + g[r]
        dbs = dbs + g2[r]
    return g2, db, dbs


def duel_bwd_prep_f32(g, feout, split):
    """arl_noisy_duel_bwd_prep -> (g2_lo [rows][split], g2_hi [rows][units - split], db, db_sigma)."""
    g2, db, dbs = bwd_prep_f32(g, feout)
    return np.ascontiguousarray(g2[:, :split]), np.ascontiguousarray(g2[:, split:]), db, dbs


def pairwise_f32(g):
    """The nearest wrong order of a row sum: a tree (adjacent pairs, then pairs of pairs, ...)."""
    v = [_f32(g[r]) for r in range(g.shape[0])]
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


def bwd_dx_f32(a, s, f):
    return _f32(a) + _f32(f) * _f32(s)


def duel_bwd_dx_f32(a, p, e, q, h):
    return (_f32(a) + _f32(e) * _f32(p)) + _f32(h) * _f32(q)


def duel_bwd_dx_other_f32(a, p, e, q, h):
    """The nearest wrong association: a + (e p + h q)."""
    return _f32(a) + (_f32(e) * _f32(p) + _f32(h) * _f32(q))


# ---- float64 versions with their bounds -----------------------------------------------------------------------------

def fold_f64(part, splits, zgn, bias=None):
    """-> (value f64[n], bound f64[n])."""
    part = np.asarray(part, np.float64)
    if splits == 0:
        return part[0].copy(), np.zeros(part.shape[1])
    v, t = part[:splits].sum(axis=0), np.abs(part[:splits]).sum(axis=0)
    if bias is not None:
        v, t = v + np.asarray(bias, np.float64), t + np.abs(np.asarray(bias, np.float64))
    return v, (-(-splits // zgn) + zgn + 1) * EPS * t


def _finish_f64(a, b_a, s, b_s, feout, relu, fein_next):
    fe = np.asarray(feout, np.float64).reshape(-1)
    p = fe * s
    v = a + p
    b_y = (b_a + np.abs(fe) * b_s + EPS * (np.abs(p) + np.abs(v))) * (1 + 2. ** -20)
    y = np.maximum(v, 0) if relu else v
    if fein_next is None:
        return y, b_y, None, None
    fn = np.asarray(fein_next, np.float64).reshape(-1)
    xs = y * fn
    return y, b_y, xs, np.abs(fn) * b_y + EPS * np.abs(xs)


def combine_f64(pw, sw, ps, ss, bias, b_sigma, feout, rows, units, relu, fein_next=None, wide_from=WIDE_FROM):
    """-> (y, bound of y, xs_next or None, its bound or None)."""
    a, b_a = fold_f64(pw, sw, zgn_of(sw, wide_from), _per_element(bias, rows))
    s, b_s = fold_f64(ps, ss, zgn_of(ss, wide_from), _per_element(b_sigma, rows))
    return _finish_f64(a, b_a, s, b_s, feout, relu, fein_next)


def duel_combine_f64(pw, sw, lo, s_lo, hi, s_hi, bias, b_sigma, feout, rows, units, split, relu, fein_next=None,
                     wide_from=WIDE_FROM):
    a, b_a = fold_f64(pw, sw, zgn_of(sw, wide_from), _per_element(bias, rows))
    (v_lo, b_lo), (v_hi, b_hi) = _duel_sigma(fold_f64, lo, s_lo, hi, s_hi, b_sigma, rows, units, split, wide_from)
    return _finish_f64(a, b_a, _stack(v_lo, v_hi, rows, units, split), _stack(b_lo, b_hi, rows, units, split), feout,
                       relu, fein_next)


def bwd_prep_f64(g, feout):
    """-> (g2, db, bound of db, db_sigma, bound of db_sigma)."""
    g, fe = np.asarray(g, np.float64), np.asarray(feout, np.float64)
    g2, rows = g * fe, g.shape[0]
    return g2, g.sum(axis=0), rows * EPS * np.abs(g).sum(axis=0), g2.sum(axis=0), (rows + 1) * EPS * np.abs(g2).sum(axis=0)


def ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 = 0: a zero bound demands equality)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.isfinite(err).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0., err / bound)
    return float(r.max())


# ---- input builders (deterministic; arrays are fresh on every call) -------------------------------------------------

def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy()


def fold_parts(seed, splits, n):
    """f32[max(splits, 1)][n] of N(0, 1); column 0 alternates +-3e4 over the splits, plus the noise.  Every third split
    of that column stays plain noise: were every value near 3e4, all of them and all their partial sums would sit on
    one 2^-9 grid, most additions would be exact, and the order would show less often."""
    for attempt in range(32):
        part = _randn(seed + 7919 * attempt, max(splits, 1), n)
        if splits > 0:
            z = np.arange(part.shape[0])
            part[:, 0] += (F32(3e4) * (1 - 2 * (z % 2)) * (z % 3 != 2)).astype(F32)
        if splits < 17 or tells_fold_orders_apart(part, splits):
            return part     # (a single element shows the order about 9 times in 10, so a 1-element case may redraw)
    raise AssertionError("no draw tells the fold orders apart")


def tells_fold_orders_apart(part, splits):
    """The fold in its own width, in the other width and as a sequential sum give three different results."""
    own = fold_f32(part, splits, zgn_of(splits)).tobytes()
    return own != fold_f32(part, splits, 80 - zgn_of(splits)).tobytes() and own != sequential_f32(part, splits).tobytes()


def fe_like(seed, *shape):
    """Values distributed as f(e) = sgn(e) sqrt(|e|) of a normal e."""
    e = _randn(seed, *shape)
    return (np.sign(e) * np.sqrt(np.abs(e))).astype(F32)


def bwd_prep_case(seed, rows, units):
    """-> (g, feout) f32[rows][units]; columns 0, units // 2 and units - 1 of g alternate +-1e4 (1 + r / 7) over the rows
    (every third row stays plain noise, as in fold_parts) plus the noise: their sums cancel, so the order of summation
    shows in the rounding.  Redrawn until a tree of rows differs from the row order in db and in db_sigma (three rows
    or more; a 1-unit case is one element, which shows it about 9 times in 10)."""
    r = np.arange(rows)
    big = (F32(1e4) * (1 + r / 7.) * (1 - 2 * (r % 2)) * (r % 3 != 2)).astype(F32)
    for attempt in range(32):
        g = _randn(seed + 7919 * attempt, rows, units)
        for c in {0, units // 2, units - 1}:
            g[:, c] += big
        feout = fe_like(seed + 7919 * attempt + 1, rows, units)
        if rows < 3 or tells_row_orders_apart(g, feout):
            return g, feout
    raise AssertionError("no draw tells the row orders apart")


def tells_row_orders_apart(g, feout):
    g2, db, dbs = bwd_prep_f32(g, feout)
    return db.tobytes() != pairwise_f32(g).tobytes() and dbs.tobytes() != pairwise_f32(g2).tobytes()


def bwd_dx_case(seed, rows, fan_in):
    """-> (a, p, e, q, h) f32[rows][fan_in]: dx_w, dx_sigma_lo, fein_lo, dx_sigma_hi, fein_hi.  Element 0 is planted so
    that the association shows whatever the draw (a 4-element case has little else): a = 1, e p = h q = 2^-24 -- (1 + 2^-24) + 2^-24 rounds to 1 twice (ties
    to even), 1 + (2^-24 + 2^-24) = 1 + 2^-23 exactly."""
    a, p, q = (_randn(seed + i, rows, fan_in) for i in range(3))
    e, h = fe_like(seed + 3, rows, fan_in), fe_like(seed + 4, rows, fan_in)
    a[0, 0], p[0, 0], e[0, 0], q[0, 0], h[0, 0] = 1, 2. ** -12, 2. ** -12, 2. ** -12, 2. ** -12
    # element 1 shows a contracted multiply-add: e p = 1 + 2^-11 + 2^-24 rounds (a tie, to even) to 1 + 2^-11 = -a, so the
    # two-rounding result is 0 (then + h q = 0), a fused one 2^-24
    a[0, 1], p[0, 1], e[0, 1], q[0, 1], h[0, 1] = -(1 + 2. ** -11), 1 + 2. ** -12, 1 + 2. ** -12, 0, 1
    return a, p, e, q, h


def bwd_dx_fused(a, s, f):
    """What a + f s gives if the compiler contracts it into one fused multiply-add (the product of two floats is exact in
    double; the double sum's own rounding is far below a float's)."""
    return (np.asarray(a, np.float64) + np.asarray(f, np.float64) * np.asarray(s, np.float64)).astype(F32)


# ---- the cases of the device tests (the host file proves on the CPU that these inputs tell the orders apart) --------

FOLD_SHAPES = [(1, 1), (1, 3), (5, 7), (3, 32), (33, 52), (257, 6)]
FOLD_SPLITS = [(0, 0), (1, 0), (0, 1), (2, 15), (16, 17), (31, 32), (33, 63), (64, 65), (127, 128), (129, 255),
               (4096, 1)]


def fold_cases(rows, units):
    """The (W splits, sigma splits) pairs run at this shape: all whose partial sums fit MAX_PART_FLOATS."""
    n = rows * units
    return [(sw, ss) for sw, ss in FOLD_SPLITS if max(sw, ss, 1) * n <= MAX_PART_FLOATS]


def fold_seed(rows, units, which, splits):
    return 1000 * rows + 10 * units + which + 7 * splits


DUEL_SHAPES = [(2, 1), (7, 3), (8, 4), (64, 63), (1024, 512)]                   # (units, split)
DUEL_ROWS = [1, 5, 33]
DUEL_SPLITS = [(17, 0, 129), (128, 16, 16), (0, 0, 0), (1, 1, 1), (16, 17, 17), (5, 20, 20), (0, 3, 0), (2, 0, 40)]


def duel_rows(units):
    return [5] if units == 1024 else DUEL_ROWS


def duel_cases(rows, units, split):
    """(W, lo, hi) split counts run at this shape: all whose partial sums fit MAX_PART_FLOATS."""
    return [(sw, sl, sh) for sw, sl, sh in DUEL_SPLITS
            if max(max(sw, 1) * rows * units, max(sl, 1) * rows * split, max(sh, 1) * rows * (units - split))
            <= MAX_PART_FLOATS]


PREP_SHAPES = [(1, 1), (2, 6), (257, 255), (1000, 256), (33, 257), (5, 1024)]   # (rows, units)
DUEL_PREP_SHAPES = [(2, 1), (7, 3), (257, 1), (513, 512), (600, 300)]           # (units, split)
DUEL_PREP_ROWS = [1, 33]
DX_SHAPES = [(1, 4), (3, 8), (5, 52), (1, 1028), (257, 260)]                    # (rows, fan_in)
