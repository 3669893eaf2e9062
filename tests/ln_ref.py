"""TEST INFRASTRUCTURE shared by tests/test_ln_pool_scan_limits_host.py and tests/test_ln_pool_scan_limits_gpu.py: the
LayerNorm + rectifier kernels (csrc/layernorm.hip) restated in NumPy float32 in the lane layout and summation order that
include/accel_rl_hip.h states, operation for operation, vectorised over the rows.  Written from the header's text alone.

csrc/layernorm.hip is compiled without contraction and is fp32 element-wise arithmetic in a stated order; NumPy float32
array arithmetic rounds every operation to float32 (round to nearest even), np.sqrt and / are correctly rounded, and
nothing below lets two operations share one rounding -- so the device is compared with these BIT FOR BIT.  The float64
restatements and the first-order bounds stay in tests/pqn_ref.py (ln_relu_fwd64, ln_relu_bwd64, ln_fwd_bound,
ln_bwd_bound, ln_shape); the fold of the partial rows is tests/noisy_ref.py's fold_f32.

  row_sums32          the header's row sum: q_v = ((x + y) + z) + w per float4, s = q_0, s = s + q_v (v ascending), the
                      butterfly s = s + s[lane ^ off] over a wave's 64 lanes (64 / LPR consecutive rows share a wave)
  ln_relu_fwd32       -> (y, stats)
  ln_relu_bwd32       -> (dz, part_g [grid][width], part_b [grid][width]) from the stats it is given
  ln_fold32           the partial rows folded in arl_fold_many's order
  ln_fwd_grid         the forward's (grid, iters): min(2048, ceil(rows / RPB)) blocks
  ln_case             _ln_case of tests/test_pqn_gpu.py for the shapes of the limits suite
The keyword arguments `butterfly`, `plain` and `v_descending` restate the nearest WRONG orders (a butterfly as wide as
the wave where LPR is smaller: it mixes the rows that share the wave; a left-to-right sum over the row; the float4 slots
of a lane taken last first): the host file proves that the inputs of the device tests tell them from the stated order."""
import numpy as np

import noisy_ref
import pqn_ref as pr

F32 = np.float32
EPS = 1e-5
LN_WIDTHS, LN_ROWS = (8, 36, 68, 256, 260, 516, 768, 1020), (1, 3, 65, 1031)
# one case per LPR (and one more with V = 4) at the smallest row count whose forward takes a second, ragged trip
LN_SECOND_TRIP = ((2048 * 32 + 33, 32), (2048 * 16 + 17, 64), (2048 * 4 + 5, 68), (2048 * 4 + 5, 516))
LN_FWD_MAX_GRID = 2048


def ln_case(rows, width):
    """test_pqn_gpu._ln_case: gamma / beta away from 1 / 0, one large entry in row 0 and, from three rows on, a constant
    last row (0.75: every partial sum exact, var = 0 exactly)."""
    rs = np.random.RandomState(rows * 7919 + width)
    z = rs.randn(rows, width).astype(F32)
    z[0, width // 3] = 50.0
    if rows >= 3:
        z[-1] = 0.75
    gamma = (1.0 + 0.5 * rs.randn(width)).astype(F32)
    beta = (0.3 * rs.randn(width)).astype(F32)
    dy = rs.randn(rows, width).astype(F32)
    return z, gamma, beta, dy


def ln_fwd_grid(rows, width):
    """The forward's launch: (grid, iters) with RPB = 256 / LPR row slots per block."""
    rpb = 256 // pr.ln_shape(rows, width)[0]
    blocks = -(-rows // rpb)
    grid = min(blocks, LN_FWD_MAX_GRID)
    return grid, -(-blocks // grid)


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def row_sums32(e, butterfly=None, plain=False, v_descending=False):
    """e f32[rows][width], zero wherever a float4 past the row's end would be read -> f32[rows], the row sums."""
    e = _f32(e)
    rows, width = e.shape
    if plain:
        s = e[:, 0].copy()
        for j in range(1, width):
            s = s + e[:, j]
        return s
    lpr, v = pr.ln_shape(rows, width)[:2]
    rpw = 64 // lpr                                             # rows per wave: consecutive row slots
    waves = -(-rows // rpw)
    lanes = np.zeros((waves * rpw, v * lpr * 4), F32)           # a dead float4, a dead row slot: zeros
    lanes[:rows, :width] = e
    f4 = lanes.reshape(waves * rpw, v, lpr, 4)                  # float4 number v * LPR + l is lane l's slot v
    q = ((f4[..., 0] + f4[..., 1]) + f4[..., 2]) + f4[..., 3]
    order = range(v - 1, -1, -1) if v_descending else range(v)
    s = None
    for k in order:
        s = q[:, k] if s is None else s + q[:, k]
    s = s.reshape(waves, 64)                                    # lane of the wave = slot-in-wave * LPR + l
    lane = np.arange(64)
    off = (butterfly or lpr) // 2
    while off >= 1:
        s = s + s[:, lane ^ off]
        off //= 2
    s = s.reshape(waves * rpw, lpr)
    assert (s == s[:, :1]).all() or np.isnan(s).any()           # both partners add the same two numbers
    return s[:rows, 0].copy()


def ln_relu_fwd32(z, gamma, beta, eps=EPS, **order):
    """-> (y f32[rows][width], stats f32[rows][2] = (mean, rstd))."""
    z, gamma, beta = _f32(z), _f32(gamma), _f32(beta)
    width_f = F32(z.shape[1])
    mean = (row_sums32(z, **order) / width_f)[:, None]
    d = z - mean                                                # (a float4 past the row's end stays 0: row_sums32 pads)
    var = row_sums32(d * d, **order) / width_f
    rstd = (F32(1) / np.sqrt(var + F32(eps)))[:, None]
    y = np.maximum(F32(0), gamma * (d * rstd) + beta)
    assert y.dtype == np.float32 and rstd.dtype == np.float32
    return y, np.concatenate([mean, rstd], axis=1)


def ln_relu_bwd32(dy, y, z, stats, gamma, dy_masked, **order):
    """-> (dz f32[rows][width], part_g f32[grid][width], part_b f32[grid][width]); y is not read with dy_masked."""
    dy, z, stats, gamma = _f32(dy), _f32(z), _f32(stats), _f32(gamma)
    rows, width = z.shape
    width_f = F32(width)
    mean, rstd = stats[:, :1], stats[:, 1:]
    g = dy if dy_masked else np.where(_f32(y) > 0, dy, F32(0))
    xhat = (z - mean) * rstd
    h = g * gamma
    m1 = (row_sums32(h, **order) / width_f)[:, None]
    m2 = (row_sums32(h * xhat, **order) / width_f)[:, None]
    dz = rstd * ((h - m1) - xhat * m2)
    # column sums: slot k of block b walks rows b * RPB + k + i * grid * RPB, i ascending, from +0; a slot past the last row
    # adds nothing (here: +0, the same bits -- an accumulator that started at +0 is never -0); then the slots in slot order
    lpr, _, grid, iters = pr.ln_shape(rows, width)[:4]
    rpb = 256 // lpr
    parts = []
    for term in (g * xhat, g):
        t = np.zeros((iters * grid * rpb, width), F32)
        t[:rows] = term
        t = t.reshape(iters, grid, rpb, width)
        acc = np.zeros((grid, rpb, width), F32)
        for i in range(iters):
            acc = acc + t[i]
        s = acc[:, 0]
        for k in range(1, rpb):
            s = s + acc[:, k]
        parts.append(s)
    assert dz.dtype == np.float32 and parts[0].dtype == np.float32
    return dz, parts[0], parts[1]


def ln_fold32(part):
    """part f32[grid][width] -> f32[width] in arl_fold_many's order (noisy_ref.fold_f32 as it stands)."""
    grid = part.shape[0]
    return noisy_ref.fold_f32(part, grid, noisy_ref.zgn_of(grid))


def bits(a):
    return np.ascontiguousarray(_f32(a)).view(np.uint32)
