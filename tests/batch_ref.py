"""References and case tables of tests/test_batch_limits_host.py and tests/test_batch_limits_gpu.py: the kernels between
rollout and learner (csrc/scan.hip, csrc/batch_ops.hip, the element-wise kernels of csrc/learner.hip) at the edges of
what their entry points accept.

Everything here is NumPy on the CPU.  The device file compares the kernels with these references; the host file shows
on the very same inputs that each nearest wrong version of a kernel would give another answer, so the comparisons
cannot pass by accident.  What is compared how:
- scans: oracle.ref_port.gae_scan / nstep_returns, bit for bit (both exact promotions);
- valids: ref_port.valid_mask / zero_invalid, equal;
- standardise: a float64 two-pass restatement, within standardize_bound() (derived below, not fitted);
- sampling: ref_port.sample_actions, equal;
- gathers: obs[idx] * float32(scale), equal;
- bias + ReLU and its backward: NumPy float32, bit for bit; the bias gradient in the summation order the kernels fix
  (dbias_restatement)."""
import numpy as np

from oracle import ref_port as P

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24                  # unit roundoff of float32
U64 = 2.0 ** -53                  # ... of float64


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.int8}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def same_bits_nan(a, b):
    """Equal bits, except that any NaN equals any NaN (the payload of a NaN is not pinned)."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and bool((bits(a)[~na] == bits(b)[~nb]).all())


# ====================================================================================================== scans

ROUTES = ("lds256", "lds128", "lds64", "lds64x256", "chunked", "lds32", "lds8", "direct")
# envs per workgroup of each route (direct: a 256-thread block, one env per thread)
TILE_ENVS = dict(lds256=256, lds128=128, lds64=64, lds64x256=64, chunked=32, lds32=32, lds8=8, direct=256)


def scan_route(n_env, T, aligned):
    """The kernel that dispatch() in csrc/scan.hip launches for an exact promotion.  This MIRRORS dispatch() and must
    be changed with it: the case table below is only worth what this function knows about the routes.
    aligned: rewards, values and both outputs 16-byte aligned and dones 4-byte aligned (vec_ok)."""
    if aligned and T <= 17:
        epb = 256 if T <= 8 else 128
        while epb > 64 and (n_env + epb - 1) // epb < 512:
            epb >>= 1
        return "lds%d" % epb
    if aligned and T <= 34:
        return "lds64x256"                      # 64 envs streamed by 256 threads
    if aligned and T % 4 == 0:
        return "chunked"                        # 32 envs x 64-step chunks
    if aligned and T <= 136:
        return "lds32"
    if aligned and T <= 544:
        return "lds8"
    return "direct"


# (route, n_env, T): the smallest shapes that reach each route, with one env, a ragged last tile, several tiles, an
# even horizon (skewed LDS) and an odd one, a partial chunk, and both sides of each threshold
SCAN_CASES = [
    ("lds256", 130817, 8), ("lds256", 130900, 7), ("lds256", 130900, 1),
    ("lds128", 65409, 6), ("lds128", 65500, 9), ("lds128", 65409, 17), ("lds128", 65600, 16),
    ("lds64", 65408, 9), ("lds128", 130816, 8),                       # just under both thresholds
    ("lds64x256", 1, 18), ("lds64x256", 129, 33), ("lds64x256", 65, 34),
    ("chunked", 1, 36), ("chunked", 33, 36), ("chunked", 95, 68), ("chunked", 64, 100), ("chunked", 37, 192),
    ("chunked", 33, 548),
    ("lds32", 1, 35), ("lds32", 33, 37), ("lds32", 95, 135),
    ("lds8", 9, 137), ("lds8", 17, 543),
    ("direct", 5, 545), ("direct", 300, 546),
]
# one case per route (the smallest with more than one tile): parameters, isolation
SCAN_SUB = [2, 3, 7, 11, 14, 19, 21, 24]
SCAN_PARAMS = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.5), (0.99, 0.0), (0.5, 1.0)]
DONE_PATTERNS = ("none", "all", "first", "last", "alternating", "random")
DONE_BYTES = (2, 255, 1)          # the k-th set byte of a case holds DONE_BYTES[k % 3]: the first one is never 1
PROMOS = ((0, "nep50"), (1, "legacy"))
WAVE_BAR = 1e-5                   # BASELINE.json's bar of the tolerance mode: 1e-5 max(1, |x|)


def done_bytes(n, T, pattern, rs):
    if pattern == "none":
        m = np.zeros((n, T), bool)
    elif pattern == "all":
        m = np.ones((n, T), bool)
    elif pattern == "first":
        m = np.zeros((n, T), bool)
        m[:, 0] = True
    elif pattern == "last":
        m = np.zeros((n, T), bool)
        m[:, T - 1] = True
    elif pattern == "alternating":
        m = ((np.arange(n)[:, None] + np.arange(T)[None, :]) & 1).astype(bool)
    else:
        m = rs.rand(n, T) < 0.15
    d = np.zeros(n * T, np.uint8)
    flat = m.reshape(-1)
    d[flat] = np.asarray(DONE_BYTES, np.uint8)[np.arange(int(flat.sum())) % 3]
    return d.reshape(n, T)


def scan_inputs(n, T, pattern, seed):
    """-> dict(r, v [n, T] float32, d [n, T] uint8 with set bytes 1, 2 and 255, lv [n] float32)."""
    rs = np.random.RandomState(seed)
    r = rs.randn(n, T).astype(F32)
    v = (rs.randn(n, T) * 2).astype(F32)
    lv = rs.randn(n).astype(F32)
    return dict(r=r, v=v, d=done_bytes(n, T, pattern, rs), lv=lv, n=n, T=T)


def scan_case_inputs(i):
    route, n, T = SCAN_CASES[i]
    return scan_inputs(n, T, DONE_PATTERNS[i % len(DONE_PATTERNS)], 1000 + i)


def scan_oracle(x, scan, pname, gamma, lam, done=None):
    """(out0, out1) in the entry point's order: GAE -> (advantages, returns); n-step -> (returns, advantages).
    done: what counts as a set byte (default: the oracle's own d != 0)."""
    d = (x["d"] != 0) if done is None else done(x["d"])
    with np.errstate(all="ignore"):
        if scan == "gae":
            return P.gae_scan(x["r"], x["v"], d, x["lv"], gamma, lam, pname)
        return P.nstep_returns(x["r"], d, x["v"], x["lv"], gamma, pname)


def poisoned_envs(route, n):
    """One env in the middle of a tile and one at a tile's edge (the last lane of that tile), in a tile in the middle
    of the batch."""
    w = TILE_ENVS[route]
    t0 = ((n // w) // 2) * w
    return sorted(set(min(t0 + e, n - 1) for e in (w // 2, w - 1)))


def poison(x, envs):
    """A NaN reward at t = T - 1 and a +inf value at t = 0 in each of `envs` (a copy)."""
    y = dict(x, r=x["r"].copy(), v=x["v"].copy())
    for e in envs:
        y["r"][e, x["T"] - 1] = np.nan
        y["v"][e, 0] = np.inf
    return y


def within_wave_bar(got, want):
    return bool(np.all(np.abs(got - want) <= WAVE_BAR * np.maximum(1.0, np.abs(want))))


# ====================================================================================================== valids

VALIDS_N, VALIDS_T = (1, 257, 70001), (1, 2, 5, 64)
FLAG_PATTERNS = ("none", "first", "last", "random")


def reset_flags(n, T, pattern, seed):
    """uint8 [n, T]; set bytes alternate between 1 and 255."""
    rs = np.random.RandomState(seed)
    m = np.zeros((n, T), bool)
    if pattern == "first":
        m[:, 0] = True
    elif pattern == "last":
        m[:, T - 1] = True
    elif pattern == "random":
        m = rs.rand(n, T) < 0.2
    f = np.zeros((n, T), np.uint8)
    f[m] = np.where(np.arange(int(m.sum())) & 1, 1, 255)
    return f


def valids_base(n, T, seed):
    rs = np.random.RandomState(seed)
    return [rs.randn(n, T).astype(F32) for _ in range(3)]


def valids_payload(base, valids):
    """advantages, returns, values: `base` where valid, NaN / +inf / -inf past the reset."""
    n, T = valids.shape
    out = []
    for k, a in enumerate(base):
        bad = np.asarray([np.nan, np.inf, -np.inf], F32)[(np.arange(n * T).reshape(n, T) + k) % 3]
        out.append(np.where(valids == 0, bad, a).astype(F32))
    return out


# ================================================================================================== standardise

STD_BLOCKS = 512                                  # csrc/batch_ops.hip: partial-moment slots
STD_N = (1, 2, 255, 256, 257, 131072, 131073)
STD_EPS = (1e-6, 0.5)
STD_RATIOS = (0.0, 1e2, 1e4, 1e6)                 # mu / sigma of the inputs
STD_SIGMA = 1.5
VALID_BYTES = np.asarray([1, 2, 127, -1], np.int8)         # non-zero means valid


def std_inputs(n, masked, ratio, seed):
    """x ~ N(ratio * sigma, sigma) in float32; valids: ~30 % zeros, the rest from VALID_BYTES (valids[0] is set)."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(n) * STD_SIGMA + ratio * STD_SIGMA).astype(F32)
    valids = None
    if masked:
        valids = np.where(rs.rand(n) < 0.7, VALID_BYTES[rs.randint(0, 4, n)], 0).astype(np.int8)
        valids[0] = 2
    return x, valids


def std_cases(n, masked):
    """[(eps, ratio, x, valids)] of one size."""
    out = []
    for ei, eps in enumerate(STD_EPS):
        for ri, ratio in enumerate(STD_RATIOS):
            x, valids = std_inputs(n, masked, ratio, 77 * n % 9973 + 10 * ri + ei + (500 if masked else 0))
            out.append((eps, ratio, x, valids))
    return out


def std_reference(x, valids, eps):
    """The float64 two-pass reference over the valid elements: mean, population variance,
    (x - m) / (sqrt(var) + eps), eps being the float32 the entry point hands its kernel.
    -> (sel, y, m, var, d): the valid mask, y for the valid elements, and the moments."""
    sel = np.ones(x.shape, bool) if valids is None else (valids != 0)
    xs = x[sel].astype(F64)
    m = xs.mean()
    var = ((xs - m) ** 2).mean()
    d = np.sqrt(var) + float(F32(eps))
    return sel, (xs - m) / d, m, var, d


def std_sum_depth(n):
    """Longest chain of float64 additions a moment goes through in moments_kernel + standardize_kernel: a thread's own
    elements, 6 shuffle levels, 4 waves; then the fold of the partials: a thread's slots, 6 levels, 4 waves."""
    nb = min((n + 255) // 256, STD_BLOCKS)
    return -(-n // (nb * 256)) + 10 + -(-nb // 256) + 10


def standardize_bound(y, m, var, d, n):
    """|kernel - float64 reference| per valid element, from the kernel's steps (u = 2^-24, u64 = 2^-53):

        bound = (u |m| / d  +  (4 u + e64) |y|) (1 + 2^-20)

    - u |m| / d: the mean is rounded to float32 before the subtraction (mean32 = m (1 + delta), |delta| <= u);
    - 4 u |y|: two roundings of the denominator ((float) sqrt(var), then + eps in float32), one of the subtraction
      x - mean32, one of the division;
    - e64 |y|: the moments are ONE pass in float64, var = ss / c - mean^2.  A sum of depth D carries a relative error
      of at most D u64 (all terms of ss are >= 0; for s the error is relative to sum |x| <= c sqrt(m^2 + var)), so
      var carries at most (3 D + 6) u64 (m^2 + var), and sqrt(var) half of that relatively:
      e64 = (3 D + 6) / 2 * u64 * (1 + m^2 / var), D = std_sum_depth(n).  At mu = 10^4 sigma that is 5e-7, below the
      mean's term (6e-4); at 10^6 sigma 4e-3 against 6e-2.
    - (1 + 2^-20) covers the products of these terms.
    var == 0 (one valid element, a constant array) has no bound: the kernel must give +0 exactly."""
    assert var > 0
    e64 = 0.5 * (3 * std_sum_depth(n) + 6) * U64 * (1.0 + m * m / var)
    return (U32 * abs(m) / d + (4 * U32 + e64) * np.abs(y)) * (1 + 2.0 ** -20)


def std_restatement_f32(x, valids, eps, variant=None):
    """NumPy restatement with the kernel's float32 steps (float64 one-pass moments, float32 mean, denominator,
    subtraction and division).  variant: a nearest WRONG version -- "ddof1", "all" (moments over all elements, not the
    valid ones), "eps_under_root"."""
    sel = np.ones(x.shape, bool) if valids is None else (valids != 0)
    msel = np.ones(x.shape, bool) if variant == "all" else sel
    xs = x[msel].astype(F64)
    c = float(xs.size)
    mean = xs.sum() / c
    var = max((xs * xs).sum() / c - mean * mean, 0.0)
    if variant == "ddof1" and c > 1:
        var = var * c / (c - 1.0)
    mean32, eps32 = F32(mean), F32(eps)
    denom = F32(np.sqrt(var + float(eps32))) if variant == "eps_under_root" else F32(F32(np.sqrt(var)) + eps32)
    out = x.copy()
    out[sel] = (x[sel] - mean32) / denom
    return out


def std_recover_denominator(x_valid, got_valid, m):
    """The kernel's float32 denominator, recovered from its outputs: the float32 d near median((x - mean32) / y) for
    which (x - mean32) / d reproduces EVERY output bit for bit (mean32 = the float32 nearest the float64 mean).
    None where no such d exists within 4 ulps of the estimate (then mean32 was another float, or var == 0)."""
    a = x_valid - F32(m)
    big = np.abs(got_valid) > 0.5
    if not big.any():
        return None
    est = F32(np.median(a[big].astype(F64) / got_valid[big].astype(F64)))
    cands = [est]
    for _ in range(4):
        cands = [np.nextafter(cands[0], F32(-np.inf))] + cands + [np.nextafter(cands[-1], F32(np.inf))]
    hits = [d for d in cands if same_bits((a / d).astype(F32), got_valid)]
    if not hits:
        return None
    return min(hits, key=lambda d: abs(float(d) - float(est)))


# ===================================================================================================== sampling

SAMPLE_A, SAMPLE_B = (1, 2, 255, 256), (1, 257, 70001)
SAMPLE_BANK = 257                  # distinct probability rows; row b of a batch is bank row b % 257
N_U_KINDS = 11                     # (first, middle, last action) x (cumsum, just below, just above), u = 0, u = 1


def prob_bank(A, seed):
    """[257, A] float32, every entry a multiple of 2^-10 and every row summing to 1: the float32 running sum of a row
    is exact in any order.  Rows have zeros (repeated cumulative sums) once A > 2."""
    rs = np.random.RandomState(seed)
    cuts = np.sort(rs.randint(0, 1025, size=(SAMPLE_BANK, A - 1)), axis=1)
    edges = np.concatenate([np.zeros((SAMPLE_BANK, 1), int), cuts, np.full((SAMPLE_BANK, 1), 1024)], axis=1)
    return (np.diff(edges, axis=1) / 1024.0).astype(F32)


def sample_inputs(A, B, shift=0, seed=3):
    """prob [B, A] and u [B]: row b takes tie kind (b + shift) % 11."""
    p = prob_bank(A, seed)[np.arange(B) % SAMPLE_BANK]
    csum = np.cumsum(p, axis=1, dtype=F32).astype(F64)
    kind = (np.arange(B) + shift) % N_U_KINDS
    action = np.asarray([0, A // 2, A - 1])[np.minimum(kind // 3, 2)]
    at = csum[np.arange(B), action]
    u = np.where(kind % 3 == 0, at, np.where(kind % 3 == 1, np.nextafter(at, -np.inf), np.nextafter(at, np.inf)))
    u = np.where(kind == 9, 0.0, np.where(kind == 10, 1.0, u))
    return p, u.astype(F64)


def sample_edge_rows(A):
    """Rows that sum to 0.5 with u = 0.9 (the count reaches A and is clamped), all-zero rows, and a NaN probability
    (every later comparison is false) at the first, a middle and the last action."""
    half = prob_bank(A, 9)[:3] * F32(0.5)
    zero = np.zeros((2, A), F32)
    nan = prob_bank(A, 10)[:3].copy()
    for i, j in enumerate((0, A // 2, A - 1)):
        nan[i, j] = np.nan
    p = np.concatenate([half, zero, nan])
    u = np.asarray([0.9, 0.9, 0.9, 0.0, 0.5, 0.3, 0.6, 0.999], F64)
    return p, u


def sample_le(prob, u):
    """The nearest wrong version of ref_port.sample_actions: `<=` where the reference compares with `<`."""
    csum = np.cumsum(np.asarray(prob, F32), axis=1, dtype=F32)
    k = (csum.astype(F64) <= np.asarray(u, F64).reshape(-1, 1)).sum(axis=1)
    return np.minimum(k, prob.shape[1] - 1).astype(np.uint8)


# ====================================================================================================== gathers

GATHER_ROW_BYTES, GATHER_BATCH = (16, 48, 33280), (1, 3, 257)
NHWC_PLANE_BYTES, NHWC_BATCH = (16, 48, 8320), (1, 5)
GATHER_SCALES = (1.0 / 255.0, 1.0, 0.0)
IDX_FORMS = ("null", "reversed", "repeats")


def gather_obs(n_rows, row_bytes, seed):
    """uint8 [n_rows, row_bytes] with every byte value 0 .. 255 present (a ramp through the first 256 bytes)."""
    rs = np.random.RandomState(seed)
    obs = rs.randint(0, 256, size=n_rows * row_bytes).astype(np.uint8)
    ramp = np.arange(256, dtype=np.uint8)
    obs[:min(256, obs.size)] = ramp[:min(256, obs.size)]
    return obs.reshape(n_rows, row_bytes)


def gather_idx(form, batch, n_rows, seed):
    if form == "null":
        return None
    if form == "reversed":
        return (n_rows - 1 - np.arange(batch)).astype(np.int32)
    idx = np.random.RandomState(seed).randint(0, n_rows, size=batch).astype(np.int32)
    idx[batch // 2:] = idx[:batch - batch // 2]             # every row of the first half again
    return idx


def gather_ref(obs, idx, batch, scale):
    rows = obs[:batch] if idx is None else obs[idx]
    return rows.astype(F32) * F32(scale)


def gather_nhwc_ref(obs4, idx, batch, scale):
    """obs4 uint8 [n, 4, plane] -> float32 [batch, plane, 4]."""
    rows = obs4[:batch] if idx is None else obs4[idx]
    return np.ascontiguousarray(rows.transpose(0, 2, 1)).astype(F32) * F32(scale)


# ============================================================================================ bias + ReLU, backward

RELU_CHANNELS, RELU_ROWS = (4, 12, 1020, 1024), (1, 85, 86, 300, 21761)
RELU_BLOCK_CAP = 256              # relu_bwd_bias_kernel's grid cap = the partials fold_partials_kernel folds


def relu_inputs(rows, channels, seed):
    """x, bias, dy.  Planted: x + b == 0 exactly (x = -b), x = -0.0 (under bias -0.0 too: x + b = -0.0), so the
    forward output holds exact zeros under a non-zero dy; a NaN dy under some of those masked elements."""
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((rows, channels), dtype=F32)
    b = rs.standard_normal(channels, dtype=F32)
    b[1] = F32(-0.0)
    dy = rs.standard_normal((rows, channels), dtype=F32) + F32(0.25)
    flat = np.arange(rows * channels).reshape(rows, channels)
    cancel = flat % 7 == 0
    x[flat % 11 == 1] = F32(-0.0)
    x[cancel] = np.broadcast_to(-b, x.shape)[cancel]
    y = relu_fwd_ref(x, b)
    assert (y[cancel] == 0).all() and (dy != 0).all()
    nan_at = (y == 0) & (flat % 3 == 0)
    dy[nan_at] = np.nan
    return x, b, dy


def relu_fwd_ref(x, b):
    s = x + b[None, :]
    return np.where(s > 0, s, F32(0.0)).astype(F32)


def relu_bwd_ref(dy, y):
    """The masked gradient: a SELECT, so a NaN under the mask becomes +0."""
    return np.where(y > 0, dy, F32(0.0)).astype(F32)


def relu_grid(rows, channels):
    rpi = 256 // (channels // 4)
    return min((rows + rpi - 1) // rpi, RELU_BLOCK_CAP), rpi


def dbias_restatement(g):
    """Column sums of the masked gradient g [rows, channels] in the order relu_bwd_bias_kernel and
    fold_partials_kernel fix (plain float32 adds, no contraction):
      1. a thread (block, row lane rl, float4 column) adds rows block * rpi + rl, stepping by grid * rpi, in order;
      2. the block's row lanes 0 .. rpi - 1 are added in order -> partials[block];
      3. fold: wave w adds partials w, w + 32, ... into s0 and w + 16, w + 48, ... into s1, then a tail partial into
         s0, then s0 + s1;
      4. the 16 waves are added in order.
    Every accumulator starts at +0, so rows beyond the end can be restated as added +0 (x + 0 == x for every x an
    accumulator can hold: it is never -0)."""
    rows, channels = g.shape
    grid, rpi = relu_grid(rows, channels)
    sweep = grid * rpi
    k = -(-rows // sweep)
    pad = np.zeros((k * sweep, channels), F32)
    pad[:rows] = g
    pad = pad.reshape(k, grid, rpi, channels)
    acc = np.zeros((grid, rpi, channels), F32)
    for j in range(k):
        acc = acc + pad[j]
    part = np.zeros((grid, channels), F32)
    for r in range(rpi):
        part = part + acc[:, r]
    out = np.zeros(channels, F32)
    for w in range(16):
        s0, s1 = np.zeros(channels, F32), np.zeros(channels, F32)
        i = w
        while i + 16 < grid:
            s0 = s0 + part[i]
            s1 = s1 + part[i + 16]
            i += 32
        if i < grid:
            s0 = s0 + part[i]
        out = out + (s0 + s1)
    return out
