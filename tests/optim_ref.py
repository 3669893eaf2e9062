"""Shared by tests/test_optim_limits_host.py and tests/test_optim_limits_gpu.py: the NumPy float32 restatement of the
flat-bucket optimiser update (csrc/optim.hip, csrc/arl_optim_dev.h), its float64 version with derived error bounds, the
nearest wrong versions of it, and the input builders and case lists of both files.

csrc/optim.hip is compiled with -ffp-contract=off and the update is fp32 element-wise arithmetic in a stated order
(arl::update_one), so the restatement is compared with the device BIT FOR BIT.  NumPy float32 arithmetic rounds every
operation to float32 (round to nearest even), sqrt and / included, which is what the device does with contraction off
and correctly rounded sqrtf and division; nothing below lets two operations share one rounding.

The order (update_one; b1 is rho for RMSprop):
  gg = (g * avg) * cscale
  Adam:     m = b1 * s0 + (1 - b1) * gg;  v = b2 * s1 + (1 - b2) * (gg * gg);  p -= (a_t * m) / (sqrt(v) + eps)
  RMSprop:  acc = b1 * s0 + (1 - b1) * (gg * gg);                              p -= (lr * gg) / sqrt(acc + eps)
The scalars, all float32:
  lr     = lr_base * lr_mult
  norm   = avg * (float) sqrt(S),  S the float64 sum of the squared raw gradient (any order: see below)
  cscale = fmin(fmax(norm, 0), clip) / (1e-7 + norm)  when clip > 0 (Lasagne's total_norm_constraint: NOT 1 when the
           norm is below the clip), else 1
  a_t    = (lr * sqrt(1 - b2^t)) / (1 - b1^t),  the powers from the device's powf.

What can be pinned and what cannot.
  s0, s1 and RMSprop's parameters depend on none of the scalars that involve a sum or a power (given cscale): bit for bit.
  The norm: the float64 sum's own error is n 2^-53 relative, far below 2^-24, so the device's summation order can move
    the float32 value only across a rounding boundary: one ulp for (float) sqrt(S), one more for the multiply by avg.
    It is read from grad_norm_log and required within 2 ulps of norm_f32 -- and EXACTLY equal where S is exact in float64
    and a perfect square (exact_norm_gradient).  With clipping, cscale is computed from the LOGGED norm.
  a_t: powf is not NumPy's, and 1 - P cancels (t = 1, b2 = 0.999: one ulp of P2 moves a_t by hundreds of ulps).
    a_t_candidates lists every a_t from P1, P2 within `ulps` float32 ulps of the correctly rounded float64 power, the rest
    in exact float32; Adam's parameters must match ONE candidate bit for bit, the same for every element of the bucket.

Bounds of the float32 restatement against the float64 version of the same formulas (EPS = 2^-24, one rounding; first
order, times 1 + 2^-20 for the rest; inputs without underflow -- the `plain` gradients of the host test).
  gg: two roundings, 2 EPS |gg|.
  m = b1 s0 + (1 - b1) gg: 1 - b1 and b1 s0 one rounding each; (1 - b1) gg carries 1 + 2 + 1 = 4; the sum one more on
    |m| <= |b1 s0| + |(1 - b1) gg|:          B_m = EPS (2 |b1 s0| + 5 |(1 - b1) gg|).
  v (Adam) / acc (RMSprop) = b s + (1 - b) gg^2, all terms >= 0: gg^2 carries 2 * 2 + 1 = 5, times (1 - b) 7, the other
    term 1, the sum 1:                       B_v = 8 EPS v.
  Adam's step a_t m / (sqrt(v) + eps): sqrt halves v's 8 and rounds, 5; + eps rounds, 6; a_t m rounds, the division
    rounds:                                  B_step = |a_t| B_m / (sqrt(v) + eps) + 8 EPS |step|.
  RMSprop's step lr gg / sqrt(acc + eps): acc + eps 9, sqrt 4.5 + 1; lr gg 2 + 1; the division 1:
                                             B_step = 10 EPS |step|.
  p - step rounds once:                      B_p = B_step + EPS |p - step|.
  The reference's own float32 code (oracle/ref_port.py) does the same operations with (1 - b) g g associated as
  ((1 - b) g) g: the same counts, so it lies within the same bounds of the float64 version.
  Its norm sums the squares in float32: n - 1 additions of non-negative terms and the squares' rounding, n EPS relative
  on the sum, half of it after the root, plus the root's and the float64 side's roundings: (n / 2 + 3) EPS norm."""
import math

import numpy as np

EPS = 2.0 ** -24
F32 = np.float32
F64 = np.float64
ADAM, RMSPROP = 0, 1                    # ARL_OPT_ADAM, ARL_OPT_RMSPROP
OPT_PARTIALS, NORM_SLOTS, NORM_BLOCKS = 1024, 64, 2048
METHODS = {"adam": ADAM, "rmsprop": RMSPROP}

# the nearest wrong versions (update_f32 / cscale_f32 `variant=`)
VARIANTS = ("eps_moved",        # Adam: a_t m / sqrt(v + eps);  RMSprop: lr gg / (sqrt(acc) + eps)
            "assoc",            # gg = g * (avg * cscale)
            "omb_f64",          # 1 - b taken in float64 from the caller's double (1 - 0.9 -> 0.1f, not 1.f - 0.9f)
            "fused",            # b * s + (1 - b) * x with one rounding (what -ffp-contract=fast makes of it)
            "scale_last",       # m / (sqrt(v) + eps) * a_t;  gg / sqrt(acc + eps) * lr
            "cscale_shortcut")  # cscale = 1 when the norm is below the clip


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


# ---- the scalars ----------------------------------------------------------------------------------------------------

def lr_f32(lr_base, lr_mult):
    return F32(lr_base) * F32(lr_mult)


def sumsq_f64(g):
    g = _f32(g).astype(F64)
    with np.errstate(all="ignore"):
        return F64(np.sum(g * g))


def norm_f32(avg, g):
    """avg * (float) sqrt(S), S summed in float64 (NumPy's order, not the device's: within 2 ulps, see the module text)."""
    with np.errstate(all="ignore"):
        return F32(avg) * F32(np.sqrt(sumsq_f64(g)))


def cscale_f32(norm, clip, variant=None):
    """clip <= 0, -0.0 and NaN all fail `clip > 0.f`: no clip.  fminf / fmaxf return the other operand for a NaN."""
    norm, clip = F32(norm), F32(clip)
    if not clip > 0:
        return F32(1)
    if variant == "cscale_shortcut" and norm < clip:
        return F32(1)
    with np.errstate(all="ignore"):
        return F32(np.fmin(np.fmax(norm, F32(0)), clip) / (F32(1e-7) + norm))


def ulp_distance(a, b):
    """Float32 ulps between two finite values of one sign (or equal bits -> 0)."""
    a, b = F32(a), F32(b)
    ia, ib = int(a.view(np.int32)), int(b.view(np.int32))
    return abs(ia - ib)


def pow_f32(b, t):
    """The float64 power of the float32 b, rounded to float32 (b in [0, 1), t >= 1: underflow gives 0)."""
    return F32(math.pow(float(F32(b)), float(t)))


def _neighbours(x, ulps):
    """[(offset, x moved by `offset` float32 ulps)]; a power that is exactly 0 (b = 0, or b^t below half the smallest
    subnormal: 1 - P is 1 for any P that small) has the one candidate."""
    if x == 0:
        return [(0, x)]
    out = [(0, x)]
    lo = hi = x
    for k in range(1, ulps + 1):
        lo, hi = np.nextafter(lo, F32(-1)), np.nextafter(hi, F32(2))
        out += [(-k, lo), (k, hi)]
    return sorted(out)


def a_t_of(lr, p1, p2):
    with np.errstate(all="ignore"):
        return F32(F32(lr) * np.sqrt(F32(1) - F32(p2)) / (F32(1) - F32(p1)))


def a_t_candidates(lr, b1, b2, t, ulps=2):
    """[(a_t, offset of b1^t, offset of b2^t)] for every pair of offsets within `ulps`: (2 ulps + 1)^2 entries unless a
    power is exactly 0 (one offset for it).  Entry (., 0, 0) is a_t from the correctly rounded powers."""
    return [(a_t_of(lr, p1, p2), o1, o2) for o1, p1 in _neighbours(pow_f32(b1, t), ulps)
            for o2, p2 in _neighbours(pow_f32(b2, t), ulps)]


# ---- the update -----------------------------------------------------------------------------------------------------

def _one_minus(b, variant):
    if variant == "omb_f64":
        return F32(1.0 - float(b))              # b as the caller wrote it (a Python double)
    return F32(1) - F32(b)


def _decay(b, omb, s, x, variant):
    b = F32(b)
    if variant == "fused":
        return (b.astype(F64) * s.astype(F64) + F64(omb) * x.astype(F64)).astype(F32)      # products exact, one sum
    return b * s + omb * x


def update_f32(method, p, g, s0, s1, avg, cscale, lr, a_t, b1, b2, eps, variant=None):
    """arl::update_one on whole arrays -> (p, s0, s1) (s1 None for RMSprop).  b1, b2 as the caller wrote them (Python
    doubles; the device gets their float32 values, and so does everything here but the omb_f64 variant)."""
    p, g, s0 = _f32(p), _f32(g), _f32(s0)
    avg, cscale, lr, a_t, eps = F32(avg), F32(cscale), F32(lr), F32(a_t), F32(eps)
    with np.errstate(all="ignore"):
        gg = g * (avg * cscale) if variant == "assoc" else (g * avg) * cscale
        if method == ADAM:
            m = _decay(b1, _one_minus(b1, variant), s0, gg, variant)
            v = _decay(b2, _one_minus(b2, variant), _f32(s1), gg * gg, variant)
            return adam_apply_f32(p, m, v, a_t, eps, variant), m, v
        acc = _decay(b1, _one_minus(b1, variant), s0, gg * gg, variant)
        if variant == "eps_moved":
            d = np.sqrt(acc) + eps
        else:
            d = np.sqrt(acc + eps)
        step = gg / d * lr if variant == "scale_last" else lr * gg / d
        return p - step, acc, None


def adam_apply_f32(p, m, v, a_t, eps, variant=None):
    """p - (a_t * m) / (sqrt(v) + eps): the one place a_t enters (the candidates are tried here)."""
    a_t, eps = F32(a_t), F32(eps)
    with np.errstate(all="ignore"):
        d = np.sqrt(v + eps) if variant == "eps_moved" else np.sqrt(v) + eps
        step = m / d * a_t if variant == "scale_last" else a_t * m / d
        return _f32(p) - step


def same_bits(a, b):
    return _f32(a).tobytes() == _f32(b).tobytes()


def same_bits_nan(a, b):
    """Equal bits wherever neither is NaN, NaN in the same places (a NaN's payload is not part of the contract)."""
    a, b = _f32(a), _f32(b)
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.int32)[~na] == b.view(np.int32)[~na]).all())


def matching_candidates(p_got, p0, m, v, eps, cands):
    """The (offset1, offset2) of every candidate whose a_t gives p_got bit for bit on ALL elements."""
    p_got, head = _f32(p_got), slice(0, 1024)
    hits, seen = [], {}
    for a_t, o1, o2 in cands:
        key = F32(a_t).tobytes()
        if key not in seen:
            ok = same_bits_nan(adam_apply_f32(p0[head], m[head], v[head], a_t, eps), p_got[head])
            seen[key] = ok and same_bits_nan(adam_apply_f32(p0, m, v, a_t, eps), p_got)
        if seen[key]:
            hits.append((o1, o2))
    return hits


# ---- float64 versions and bounds ------------------------------------------------------------------------------------

def update_f64(method, p, g, s0, s1, avg, cscale, lr, a_t, b1, b2, eps):
    """The same formulas in float64 on the float32 inputs and scalars -> (p, B_p, s0, B_s0, s1, B_s1)."""
    p, g, s0 = (_f32(x).astype(F64) for x in (p, g, s0))
    avg, cscale, lr, a_t, eps, b1, b2 = (F64(F32(x)) for x in (avg, cscale, lr, a_t, eps, b1, b2))
    slack = 1 + 2.0 ** -20
    gg = g * avg * cscale
    if method == ADAM:
        s1 = _f32(s1).astype(F64)
        m = b1 * s0 + (1 - b1) * gg
        v = b2 * s1 + (1 - b2) * gg * gg
        b_m = EPS * (2 * np.abs(b1 * s0) + 5 * np.abs((1 - b1) * gg))
        d = np.sqrt(v) + eps
        step = a_t * m / d
        b_step = abs(a_t) * b_m / d + 8 * EPS * np.abs(step)
        pn = p - step
        return pn, slack * (b_step + EPS * np.abs(pn)), m, slack * b_m, v, slack * 8 * EPS * v
    acc = b1 * s0 + (1 - b1) * gg * gg
    step = lr * gg / np.sqrt(acc + eps)
    pn = p - step
    return pn, slack * (10 * EPS * np.abs(step) + EPS * np.abs(pn)), acc, slack * 8 * EPS * acc, None, None


def norm_bound(n, norm):
    return (n / 2.0 + 3) * EPS * float(norm)


def ratio(got, want, bound):
    """max |got - want| / bound (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(got, F64) - want)
    bound = np.asarray(bound, F64)
    return float(np.max(np.where(err == 0, 0., err / np.where(bound > 0, bound, 2.0 ** -1074))))


# ---- inputs ---------------------------------------------------------------------------------------------------------

KINDS = ("wide", "small", "plain", "zero", "nonfinite")


def _spread(rs, n, lo, hi):
    """Normal draws times 10^U(lo, hi): every binade in between is hit."""
    return (rs.randn(n) * 10.0 ** rs.uniform(lo, hi, n)).astype(F32)


def gradient(seed, n, kind):
    """wide:  10^-12 .. 10^2 and planted exact zeros, float32 subnormals and values near +-1e19 (squares overflow
              float32: v, acc become inf and the step 0; the float64 sum of squares stays finite).
    small:    10^-12 .. 10^-4 with zeros and subnormals: the norm stays far below 1, so norm / (1e-7 + norm) != 1.
    plain:    10^-3 .. 10^1, nothing planted (no underflow: the float64 bounds hold).
    zero:     all +0.
    nonfinite: wide with one +inf and one NaN (n >= 2; n == 1: the NaN)."""
    rs = np.random.RandomState(seed)
    if kind == "zero":
        return np.zeros(n, F32)
    if kind == "plain":
        return _spread(rs, n, -3, 1)
    g = _spread(rs, n, -12, -4 if kind == "small" else 2)
    g[4::5] = 0
    sub = (rs.randint(1, 2 ** 22, size=len(g[1::11])) * 2.0 ** -149).astype(F32)
    g[1::11] = sub * np.where(rs.rand(len(sub)) < 0.5, -1, 1).astype(F32)
    if kind != "small":
        big = (1e19 * rs.uniform(0.5, 2, len(g[2::17]))).astype(F32)
        g[2::17] = big * np.where(np.arange(len(big)) % 2, -1, 1).astype(F32)
    if kind == "nonfinite":
        g[n // 2] = np.nan
        if n >= 2:
            g[n // 3] = np.inf
    return g


def exact_norm_gradient(n):
    """-> (g, sqrt(S)) with S exact in float64 and a perfect square: k^2 twos (k = floor(sqrt n)), signs alternating,
    spread over the whole bucket with zeros between them; n < 4: 3, 4, 0 -> 5 (n = 1: 3)."""
    if n < 4:
        g = np.array([3, 4, 0][:n], F32)
        return g, {1: 3.0, 2: 5.0, 3: 5.0}[n]
    k = int(math.isqrt(n))
    g = np.zeros(n, F32)
    at = np.linspace(0, n - 1, k * k).astype(np.int64) if k * k < n else np.arange(n)
    assert len(set(at.tolist())) == k * k
    g[at] = np.where(np.arange(k * k) % 2, -2, 2).astype(F32)
    return g, 2.0 * k


def bucket(seed, n, kind, method):
    """-> dict(p, g, s0, s1): parameters 10^-9 .. 10^1 (many smaller than their step, so that the step's low bits reach
    p), Adam's m signed over 10^-13 .. 1, v / RMSprop's accumulator its like squared; slots do not start at zero (an
    all-zero gradient then still moves Adam's p, and a decay that is skipped shows)."""
    rs = np.random.RandomState(seed + 7919)
    p = _spread(rs, n, -9, 1)
    m = _spread(rs, n, -13, 0)
    v = np.square(_spread(rs, n, -13, 0))
    g = gradient(seed, n, kind)
    return dict(p=p, g=g, s0=m if method == ADAM else v, s1=v if method == ADAM else None)


class Case(object):
    """One update's inputs and arguments.  clip_case: above / equal / below (of the norm), zero (all-zero gradient, clip 1),
    none0 / neg / negzero / nan (no clip).  make() redraws the bucket (seed, seed + 1000, ...) until every variant that
    applies to the case changes at least one bit of (p, s0, s1): a single element shows an order only some of the time."""
    CLIP_CASES = ("above", "equal", "below", "zero", "none0", "neg", "negzero", "nan")
    DEFAULTS = {ADAM: dict(lr_base=1e-3, b1=0.9, b2=0.999, eps=1e-5), RMSPROP: dict(lr_base=7e-4, b1=0.9, b2=0.0, eps=1e-6)}

    def __init__(self, method, n, avg=1.0, clip_case="none0", kind=None, seed=None, lr_mult=1.0, t0=0.0, **hyper):
        self.method, self.n, self.avg, self.clip_case = method, int(n), avg, clip_case
        self.kind = kind or {"above": "small", "equal": "small", "below": "wide", "zero": "zero"}.get(clip_case, "wide")
        self.seed = (n * 31 + method * 7 + Case.CLIP_CASES.index(clip_case)) % 100003 if seed is None else seed
        self.lr_mult, self.t0 = lr_mult, t0
        h = dict(Case.DEFAULTS[method])
        h.update(hyper)
        self.lr_base, self.b1, self.b2, self.eps = h["lr_base"], h["b1"], h["b2"], h["eps"]
        self._made = None

    def __repr__(self):
        return "Case(%s n=%d avg=%.3g %s %s)" % ("adam" if self.method == ADAM else "rmsprop", self.n, self.avg,
                                                 self.clip_case, self.kind)

    # -- scalars
    def lr(self):
        return lr_f32(self.lr_base, self.lr_mult)

    def t(self):
        return F32(self.t0) + F32(1)

    def clip(self, norm):
        """The clip argument of the case, given the norm of this gradient (`equal` wants the device's own)."""
        c = self.clip_case
        if not np.isfinite(norm) and c in ("equal", "below"):
            return F32(0.5)                         # (a NaN clip would mean "no clip")
        with np.errstate(all="ignore"):
            return {"above": F32(1), "equal": F32(norm), "below": F32(norm) / F32(3), "zero": F32(1), "none0": F32(0),
                    "neg": F32(-1), "negzero": F32(-0.0), "nan": F32(np.nan)}[c]

    def a_t0(self):
        return a_t_of(self.lr(), pow_f32(self.b1, self.t()), pow_f32(self.b2, self.t())) if self.method == ADAM else F32(0)

    def update(self, b, norm, a_t=None, variant=None):
        """The restated update of bucket b with cscale from `norm` -> (p, s0, s1)."""
        cs = cscale_f32(norm, self.clip(norm), variant)
        return update_f32(self.method, b["p"], b["g"], b["s0"], b["s1"], self.avg, cs, self.lr(),
                          self.a_t0() if a_t is None else a_t, self.b1, self.b2, self.eps, variant)

    # -- which variants apply
    def not_applicable(self, variant):
        """None if the variant must show on this case, else the reason it cannot."""
        clipped = self.clip_case in ("above", "equal", "below", "zero")
        dyadic = math.frexp(self.avg)[0] == 0.5
        if self.kind == "nonfinite" and clipped:
            return "a NaN in the gradient makes cscale NaN and every output NaN under any order"
        if variant == "cscale_shortcut":
            return None if self.clip_case == "above" else "the norm is not below a positive clip"
        if self.kind == "zero":
            if variant in ("assoc", "omb_f64", "fused"):
                return "gg = 0 whatever the order, and b s + (1 - b) 0 rounds once either way"
            if self.method == RMSPROP:
                return "the step is lr 0 / d = 0 wherever epsilon stands"
        if variant == "assoc":
            if not clipped:
                return "cscale = 1: (g avg) 1 = g (avg 1)"
            if dyadic:
                return "avg is a power of two: scaling by it is exact either way (but for subnormals, not relied on)"
        if variant == "omb_f64":
            bs = (self.b1, self.b2) if self.method == ADAM else (self.b1,)
            if all(_one_minus(b, None) == _one_minus(b, variant) for b in bs):
                return "1 - b is the same float32 either way for these b"
        if variant in ("scale_last", "eps_moved") and float(self.lr()) == 0.0:
            return "lr = 0: the step is 0 either way"
        if variant == "fused" and all(b == 0 for b in ((self.b1, self.b2) if self.method == ADAM else (self.b1,))):
            return "b = 0: 0 s + 1 x rounds once either way"
        return None

    _cache = {}

    def make(self):
        key = (self.method, self.n, self.kind, self.avg, self.clip_case, self.seed, self.lr_mult, self.t0, self.lr_base,
               self.b1, self.b2, self.eps)
        self._made = Case._cache.get(key)
        if self._made is None:
            for attempt in range(3000):
                b = bucket(self.seed + 1000 * attempt, self.n, self.kind, self.method)
                norm = norm_f32(self.avg, b["g"])
                head = dict((k, None if v is None else v[:4096]) for k, v in b.items())    # enough to show an order
                own = self.update(head, norm)
                if all(self.not_applicable(v) or self.differs(own, self.update(head, norm, variant=v)) for v in VARIANTS):
                    self._made = Case._cache[key] = b
                    break
            else:
                raise AssertionError("no draw tells every variant apart: %r" % self)
        return dict((k, None if v is None else v.copy()) for k, v in self._made.items())

    @staticmethod
    def differs(x, y):
        return any(a is not None and not same_bits_nan(a, b) for a, b in zip(x, y))


# ---- case lists -----------------------------------------------------------------------------------------------------

# where each loop shape changes: tail only (no float4), one float4 and a tail, one workgroup +- 1 (256 lanes x float4),
# two workgroups +- 1; past ARL_OPT_PARTIALS x 256 x 4 sumsq_kernel's grid stops growing and its loop takes a second trip;
# past 2048 x 256 x 4 the update kernels' does (ragged tail)
SMALL_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 2047, 2048, 2049]
BIG_SIZES = [OPT_PARTIALS * 256 * 4 + 1024 + 5, 2048 * 256 * 4 + 1024 + 3]
AVGS = [1.0, 0.5, 1.0 / 3]
PAIR_N = 1027                          # every (avg, clip case) pair runs at this size


def step_cases(method):
    """arl_opt_step: every size (avg and clip case rotating through all of them), then every (avg, clip case) pair."""
    out = []
    for i, n in enumerate(SMALL_SIZES + BIG_SIZES):
        out.append(Case(method, n, AVGS[(i + method) % 3], Case.CLIP_CASES[(i + 3 * method) % 8]))
    for avg in AVGS:
        for c in Case.CLIP_CASES:
            out.append(Case(method, PAIR_N, avg, c))
    out.append(Case(method, PAIR_N, 1.0 / 3, "none0", kind="nonfinite"))
    out.append(Case(method, PAIR_N, 1.0 / 3, "below", kind="nonfinite"))
    return out


# (n, hole_first, hole_count): a hole at the start, ending at the last float4 with n % 4 = 0 and 3, 4 elements long, the
# whole bucket with and without a tail, no hole, and one where both caps of opt_split_plan bind (rest > 1 048 576 elements
# -> 1024 workgroups, hole > 2 097 152 -> the 1024 that are left)
SPLIT_HOLES = [(5000, 0, 1024), (4096, 1024, 3072), (4099, 2048, 2048), (3001, 1500, 4), (2048, 0, 2048), (2051, 0, 2048),
               (3001, 0, 0), (4096 + 2048 * 1025 + 1024 * 1025 + 3, 4096, 2048 * 1025)]


def split_plan(n, hole_count):
    """opt_split_plan -> (rest, hole) workgroups."""
    n4, h4 = n >> 2, hole_count >> 2
    rest = min(max((n4 - h4 + 255) // 256, 1), 2048)
    if h4 > 0 and rest > NORM_BLOCKS // 2:
        rest = NORM_BLOCKS // 2
    hb = min((h4 + 511) // 512, NORM_BLOCKS - rest)
    return rest, (max(hb, 1) if h4 > 0 else 0)


# co-run (n, hole_first, hole_count, ARL_CORUN_BLOCKS or None): one workgroup's worth; 5 slots run by 1 and by 3
# workgroups; more slots (293) than the 256 hosting workgroups
CORUN_HOLES = [(3001, 1000, 2000, None), (12003, 1024, 10240, "1"), (12003, 1024, 10240, "3"), (700003, 4096, 600000, None)]


def noclip_cases(method):
    """The buckets of the no-clip, split, co-run and range tests: all `wide`, clip none0."""
    out = []
    for n, _, _ in SPLIT_HOLES:
        out.append(Case(method, n, 1.0 / 3))
    for n, _, _, _ in CORUN_HOLES:
        out.append(Case(method, n, 0.5))
    return out


CHAIN_N = 1027
CHAIN_CALLS = (1, 2, 63, 64)            # updates per call, back to back: odd and even lengths, step_pp ping-pongs


def chain_cases(method):
    """The no-clip calls' updates in order: a fresh gradient and another lr_mult per update, t counting on."""
    return [Case(method, CHAIN_N, 1.0 / 3, "none0", seed=1000 + i, lr_mult=1.0 - 0.125 * (i % 5), t0=float(i))
            for i in range(sum(CHAIN_CALLS))]


def multi_step_cases(method):
    """Three consecutive arl_opt_step calls: another clip case and lr_mult each, lr_mult = 0 in the middle."""
    plan = [("below", 1.0), ("none0", 0.0), ("above", 0.5)]
    return [Case(method, PAIR_N, 1.0 / 3, c, kind="wide" if c != "above" else "small", seed=500 + i, lr_mult=m, t0=float(i))
            for i, (c, m) in enumerate(plan)]


T_STUCK = 2.0 ** 24


def counter_cases(method):
    """t0 = 2^24 - 2, then what the float32 counter does: 2^24 - 1, 2^24, and 2^24 again (2^24 + 1 rounds to even)."""
    return [Case(method, PAIR_N, 0.5, "none0", seed=600 + i, t0=min(T_STUCK - 2 + i, T_STUCK)) for i in range(3)]


def zero_beta_case():
    return Case(ADAM, PAIR_N, 1.0 / 3, "none0", seed=700, b1=0.0, b2=0.0)


RANGE_OFF, RANGE_N, RANGE_AFTER = 1024, 517, 255       # the bucket: [off before][the range][after]


def range_cases():
    """FqfOptimizer's fraction range with the paper's RMSprop arguments: most steps are below half an ulp of p."""
    return [Case(RMSPROP, RANGE_N, 1.0, "none0", seed=800, lr_base=2.5e-9, b1=0.95, eps=1e-5)]


def ring_cases(method, log_len):
    """Three steps from an externally written step_count of 1000: the ring index is ((int) t - 1) % norm_log_len."""
    return [Case(method, PAIR_N, 0.5, "none0", seed=900 + 10 * log_len + i, t0=1000.0 + i) for i in range(3)]


def sequences(method):
    out = [chain_cases(method), multi_step_cases(method), counter_cases(method), ring_cases(method, 1), ring_cases(method, 3)]
    return out + ([[zero_beta_case()]] if method == ADAM else [])


def sequence_buckets(cases):
    """[(case, bucket)]: the first case's own bucket, then each case's gradient on the state the restated update of the
    one before left (a_t from the correctly rounded powers, the norm from the float64 sum)."""
    out, state = [], None
    for c in cases:
        b = c.make()
        if state is not None:
            b["p"], b["s0"], b["s1"] = state
        out.append((c, b))
        state = c.update(b, norm_f32(c.avg, b["g"]))
    return out
