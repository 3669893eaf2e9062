"""The optimiser kernels (csrc/optim.hip, csrc/arl_optim_dev.h) at the edges of what their entry points accept, driven
directly through the C entry points and compared BIT FOR BIT with the NumPy float32 restatement of tests/optim_ref.py
(the file is compiled with -ffp-contract=off; the update is fp32 element-wise arithmetic in a stated order).

The rules of every comparison (tests/optim_ref.py derives them):
- s0, s1 and RMSprop's parameters: equal bits, unconditionally (NaN in the same places where the gradient is not finite);
- Adam's parameters: equal bits for ONE a_t of a_t_candidates(ulps = 2) -- the device's powf within 2 float32 ulps of
  the correctly rounded power -- the same one for every element of the bucket;
- the norm is read from grad_norm_log and must lie within 2 float32 ulps of the restatement's (float64 sum of squares),
  and equal it EXACTLY where the sum of squares is exact and a perfect square; with clipping, cscale comes from the
  logged norm;
- p, g, s0, s1 and the log sit inside NaN-guarded allocations and the guards are unchanged afterwards; `partials` and
  `norm_parts` are NaN-poisoned before every launch that reads them back, so a slot read without having been written
  turns the logged norm into NaN; step_count and lr_mult sit between guards of their own;
- every update runs twice from the same state and gives the same bits.

tests/test_optim_limits_host.py shows on the CPU that these very inputs (same Case objects, same seeds) give other bits
under each nearest wrong order, so the comparisons below cannot pass by accident.

Measured on an MI355X (printed at the end of the module, run with -s): of the 136 (b1, b2, t)
tried (t = 1 .. 130, 1001 .. 1003, 2^24 - 1, 2^24 at b = (0.9, 0.999); t = 1 at b = (0, 0)) 127 match with both powers
correctly rounded; the device's powf gave 0.9^t one ulp high at t = 3 and 15, 0.999^t one ulp low at t = 64, 71, 85, 109
and one ulp high at t = 66, 67, 87.  Never more than 1 ulp: ulps = 2 was not widened.  Largest deviation of a logged norm:
0 ulps.  The 53 tests take 4.5 s."""
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from optim_ref import ADAM, RMSPROP, F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
LOG_FILL = -7.0                 # what an unwritten word of the norm log holds
POW = {}                        # (b1, b2, t) -> the offsets (of b1^t, of b2^t) that reproduced the device's p in EVERY update
NORM = {"ulps": 0}              # largest |logged norm - restated norm| seen, in float32 ulps


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    yield _lib
    print("\noptimiser limits: largest norm deviation %d ulps; powf: %s" % (NORM["ulps"], _pow_report()))


def _host(t):
    return t.detach().cpu().numpy().copy()


class Guarded(object):
    """n floats at a 16-byte boundary inside a NaN-filled buffer, 64 NaNs (at least) on either side."""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((GUARD + (n + 3) // 4 * 4 + GUARD,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        assert self.t.data_ptr() % 16 == 0
        self.inside = np.zeros(self.buf.numel(), bool)
        self.inside[GUARD:GUARD + n] = True

    def set(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def check(self, what=""):
        raw = _host(self.buf)
        assert np.isnan(raw[~self.inside]).all(), "a launch wrote outside its buffer: %s" % (what,)


class Rig(object):
    """The device side of one bucket: guarded p, g, s0, s1 and norm log, t and lr_mult between guards, poisoned scratch.
    `embed` = (before, after): params and grads are a range inside a larger guarded bucket (FqfOptimizer's second state)."""

    def __init__(self, L, method, n, log_len=4, embed=(0, 0)):
        self.L, self.method, self.n, self.embed = L, method, n, embed
        total = embed[0] + n + embed[1]
        self.P, self.G = Guarded(total), Guarded(total)
        self.S0, self.S1 = Guarded(n), (Guarded(n) if method == ADAM else None)
        self.p, self.g = self.P.t[embed[0]:embed[0] + n], self.G.t[embed[0]:embed[0] + n]
        self.scal = torch.full((8,), float("nan"), device=DEV)          # [2] = step_count, [5] = lr_mult, NaN around
        self.pp = torch.full((6,), float("nan"), device=DEV)            # [2:4] = step_pp
        self.log = Guarded(log_len) if log_len else None
        self.partials = torch.empty(L.OPT_PARTIALS, dtype=torch.float64, device=DEV)
        self.parts = torch.empty(L.OPT_NORM_SLOTS * L.OPT_NORM_BLOCKS, dtype=torch.float64, device=DEV)
        st = L.ArlOptState()
        st.n_params = n
        st.params, st.grads, st.slot0 = self.p.data_ptr(), self.g.data_ptr(), self.S0.t.data_ptr()
        st.slot1 = self.S1.t.data_ptr() if self.S1 else None
        st.step_count, st.lr_mult = self.scal[2:3].data_ptr(), self.scal[5:6].data_ptr()
        st.partials = self.partials.data_ptr()
        st.grad_norm_log, st.norm_log_len = (self.log.t.data_ptr(), log_len) if log_len else (None, 0)
        self.st = st
        self.step_pp = self.pp[2:4]
        if self.log:
            self.log.t.fill_(LOG_FILL)
        self.poison()

    def poison(self):
        self.partials.fill_(float("nan"))
        self.parts.fill_(float("nan"))

    def load(self, state, g, lr_mult):
        """state: dict(p, s0, s1, t[, pp]) on the host."""
        self.p.copy_(torch.from_numpy(state["p"]))
        self.g.copy_(torch.from_numpy(g))
        self.S0.set(state["s0"])
        if self.S1:
            self.S1.set(state["s1"])
        self.scal[2], self.scal[5] = float(state["t"]), float(lr_mult)
        pp = state.get("pp", (state["t"], state["t"]))
        self.pp[2], self.pp[3] = float(pp[0]), float(pp[1])

    def read(self):
        torch.cuda.synchronize()
        return dict(p=_host(self.p), s0=_host(self.S0.t), s1=_host(self.S1.t) if self.S1 else None,
                    t=F32(self.scal[2].item()), pp=_host(self.step_pp), log=_host(self.log.t) if self.log else None,
                    bucket=_host(self.P.t))

    def check(self, g, lr_mult, what=""):
        for x in (self.P, self.G, self.S0, self.S1, self.log):
            if x is not None:
                x.check(what)
        scal, pp = _host(self.scal), _host(self.pp)
        assert np.isnan(scal[[0, 1, 3, 4, 6, 7]]).all() and np.isnan(pp[[0, 1, 4, 5]]).all(), what
        assert scal[5] == F32(lr_mult), what
        assert _host(self.g).tobytes() == g.tobytes(), "the gradient was written: %s" % (what,)


def _same(a, b, what):
    if a is None and b is None:
        return
    assert R.same_bits_nan(a, b), (what, int((a.view(np.int32) != b.view(np.int32)).sum()))


def _same_outputs(x, y, what):
    for k in ("p", "s0", "s1", "log", "pp", "bucket"):
        _same(x[k], y[k], (what, k, "second run differs"))
    assert x["t"] == y["t"], what


def _args(c, clip=None):
    """The hyper-parameter arguments of the entry points for case c (Python doubles: the call rounds them to float32)."""
    head = (c.method, c.lr_base, c.avg)
    return head + ((float(clip),) if clip is not None else ()) + (c.b1, c.b2, c.eps)


def _norm_close(logged, g, avg, what, exact=None):
    """The logged norm against the restatement: 2 ulps, exact where stated; non-finite: the same non-finite value."""
    want = R.norm_f32(avg, g) if exact is None else F32(avg) * F32(exact)
    logged = F32(logged)
    if not np.isfinite(want):
        assert (np.isnan(want) and np.isnan(logged)) or want == logged, (what, logged, want)
        return
    assert np.isfinite(logged), (what, logged, want)
    d = R.ulp_distance(logged, want)
    NORM["ulps"] = max(NORM["ulps"], d)
    assert d <= (0 if exact is not None else 2), (what, logged, want, d)


def _verify(c, pre, g, got, cscale, what):
    """got = the device's (p, s0, s1) after case c's update of state `pre` with gradient g."""
    p, s0, s1 = R.update_f32(c.method, pre["p"], g, pre["s0"], pre["s1"], c.avg, cscale, c.lr(), 0, c.b1, c.b2, c.eps)
    _same(got["s0"], s0, (what, "s0"))
    _same(got["s1"], s1, (what, "s1"))
    if c.method == RMSPROP:
        _same(got["p"], p, (what, "p"))
        return None
    t = F32(pre["t"]) + F32(1)
    cands = R.a_t_candidates(c.lr(), c.b1, c.b2, t, 2)
    hits = R.matching_candidates(got["p"], pre["p"], s0, s1, c.eps, cands)
    assert hits, (what, "no a_t within 2 ulps of the correctly rounded powers reproduces p", t)
    if float(c.lr()) != 0.0 and np.isfinite(cscale):
        # powf(b, t) is one value per (b, t): its offsets lie in every update's set of matches
        key = (c.b1, c.b2, float(t))
        POW[key] = POW.get(key, set(hits)) & set(hits)
        assert POW[key], (what, "no one pair of powf offsets explains every update at this (b1, b2, t)", key)
    return cands


def _state_of(b, t):
    return dict(p=b["p"], s0=b["s0"], s1=b["s1"], t=F32(t))


def _partials_written(rig, n, g, what):
    """arl_opt_step's sum-of-squares launch wrote its nb partials and nothing else of the poisoned scratch."""
    nb = min(max(((n >> 2) + 255) // 256, 1), R.OPT_PARTIALS)
    part = _host(rig.partials)
    assert np.isnan(part[nb:]).all(), what
    if np.isfinite(g).all():
        assert np.isfinite(part[:nb]).all(), what


def _one_step(L, rig, c, pre, g, clip, what, exact=None):
    """arl_opt_step of case c from state `pre`, twice; everything checked -> the state it left."""
    outs = []
    for _ in range(2):
        rig.load(pre, g, c.lr_mult)
        if rig.log:
            rig.log.t.fill_(LOG_FILL)
        rig.poison()
        L.opt_step(rig.st, *_args(c, clip))
        outs.append(rig.read())
    got = outs[0]
    _same_outputs(got, outs[1], what)
    rig.check(g, c.lr_mult, what)
    _partials_written(rig, c.n, g, what)
    t = F32(pre["t"]) + F32(1)
    assert got["t"] == t and got["t"] == c.t(), (what, got["t"], t)
    cscale = F32(1)
    if rig.log:
        idx = (int(t) - 1) % rig.st.norm_log_len                 # arl_opt_step's ring index: Lasagne's t, not k
        others = np.delete(got["log"], idx)
        assert (others == F32(LOG_FILL)).all(), (what, got["log"])
        _norm_close(got["log"][idx], g, c.avg, what, exact)
        cscale = R.cscale_f32(got["log"][idx], clip)
    cands = _verify(c, pre, g, got, cscale, what)
    return dict(p=got["p"], s0=got["s0"], s1=got["s1"], t=got["t"]), cands, cscale


def _clip_of(L, rig, c, pre, g):
    """The clip argument of the case; `equal` takes the device's own norm from an unclipped probe launch."""
    if c.clip_case != "equal":
        return c.clip(R.norm_f32(c.avg, g))
    rig.load(pre, g, c.lr_mult)
    rig.poison()
    L.opt_step(rig.st, *_args(c, 0.0))
    idx = (int(F32(pre["t"]) + F32(1)) - 1) % rig.st.norm_log_len
    return F32(rig.read()["log"][idx])


# ------------------------------------------------------------------------------------------------ arl_opt_step

def _run_single(L, c):
    b = c.make()
    rig = Rig(L, c.method, c.n, log_len=4)
    pre = _state_of(b, c.t0)
    clip = _clip_of(L, rig, c, pre, b["g"])
    post, _, cscale = _one_step(L, rig, c, pre, b["g"], clip, c)
    return b, post, cscale, clip


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_step_at_every_loop_shape(L, method):
    """Every bucket size at which a loop shape changes (tests/optim_ref.py SMALL_SIZES, BIG_SIZES), avg and clip case
    rotating through all of them."""
    cases = R.step_cases(R.METHODS[method])[:len(R.SMALL_SIZES) + len(R.BIG_SIZES)]
    assert [c.n for c in cases] == R.SMALL_SIZES + R.BIG_SIZES
    for c in cases:
        _run_single(L, c)
    print("norm: largest deviation so far %d ulps; powf offsets so far %s" % (NORM["ulps"], _pow_report()))


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_step_every_avg_and_clip_case(L, method):
    """avg 1, 1/2, 1/3 x clip above / equal to / below the norm, an all-zero gradient, and the four spellings of "no
    clip" (0, -1, -0.0, NaN); then a gradient with one +inf and one NaN, unclipped and clipped."""
    mid = R.METHODS[method]
    cases = R.step_cases(mid)[len(R.SMALL_SIZES) + len(R.BIG_SIZES):]
    assert len(cases) == 3 * 8 + 2
    for c in cases:
        b, post, cscale, clip = _run_single(L, c)
        if c.clip_case == "above":
            assert cscale != 1 and clip > R.norm_f32(c.avg, b["g"])               # Lasagne's quirk: not 1
        if c.clip_case == "equal":
            assert 0 < cscale < 1
        if c.clip_case == "below" and c.kind == "wide":
            assert 0.3 < cscale < 0.34
        if c.clip_case == "zero":
            assert cscale == 0 and not b["g"].any()
            assert (post["s0"] != b["s0"]).any()                                   # the slots decay ...
            assert (post["p"] != b["p"]).any() == (mid == ADAM)                    # ... and Adam's m still moves p
        if c.clip_case in ("none0", "neg", "negzero", "nan") and c.kind == "wide":
            assert cscale == 1
        if c.kind == "nonfinite":
            bad = np.isnan(post["p"])
            assert bad.all() if c.clip_case == "below" else (bad.sum() == 2 and np.isnan(b["g"]).sum() == 1)
    print("norm: largest deviation so far %d ulps; powf offsets so far %s" % (NORM["ulps"], _pow_report()))


def _run_sequence(L, cases, log_len, checks=None):
    """Consecutive arl_opt_step calls with carried state -> [(case, pre, post, candidates)]."""
    rig = Rig(L, cases[0].method, cases[0].n, log_len=log_len)
    pre, out = None, []
    for c in cases:
        b = c.make()
        pre = _state_of(b, c.t0) if pre is None else dict(p=post["p"], s0=post["s0"], s1=post["s1"], t=post["t"])
        clip = _clip_of(L, rig, c, pre, b["g"])
        post, cands, _ = _one_step(L, rig, c, pre, b["g"], clip, c)
        out.append((c, pre, post, cands))
    return out


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_three_steps_with_a_changing_lr_mult(L, method):
    steps = _run_sequence(L, R.multi_step_cases(R.METHODS[method]), 4)
    (c, pre, post, _), = [s for s in steps if s[0].lr_mult == 0.0]
    assert post["p"].tobytes() == pre["p"].tobytes()                               # lr_mult = 0: p stays, bit for bit
    assert post["s0"].tobytes() != pre["s0"].tobytes() and post["t"] == pre["t"] + 1     # ... while slots and t advance
    assert [float(s[2]["t"]) for s in steps] == [1.0, 2.0, 3.0]


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
@pytest.mark.parametrize("log_len", [1, 3])
def test_ring_index_from_an_external_step_count(L, method, log_len):
    """step_count written from outside (1000): the norm of the step that makes t lands at (t - 1) % norm_log_len
    (_one_step checks the word and that the others stay untouched)."""
    steps = _run_sequence(L, R.ring_cases(R.METHODS[method], log_len), log_len)
    assert [float(s[2]["t"]) for s in steps] == [1001.0, 1002.0, 1003.0]
    assert [(int(s[2]["t"]) - 1) % log_len for s in steps] == ([0, 0, 0] if log_len == 1 else [1, 2, 0])


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_step_without_a_norm_log(L, method):
    """grad_norm_log = NULL: the update (clipped: the norm still matters) is the one with a log, bit for bit."""
    c = R.step_cases(R.METHODS[method])[len(R.SMALL_SIZES) + len(R.BIG_SIZES) + 2 * 8 + 2]
    assert c.clip_case == "below" and c.avg == R.AVGS[2]
    b, post, cscale, clip = _run_single(L, c)
    rig = Rig(L, c.method, c.n, log_len=0)
    pre = _state_of(b, c.t0)
    outs = []
    for _ in range(2):
        rig.load(pre, b["g"], c.lr_mult)
        rig.poison()
        L.opt_step(rig.st, *_args(c, clip))
        outs.append(rig.read())
    rig.check(b["g"], c.lr_mult, c)
    for got in outs:
        for k in ("p", "s0", "s1"):
            _same(got[k], post[k], (c, k))
        assert got["t"] == post["t"]


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_step_counter_at_two_to_the_24(L, method):
    """From step_count = 2^24 - 2: t reaches 2^24 and stays there (2^24 + 1 is not a float32), the ring index stays at
    (2^24 - 1) % len, and for Adam with the default betas both powers have underflowed to 0 long before, so a_t == lr
    exactly: ONE candidate, an unconditional bit-for-bit comparison of Adam's parameters."""
    mid = R.METHODS[method]
    steps = _run_sequence(L, R.counter_cases(mid), 3)
    assert [float(s[2]["t"]) for s in steps] == [2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24]
    if mid == ADAM:
        for c, _, _, cands in steps:
            assert len(cands) == 1 and cands[0][0].tobytes() == c.lr().tobytes()
        c = R.zero_beta_case()                                                      # b1 = b2 = 0: the powers are 0
        (_, _, _, cands), = _run_sequence(L, [c], 4)
        assert len(cands) == 1 and cands[0][0].tobytes() == c.lr().tobytes()
    # the one-launch update reads and writes the same counter: stuck at 2^24 as well
    cases = R.counter_cases(mid)[1:]
    rig = Rig(L, mid, cases[0].n, log_len=4)
    pre = _state_of(cases[0].make(), cases[0].t0)
    for k, c in enumerate(cases):
        pre = _noclip_update(L, rig, c, pre, c.make()["g"], k, c)
        assert pre["t"] == F32(2.0 ** 24) and pre["pp"][(k + 1) & 1] == F32(2.0 ** 24)


# ------------------------------------------------------------------------ arl_opt_step_noclip / arl_opt_finish

def _noclip_update(L, rig, c, pre, g, k, what, launch=None):
    """Update k of a call, twice from state `pre` (with its step_pp) -> the state it left (p, s0, s1, t, pp).
    launch(): the launches that make up the update (default: arl_opt_step_noclip)."""
    outs = []
    for _ in range(2):
        rig.load(pre, g, c.lr_mult)
        if launch is None:
            L.opt_step_noclip(rig.st, *_args(c), k, rig.step_pp, rig.parts)
        else:
            launch()
        outs.append(rig.read())
    got = outs[0]
    _same_outputs(got, outs[1], what)
    rig.check(g, c.lr_mult, what)
    pp = pre.get("pp", (pre["t"], pre["t"]))
    t = F32(pp[k & 1]) + F32(1)
    assert got["t"] == t and got["pp"][(k + 1) & 1] == t and got["pp"][k & 1] == F32(pp[k & 1]), (what, got["pp"], t)
    _verify(c, dict(pre, t=pp[k & 1]), g, got, F32(1), what)
    return dict(p=got["p"], s0=got["s0"], s1=got["s1"], t=got["t"], pp=got["pp"])


def _finish(L, rig, n_upd, avg, hole_count=0):
    L.opt_finish(rig.st, n_upd, avg, rig.step_pp, rig.parts, hole_count=hole_count)
    out = rig.read()
    L.opt_finish(rig.st, n_upd, avg, rig.step_pp, rig.parts, hole_count=hole_count)       # idempotent: same bits
    again = rig.read()
    _same_outputs(out, again, "finish")
    return out


def _parts_rows(rig, n_upd, used, what):
    """norm_parts after a call: rows k < n_upd hold `used` written partial sums, everything else is still poison."""
    parts = _host(rig.parts).reshape(R.NORM_SLOTS, R.NORM_BLOCKS)
    assert np.isfinite(parts[:n_upd, :used]).all(), what
    assert np.isnan(parts[:n_upd, used:]).all() and np.isnan(parts[n_upd:]).all(), what
    return parts


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_noclip_calls_of_1_2_63_and_64_updates(L, method):
    """Back to back on one bucket, a fresh gradient and another lr_mult per update: p, s0, s1, both words of step_pp
    and step_count after every update; every logged norm of every call, the log's other words, and norm_parts."""
    mid = R.METHODS[method]
    cases = R.chain_cases(mid)
    rig = Rig(L, mid, R.CHAIN_N, log_len=R.NORM_SLOTS)
    state = _state_of(cases[0].make(), 0.0)
    log_before = np.full(R.NORM_SLOTS, LOG_FILL, F32)
    i = 0
    for n_upd in R.CHAIN_CALLS:
        rig.poison()
        grads = []
        for k in range(n_upd):
            c = cases[i]
            g = c.make()["g"]
            assert float(state["t"]) == c.t0
            state = _noclip_update(L, rig, c, state, g, k, (n_upd, k))
            grads.append(g)
            i += 1
        out = _finish(L, rig, n_upd, c.avg)
        t = F32(i)
        assert out["t"] == t and (out["pp"] == t).all(), (n_upd, out["pp"])           # both words levelled
        for k in ("p", "s0", "s1"):
            _same(out[k], state[k], ("finish moved", k))
        for k, g in enumerate(grads):
            _norm_close(out["log"][k], g, c.avg, (n_upd, k))
        assert out["log"][n_upd:].tobytes() == log_before[n_upd:].tobytes()           # the other words: as they were
        log_before = out["log"]
        _parts_rows(rig, n_upd, R.split_plan(R.CHAIN_N, 0)[0], n_upd)
        state = dict(p=out["p"], s0=out["s0"], s1=out["s1"], t=out["t"], pp=out["pp"])
    assert i == sum(R.CHAIN_CALLS) == 130
    print("norm: largest deviation so far %d ulps; powf offsets so far %s" % (NORM["ulps"], _pow_report()))


# --------------------------------------------------------------------- arl_opt_step_noclip_split, arl_corun_job

def _split_call(L, rig, c, b, first, count, hole_launch, what, exact=None):
    """A call of two updates (k = 0 on the case's bucket, k = 1 with the same gradient on the state that left), each
    as hole_launch(k) (None: no launch for the hole) then part 0, closed by arl_opt_finish_split; all checked against
    the restatement -> (state after, norm_parts)."""
    state = _state_of(b, c.t0)
    rig.poison()
    for k in range(2):
        def launch():
            if hole_launch is not None:
                hole_launch(k)
            L.opt_step_noclip_split(rig.st, *_args(c), k, rig.step_pp, rig.parts, first, count, 0)
        state = _noclip_update(L, rig, c, state, b["g"], k, (what, k), launch)
    out = _finish(L, rig, 2, c.avg, hole_count=count)
    assert out["t"] == F32(c.t0) + F32(2) and (out["pp"] == out["t"]).all()
    for k in range(2):
        _norm_close(out["log"][k], b["g"], c.avg, (what, "norm", k), exact)
    assert (out["log"][2:] == F32(LOG_FILL)).all()
    rest, hole = R.split_plan(c.n, count)
    return state, _parts_rows(rig, 2, rest + hole, what)


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
@pytest.mark.parametrize("hole", range(len(R.SPLIT_HOLES)), ids=["%d-%d-%d" % h for h in R.SPLIT_HOLES])
def test_split_update_against_the_restatement(L, method, hole):
    """Part 1 (the hole) as its own launch, then part 0: every element updated exactly once whatever the hole -- at the
    start, ending at the last float4, 4 long, the whole bucket (part 0 still does the tail and advances t), none at
    all, and one where both caps of opt_split_plan bind."""
    mid = R.METHODS[method]
    n, first, count = R.SPLIT_HOLES[hole]
    c = R.noclip_cases(mid)[hole]
    assert c.n == n
    b = c.make()
    rig = Rig(L, mid, n, log_len=4)
    rest, hb = R.split_plan(n, count)
    if hole == len(R.SPLIT_HOLES) - 1:
        assert n - count > 1048576 and count > 2097152 and (rest, hb) == (1024, 1024)          # both caps bind

    def own(k):
        L.opt_step_noclip_split(rig.st, *_args(c), k, rig.step_pp, rig.parts, first, count, 1)
    state, _ = _split_call(L, rig, c, b, first, count, own if count else None, (c, first, count))
    if count == 0:
        # no hole, part 0: the plain update's bits, the logged norms included (the same grid, the same partial sums)
        plain = Rig(L, mid, n, log_len=4)
        pre = _state_of(b, c.t0)
        for k in range(2):
            pre = _noclip_update(L, plain, c, pre, b["g"], k, ("plain", k))
        out = _finish(L, plain, 2, c.avg)
        for k in ("p", "s0", "s1"):
            _same(out[k], state[k], ("plain", k))
        assert out["log"].tobytes() == rig.read()["log"].tobytes()


def _conv3_host(L):
    """conv 3's data gradient at 8 images: the launch that hosts a job."""
    geom = L.conv_geom(8, 12, 9, 64, 64, 3, 3, 1, 1, 1)
    gen = torch.Generator(device=DEV).manual_seed(5)
    dy = torch.randn(8, 12, 9, 64, device=DEV, generator=gen)
    wt = torch.randn(64, 3, 3, 64, device=DEV, generator=gen) * 0.05
    dx_ref = torch.empty(8, 12, 9, 64, device=DEV)
    assert not L.conv2d_bwd_data(dy, wt, None, dx_ref, geom)                  # no job: none taken
    return geom, dy, wt, dx_ref


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
@pytest.mark.parametrize("carrier", ["data gradient", "corun_job_run"])
@pytest.mark.parametrize("hole", range(len(R.CORUN_HOLES)), ids=["%d-%d-%d-%s" % h for h in R.CORUN_HOLES])
def test_corun_job_against_the_restatement(L, method, carrier, hole):
    """The hole's update as a job: inside conv 3's data-gradient launch (whose dx must not change), or run by
    arl_corun_job_run.  With ARL_CORUN_BLOCKS = 1 and 3, and with a hole of more slots than the 256 hosting workgroups,
    fewer workgroups run the part than it has norm slots: workgroup 0 zero-fills the others -- norm_parts is poisoned,
    so a missing zero-fill turns the logged norm into NaN.  A job that is made and never run changes nothing."""
    mid = R.METHODS[method]
    n, first, count, env = R.CORUN_HOLES[hole]
    c = R.noclip_cases(mid)[len(R.SPLIT_HOLES) + hole]
    assert c.n == n
    b = c.make()
    rig = Rig(L, mid, n, log_len=4)
    geom, dy, wt, dx_ref = _conv3_host(L)
    rest, slots = R.split_plan(n, count)
    hosted = carrier == "data gradient"
    ran = min(slots, int(env) if env else 256) if hosted else slots
    old = os.environ.get("ARL_CORUN_BLOCKS")
    try:
        if env:
            os.environ["ARL_CORUN_BLOCKS"] = env                              # read by arl_corun_job_init

        def job_launch(k):
            abandoned = L.corun_job(rig.st, *_args(c), k, rig.step_pp, rig.parts, first, count)     # never run: nothing
            job = L.corun_job(rig.st, *_args(c), k, rig.step_pp, rig.parts, first, count)
            del abandoned
            if hosted:
                dx = torch.full_like(dx_ref, float("nan"))
                assert L.conv2d_bwd_data(dy, wt, None, dx, geom, corun=job)   # the launch took the job
                assert torch.equal(dx, dx_ref)
            else:
                L.corun_job_run(job)
        state, parts = _split_call(L, rig, c, b, first, count, job_launch, (c, first, count, env, carrier))
    finally:
        if old is None:
            os.environ.pop("ARL_CORUN_BLOCKS", None)
        else:
            os.environ["ARL_CORUN_BLOCKS"] = old
    # the slots of workgroups that did not run read exactly 0
    assert (parts[:2, rest + ran:rest + slots] == 0).all() and (ran < slots) == (hosted and hole > 0)
    # a job that was made and not run: the bucket is as the call left it
    L.corun_job(rig.st, *_args(c), 0, rig.step_pp, rig.parts, first, count)
    after = rig.read()
    for k in ("p", "s0", "s1"):
        _same(after[k], state[k], ("abandoned job", k))


# ------------------------------------------------------------------------------------------------ exact norms

@pytest.mark.parametrize("path", ["step", "noclip", "split"])
def test_norm_is_exact_where_the_sum_of_squares_is(L, path):
    """Gradients of +-2 and 0 (3, 4 for n < 4): the sum of squares is exact in float64 in any order and a perfect square,
    so the logged norm must EQUAL avg * sqrt(S) -- for avg = 1/3 too (one float32 multiply)."""
    if path == "split":
        sizes = [(n, f, k) for n, f, k in R.SPLIT_HOLES if k]
    else:
        sizes = [(n, 0, 0) for n in R.SMALL_SIZES + R.BIG_SIZES]
    for i, (n, first, count) in enumerate(sizes):
        c = R.Case(RMSPROP, n, R.AVGS[i % 3], "none0", seed=40 + i)
        b = c.make()
        g, root = R.exact_norm_gradient(n)
        b["g"] = g
        rig = Rig(L, RMSPROP, n, log_len=4)
        if path == "step":
            _one_step(L, rig, c, _state_of(b, 0.0), g, F32(0), (path, n), exact=root)
            continue

        def own(k):
            L.opt_step_noclip_split(rig.st, *_args(c), k, rig.step_pp, rig.parts, first, count, 1)
        _split_call(L, rig, c, b, first, count, own if count else None, (path, n), exact=root)


# --------------------------------------------------------------------------- a range inside a bucket (FqfOptimizer)

def test_range_inside_a_bucket_with_the_fqf_arguments(L):
    """params and grads point 4 * off bytes into a larger bucket, the slots are the range's own (FqfOptimizer's second
    state), RMSprop with the paper's arguments (2.5e-9, 0.95, 1e-5), clip = 0: the range updates bit for bit -- most
    steps are below half an ulp of p, and exactly the elements the restatement moves have moved -- and the bucket on
    either side is untouched."""
    c, = R.range_cases()
    b = c.make()
    rs = np.random.RandomState(5)
    before, after = rs.randn(R.RANGE_OFF).astype(F32), rs.randn(R.RANGE_AFTER).astype(F32)
    rig = Rig(L, RMSPROP, c.n, log_len=1, embed=(R.RANGE_OFF, R.RANGE_AFTER))
    assert rig.st.params == rig.P.t.data_ptr() + 4 * R.RANGE_OFF
    whole = np.concatenate([before, b["p"], after])
    rig.P.set(whole)
    rig.G.set(rs.randn(len(whole)).astype(F32))                      # (outside the range: never read)
    post, _, _ = _one_step(L, rig, c, _state_of(b, 0.0), b["g"], F32(0), c)
    out = rig.read()["bucket"]
    assert out[:R.RANGE_OFF].tobytes() == before.tobytes() and out[R.RANGE_OFF + c.n:].tobytes() == after.tobytes()
    want, _, _ = c.update(b, R.norm_f32(c.avg, b["g"]))
    moved = post["p"].view(np.int32) != b["p"].view(np.int32)
    assert (moved == (want.view(np.int32) != b["p"].view(np.int32))).all() and 0 < moved.sum() < c.n
    print("fraction range: %d of %d parameters moved" % (moved.sum(), c.n))


# ------------------------------------------------------------------------------------------------ refusals

def test_finish_refuses_more_updates_than_log_words(L):
    """Update k logs at k % norm_log_len from a workgroup of its own; with n_updates > norm_log_len two workgroups would
    write one word in an undefined order.  Refused (ARL_E_RANGE), nothing launched, nothing written; without a log the
    same call is fine."""
    c = R.Case(RMSPROP, 1027, 0.5, "none0", seed=41)
    b = c.make()
    rig = Rig(L, RMSPROP, c.n, log_len=2)
    state = _state_of(b, 0.0)
    rig.poison()
    for k in range(3):
        state = _noclip_update(L, rig, c, state, b["g"], k, ("refusal", k))
    before = rig.read()
    with pytest.raises(RuntimeError, match="code -2"):
        L.opt_finish(rig.st, 3, c.avg, rig.step_pp, rig.parts)
    after = rig.read()
    _same_outputs(before, after, "a refused finish wrote")
    assert (after["log"] == F32(LOG_FILL)).all() and after["pp"][0] != after["pp"][1]
    rig.st.grad_norm_log = None
    L.opt_finish(rig.st, 3, c.avg, rig.step_pp, rig.parts)
    out = rig.read()
    assert out["t"] == 3 and (out["pp"] == 3).all() and (out["log"] == F32(LOG_FILL)).all()


def _pow_report():
    """What the matches say about the device's powf.  Several offsets can give one a_t (1 - P absorbs an ulp of a small
    P), so a match names a set; reported: how many (b1, b2, t) matched with both powers correctly rounded, and every
    (b1, b2, t) that did not, with the offsets that matched instead."""
    exact = sum((0, 0) in hits for hits in POW.values())
    off = ["b=(%g, %g) t=%g: %s" % (b1, b2, t, sorted(hits, key=lambda h: (abs(h[0]) + abs(h[1]), h))[:3])
           for (b1, b2, t), hits in sorted(POW.items()) if (0, 0) not in hits]
    return "%d of %d (b1, b2, t) match at offsets (0, 0); the others: %s" % (exact, len(POW), off)
