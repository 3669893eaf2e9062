"""CPU half of the optimiser limits tests (csrc/optim.hip, csrc/arl_optim_dev.h; the device half is
tests/test_optim_limits_gpu.py):

- the float32 restatement of tests/optim_ref.py is the reference's formula (oracle/ref_port.adam_step, rmsprop_step,
  clip_by_total_norm) to float32 round-off: both stay within the bounds derived there of the float64 version;
- on the very input sets the device tests use (same Case objects, same seeds) every wrong variant that applies -- epsilon
  on the other side of the square root, g * (avg * cscale), 1 - b from the double, a fused multiply-add, the step scaled
  last, cscale = 1 below the clip -- changes at least one bit of (p, s0, s1), so a device kernel with that order could not
  pass the bit-for-bit comparisons; a variant that cannot apply to a case is named with its reason;
- a_t_candidates holds the value from the correctly rounded powers and has the expected count;
- every refusal of the optimiser entry points that needs no device, with its exact code."""
import ctypes

import numpy as np
import pytest

import optim_ref as R
from optim_ref import ADAM, RMSPROP, F32

ARG, RANGE, ALIGN = -1, -2, -3


# ---------------------------------------------------------------------------------------------- the oracle

@pytest.mark.parametrize("method", ["adam", "rmsprop"])
@pytest.mark.parametrize("clip", [None, 0.5, 1e6])
def test_restatement_is_the_reference_formula(method, clip):
    """Three steps on `plain` gradients, each from the reference's own float32 state: the clipped gradient is the
    reference's bit for bit (same operations), the rest lies within the derived bounds of the float64 version -- the
    restatement and the reference both."""
    from oracle import ref_port as P
    n, avg = 1000, 0.5
    mid = R.METHODS[method]
    b = R.bucket(11, n, "plain", mid)
    p, s0, s1, t = b["p"], b["s0"], b["s1"], F32(0)
    worst = 0.
    for it in range(3):
        g = R.gradient(100 + it, n, "plain")
        lr = R.lr_f32(1e-3, 1.0 - 0.25 * it)
        gavg = g * F32(avg)
        gc, norm = P.clip_by_total_norm(gavg, clip)
        mine = R.norm_f32(avg, g)
        assert abs(float(norm) - float(mine)) <= R.norm_bound(n, mine), (norm, mine)
        cs = R.cscale_f32(norm, 0.0 if clip is None else clip)          # from the reference's own norm
        assert R.same_bits((g * F32(avg)) * cs, gc)
        if mid == ADAM:
            tt = t + F32(1)
            a_t = F32(lr * np.sqrt(F32(1) - F32(0.999) ** tt) / (F32(1) - F32(0.9) ** tt))    # as ref_port.adam_step
            assert a_t.tobytes() in [c[0].tobytes() for c in R.a_t_candidates(lr, 0.9, 0.999, tt, 2)]
            want = P.adam_step(p, gc, s0, s1, t, lr, eps=1e-5)[:3]
            got = R.update_f32(ADAM, p, g, s0, s1, avg, cs, lr, a_t, 0.9, 0.999, 1e-5)
            assert R.same_bits(got[1], want[1])                         # m: the very same operations
            f64 = R.update_f64(ADAM, p, g, s0, s1, avg, cs, lr, a_t, 0.9, 0.999, 1e-5)
            t = tt
        else:
            want = P.rmsprop_step(p, gc, s0, lr) + (None,)
            got = R.update_f32(RMSPROP, p, g, s0, None, avg, cs, lr, 0, 0.9, 0.0, 1e-6)
            f64 = R.update_f64(RMSPROP, p, g, s0, None, avg, cs, lr, 0, 0.9, 0.0, 1e-6)
        for k in range(3 if mid == ADAM else 2):
            for side in (got, want):
                r = R.ratio(side[k], f64[2 * k], f64[2 * k + 1])
                assert r <= 1, (it, k, r)
                worst = max(worst, r)
        p, s0, s1 = want
    print("%s clip %s: largest error / bound = %.4f" % (method, clip, worst))


def test_exact_norm_gradients_are_exact():
    for n in R.SMALL_SIZES + R.BIG_SIZES:
        g, root = R.exact_norm_gradient(n)
        assert float(R.sumsq_f64(g)) == root * root and float(int(root)) == root
        for avg in R.AVGS:
            assert R.norm_f32(avg, g) == F32(avg) * F32(root)


# ------------------------------------------------------------------------------------------ telling variants apart

def _device_inputs(method):
    """[(case, bucket)] of everything the device file runs for this method: the single updates on their own buckets, the
    sequences on the state the update before left."""
    singles = R.step_cases(method) + R.noclip_cases(method) + [c for c in R.range_cases() if c.method == method]
    out = [(c, c.make()) for c in singles]
    for seq in R.sequences(method):
        out += R.sequence_buckets(seq)
    return out


@pytest.mark.parametrize("method", ["adam", "rmsprop"])
def test_device_inputs_tell_every_variant_apart(method):
    mid = R.METHODS[method]
    inputs = _device_inputs(mid)
    cases = [c for c, _ in inputs]
    shown = dict((v, 0) for v in R.VARIANTS)
    named = {}
    for c, b in inputs:
        norm = R.norm_f32(c.avg, b["g"])
        own = c.update(b, norm)
        for v in R.VARIANTS:
            why = c.not_applicable(v)
            if why:
                named.setdefault((v, why), []).append(repr(c))
                continue
            assert c.differs(own, c.update(b, norm, variant=v)), (c, v)
            shown[v] += 1
    for (v, why), who in sorted(named.items()):
        print("%s cannot show on %d cases (%s), e.g. %s" % (v, len(who), why, who[0]))
    print("shown:", shown)
    assert all(k > 0 for k in shown.values()), shown
    # every (avg, clip case) pair the device runs is among them, and every pair is run
    pairs = {(c.avg, c.clip_case) for c in R.step_cases(mid)}
    assert pairs == {(a, k) for a in R.AVGS for k in R.Case.CLIP_CASES}
    # 1 / 3 with a clip shows the association; the clip above the norm shows the shortcut
    assert any(c.avg == R.AVGS[2] and c.not_applicable("assoc") is None for c in cases)
    assert any(c.not_applicable("cscale_shortcut") is None for c in cases)


def test_the_fraction_step_is_below_half_an_ulp_for_some_elements_only():
    """The range case (the FQF paper's RMSprop arguments): the restatement moves some parameters and leaves others where
    they were -- a kernel that does nothing, and one that moves everything, both differ from it."""
    for c in R.range_cases():
        b = c.make()
        p, _, _ = c.update(b, R.norm_f32(c.avg, b["g"]))
        moved = p.view(np.int32) != b["p"].view(np.int32)
        assert 0.02 < moved.mean() < 0.98, moved.mean()


# ---------------------------------------------------------------------------------------------- a_t candidates

def test_a_t_candidates():
    lr = R.lr_f32(1e-3, 0.75)
    for t in (1, 2, 3, 10, 130):
        c = R.a_t_candidates(lr, 0.9, 0.999, F32(t), 2)
        assert len(c) == 25 and len({(o1, o2) for _, o1, o2 in c}) == 25
        p1, p2 = F32(float(F32(0.9)) ** t), F32(float(F32(0.999)) ** t)
        centre = F32(lr * np.sqrt(F32(1) - p2) / (F32(1) - p1))
        assert [a for a, o1, o2 in c if (o1, o2) == (0, 0)][0].tobytes() == centre.tobytes()
        assert len(R.a_t_candidates(lr, 0.9, 0.999, F32(t), 1)) == 9
    # t = 1, b2 = 0.999: one ulp of the power moves a_t by hundreds of ulps (why a_t cannot be pinned from float64)
    c = dict(((o1, o2), a) for a, o1, o2 in R.a_t_candidates(lr, 0.9, 0.999, F32(1), 1))
    assert R.ulp_distance(c[(0, 0)], c[(0, 1)]) > 100
    # powers that are exactly 0: one candidate, a_t == lr
    for b1, b2, t in ((0.0, 0.0, 1), (0.9, 0.999, 2 ** 24), (0.9, 0.999, 2 ** 24 - 1)):
        c = R.a_t_candidates(lr, b1, b2, F32(t), 2)
        assert len(c) == 1 and c[0][0].tobytes() == lr.tobytes()
    assert len(R.a_t_candidates(lr, 0.0, 0.999, F32(5), 2)) == 5
    assert len(R.a_t_candidates(lr, 0.9, 0.999, F32(1001), 2)) == 5          # 0.9^1001 < 2^-150: 0 in float32


# ---------------------------------------------------------------------------------------------- refusals

@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


OK, ODD = 16, 20                     # never dereferenced: every call below is refused before any launch
ADAM_ARGS, RMS_ARGS = (1e-3, 0.5, 0.9, 0.999, 1e-5), (7e-4, 0.5, 0.9, 0.0, 1e-6)     # lr, avg, b1, b2, eps


def _refused(lib, rc, code, text):
    assert rc == code, (rc, lib.arl_last_error())
    assert text.encode() in lib.arl_last_error(), lib.arl_last_error()


def _state(**kw):
    from accel_rl_amd import _lib
    st = _lib.ArlOptState()
    st.n_params = 1000
    st.params = st.grads = st.slot0 = st.slot1 = st.step_count = st.lr_mult = st.partials = st.grad_norm_log = OK
    st.norm_log_len = 4
    for k, v in kw.items():
        setattr(st, k, v)
    return ctypes.byref(st)


def _entries(lib):
    """Every entry point that takes (state, method, hyper-parameters): f(state, method, lr, avg, b1, b2, eps) -> rc."""
    from accel_rl_amd import _lib
    job = _lib.ArlCorunJob()
    return {
        "arl_opt_step": lambda st, m, lr, avg, b1, b2, eps: lib.arl_opt_step(st, m, lr, avg, 0.5, b1, b2, eps, None),
        "arl_opt_step_noclip": lambda st, m, lr, avg, b1, b2, eps:
            lib.arl_opt_step_noclip(st, m, lr, avg, b1, b2, eps, 0, OK, OK, None),
        "arl_opt_step_noclip_split": lambda st, m, lr, avg, b1, b2, eps:
            lib.arl_opt_step_noclip_split(st, m, lr, avg, b1, b2, eps, 0, OK, OK, 0, 8, 1, None),
        "arl_corun_job_init": lambda st, m, lr, avg, b1, b2, eps:
            lib.arl_corun_job_init(ctypes.byref(job), st, m, lr, avg, b1, b2, eps, 0, OK, OK, 0, 8),
    }


@pytest.mark.parametrize("entry", ["arl_opt_step", "arl_opt_step_noclip", "arl_opt_step_noclip_split",
                                   "arl_corun_job_init"])
def test_state_and_hyper_parameter_refusals(lib, entry):
    f = _entries(lib)[entry]
    _refused(lib, f(None, ADAM, *ADAM_ARGS), ARG, "null state")
    for field in ("params", "grads", "slot0", "step_count", "lr_mult"):
        _refused(lib, f(_state(**{field: None}), ADAM, *ADAM_ARGS), ARG, "null pointer in state")
    for method in (-1, 2):
        _refused(lib, f(_state(), method, *ADAM_ARGS), ARG, "unknown method")
    _refused(lib, f(_state(slot1=None), ADAM, *ADAM_ARGS), ARG, "adam needs slot1")
    for n in (0, -4):
        _refused(lib, f(_state(n_params=n), ADAM, *ADAM_ARGS), ARG, "n_params <= 0")
    for n in (0, -1):
        _refused(lib, f(_state(norm_log_len=n), ADAM, *ADAM_ARGS), ARG, "norm_log_len <= 0")
    for field in ("params", "grads", "slot0", "slot1"):
        _refused(lib, f(_state(**{field: ODD}), ADAM, *ADAM_ARGS), ALIGN, "16-byte aligned")
    nan = float("nan")
    # what the arithmetic cannot survive: 1 - beta^t = 0, the root of a negative number
    for b1, b2 in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, -0.1), (1.5, 0.999), (nan, 0.999), (0.9, nan)):
        _refused(lib, f(_state(), ADAM, 1e-3, 0.5, b1, b2, 1e-5), RANGE, "beta1 and beta2 in [0, 1)")
    for rho in (-0.1, 1.5, nan):
        _refused(lib, f(_state(slot1=None), RMSPROP, 7e-4, 0.5, rho, 0.0, 1e-6), RANGE, "rho in [0, 1]")
    for method, args in ((ADAM, ADAM_ARGS), (RMSPROP, RMS_ARGS)):
        for eps in (-1e-8, nan):
            _refused(lib, f(_state(), method, args[0], args[1], args[2], args[3], eps), RANGE, "epsilon")
        for lr in (-1e-3, nan):
            _refused(lib, f(_state(), method, lr, *args[1:]), RANGE, "learning_rate")


def test_step_refuses_null_partials(lib):
    _refused(lib, lib.arl_opt_step(_state(partials=None), ADAM, 1e-3, 0.5, 0.0, 0.9, 0.999, 1e-5, None), ARG,
             "null pointer in state")


def test_noclip_refusals(lib):
    from accel_rl_amd import _lib
    job = ctypes.byref(_lib.ArlCorunJob())

    def split(k=0, pp=OK, parts=OK, first=0, count=8, part=1, st=None):
        return lib.arl_opt_step_noclip_split(st or _state(), ADAM, *ADAM_ARGS, k, pp, parts, first, count, part, None)

    def init(k=0, pp=OK, parts=OK, first=0, count=8, part=1, st=None):       # (a job is always part 1)
        return lib.arl_corun_job_init(job, st or _state(), ADAM, *ADAM_ARGS, k, pp, parts, first, count)

    for call in (split, init):
        _refused(lib, call(pp=None), ARG, "null pointer")
        _refused(lib, call(parts=None), ARG, "null pointer")
        _refused(lib, call(k=-1), RANGE, "update index")
        _refused(lib, call(k=_lib.OPT_NORM_SLOTS), RANGE, "update index")
        _refused(lib, call(first=-4), ARG, "hole")
        _refused(lib, call(first=2), ARG, "hole")
        _refused(lib, call(count=6), ARG, "hole")
        _refused(lib, call(count=-4), ARG, "hole")
        _refused(lib, call(first=996, count=8), ARG, "hole")                # past the end of the bucket
        _refused(lib, call(first=0, count=1004), ARG, "hole")
        _refused(lib, call(count=0), ARG, "part 1 needs a hole")
    _refused(lib, lib.arl_corun_job_init(None, _state(), ADAM, *ADAM_ARGS, 0, OK, OK, 0, 8), ARG, "null pointer")
    _refused(lib, lib.arl_corun_job_run(None, None), ARG, "null pointer")
    for k in (-1, _lib.OPT_NORM_SLOTS):
        _refused(lib, lib.arl_opt_step_noclip(_state(), ADAM, *ADAM_ARGS, k, OK, OK, None), RANGE, "update index")
    _refused(lib, lib.arl_opt_step_noclip(_state(), ADAM, *ADAM_ARGS, 0, None, OK, None), ARG, "null pointer")
    _refused(lib, lib.arl_opt_step_noclip(_state(), ADAM, *ADAM_ARGS, 0, OK, None, None), ARG, "null pointer")


def test_finish_refusals(lib):
    from accel_rl_amd import _lib

    def finish(n=1, pp=OK, parts=OK, hole=0, st=None):
        return lib.arl_opt_finish_split(st or _state(norm_log_len=64), n, 0.5, pp, parts, hole, None)
    _refused(lib, lib.arl_opt_finish_split(None, 1, 0.5, OK, OK, 0, None), ARG, "null pointer")
    _refused(lib, finish(st=_state(step_count=None)), ARG, "null pointer")
    _refused(lib, finish(pp=None), ARG, "null pointer")
    _refused(lib, finish(parts=None), ARG, "null pointer")
    _refused(lib, finish(n=0), RANGE, "n_updates outside")
    _refused(lib, finish(n=_lib.OPT_NORM_SLOTS + 1), RANGE, "n_updates outside")
    for hole in (-4, 6, 1004):
        _refused(lib, finish(hole=hole), ARG, "hole size")
    _refused(lib, finish(st=_state(norm_log_len=0)), ARG, "norm_log_len <= 0")
    # two updates of one call never share a word of the log: n_updates > norm_log_len is refused when a log is given
    _refused(lib, finish(n=5, st=_state(norm_log_len=4)), RANGE, "n_updates above norm_log_len")
    _refused(lib, lib.arl_opt_finish(_state(norm_log_len=4), 5, 0.5, OK, OK, None), RANGE, "n_updates above norm_log_len")
    _refused(lib, lib.arl_opt_finish(_state(), 0, 0.5, OK, OK, None), RANGE, "n_updates outside")
