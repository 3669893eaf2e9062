"""R2D2 without a GPU: the float64 restatements of tests/r2d2_ref.py against themselves, the sampleable-slot predicate of
the sequence replay against a brute-force simulation of the ring, and every refusal that needs no device -- the three
entry points of csrc/r2d2.hip, SequenceReplayBuffer's constructor, DQN with a recurrent policy, R2D2 with a feed-forward
one."""
import ctypes

import numpy as np
import pytest

import r2d2_ref as rr

NAN, INF = float("nan"), float("inf")
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3


# ---- the restatement against itself -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mag", [0.0, 1e-6, 1e-3, 0.5, 3.0, 250.0, 1e4])
def test_rescaling_and_its_inverse_undo_each_other(mag):
    """h_inv(h(x)) and h(h_inv(x)) return x within 1e-9 |x|, both signs, with the formulae exactly as the kernel states
    them.  Measured (float64 NumPy), worst |error| / |x| over both directions and signs: 5.5e-16 at 1e4, 3.4e-16 at 250,
    1.5e-16 at 3, 4.4e-16 at 0.5, 1.0e-13 at 1e-3 and 1.2e-10 at 1e-6 (what is left there is h's own sqrt(|z| + 1) - 1).
    The inverse is evaluated as dl (dl + 2): the closed form's u * u - 1 would leave 1.1e-7 at 1e-6 (next test)."""
    eps = 1e-3
    x = np.array([mag, -mag])
    for name, back in (("h_inv(h(x))", rr.h_inv64(rr.h64(x, eps), eps)), ("h(h_inv(x))", rr.h64(rr.h_inv64(x, eps), eps))):
        err = np.abs(back - x)
        print("%s at |x| = %g: worst |error| %.3g, bound %.3g" % (name, mag, err.max(), 1e-9 * mag))
    for back in (rr.h_inv64(rr.h64(x, eps), eps), rr.h64(rr.h_inv64(x, eps), eps)):
        assert (np.abs(back - x) <= 1e-9 * np.abs(x)).all()
    assert (np.sign(rr.h64(x, eps)) == np.sign(x)).all()


def test_the_inverse_is_the_closed_form_without_its_cancellation():
    """dl (dl + 2) with dl = 2 |x| / (s + 1 + 2 eps) is ((s - 1) / (2 eps))^2 - 1: the two agree to the closed form's own
    rounding (an absolute error of about 2^-53 / (2 eps) (1 + |u|) from u = (s - 1) / (2 eps)), and only the closed form
    loses the round trip near zero."""
    eps = 1e-3
    mags = np.array([0.0, 1e-6, 1e-3, 0.5, 3.0, 250.0, 1e4])
    x = np.concatenate([mags, -mags])
    stable, closed = rr.h_inv64(x, eps), rr.h_inv_closed_form64(x, eps)
    u = (np.sqrt(1.0 + 4.0 * eps * (np.abs(x) + 1.0 + eps)) - 1.0) / (2.0 * eps)
    bound = 4 * 2.0 ** -53 / (2.0 * eps) * (1.0 + u) * u + 4 * 2.0 ** -52 * np.abs(stable)
    print("worst |stable - closed| / bound: %.3g" % (np.abs(stable - closed) / np.maximum(bound, 1e-300)).max())
    assert (np.abs(stable - closed) <= bound).all() and (stable[x == 0] == 0).all()
    small = np.array([1e-6, -1e-6])
    assert (np.abs(rr.h_inv_closed_form64(rr.h64(small, eps), eps) - small) > 1e-9 * 1e-6).all()
    assert (np.abs(rr.h_inv64(rr.h64(small, eps), eps) - small) <= 1e-9 * 1e-6).all()


def test_without_rescaling_and_burn_in_one_train_step_is_n_step_double_dqn():
    rng = np.random.RandomState(5)
    for dueling in (False, True):
        for n in (1, 3):
            batch, n_act, stride, gamma_n = 7, 6, 8, 0.99 ** n
            U = 1 + n
            q = rng.randn(batch * U, stride).astype(np.float32)
            qt = rng.randn(batch * U, stride).astype(np.float32)
            act = rng.randint(0, n_act, batch * U).astype(np.uint8)
            ret = rng.randn(batch * U).astype(np.float32)
            term = (rng.rand(batch * U) < 0.3).astype(np.uint8)
            isw = rng.rand(batch).astype(np.float32)
            out = rr.r2d2_loss64(q, qt, act, ret, term, isw, batch, 0, 1, n, n_act, dueling, gamma_n, 0.0, 0.9)
            for b in range(batch):                  # the target written out directly, row by row
                r0, rn = b * U, b * U + n
                merge = lambda row: (row[:n_act].astype(np.float64) if not dueling else                 # noqa: E731
                                     float(row[n_act]) + (row[:n_act].astype(np.float64) -
                                                          sum(float(v) for v in row[:n_act]) / n_act))
                a_star = int(np.argmax(merge(q[rn])))
                y = float(ret[r0]) + (0.0 if term[r0] else gamma_n * merge(qt[rn])[a_star])
                d = y - merge(q[r0])[act[r0]]
                assert out["d"][b, 0] == d
                assert out["loss_rows"][b] == np.float32(float(isw[b]) / batch * (0.5 * (d * d)))
                assert out["priorities"][b] == np.float32(0.9 * abs(d) + (1.0 - 0.9) * abs(d))
                assert out["td_abs"][b, 0] == np.float32(abs(d))


def test_priorities_of_a_constant_error_are_that_constant():
    """q == 0 everywhere, returns == c, no rescaling, every row terminal: d == c in every train step."""
    batch, burn_in, train_len, n, n_act, stride = 3, 2, 5, 2, 4, 4
    rows = batch * (burn_in + train_len + n)
    zeros = np.zeros((rows, stride), np.float32)
    for c in (0.25, 3.0, 1e4):
        for eta in (0.0, 0.3, 0.9, 1.0):
            out = rr.r2d2_loss64(zeros, zeros, np.zeros(rows, np.uint8), np.full(rows, c, np.float32),
                                 np.ones(rows, np.uint8), None, batch, burn_in, train_len, n, n_act, False, 0.99, 0.0, eta)
            assert (out["td_abs"] == np.float32(c)).all()
            np.testing.assert_allclose(out["priorities"], c, rtol=1e-15 * 8, atol=0)
            assert (out["priorities"] == np.float32(c)).all()


def test_loss_cases_contain_their_plants():
    for shape in [(1, 0, 1, 1, 1, 4, 0), (3, 2, 5, 3, 6, 8, 1), (5, 40, 80, 5, 4, 8, 0)]:
        batch, burn_in, train_len, n, n_act, stride, duel = shape
        c = rr.loss_case(1, *shape, gamma_n=0.99)
        out = rr.r2d2_loss64(c["q"], c["q_tgt"], c["actions"], c["returns"], c["terminals"], c["is_weights"], batch,
                             burn_in, train_len, n, n_act, bool(duel), 0.99, 1e-3, 0.9)
        assert c["terminals"][burn_in] and c["terminals"][burn_in + train_len - 1]
        assert (out["x"] == 0).any() and (out["z"] == 0).any() and (c["actions"] >= n_act).any()
        assert (c["q"][:, n_act + duel:] == rr.PAD).all()


# ---- which slots can be sampled -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,S,U,n_stack,n", [(16, 2, 5, 2, 1), (24, 4, 9, 4, 2), (40, 8, 8, 4, 3)])
def test_sampleable_slots_equal_brute_force_for_every_cursor_over_two_laps(size, S, U, n_stack, n):
    from accel_rl_amd.algos.dqn.replay_buffers.sequence import sampleable_slots, slot_zeros
    zf, zb = slot_zeros(S, U, n_stack)
    seen_some = False
    for written in range(0, 2 * size + 1, S):                # the cursor moves in multiples of the stride
        cursor, full = written % size, written >= size
        got = sampleable_slots(cursor, full, size, S, U, n_stack)
        want = rr.brute_sampleable(written, size, S, U, n_stack, n)
        np.testing.assert_array_equal(got, want, err_msg="written %d" % written)
        seen_some |= bool(want.any())
        if full:                # the same set in the sum tree's terms: zf slots off from the cursor on, zb behind it
            k = np.arange(size // S)
            ahead = (k - cursor // S) % (size // S)
            np.testing.assert_array_equal(got, (ahead >= zf) & (ahead < size // S - zb))
    assert seen_some
    with pytest.raises(ValueError):                           # a cursor off the stride, a ring that is no multiple of it
        sampleable_slots(S + 1, True, size, S, U, n_stack) if S > 1 else sampleable_slots(0, True, 17, 2, U, n_stack)
    with pytest.raises(ValueError):
        sampleable_slots(0, True, size + 1, S, U, n_stack)


# ---- refusals ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


def _f(n):
    return (ctypes.c_float * n)()            # host memory: a refused call reads none of it


def _u8(n):
    return (ctypes.c_uint8 * n)()


def _i32(n):
    return (ctypes.c_int32 * n)()


P = ctypes.addressof


def test_r2d2_loss_refusals_need_no_device(lib):
    batch, burn_in, train_len, n, n_act, stride = 2, 1, 3, 2, 5, 8
    rows = batch * (burn_in + train_len + n)
    q, qt, dq, ret, isw = _f(rows * stride + 8), _f(rows * stride), _f(rows * stride + 8), _f(rows), _f(batch)
    act, term = _u8(rows), _u8(rows)
    td, lr, pr = _f(batch * train_len), _f(batch), _f(batch)

    def loss(q_=P(q), qt_=P(qt), act_=P(act), ret_=P(ret), term_=P(term), isw_=P(isw), b=batch, bi=burn_in, tl=train_len,
             n_=n, a=n_act, s=stride, duel=0, g=0.99, eps=1e-3, eta=0.9, dq_=P(dq), td_=P(td), lr_=P(lr), pr_=P(pr)):
        return lib.arl_r2d2_loss(q_, qt_, act_, ret_, term_, isw_, b, bi, tl, n_, a, s, duel, g, eps, eta, dq_, td_, lr_,
                                 pr_, None)

    for k in ("q_", "qt_", "act_", "ret_", "term_", "dq_", "td_", "lr_", "pr_"):
        assert loss(**{k: None}) == E_ARG and b"null" in lib.arl_last_error(), k
    for kw in (dict(g=NAN), dict(g=INF), dict(eps=NAN), dict(eta=INF)):
        assert loss(**kw) == E_ARG, kw
    for kw in (dict(b=0), dict(tl=0), dict(tl=1025), dict(bi=-1), dict(bi=1025), dict(n_=0), dict(n_=17), dict(a=0),
               dict(a=256, s=256), dict(s=10), dict(a=8, s=8, duel=1), dict(a=6, s=4),
               dict(b=2 ** 31 - 1, bi=1024, tl=1024, n_=16)):
        assert loss(**kw) == E_RANGE, kw
    assert loss(dq_=P(dq) + 4) == E_ALIGN and loss(q_=P(q) + 2) == E_ALIGN and loss(pr_=P(pr) + 1) == E_ALIGN
    assert all(v == 0 for v in dq) and all(v == 0 for v in td) and all(v == 0 for v in lr) and all(v == 0 for v in pr)


def test_seq_entry_point_refusals_need_no_device(lib):
    n_env, horizon, size, S, hidden, batch, U = 2, 4, 8, 2, 8, 3, 5
    st_in, st_store, st_out = _f(n_env * horizon * hidden + 4), _f(n_env * (size // S) * hidden + 4), _f(batch * hidden + 4)
    resets, ring, r_out = _u8(n_env * horizon), _u8(n_env * size), _u8(batch * U)
    env, slot, env_rows, step_rows = _i32(batch), _i32(batch), _i32(batch * U), _i32(batch * U)
    arr = lambda *ptrs: (ctypes.c_void_p * 2)(*ptrs)                                    # noqa: E731

    def store(sin=arr(P(st_in)), ns=1, h=hidden, rs=P(resets), ne=n_env, t=horizon, sz=size, s=S, idx=0,
              sst=arr(P(st_store)), rg=P(ring)):
        return lib.arl_seq_store(sin, ns, h, rs, ne, t, sz, s, idx, sst, rg, None)

    for kw in (dict(rs=None), dict(rg=None), dict(sin=None), dict(sst=None), dict(sin=arr(None)), dict(sst=arr(None))):
        assert store(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(ns=3), dict(ns=-1), dict(h=6), dict(h=1028), dict(h=0), dict(ne=0), dict(t=0), dict(sz=0), dict(s=0),
               dict(t=3), dict(sz=9), dict(t=16, sz=8), dict(idx=-1), dict(idx=8)):
        assert store(**kw) == E_RANGE, kw
    assert store(sin=arr(P(st_in) + 4)) == E_ALIGN and store(sst=arr(P(st_store) + 8)) == E_ALIGN
    assert store(ns=0, h=0, sin=None, sst=None, ne=0) == E_RANGE            # (no state tensors is a valid call shape)
    assert all(v == 0 for v in ring) and all(v == 0 for v in st_store)

    def prepare(e=P(env), sl=P(slot), b=batch, u=U, sz=size, s=S, sst=arr(P(st_store)), ns=1, h=hidden, rg=P(ring),
                er=P(env_rows), sr=P(step_rows), so=arr(P(st_out)), ro=P(r_out)):
        return lib.arl_seq_prepare(e, sl, b, u, sz, s, sst, ns, h, rg, er, sr, so, ro, None)

    for kw in (dict(e=None), dict(sl=None), dict(rg=None), dict(er=None), dict(sr=None), dict(ro=None), dict(sst=None),
               dict(so=arr(None))):
        assert prepare(**kw) == E_ARG and b"null" in lib.arl_last_error(), kw
    for kw in (dict(b=0), dict(u=0), dict(sz=0), dict(s=0), dict(sz=9), dict(b=2 ** 16, u=2 ** 15), dict(ns=3), dict(h=2),
               dict(h=2048)):
        assert prepare(**kw) == E_RANGE, kw
    assert prepare(so=arr(P(st_out) + 4)) == E_ALIGN
    assert all(v == 0 for v in env_rows) and all(v == 0 for v in step_rows) and all(v == 0 for v in st_out)


class _Space(object):
    def __init__(self, shape):
        self.shape = shape


class _Spec(object):
    observation_space = _Space((4, 8, 8))


def _buffer_args(**kw):
    args = dict(env_spec=_Spec(), size=2 * 64, reward_horizon=2, sampling_horizon=8, n_environments=2, discount=0.99,
                burn_in=4, train_len=4, seq_stride=4, state_keys=("hprev_0", "cprev_0"), hidden=64, device="cpu")
    args.update(kw)
    return args


@pytest.mark.parametrize("kw,match", [
    (dict(seq_stride=3), "sampling_horizon"),                        # sampling_horizon % S != 0
    (dict(size=2 * 8), "do not fit"),                                # a ring of 8 steps: U = 10 > 8 - 3
    (dict(size=2 * 16, burn_in=8), "do not fit"),                    # a ring of 16 steps: U = 14 > 16 - 3
    (dict(n_step=3), "reward_horizon"),                              # reward_horizon != n
    (dict(hidden=6), "state tensors"),
    (dict(state_keys=()), "state tensors"),
    (dict(size=2 * 16), "sum tree"),            # 4 slots per env: 1 ahead + 2 behind the cursor off, 2 appended per batch
    (dict(train_len=0), "train_len"),
])
def test_sequence_replay_refuses_before_touching_the_device(kw, match):
    """device="cpu": a constructor that got as far as the library or a device tensor would fail differently (there is no
    CPU path).  (env_replay_size % S != 0 cannot be reached through this constructor: the ring is rounded up to whole
    sampler batches, and sampling_horizon % S == 0 is checked first.)"""
    from accel_rl_amd.algos.dqn.replay_buffers.sequence import SequenceReplayBuffer
    with pytest.raises(ValueError, match=match):
        SequenceReplayBuffer(**_buffer_args(**kw))


def _spec(**kw):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    return dict(dict(cnn_specs[0], hidden_sizes=[64]), **kw)


def test_dqn_still_refuses_a_recurrent_policy_and_names_r2d2():
    from accel_rl_amd.algos.dqn.dqn import DQN
    from accel_rl_amd.policies.dqn.atari_r2d2_policy import AtariR2d2Policy
    policy = AtariR2d2Policy(**_spec())
    assert policy.recurrent and policy.state_info_keys == ["hprev_0", "cprev_0"]
    with pytest.raises(NotImplementedError, match="R2D2"):
        DQN().initialize(policy, None, 64, 8, True)


def test_r2d2_refuses_a_feed_forward_policy_and_bad_arguments():
    from accel_rl_amd.algos.dqn.r2d2 import R2D2
    from accel_rl_amd.policies.atari_lstm_policy import AtariLstmPolicy
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    with pytest.raises(NotImplementedError, match="recurrent Q policy.*AtariDqnPolicy"):
        R2D2().initialize(AtariDqnPolicy(**_spec()), None, 64, 8, True)
    with pytest.raises(NotImplementedError, match="r2d2_loss_and_grads"):           # recurrent, but no Q policy
        R2D2().initialize(AtariLstmPolicy(**_spec()), None, 64, 8, True)
    from accel_rl_amd.policies.dqn.atari_r2d2_policy import AtariR2d2Policy
    policy = AtariR2d2Policy(**_spec())
    with pytest.raises(NotImplementedError, match="mid_batch_reset"):
        R2D2().initialize(policy, None, 64, 8, False)
    with pytest.raises(ValueError, match="multiple of batch_size \\* train_len"):
        R2D2(batch_size=4, train_len=5, training_intensity=1).initialize(policy, None, 64, 8, True)
    for kw in (dict(burn_in=-1), dict(train_len=0), dict(seq_stride=0), dict(reward_horizon=0), dict(priority_eta=1.5),
               dict(priority_eta=NAN), dict(rescale_eps=0.0), dict(rescale_eps=NAN), dict(train_len=2.5)):
        with pytest.raises(ValueError):
            R2D2(**kw)
    assert R2D2(value_rescale=False, rescale_eps=0.0).value_rescale is False


def test_defaults_table():
    from accel_rl_amd.algos.dqn.r2d2 import R2D2
    from accel_rl_amd.optimizers.dqn import DqnOptimizer
    algo = R2D2()
    assert (algo.burn_in, algo.train_len, algo.seq_stride, algo.reward_horizon, algo.batch_size) == (40, 80, 40, 5, 64)
    assert (algo.discount, algo.value_rescale, algo.rescale_eps, algo.priority_eta) == (0.997, True, 1e-3, 0.9)
    assert algo.prioritized_replay and algo.double_dqn and algo.dueling_dqn and algo.delta_clip is None
    assert algo._priority_args == dict(alpha=0.9, beta_initial=0.6, default_priority=1.)
    assert (algo._priority_beta_initial, algo._priority_beta_final) == (0.6, 0.6)
    opt = algo.optimizer
    assert type(opt) is DqnOptimizer and opt._learning_rate == 1e-4 and opt._update_method.name == "adam"
    assert opt._update_args["epsilon"] == 1e-3 and opt._grad_norm_clip is None
    assert algo.opt_info_keys == ["Priority", "Loss"]
