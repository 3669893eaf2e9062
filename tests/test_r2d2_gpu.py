"""R2D2 on the GPU: arl_r2d2_loss against its float64 restatement (tests/r2d2_ref.py) within one float32 ulp,
arl_seq_store / arl_seq_prepare against NumPy bit for bit, SequenceReplayBuffer against the host predicate, the frame
replay's own gather and the appended rows, AtariR2d2Policy's losses and gradients against float64 autograd at the bars of
tests/test_recurrent_ppo_gpu.py, its serving calls, and R2D2 end to end through the sampler -- replayed from the captured
graphs against an eager run, bit for bit."""
import numpy as np
import pytest
import torch

import r2d2_ref as rr
from test_recurrent_ppo_gpu import GRAD_ATOL, GRAD_RTOL, _flat_grads, _ref_features, _ref_params, _ref_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- arl_r2d2_loss ------------------------------------------------------------------------------------------------------

SHAPES = [(1, 0, 1, 1, 1, 4, 0), (3, 2, 5, 3, 6, 8, 1), (2, 0, 65, 1, 18, 20, 1), (5, 40, 80, 5, 4, 8, 0),
          (33, 1, 3, 16, 18, 32, 0)]
NOT_BIT_EQUAL = dict(elements=0, differing=0)


@pytest.mark.parametrize("shape", SHAPES)
def test_loss_kernel_equals_the_float64_restatement_within_one_ulp(L, shape):
    batch, burn_in, train_len, n, n_act, stride, duel = shape
    U = burn_in + train_len + n
    gamma_n = 0.997 ** n
    c = rr.loss_case(10 * batch + n_act, *shape, gamma_n=gamma_n)
    q, qt = c["q"], c["q_tgt"]
    # the plants are there
    first, last = burn_in, burn_in + train_len - 1
    assert c["terminals"][first] and c["terminals"][last] and (c["actions"] >= n_act).any()
    assert (q[:, n_act + duel:] == rr.PAD).all() and (qt[:, n_act + duel:] == rr.PAD).all()
    tie_row = rr.merged64(q[first + n:first + n + 1], n_act, bool(duel))[0]
    assert (q[first + n, :n_act] == np.round(q[first + n, :n_act])).all()               # integer-valued
    if n_act > 1:
        assert tie_row[0] == tie_row[n_act - 1] == tie_row.max() and (tie_row == tie_row.max()).sum() >= 2
    if batch >= 2:
        assert np.abs(q[U:2 * U, :n_act]).max() > 5e3
    dc = {k: _dev(v) for k, v in c.items()}
    for eps in (1e-3, 0.0):
        for weighted in (True, False):
            want = rr.r2d2_loss64(q, qt, c["actions"], c["returns"], c["terminals"], c["is_weights"] if weighted else None,
                                  batch, burn_in, train_len, n, n_act, bool(duel), gamma_n, eps, 0.9)
            assert (want["x"] == 0).any() and (want["z"] == 0).any()
            assert want["a_star"][0, 0] == 0                                            # the tie goes to the first action
            dq = torch.full((batch * U, stride), NAN, device=DEV)
            td = torch.full((batch, train_len), NAN, device=DEV)
            pack = torch.full((2, batch), NAN, device=DEV)
            L.r2d2_loss(dc["q"], dc["q_tgt"], dc["actions"], dc["returns"], dc["terminals"],
                        dc["is_weights"] if weighted else None, batch, burn_in, train_len, n, n_act, gamma_n, eps, 0.9, dq,
                        td, pack[0], pack[1], dueling=bool(duel))
            got = dict(dq=_host(dq), td_abs=_host(td), loss_rows=_host(pack[0]), priorities=_host(pack[1]))
            what = "%s eps %g weights %s" % (shape, eps, weighted)
            for key in ("dq", "td_abs", "loss_rows", "priorities"):
                assert np.isfinite(got[key]).all(), (what, key)
                ok = rr.within_one_ulp(got[key], want[key])
                differing = int((_bits(got[key]) != _bits(want[key])).sum())
                NOT_BIT_EQUAL["elements"] += got[key].size
                NOT_BIT_EQUAL["differing"] += differing
                print("%s %s: %d of %d elements not bit-equal, %d outside 1 ulp (bound: 0)" % (
                    what, key, differing, got[key].size, int((~ok).sum())))
                assert ok.all(), (what, key)
            # exact +0 outside the train window, in the padding columns and (without dueling) in every other action
            zero = np.ones((batch, U, stride), bool)
            act = np.minimum(c["actions"].astype(np.int64), n_act - 1).reshape(batch, U)
            for b in range(batch):
                for t in range(burn_in, burn_in + train_len):
                    if duel:
                        zero[b, t, :n_act + 1] = False
                    else:
                        zero[b, t, act[b, t]] = False
            assert (_bits(got["dq"]).reshape(batch, U, stride)[zero] == 0).all(), what
            assert (got["dq"].reshape(batch, U, stride)[~zero] != 0).any()
            # the priorities are the mix of the returned |d|'s maximum and mean
            t64 = got["td_abs"].astype(np.float64)
            s, mx = np.zeros(batch), np.zeros(batch)
            for t in range(train_len):
                s = s + t64[:, t]
                mx = np.maximum(mx, t64[:, t])
            again = (0.9 * mx + (1.0 - 0.9) * (s / float(train_len))).astype(np.float32)
            assert rr.within_one_ulp(got["priorities"], again).all(), what
    print("so far: %(differing)d of %(elements)d output elements not bit-equal to the restatement" % NOT_BIT_EQUAL)


def test_loss_kernel_is_deterministic_and_leaves_its_inputs_alone(L):
    shape = (5, 40, 80, 5, 4, 8, 0)
    batch, burn_in, train_len, n, n_act, stride, duel = shape
    c = rr.loss_case(3, *shape, gamma_n=0.98)
    dc = {k: _dev(v) for k, v in c.items()}
    outs = []
    for _ in range(2):
        dq = torch.full((batch * (burn_in + train_len + n), stride), NAN, device=DEV)
        td = torch.full((batch, train_len), NAN, device=DEV)
        pack = torch.full((2, batch), NAN, device=DEV)
        L.r2d2_loss(dc["q"], dc["q_tgt"], dc["actions"], dc["returns"], dc["terminals"], dc["is_weights"], batch, burn_in,
                    train_len, n, n_act, 0.98, 1e-3, 0.9, dq, td, pack[0], pack[1])
        outs.append((dq, td, pack))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    for k, v in c.items():
        np.testing.assert_array_equal(_host(dc[k]), v)


# ---- arl_seq_store / arl_seq_prepare ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_env", [1, 3])
@pytest.mark.parametrize("size,S", [(16, 2), (16, 8), (40, 2), (40, 8)])
def test_seq_store_and_prepare_move_bits(L, n_env, size, S):
    horizon, U = 8, 11
    for hidden in (4, 64):
        for n_state in (1, 2):
            rs = np.random.RandomState(size + S + hidden + n_state)
            model = rr.SeqModel(n_env, size, S, hidden, n_state)
            stores = [_dev(m.copy()) for m in model.stores]
            ring = _dev(model.ring.copy())
            idx = 0
            for k in range(2 * size // horizon + 1):                                     # two laps and one more batch
                states = [rs.randn(n_env * horizon, hidden).astype(np.float32) for _ in range(n_state)]
                for st in states:                                                        # -0.0, a denormal, inf: bits, not values
                    st.reshape(-1)[:3] = np.array([-0.0, 1e-42, np.inf], np.float32)
                resets = (rs.rand(n_env * horizon) < 0.3).astype(np.uint8) * (1 + k)
                model.store(states, resets, horizon, idx)
                L.seq_store([_dev(s) for s in states], _dev(resets), n_env, horizon, size, S, idx, stores, ring)
                idx = (idx + horizon) % size
                for got, want in zip(stores, model.stores):
                    np.testing.assert_array_equal(_bits(_host(got)), _bits(want))
                np.testing.assert_array_equal(_host(ring), model.ring)
            # sequences: every slot of every env (those near the end cross the wrap), with repeats
            n_slots = size // S
            env = np.concatenate([np.repeat(np.arange(n_env), n_slots), [n_env - 1, n_env - 1, 0]]).astype(np.int32)
            slot = np.concatenate([np.tile(np.arange(n_slots), n_env), [n_slots - 1, n_slots - 1, 0]]).astype(np.int32)
            assert ((slot.astype(np.int64) * S + U) > size).any()
            b = len(env)
            env_rows = torch.full((b * U,), -7, dtype=torch.int32, device=DEV)
            step_rows = torch.full((b * U,), -7, dtype=torch.int32, device=DEV)
            r_out = torch.full((b * U,), 99, dtype=torch.uint8, device=DEV)
            outs = [torch.full((b, hidden), NAN, device=DEV) for _ in range(n_state)]
            L.seq_prepare(_dev(env), _dev(slot), U, size, S, stores, ring, env_rows, step_rows, outs, r_out)
            w_env, w_step, w_states, w_resets = model.prepare(env, slot, U)
            np.testing.assert_array_equal(_host(env_rows), w_env)
            np.testing.assert_array_equal(_host(step_rows), w_step)
            np.testing.assert_array_equal(_host(r_out), w_resets)
            for got, want in zip(outs, w_states):
                np.testing.assert_array_equal(_bits(_host(got)), _bits(want))


def test_seq_wrappers_check_their_shapes(L):
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)                # noqa: E731
    with pytest.raises(ValueError):
        L.seq_store([z(16, 8)], z(16, dt=torch.uint8), 2, 8, 16, 4, 0, [z(2, 4, 8), z(2, 4, 8)], z(2, 16, dt=torch.uint8))
    with pytest.raises(ValueError):
        L.seq_store([z(16, 8)], z(15, dt=torch.uint8), 2, 8, 16, 4, 0, [z(2, 4, 8)], z(2, 16, dt=torch.uint8))
    with pytest.raises(RuntimeError, match="code -2"):                                   # horizon % seq_stride != 0
        L.seq_store([z(16, 8)], z(16, dt=torch.uint8), 2, 8, 16, 3, 0, [z(2, 5, 8)], z(2, 16, dt=torch.uint8))
    i32 = lambda k: z(k, dt=torch.int32)                                                 # noqa: E731
    with pytest.raises(ValueError):
        L.seq_prepare(i32(3), i32(3), 5, 16, 4, [z(2, 4, 8)], z(2, 16, dt=torch.uint8), i32(15), i32(14), [z(3, 8)],
                      z(15, dt=torch.uint8))
    with pytest.raises(TypeError):
        L.seq_prepare(i32(3).long(), i32(3), 5, 16, 4, [z(2, 4, 8)], z(2, 16, dt=torch.uint8), i32(15), i32(15),
                      [z(3, 8)], z(15, dt=torch.uint8))


# ---- SequenceReplayBuffer --------------------------------------------------------------------------------------------------

def _small_spec(n_act=6, shape=(4, 16, 16)):
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    return EnvSpec(UintBox(shape), Discrete(n_act))


def _sampler_batch(rs, n_env, horizon, hidden, keys, shape=(4, 16, 16)):
    rows = n_env * horizon
    dones = rs.rand(rows) < 0.15
    need_reset = dones & (rs.rand(rows) < 0.6)                   # episodic lives: a done without a reset
    return dict(observations=_dev(rs.randint(0, 256, size=(rows,) + shape, dtype=np.uint8)),
                actions=_dev(rs.randint(0, 6, size=rows).astype(np.uint8)),
                rewards=_dev(rs.randn(rows).astype(np.float32)), dones=_dev(dones),
                env_infos=dict(need_reset=_dev(need_reset.astype(np.uint8))),
                agent_infos={k: _dev(rs.randn(rows, hidden).astype(np.float32)) for k in keys})


def test_sequence_replay_against_the_predicate_the_frame_replay_and_the_appended_rows():
    from accel_rl_amd.algos.dqn.replay_buffers.frame import FrameReplayBuffer
    from accel_rl_amd.algos.dqn.replay_buffers.sequence import SequenceReplayBuffer, sampleable_slots
    n_env, horizon, S, hidden, keys = 2, 8, 4, 8, ("hprev_0", "cprev_0")
    common = dict(env_spec=_small_spec(), size=n_env * 32, reward_horizon=2, sampling_horizon=horizon,
                  n_environments=n_env, discount=0.99, device=DEV)
    buf = SequenceReplayBuffer(burn_in=2, train_len=3, seq_stride=S, state_keys=keys, hidden=hidden, alpha=0.5, **common)
    plain = FrameReplayBuffer(**common)
    size, U = buf.env_replay_size, buf.seq_len
    assert (size, U, buf.n_slots) == (32, 7, 8)
    rs = np.random.RandomState(4)
    state_log = np.full((2, n_env, size, hidden), np.nan, np.float32)
    reset_log = np.zeros((n_env, size), np.uint8)
    tree = buf.priority_tree
    for k in range(6):                                           # 48 steps: one lap and a half
        idx = buf.idx
        data = _sampler_batch(rs, n_env, horizon, hidden, keys)
        buf.append_data(data)
        plain.append_data(data)
        pos = (idx + np.arange(horizon)) % size
        for i, key in enumerate(keys):
            state_log[i][:, pos] = _host(data["agent_infos"][key]).reshape(n_env, horizon, hidden)
        reset_log[:, pos] = _host(data["env_infos"]["need_reset"]).reshape(n_env, horizon)
        want = sampleable_slots(buf.idx, (k + 1) * horizon >= size, size, S, U, 4)
        np.testing.assert_array_equal(buf.sampleable(), want)
        leaves = _host(tree.tree)[tree.t_l_shift:tree.t_l_shift + n_env * buf.n_slots].reshape(n_env, buf.n_slots)
        assert np.isfinite(leaves).all() and (leaves >= 0).all()
        np.testing.assert_array_equal(leaves != 0, np.tile(want, (n_env, 1)), err_msg="after %d appends" % (k + 1))
        if not want.any():
            continue
        slots = np.flatnonzero(want)
        env = np.repeat(np.arange(n_env), len(slots)).astype(np.int32)
        slot = np.tile(slots, n_env).astype(np.int32)
        obs, act, ret, term, resets, h0, c0 = buf.extract_sequences(env, slot)
        env_rows = np.repeat(env, U)
        step_rows = ((slot.astype(np.int64)[:, None] * S + np.arange(U)[None]) % size).reshape(-1).astype(np.int32)
        w_obs, _, w_act, w_ret, w_term = plain.extract_batch(env_rows, step_rows)
        for got, ref in ((obs, w_obs), (act, w_act), (term, w_term)):
            assert torch.equal(got, ref)
        np.testing.assert_array_equal(_bits(_host(ret)), _bits(_host(w_ret)))
        np.testing.assert_array_equal(_host(resets), reset_log[env_rows, step_rows])
        for i, got in enumerate((h0, c0)):
            np.testing.assert_array_equal(_bits(_host(got)), _bits(state_log[i][env, slot * S]))
    assert buf._buffer_full
    # sampling and priorities: alpha = 0.5 and squared priorities make the powers exact
    np.random.seed(11)
    batch = 4
    out = buf.sample_batch(batch)
    assert len(out) == 8 and out[0].shape == (batch * U, 4, 16, 16) and out[-1].shape == (batch,)
    assert out[-1].dtype == torch.float32 and float(out[-1].max()) == 1.0
    idxs = _host(tree.last_tree_idxs).astype(np.int64)
    leaf = idxs - tree.t_l_shift
    assert len(set(idxs)) == batch and buf.sampleable()[leaf % buf.n_slots].all()
    pri = np.array([4.0, 9.0, 0.25, 16.0], np.float32)
    buf.update_batch_priorities(_dev(pri))
    np.testing.assert_array_equal(_host(tree.tree)[idxs], np.sqrt(pri.astype(np.float64)))
    total = float(_host(tree.tree)[0])
    assert np.isfinite(total) and abs(total - _host(tree.tree)[tree.t_l_shift:].sum()) < 1e-9
    # uniform mode draws from the same set
    uni = SequenceReplayBuffer(burn_in=2, train_len=3, seq_stride=S, state_keys=keys, hidden=hidden, prioritized=False,
                               **common)
    with pytest.raises(RuntimeError, match="no sequence"):
        uni.sample_batch(2)
    for k in range(3):
        uni.append_data(_sampler_batch(rs, n_env, horizon, hidden, keys))
    e, s = uni.sample_idxs(64)
    assert uni.sampleable()[s].all() and set(e) == {0, 1} and not hasattr(uni, "priority_tree")
    assert float(uni.sample_batch(3)[-1].min()) == 1.0


# ---- AtariR2d2Policy -------------------------------------------------------------------------------------------------------

def _make_policy(dueling, n_act=6, eps=0.0):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_r2d2_policy import AtariR2d2Policy
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    from accel_rl_amd.util.seed import set_seed
    set_seed(8)
    spec = dict(cnn_specs[0], hidden_sizes=[64])
    policy = AtariR2d2Policy(epsilon=eps, dueling=dueling, **spec)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(n_act)), device=DEV)
    return policy, spec


def _ref_q(rp, spec, obs, init, resets, nb, u_len, dueling, n_act, detach_at=None):
    """float64 merged action values [nb * u_len, A] of the rows [sequence][time]: torch conv, an LSTM written out (the
    reference's layout: test_recurrent_ppo_gpu._ref_step), the state zeroed after flagged rows and -- detach_at -- detached
    before that step."""
    xf, k = _ref_features(rp, spec, obs.double() * np.float64(np.float32(1. / 255)))
    xf = xf.view(nb, u_len, -1)
    keep = (resets == 0).double().view(nb, u_len, 1)
    state, hs = [s.double() for s in init], []
    for t in range(u_len):
        if t > 0:
            state = [s * keep[:, t - 1] for s in state]
        if detach_at is not None and t == detach_at:
            state = [s.detach() for s in state]
        state, kp = _ref_step("lstm", rp, k, xf[:, t], state)
        hs.append(state[0])
    h_all = torch.stack(hs, dim=1).reshape(nb * u_len, -1)
    adv = h_all @ rp[kp] + rp[kp + 1]
    if not dueling:
        return adv
    val = h_all @ rp[kp + 2] + rp[kp + 3]
    return val + (adv - adv.mean(dim=1, keepdim=True))


def _h(z, eps):
    return torch.sign(z) * (torch.sqrt(torch.abs(z) + 1.0) - 1.0) + eps * z


def _h_inv(x, eps):
    u = (torch.sqrt(1.0 + 4.0 * eps * (torch.abs(x) + 1.0 + eps)) - 1.0) / (2.0 * eps)
    return torch.sign(x) * (u * u - 1.0)


@pytest.mark.parametrize("burn_in", [2, 0])
@pytest.mark.parametrize("dueling", [True, False])
def test_policy_losses_and_gradients_match_float64_autograd(dueling, burn_in):
    nb, train_len, n, n_act, eps, eta = 3, 3, 2, 6, 1e-3, 0.9
    u_len = burn_in + train_len + n
    rows = nb * u_len
    policy, spec = _make_policy(dueling)
    rs = np.random.RandomState(30 + burn_in)
    policy.flat_target.copy_(policy.flat_params * 0.9)           # a target network that differs
    obs = _dev(rs.randint(0, 256, size=(rows, 4, 104, 80), dtype=np.uint8))
    act = _dev(rs.randint(0, n_act, size=rows).astype(np.uint8))
    ret = _dev((rs.randn(rows) * 0.05).astype(np.float32))
    term = _dev((rs.rand(rows) < 0.2).astype(np.uint8))
    isw = _dev((rs.rand(nb) + 0.2).astype(np.float32))
    init = [_dev((rs.randn(nb, 64) * 0.3).astype(np.float32)) for _ in range(2)]
    m = np.zeros((nb, u_len), np.uint8)
    if burn_in:
        m[0, 0] = 1                                              # inside the burn-in
    m[1, burn_in + 1] = 1                                        # inside the train window
    m[2, burn_in + train_len - 1] = 1                            # at the last train row
    resets = _dev(m.reshape(-1))
    gamma_n = 0.997 ** n
    target_before = policy.flat_target.clone()
    loss_rows, prio = policy.r2d2_loss_and_grads(obs, act, ret, term, resets, init, isw, gamma_n, burn_in, train_len, n,
                                                 rescale_eps=eps, eta=eta)
    assert prio.data_ptr() == loss_rows.data_ptr() + 4 * nb      # adjacent: the statistics ring packs them
    got = policy.bucket_to_reference(policy.flat_grads)
    td = policy.last_td_abs.clone()
    # float64 autograd
    rp, rt = _ref_params(policy), _ref_params(policy, policy.bucket_to_reference(policy.flat_target))
    q = _ref_q(rp, spec, obs, init, resets, nb, u_len, dueling, n_act, detach_at=burn_in if burn_in else None)
    with torch.no_grad():
        q_t = _ref_q(rt, spec, obs, init, resets, nb, u_len, dueling, n_act)
    t_rows = (torch.arange(nb, device=DEV)[:, None] * u_len + burn_in + torch.arange(train_len, device=DEV)[None]).reshape(-1)
    a_star = q.detach()[t_rows + n].argmax(dim=1)
    x = q_t[t_rows + n, a_star]
    z = ret.double()[t_rows] + torch.where(term[t_rows] != 0, torch.zeros_like(x), gamma_n * _h_inv(x, eps))
    d = (_h(z, eps) - q[t_rows, act[t_rows].long()]).view(nb, train_len)
    want_rows = isw.double() / (nb * train_len) * (0.5 * d * d).sum(dim=1)
    want_prio = eta * d.abs().max(dim=1).values + (1 - eta) * d.abs().mean(dim=1)
    want = _flat_grads(want_rows.sum(), rp)
    scale = np.abs(want).max()
    print("dueling %s burn_in %d: loss %.6g want %.6g; max |d grad| %.3g of %.3g (bars rtol %g, atol %g x scale)" % (
        dueling, burn_in, loss_rows.sum().item(), want_rows.sum().item(), np.abs(got - want).max(), scale, GRAD_RTOL,
        GRAD_ATOL))
    assert np.isfinite(got).all() and scale > 0
    assert torch.allclose(loss_rows.double(), want_rows.detach(), rtol=1e-4, atol=1e-6)
    assert torch.allclose(prio.double(), want_prio.detach(), rtol=1e-4, atol=1e-6)
    assert torch.allclose(td.double(), d.abs().detach(), rtol=1e-4, atol=1e-6)
    assert np.allclose(got, want, rtol=GRAD_RTOL, atol=GRAD_ATOL * max(scale, 1e-3)), (np.abs(got - want).max(), scale)
    assert torch.equal(policy.flat_target, target_before)        # the target network is read, never written
    # discrimination: the gradient that ignores the resets, or (with a burn-in) flows through it, misses the bars
    others = [_ref_q(rp, spec, obs, init, torch.zeros_like(resets), nb, u_len, dueling, n_act,
                     detach_at=burn_in if burn_in else None)]
    if burn_in:
        others.append(_ref_q(rp, spec, obs, init, resets, nb, u_len, dueling, n_act))
    for q_o in others:
        d_o = (_h(z.detach(), eps) - q_o[t_rows, act[t_rows].long()]).view(nb, train_len)
        wrong = _flat_grads((isw.double() / (nb * train_len) * (0.5 * d_o * d_o).sum(dim=1)).sum(), rp)
        assert not np.allclose(wrong, want, rtol=GRAD_RTOL, atol=GRAD_ATOL * max(scale, 1e-3))


@pytest.mark.parametrize("dueling", [True, False])
def test_serving_advances_the_state_and_obeys_the_override(dueling):
    n_act, b = 6, 8
    policy, spec = _make_policy(dueling)
    rs = np.random.RandomState(2)
    policy.reset(n_batch=b)
    for s in policy._state:
        s.copy_(_dev((rs.randn(b, 64) * 0.3).astype(np.float32)))
    before = [s.clone() for s in policy._state]
    obs = _dev(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8))
    rp = _ref_params(policy)
    with torch.no_grad():
        q64 = _ref_q(rp, spec, obs, before, torch.zeros(b, dtype=torch.uint8, device=DEV), b, 1, dueling, n_act)
    assert torch.allclose(policy.q_values(obs).double(), q64, rtol=1e-4, atol=1e-6)
    greedy = policy.greedy_actions(obs)
    for s, v in zip(policy._state, before):
        assert torch.equal(s, v)                                 # neither call advances the state
    policy.set_step(0)
    onehot, value, h_prev, c_prev = policy.act_step(obs)         # no override table yet: greedy
    assert torch.equal(h_prev, before[0]) and torch.equal(c_prev, before[1]) and not value.any()
    assert (onehot.sum(dim=1) == 1).all() and torch.equal(onehot.argmax(dim=1).to(torch.uint8), greedy)
    chosen = q64[torch.arange(b), onehot.argmax(dim=1)]
    bar = 1e-4 * max(1.0, float(q64.abs().max()))
    print("dueling %s: worst (max q - chosen q) %.3g, bar %.3g" % (dueling, float((q64.max(dim=1).values - chosen).max()), bar))
    assert ((q64.max(dim=1).values - chosen) <= bar).all()       # every row
    with torch.no_grad():
        xf, k = _ref_features(rp, spec, obs.double() * np.float64(np.float32(1. / 255)))
        new, _ = _ref_step("lstm", rp, k, xf, [v.double() for v in before])
    for s, v, w in zip(policy._state, before, new):
        assert not torch.equal(s, v) and torch.allclose(s.double(), w, rtol=1e-4, atol=1e-6)
    # an override is obeyed: epsilon = 1 draws a random action for every env of every step
    policy.set_epsilon(1.0)
    np.random.seed(5)
    policy.host_draws(2, b)
    table = policy._overrides[b][1]
    assert tuple(table.shape) == (2, b) and bool((table >= 0).all())
    for step in (0, 1):
        policy.set_step(step)
        onehot = policy.act_step(obs)[0]
        assert torch.equal(onehot.argmax(dim=1).to(torch.int32), table[step])
    np.random.seed(6)
    acts, infos = policy.get_actions(obs, deterministic=True)
    assert acts.shape == (b,) and set(infos) == {"hprev_0", "cprev_0"}
    a, _ = policy.get_action(obs[0], deterministic=True)
    assert 0 <= a < n_act and policy._state[0].shape[0] == 1


def test_update_target_makes_the_target_unroll_equal_the_online_unroll():
    nb, burn_in, train_len, n = 2, 1, 2, 1
    u_len = burn_in + train_len + n
    rows = nb * u_len
    policy, _ = _make_policy(True)
    rs = np.random.RandomState(9)
    obs = _dev(rs.randint(0, 256, size=(rows, 4, 104, 80), dtype=np.uint8))
    act = _dev(rs.randint(0, 6, size=rows).astype(np.uint8))
    ret, term = _dev(rs.randn(rows).astype(np.float32)), _dev(np.zeros(rows, np.uint8))
    resets = _dev((rs.rand(rows) < 0.3).astype(np.uint8))
    init = [_dev((rs.randn(nb, 64) * 0.3).astype(np.float32)) for _ in range(2)]
    policy.flat_target.mul_(0.5)
    policy.r2d2_loss_and_grads(obs, act, ret, term, resets, init, None, 0.99, burn_in, train_len, n)
    assert not torch.equal(policy.last_q, policy.last_q_tgt)
    policy.update_target()
    policy.r2d2_loss_and_grads(obs, act, ret, term, resets, init, None, 0.99, burn_in, train_len, n)
    assert torch.equal(policy.last_q, policy.last_q_tgt) and bool(policy.last_q[:, :7].abs().sum() > 0)
    assert not policy.last_q[:, 7:].any()                        # the padding columns of the output layer stay zero


# ---- end to end ------------------------------------------------------------------------------------------------------------

def _train(use_graph, n_itr):
    from accel_rl_amd.algos.dqn.r2d2 import R2D2
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_r2d2_policy import AtariR2d2Policy
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="seaquest"), horizon=8, n_parallel=2, envs_per=2,
                            max_path_length=25, max_decorrelation_steps=0, mid_batch_reset=True, use_graph=use_graph,
                            device=DEV)
    algo = R2D2(burn_in=4, train_len=4, seq_stride=4, reward_horizon=2, batch_size=4, replay_size=64 * 5,
                min_steps_learn=64 * 3, training_intensity=1, target_update_steps=64 * 2,
                eps_greedy_args=dict(anneal_steps=64 * 6), optimizer_args=dict(use_graph=use_graph))
    policy = AtariR2d2Policy(**dict(cnn_specs[0], hidden_sizes=[64]))
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=64 * n_itr, seed=9, log_interval_steps=64 * n_itr)
    runner.startup()
    first = policy.flat_params.clone()
    infos = []
    for itr in range(n_itr):
        samples, _ = sampler.obtain_samples(itr)
        _, opt_info = algo.optimize_policy(itr, samples)
        tree = algo.replay_buffer.priority_tree.tree
        leaves = tree[algo.replay_buffer.priority_tree.t_l_shift:]
        assert bool(torch.isfinite(tree).all()) and bool((leaves >= 0).all())
        infos.append({k: [float(v.float().mean()) for v in vals] for k, vals in opt_info.items()})
    torch.cuda.synchronize()
    sampler.shutdown()
    return algo, first, policy.flat_params.clone(), infos


def test_r2d2_trains_end_to_end_and_the_graph_replays_the_eager_bits():
    n_itr = 12                                                   # 96 steps per env into a ring of 40: wraps twice
    algo, first, eager, infos = _train(False, n_itr)
    assert algo.replay_buffer.env_replay_size == 40 and algo.replay_buffer._buffer_full
    assert algo._updates_per_optimize == 1 * 64 // (4 * 4)
    assert bool(torch.isfinite(eager).all()) and not torch.equal(first, eager)
    learned = [i for i in infos if i]
    assert len(learned) == n_itr - 3
    for i in learned:
        assert len(i["Loss"]) == 4 and len(i["Priority"]) == 4
        assert np.isfinite(i["Loss"]).all() and np.isfinite(i["Priority"]).all() and min(i["Priority"]) >= 0
    _, first_g, graph, infos_g = _train(True, n_itr)
    assert torch.equal(first, first_g)
    assert torch.equal(eager, graph), "the captured sampler + update differ from the eager run"
    assert np.allclose(infos_g[-1]["Loss"], infos[-1]["Loss"], rtol=1e-5, atol=0)     # (the ring sums the loss rows itself)
