"""Recurrent PPO: arl_traj_minibatch (csrc/traj.hip) against numpy, RecurrentCnnPolicy.loss_and_grads on a trajectory
minibatch against float64 autograd through a plain-PyTorch restatement of the reference's networks (the construction
of test_lstm_gpu.py / test_gru_rnn_gpu.py::test_bptt_gradients_match_autograd, evaluated on the chosen segments' rows
gathered on the host), TrajPpoOptimizer's steps against the oracle's adam, and training through the sampler.
Tolerances are those of the tests named; no new one is introduced (the arithmetic is the same kernels on fewer
rows)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = 1e-8
KINDS = ["lstm", "gru", "rnn"]
CLIP, V_COEFF, ENT_COEFF = 0.2, 1.0, 0.01


# ---------------------------------------------------------------------------------------------------------------------
# check 4: the kernel against numpy
# ---------------------------------------------------------------------------------------------------------------------

def _kernel_case(rs, seg, n_traj, t_len, hidden, n_state, with_valids, all_zero=False):
    from accel_rl_amd import _lib
    n_seg = len(seg)
    states = [rs.randn(n_traj * t_len, hidden).astype(np.float32) for _ in range(n_state)]
    valids = None
    if with_valids:
        valids = np.zeros(n_traj * t_len, np.int8) if all_zero else (rs.rand(n_traj * t_len) < 0.7).astype(np.int8)
    dev = lambda a: torch.from_numpy(a).to(DEV)                                          # noqa: E731
    idx = torch.full((n_seg * t_len,), -7, dtype=torch.int32, device=DEV)
    out = [torch.full((n_seg, hidden), float("nan"), device=DEV) for _ in range(n_state)]
    inv = torch.full((1,), float("nan"), device=DEV)
    _lib.traj_minibatch(dev(seg.astype(np.int32)), t_len, [dev(s) for s in states],
                        None if valids is None else dev(valids), idx, out, inv)
    want_idx = (seg[:, None].astype(np.int64) * t_len + np.arange(t_len)[None]).reshape(-1)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx.astype(np.int32))
    for s, o in zip(states, out):
        np.testing.assert_array_equal(o.cpu().numpy().view(np.uint32), s[seg * t_len].view(np.uint32))
    count = n_seg * t_len if valids is None else int(valids[want_idx].astype(np.int64).sum())
    want_inv = np.float32(1) / np.float32(count) if count else np.float32(0)
    assert inv.cpu().numpy().view(np.uint32)[0] == np.array([want_inv], np.float32).view(np.uint32)[0], (count, inv)


@pytest.mark.parametrize("t_len", [1, 5, 32])
@pytest.mark.parametrize("hidden", [4, 256, 1024])
def test_traj_minibatch_kernel_matches_numpy(t_len, hidden):
    rs = np.random.RandomState(100 * t_len + hidden)
    n_traj = 37
    for n_state in (0, 1, 2):
        for with_valids in (False, True):
            _kernel_case(rs, rs.randint(0, n_traj, size=23), n_traj, t_len, hidden, n_state, with_valids)   # repeats
            _kernel_case(rs, rs.permutation(n_traj), n_traj, t_len, hidden, n_state, with_valids)
    _kernel_case(rs, rs.permutation(n_traj)[:9], n_traj, t_len, hidden, 2, True, all_zero=True)          # -> 0, not inf
    _kernel_case(rs, np.arange(256), 256, t_len, hidden, 2, True)                                        # config size
    _kernel_case(rs, np.array([n_traj - 1]), n_traj, t_len, hidden, 1, True)                             # one segment


def test_traj_minibatch_without_inv_count_and_wrapper_checks():
    from accel_rl_amd import _lib
    seg = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    st = torch.arange(3 * 5 * 8, dtype=torch.float32, device=DEV).view(15, 8)
    idx = torch.zeros(10, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, 8, device=DEV)
    _lib.traj_minibatch(seg, 5, [st], None, idx, [out], None)
    assert idx.tolist() == [10, 11, 12, 13, 14, 0, 1, 2, 3, 4] and torch.equal(out, st[[10, 0]])
    with pytest.raises(ValueError):
        _lib.traj_minibatch(seg, 5, [st], None, idx[:9], [out], None)
    with pytest.raises(ValueError):
        _lib.traj_minibatch(seg, 5, [st], None, idx, [out, out], None)
    with pytest.raises(TypeError):
        _lib.traj_minibatch(seg.long(), 5, [st], None, idx, [out], None)


def test_traj_minibatch_limits_leave_the_outputs_untouched():
    """The first value past each limit: ARL_E_RANGE before any launch."""
    from accel_rl_amd import _lib
    lib = _lib.load()
    seg = torch.zeros(4, dtype=torch.int32, device=DEV)
    big = torch.zeros(4 * 5 * 1028, device=DEV)
    valids = torch.ones(64, dtype=torch.int8, device=DEV)
    idx = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    outs = [torch.full((4 * 1028,), float("nan"), device=DEV) for _ in range(3)]
    inv = torch.full((1,), float("nan"), device=DEV)
    arr = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])                  # noqa: E731

    def call(n_seg=4, horizon=5, n_traj=4, n_state=2, hidden=256):
        return lib.arl_traj_minibatch(seg.data_ptr(), n_seg, horizon, n_traj, arr([big] * 3), n_state, hidden,
                                      valids.data_ptr(), idx.data_ptr(), arr(outs), inv.data_ptr(), _lib.stream_ptr())
    for kw in (dict(n_seg=0), dict(horizon=0), dict(hidden=6), dict(hidden=1028), dict(n_state=3),
               dict(n_seg=65536, horizon=32768), dict(n_traj=0)):
        assert call(**kw) == -2, kw
    torch.cuda.synchronize()
    assert (idx == -7).all() and torch.isnan(inv).all() and all(torch.isnan(o).all() for o in outs)
    assert call() == 0                                          # ... and the same call inside the limits runs
    torch.cuda.synchronize()
    assert idx[:20].tolist() == list(range(5)) * 4 and inv.item() == np.float32(1) / np.float32(20)


# ---------------------------------------------------------------------------------------------------------------------
# the policies and their plain-torch restatement (float64, the reference's parameter layout)
# ---------------------------------------------------------------------------------------------------------------------

def _policy_cls(kind):
    from accel_rl_amd.policies.atari_gru_policy import AtariGruPolicy
    from accel_rl_amd.policies.atari_lstm_policy import AtariLstmPolicy
    from accel_rl_amd.policies.atari_rnn_policy import AtariRnnPolicy
    return dict(lstm=AtariLstmPolicy, gru=AtariGruPolicy, rnn=AtariRnnPolicy)[kind]


def _env_spec(n_act=6):
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    return EnvSpec(UintBox((4, 104, 80)), Discrete(n_act))


def _make(kind, hidden=256):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.util.seed import set_seed
    set_seed(8)
    spec = dict(cnn_specs[0], hidden_sizes=[hidden])
    policy = _policy_cls(kind)(**spec)
    policy.initialize(_env_spec(), device=DEV)
    return policy, spec


def _ref_params(policy, flat=None):
    flat = policy.get_param_values() if flat is None else flat
    out, pos = [], 0
    for shape in policy._ref_shapes:
        n = int(np.prod(shape))
        out.append(torch.from_numpy(flat[pos:pos + n].reshape(shape).astype(np.float64)).to(DEV).requires_grad_())
        pos += n
    assert pos == flat.size == policy.n_params
    return out


def _ref_features(rp, spec, x):
    k = 0
    for i in range(len(spec["conv_filters"])):
        x = F.relu(F.conv2d(x, rp[k].flip(2, 3), rp[k + 1], stride=spec["conv_strides"][i], padding=tuple(spec["conv_pads"][i])))
        k += 2
    return x.flatten(1), k


def _ref_step(kind, rp, k, xf, state):
    """One step in the reference's own parameter layout: (new state, index of W_pi)."""
    if kind == "lstm":
        h, c = state
        hh = h.shape[1]
        pre = xf @ rp[k] + rp[k + 2] + h @ rp[k + 1]
        f, i, g, o = (pre[:, j * hh:(j + 1) * hh] for j in range(4))
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return [torch.sigmoid(o) * torch.tanh(c), c], k + 3
    h = state[0]
    if kind == "rnn":
        return [torch.tanh(xf @ rp[k] + h @ rp[k + 1] + rp[k + 2])], k + 3
    k += 3                                              # W_xh, W_hh, b: registered, never read
    r = torch.sigmoid(xf @ rp[k] + h @ rp[k + 1] + rp[k + 2])
    u = torch.sigmoid(xf @ rp[k + 3] + h @ rp[k + 4] + rp[k + 5])
    c = torch.tanh(xf @ rp[k + 6] + r * (h @ rp[k + 7]) + rp[k + 8])
    return [(1 - u) * h + u * c], k + 9


def _ref_prob_value(kind, rp, spec, data, segs, t_len):
    """prob, value (float64) of the rows of segments `segs`, in time order, from each segment's stored state."""
    rows = (torch.as_tensor(segs, device=DEV).long()[:, None] * t_len + torch.arange(t_len, device=DEV)[None]).reshape(-1)
    obs = data["observations"][rows]                                    # gathered outside the product's kernels
    xf, k = _ref_features(rp, spec, obs.double() * np.float64(np.float32(1. / 255)))
    nb = len(segs)
    xf = xf.view(nb, t_len, -1)
    state = [data[key][rows].double().view(nb, t_len, -1)[:, 0] for key in data["state_keys"]]
    hs = []
    for t in range(t_len):
        state, kp = _ref_step(kind, rp, k, xf[:, t], state)
        hs.append(state[0])
    h_all = torch.stack(hs, dim=1).reshape(nb * t_len, -1)
    prob = torch.softmax(h_all @ rp[kp] + rp[kp + 1], 1)
    value = (h_all @ rp[kp + 2] + rp[kp + 3]).reshape(-1)
    return prob, value, rows


def _ref_ppo_losses(kind, rp, spec, data, segs, t_len, clip=CLIP):
    """(pi, v, ent) losses of ppo.py:42-51 + aac_base.py:60-66 in float64; torch.minimum's own tie rule ("math")."""
    prob, value, rows = _ref_prob_value(kind, rp, spec, data, segs, t_len)
    n = len(rows)
    act = data["actions"][rows].long()
    adv, ret = data["advantages"][rows].double(), data["returns"][rows].double()
    valids = None if data.get("valids") is None else data["valids"][rows].double()
    mean = torch.mean if valids is None else (lambda x: torch.sum(valids * x) * (1. / torch.sum(valids)))
    pa = prob[torch.arange(n), act]
    ratio = (pa + TINY) / (data["old_prob"][rows].double()[torch.arange(n), act] + TINY)
    surr = torch.minimum(ratio * adv, torch.clamp(ratio, 1. - clip, 1. + clip) * adv)
    pi = -mean(surr)
    vl = V_COEFF * mean((value - ret) ** 2)
    el = -ENT_COEFF * mean(-torch.sum(prob * torch.log(prob + TINY), dim=1))
    return (pi, vl, el), ratio.detach()


def _data(kind, policy, spec, rs, nb, t_len, masked, hh=256):
    rows = nb * t_len
    dev = lambda a: torch.from_numpy(a).to(DEV)                                          # noqa: E731
    data = dict(observations=dev(rs.randint(0, 256, size=(rows, 4, 104, 80), dtype=np.uint8)),
                actions=dev(rs.randint(0, 6, size=rows).astype(np.uint8)),
                advantages=dev(rs.randn(rows).astype(np.float32)), returns=dev(rs.randn(rows).astype(np.float32)),
                state_keys=list(policy.state_info_keys))
    for key in data["state_keys"]:
        data[key] = dev((rs.randn(rows, hh) * 0.3).astype(np.float32))
    data["valids"] = None
    if masked:
        v = (rs.rand(rows) < 0.8).astype(np.int8)
        v[::t_len] = 1                                          # update_valids: step 0 of every segment is valid
        data["valids"] = dev(v)
    # behaviour policy = the current one, perturbed so that some likelihood ratios leave the clip range
    with torch.no_grad():
        prob, value, _ = _ref_prob_value(kind, _ref_params(policy), spec, data, np.arange(nb), t_len)
        noise = dev(rs.randn(rows, prob.shape[1]) * 0.15)
        data["old_prob"] = torch.softmax(torch.log(prob) + noise, 1).float()
        data["old_value"] = value.float()
    return data


def _mb(data, t_len, traj):
    mb = {k: v for k, v in data.items() if k != "state_keys"}
    mb.update(idx=None, horizon=t_len)
    if traj is not None:
        mb["traj"] = traj
    return mb


GRAD_RTOL, GRAD_ATOL = 2e-3, 2e-5           # test_bptt_gradients_match_autograd's bars


def _flat_grads(loss, rp):
    grads = torch.autograd.grad(loss, rp, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, rp)]
    return np.concatenate([g.detach().cpu().numpy().reshape(-1) for g in grads]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# checks 5 and 6: gradients
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_trajectory_minibatch_gradients_match_float64_autograd(kind, masked):
    """PPO loss on 4 of 8 segments x 5 steps, shuffled order: every parameter gradient in the reference's layout."""
    from accel_rl_amd import _lib
    policy, spec = _make(kind)
    rs = np.random.RandomState(4)
    nb, t_len = 8, 5
    data = _data(kind, policy, spec, rs, nb, t_len, masked)
    segs = np.array([5, 2, 7, 0])                               # 4 of the 8, not in batch order
    lr_mult = torch.ones(1, device=DEV)
    traj = torch.from_numpy(segs.astype(np.int32)).to(DEV)
    loss4 = policy.loss_and_grads(_mb(data, t_len, traj), 1, CLIP, V_COEFF, ENT_COEFF, lr_mult, None,
                                  tie_rule=_lib.PPO_TIE_MATH).clone()
    got = policy.bucket_to_reference(policy.flat_grads)
    rp = _ref_params(policy)
    (pi, vl, el), ratio = _ref_ppo_losses(kind, rp, spec, data, segs, t_len)
    outside = ((ratio < 1 - CLIP) | (ratio > 1 + CLIP)).sum().item()
    assert 0 < outside < ratio.numel(), outside                 # both branches of the surrogate are exercised
    want = _flat_grads(pi + vl + el, rp)
    print("loss4", loss4.tolist(), "want", [pi.item(), vl.item(), el.item()])
    assert torch.allclose(loss4[:3], torch.stack([pi, vl, el]).detach().float(), rtol=1e-4, atol=1e-6)
    scale = np.abs(want).max()
    print("max |got - want| = %.3g, largest entry %.3g" % (np.abs(got - want).max(), scale))
    assert np.allclose(got, want, rtol=GRAD_RTOL, atol=GRAD_ATOL * max(scale, 1e-3)), (np.abs(got - want).max(), scale)
    with pytest.raises(NotImplementedError):                    # row slicing stays refused
        policy.loss_and_grads(dict(_mb(data, t_len, None), idx=torch.arange(8, dtype=torch.int32, device=DEV)),
                              1, CLIP, V_COEFF, ENT_COEFF, lr_mult, None)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_a_minibatch_of_every_segment_is_the_whole_batch(kind, masked):
    """traj = arange(n_traj): the same kernels on the same rows in the same order -> the same bits."""
    policy, spec = _make(kind)
    rs = np.random.RandomState(5)
    nb, t_len = 8, 5
    data = _data(kind, policy, spec, rs, nb, t_len, masked)
    lr_mult = torch.ones(1, device=DEV)
    inv = (1. / data["valids"].sum(dtype=torch.float32)).reshape(1) if masked else None
    whole = policy.loss_and_grads(_mb(data, t_len, None), 1, CLIP, V_COEFF, ENT_COEFF, lr_mult, inv).clone()
    g_whole = policy.flat_grads.clone()
    policy.flat_grads.zero_()
    traj = torch.arange(nb, dtype=torch.int32, device=DEV)
    part = policy.loss_and_grads(_mb(data, t_len, traj), 1, CLIP, V_COEFF, ENT_COEFF, lr_mult, None).clone()
    g_part = policy.flat_grads.clone()
    print("max |d loss4| %.3g, max |d grad| %.3g" % ((whole - part).abs().max().item(), (g_whole - g_part).abs().max().item()))
    assert torch.equal(whole, part)
    assert torch.equal(g_whole, g_part)


# ---------------------------------------------------------------------------------------------------------------------
# check 7: one optimizer call against the oracle's update rule
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_steps_match_the_oracle_adam(kind):
    """TrajPpoOptimizer, 1 epoch x 2 minibatches of 4 segments: every step compared from the product's own state
    before it (the method and the bars of test_learner_gpu.py::test_learner_matches_plain_torch)."""
    from accel_rl_amd.algos.pg.ppo import PPO
    from accel_rl_amd.optimizers.single import TrajPpoOptimizer
    policy, spec = _make(kind)
    nb, t_len = 8, 5
    algo = PPO(OptimizerCls=TrajPpoOptimizer, optimizer_args=dict(minibatch_size=20, epochs=1), ppo_tie_rule="math",
               use_graph=False)
    algo.initialize(policy, _env_spec(), nb * t_len, t_len, mid_batch_reset=False)
    opt = algo.optimizer
    rs = np.random.RandomState(6)
    data = _data(kind, policy, spec, rs, nb, t_len, True)
    inputs = tuple(data[name] for name in opt._input_names)
    assert opt._input_names[-1] == "valids" and all(k in opt._input_names for k in data["state_keys"])

    def state():
        return (policy.get_param_values(), policy.bucket_to_reference(opt._slot0),
                policy.bucket_to_reference(opt._slot1), np.float32(opt._step_count.item()))
    snaps = []
    apply_update = opt._apply_update

    def hooked(avg_factor=1.0):
        apply_update(avg_factor)
        snaps.append(state())
    opt._apply_update = hooked
    before = state()
    np.random.seed(3)
    opt.prepare_host(nb * t_len)
    seg_mbs = opt._idx_host.numpy().copy()
    assert seg_mbs.shape == (2, 4) and sorted(seg_mbs.reshape(-1)) == list(range(nb))
    _, norms = opt.device_updates(inputs)
    torch.cuda.synchronize()
    got_norms = norms.cpu().numpy()
    assert len(snaps) == 2 and got_norms.shape == (2,)
    for k, segs in enumerate(seg_mbs):
        pw, m, v, t = before if k == 0 else snaps[k - 1]
        rp = _ref_params(policy, pw)
        (pi, vl, el), _ = _ref_ppo_losses(kind, rp, spec, data, segs, t_len)
        g, norm = P.clip_by_total_norm(_flat_grads(pi + vl + el, rp), None)
        want, m, v, t = P.adam_step(pw.copy(), g, m.copy(), v.copy(), t, np.float32(1e-3), eps=1e-5)
        got = snaps[k]
        print("step %d: norm %.6g vs %.6g, max |d param| %.3g" % (k, got_norms[k], norm, np.abs(got[0] - want).max()))
        assert np.isclose(got_norms[k], norm, rtol=5e-4), (k, got_norms[k], norm)
        assert np.allclose(got[0], want, rtol=1e-5, atol=5e-5), (k, np.abs(got[0] - want).max())
        assert np.allclose(got[1], m, rtol=2e-3, atol=2e-3 * max(np.abs(m).max(), 1e-3)), (k, np.abs(got[1] - m).max())
        assert float(got[3]) == float(t)


# ---------------------------------------------------------------------------------------------------------------------
# checks 8 and 9: through the sampler and the runner
# ---------------------------------------------------------------------------------------------------------------------

def _train(kind, use_graph=True, algo=None):
    from accel_rl_amd.algos.pg.ppo import PPO
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.optimizers.single import TrajPpoOptimizer
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="pong"), horizon=5, n_parallel=4, envs_per=4,
                            max_path_length=23, mid_batch_reset=False, max_decorrelation_steps=0, device=DEV)
    policy = _policy_cls(kind)(**dict(cnn_specs[0], hidden_sizes=[256]))
    if algo is None:
        algo = PPO(OptimizerCls=TrajPpoOptimizer, optimizer_args=dict(minibatch_size=40), use_graph=use_graph)
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=160 * 8, seed=2, log_interval_steps=640)
    runner.train()
    return runner, policy, sampler, algo


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_recurrent_ppo_trains_through_the_sampler(kind):
    finals = []
    for use_graph in (True, True, False):
        if kind == "gru" and not use_graph:
            break
        runner, policy, sampler, algo = _train(kind, use_graph)
        tab = runner.last_tabular
        assert np.isfinite(tab["GradNormAverage"]) and tab["CumCompletedTrajs"] > 0 and tab["LengthAverage"] == 24
        assert all(np.isfinite(v) for v in tab.values() if isinstance(v, (float, np.floating)))
        assert (algo._graph is not None) == use_graph           # past the two warm-up calls: replayed from one hipGraph
        assert algo.optimizer._n_minibatches == 4 * (algo._batch_size // 40)
        hp = sampler.samples_buf.agent_infos["hprev_0"]
        assert hp.abs().sum() > 0 and torch.isfinite(hp).all()
        flat = policy.get_param_values()
        assert np.isfinite(flat).all()
        finals.append(flat)
    np.testing.assert_array_equal(finals[0], finals[1])        # seeded runs agree bit for bit
    if len(finals) == 3:
        np.testing.assert_array_equal(finals[0], finals[2])    # eager minibatches = the captured ones


def test_recurrent_ppo_shell_and_the_refusals_that_stay():
    from accel_rl_amd.algos.pg.ppo import PPO, RecurrentPPO
    runner, policy, _, algo = _train("rnn", algo=RecurrentPPO(optimizer_args=dict(minibatch_size=40)))
    assert np.isfinite(runner.last_tabular["GradNormAverage"]) and algo._graph is not None
    with pytest.raises(NotImplementedError):                    # row-minibatch optimizer with a recurrent policy
        _train("lstm", algo=PPO())
    with pytest.raises(ValueError, match="48"):                 # sizes surface at initialize, with the numbers
        _train("lstm", algo=RecurrentPPO(optimizer_args=dict(minibatch_size=48)))
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    ff = AtariCnnPolicy(**cnn_specs[0])
    ff.initialize(_env_spec(), device=DEV)
    with pytest.raises(NotImplementedError, match="feed-forward"):
        RecurrentPPO(optimizer_args=dict(minibatch_size=40)).initialize(ff, _env_spec(), 80, 5, mid_batch_reset=False)
