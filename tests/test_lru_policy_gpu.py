"""AtariLruPolicy on the GPU: serving (arl_lru_fwd at T = 1 in place on the state) against training on the recorded
batch, one whole A2C and PPO step against float64 autograd (the stored state a constant; whole batch and trajectory
minibatches, with resets), and A2C / RecurrentPPO through the sampler, captured against eager.
The bar is test_attn_memory_policy_gpu.py's: `close`, rtol 2e-3, atol 2e-5 of max |want|."""
import functools

import numpy as np
import pytest
import torch

from test_attention_gpu import DEV, _dev, _host, close
from test_recurrent_ppo_gpu import CLIP, ENT_COEFF, TINY, V_COEFF, _flat_grads, _mb, _ref_features, _ref_params

pytestmark = pytest.mark.gpu

SPEC = dict(conv_filters=(8, 8), conv_filter_sizes=(4, 3), conv_strides=(2, 1), conv_pads=((0, 0), (0, 0)),
            hidden_sizes=(16,), state_size=8)
OBS, N_ACT, N_ENV, T_LEN = (4, 20, 16), 5, 3, 6
RESET_AFTER = {1: (0,), 3: (0, 2), 5: (1,)}     # step -> the environments whose state is cleared after it


def _make():
    from accel_rl_amd.policies import AtariLruPolicy
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    from accel_rl_amd.util.seed import set_seed
    set_seed(11)
    policy = AtariLruPolicy(**SPEC)
    policy.initialize(EnvSpec(UintBox(OBS), Discrete(N_ACT)), device=DEV)
    flat = policy.get_param_values()
    flat += np.random.RandomState(5).randn(flat.size).astype(np.float32) * 0.05      # the biases off zero
    policy.set_param_values(flat)
    return policy


@functools.lru_cache(maxsize=None)
def served():
    """Drive act_step for T_LEN steps; the batch env-major ([env][time]) with what was served for every row."""
    policy, rs = _make(), np.random.RandomState(2)
    policy.reset(N_ENV)
    obs = rs.randint(0, 256, size=(T_LEN, N_ENV) + OBS, dtype=np.uint8)
    resets = np.zeros((N_ENV, T_LEN), np.uint8)
    prob, value, state = [], [], []
    for t in range(T_LEN):
        p, v, prev = policy.act_step(_dev(obs[t]))
        prob.append(p.clone()), value.append(v.clone()), state.append(prev.clone())
        if t in RESET_AFTER:
            mask = np.zeros(N_ENV, np.uint8)
            mask[list(RESET_AFTER[t])] = 1
            resets[:, t] = mask
            policy.reset_rows(_dev(mask))
    rows = N_ENV * T_LEN
    env_major = lambda xs: torch.stack(xs, dim=1).reshape((rows,) + tuple(xs[0].shape[1:]))    # noqa: E731
    data = dict(observations=_dev(obs.swapaxes(0, 1).reshape((rows,) + OBS)), lru_0=env_major(state),
                actions=_dev(rs.randint(0, N_ACT, size=rows).astype(np.uint8)),
                advantages=_dev(rs.randn(rows).astype(np.float32)), returns=_dev(rs.randn(rows).astype(np.float32)),
                valids=None, old_value=env_major(value))
    noise = _dev(rs.randn(rows, N_ACT).astype(np.float32) * 0.15)
    data["old_prob"] = torch.softmax(torch.log(env_major(prob)) + noise, 1)
    return policy, data, env_major(prob), env_major(value), _dev(resets.reshape(-1))


def _learner(policy, data, segs, resets, kind=1, **kw):
    from accel_rl_amd import _lib
    policy.flat_grads.zero_()
    mb = _mb(data, T_LEN, None if segs is None else _dev(np.asarray(segs, np.int32)))
    if resets is not None:
        mb["resets"] = resets
    loss4 = policy.loss_and_grads(mb, kind, CLIP, V_COEFF, ENT_COEFF, torch.ones(1, device=DEV), None,
                                  tie_rule=_lib.PPO_TIE_MATH, **kw).clone()
    return loss4, policy.flat_grads.clone()


def test_training_sees_what_was_served():
    policy, data, prob, value, resets = served()
    _learner(policy, data, None, resets, keep_forward=True)
    got_p, got_v = policy.last_forward
    assert close(_host(got_p), _host(prob).astype(np.float64), "prob") and close(_host(got_v), _host(value).astype(np.float64), "value")


def ref_losses(policy, data, segs, resets, kind):
    """float64 autograd: the A2C (kind 0) or PPO (kind 1) losses of the segments `segs` and the reference-layout parameters they depend on."""
    rp = _ref_params(policy)
    n, nb = SPEC["state_size"], len(segs)
    rows = (torch.as_tensor(segs, device=DEV).long()[:, None] * T_LEN + torch.arange(T_LEN, device=DEV)[None]).reshape(-1)
    xf, k = _ref_features(rp, SPEC, data["observations"][rows].double() * np.float64(np.float32(1. / 255)))
    pre_e = xf @ rp[k] + rp[k + 1]
    emb = torch.relu(pre_e)
    mag = torch.exp(-torch.exp(rp[k + 2]))
    l_re, l_im, gam = mag * torch.cos(rp[k + 3]), mag * torch.sin(rp[k + 3]), torch.sqrt(1 - mag ** 2)
    u = (emb @ rp[k + 4]).view(nb, T_LEN, n, 2)
    h0 = data["lru_0"][rows].double().view(nb, T_LEN, n, 2)[:, 0]                              # a constant
    flags = torch.zeros((nb, T_LEN), device=DEV) if resets is None else resets[rows].double().view(nb, T_LEN)
    h_re, h_im, hs = h0[..., 0], h0[..., 1], []
    for t in range(T_LEN):
        keep = 1. if t == 0 else 1 - flags[:, t - 1, None]
        h_re, h_im = (keep * (l_re * h_re - l_im * h_im) + gam * u[:, t, :, 0],
                      keep * (l_re * h_im + l_im * h_re) + gam * u[:, t, :, 1])
        hs.append(torch.stack([h_re, h_im], dim=2).reshape(nb, 2 * n))
    pre = emb + torch.stack(hs, dim=1).reshape(nb * T_LEN, 2 * n) @ rp[k + 5] + rp[k + 6]
    y = torch.relu(pre)
    prob, value = torch.softmax(y @ rp[k + 7] + rp[k + 8], 1), (y @ rp[k + 9] + rp[k + 10]).reshape(-1)
    m = len(rows)
    act, adv, ret = data["actions"][rows].long(), data["advantages"][rows].double(), data["returns"][rows].double()
    pa = prob[torch.arange(m), act]
    ratio = (pa + TINY) / (data["old_prob"][rows].double()[torch.arange(m), act] + TINY)
    pi = -torch.mean(torch.minimum(ratio * adv, torch.clamp(ratio, 1. - CLIP, 1. + CLIP) * adv))
    if kind == 0:
        pi = -torch.mean(torch.log(pa + TINY) * adv)
    vl = V_COEFF * torch.mean((value - ret) ** 2)
    el = -ENT_COEFF * torch.mean(-torch.sum(prob * torch.log(prob + TINY), dim=1))
    margin = min(pre_e.abs().min().item(), pre.abs().min().item())
    return (pi, vl, el), rp, margin


@pytest.mark.parametrize("kind,segs,flags", [(0, None, None), (0, (2, 0), torch.bool), (1, None, torch.bool),
                                             (1, (2, 0), torch.uint8)])
def test_whole_step_matches_float64_autograd(kind, segs, flags):
    policy, data, _, _, resets = served()
    resets = None if flags is None else resets.to(flags)
    loss4, grads = _learner(policy, data, segs, resets, kind)
    (pi, vl, el), rp, margin = ref_losses(policy, data, np.arange(N_ENV) if segs is None else np.asarray(segs), resets, kind)
    want = _flat_grads(pi + vl + el, rp)
    print("rectifier margin %.3g" % margin)
    assert margin > 1e-4                        # orders above the fp32 error of a pre-activation of size 1
    assert close(_host(loss4), torch.stack([pi, vl, el, pi + vl + el]).detach().cpu().numpy(), "losses")
    got, pos = policy.bucket_to_reference(grads), 0
    for name, shape in zip(policy.param_short_names, policy._ref_shapes):       # every tensor at the bar, on its own scale
        n = int(np.prod(shape))
        assert close(got[pos:pos + n], want[pos:pos + n].astype(np.float64), "%s %s %s d %s" % (kind, segs, flags, name)), name
        pos += n


@pytest.mark.parametrize("name,mid_batch_reset", [("a2c", True), ("ppo", True), ("ppo", False)])
def test_learners_train_through_the_sampler_captured_as_eager(name, mid_batch_reset):
    """test_bptt_resets_gpu._train's sizes: seeded runs whose updates replay from one captured graph, then run eagerly."""
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.algos.pg.ppo import RecurrentPPO
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies import AtariLruPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    finals = []
    for use_graph in (True, False):
        kw = dict(use_graph=use_graph, bptt_resets=True) if mid_batch_reset else dict(use_graph=use_graph)
        algo = A2C(**kw) if name == "a2c" else RecurrentPPO(optimizer_args=dict(minibatch_size=40), **kw)
        sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="pong"), horizon=5, n_parallel=4, envs_per=4,
                                max_path_length=23, mid_batch_reset=mid_batch_reset, max_decorrelation_steps=0, device=DEV)
        policy = AtariLruPolicy(**dict(cnn_specs[0], hidden_sizes=[64]), state_size=32)
        runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=160 * 8, seed=2, log_interval_steps=640)
        runner.train()
        assert np.isfinite(runner.last_tabular["GradNormAverage"]) and (algo._graph is not None) == use_graph
        assert sampler.samples_buf.agent_infos["lru_0"].abs().sum() > 0
        finals.append(policy.get_param_values())
    assert np.isfinite(finals[0]).all()
    np.testing.assert_array_equal(finals[0], finals[1])         # the replayed updates = the eager ones, bit for bit
