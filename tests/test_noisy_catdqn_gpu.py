"""Noisy categorical DQN and Rainbow on the device (accel_rl_amd/policies/dqn/atari_noisy_net_cat_dqn_policy.py,
csrc/noisy.hip, csrc/dqn.hip:arl_noisy_catdqn_loss_parts, accel_rl_amd/algos/dqn/rainbow.py) against restatements of the
reference (catdqn_cnn.py:40-99 with NoisyDenseLayers, cat_dqn.py:40-109): the forward pass against a float64
reference-layout network fed with the noise rebuilt from arl_noisy_normals as include/accel_rl_hip.h states it, one
double-DQN C51 update against float64 autograd, the fused loss launch against the unfused pair bit for bit, the sigma = 0
limit against AtariCatDqnPolicy, fresh noise under graph replay, and end-to-end Rainbow under captured graphs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_catdqn_gpu import ref_cat_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ATOMS = 51
CASES = [(spec, n_act, dueling, common) for spec, n_act in ((0, 6), (1, 18)) for dueling in (False, True)
         for common in (False, True)]


def _make(n_act=6, spec_no=0, seed=5, **kw):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_noisy_net_cat_dqn_policy import AtariNoisyNetCatDqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(seed)
    spec = dict(cnn_specs[spec_no])
    policy = AtariNoisyNetCatDqnPolicy(n_atoms=N_ATOMS, **spec, **kw)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(n_act)), device=DEV)
    policy.incorporate_z(np.linspace(-10, 10, N_ATOMS, dtype=np.float32))
    return policy, spec


def _obs(rs, b):
    return torch.from_numpy(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)).to(DEV)


def _ref_params(policy, flat_bucket, dtype=torch.float64):
    flat = policy.bucket_to_reference(flat_bucket)
    out, pos = [], 0
    for shape in policy._ref_shapes:
        n = int(np.prod(shape))
        out.append(torch.from_numpy(flat[pos:pos + n].reshape(shape).copy()).to(DEV, dtype).requires_grad_())
        pos += n
    return out


def _pass_noise(policy, counter, rows, rpd, first, count):
    """The noise a pass of `rows` rows at `counter` used, rows [first, first + count), rebuilt from arl_noisy_normals as
    include/accel_rl_hip.h states it: per reference noisy layer in construction order (f(e_in) in the reference's input
    order, f(e_out)) -- hidden..., action_atoms; dueling hidden_0, action_atoms, hidden_Val_0, Val.  float64."""
    from accel_rl_amd import _lib
    co, ho, wo = policy._conv_out
    a, n, s = policy.n_act, policy.n_atoms, policy._atom_stride

    def f(layer, which, width):
        t = torch.empty((rows, width), device=DEV)
        _lib.noisy_normals(policy.noise_seed, counter, layer, which, rows, width, rpd, f=t)
        return t[first:first + count].double()

    def conv_order(t):                                                 # internal (h, w, c) -> (c, h, w)
        return t.reshape(count, ho, wo, co).permute(0, 3, 1, 2).reshape(count, -1)

    def atoms(t, acts):                                                # element a S + i -> reference unit a N + i
        return t.reshape(count, acts, s)[:, :, :n].reshape(count, acts * n)
    fan = co * ho * wo
    if policy._dueling:
        h = policy.hidden_sizes[0]
        return [(conv_order(f(0, 0, fan)), f(0, 1, h)), (f(1, 0, h), atoms(f(1, 1, a * s), a)),
                (conv_order(f(2, 0, fan)), f(2, 1, h)), (f(3, 0, h), atoms(f(3, 1, s), 1))]
    out, fan_in = [], fan
    for l, hs in enumerate(policy.hidden_sizes):
        fi = f(l, 0, fan_in)
        out.append((conv_order(fi) if l == 0 else fi, f(l, 1, hs)))
        fan_in = hs
    j = len(policy.hidden_sizes)
    return out + [(f(j, 0, fan_in), atoms(f(j, 1, a * s), a))]


def _noisy_dense(x, p, noise):
    fi, fo = noise
    return x @ p[0] + p[1] + fo * ((x * fi) @ p[2] + p[3])


def _ref_logits(rp, spec, x, noise, n_act, dueling):
    """[B, A, N] logits of the reference-layout noisy network (the dueling merge applied)."""
    k = 0
    for i in range(len(spec["conv_filters"])):
        x = F.relu(F.conv2d(x, rp[k].flip(2, 3), rp[k + 1], stride=spec["conv_strides"][i],
                            padding=tuple(spec["conv_pads"][i])))
        k += 2
    x = x.flatten(1)
    if dueling:                         # flat order: hidden_Val_0, Val, hidden_0, action_atoms
        val = _noisy_dense(F.relu(_noisy_dense(x, rp[k:k + 4], noise[2])), rp[k + 4:k + 8], noise[3])
        adv = _noisy_dense(F.relu(_noisy_dense(x, rp[k + 8:k + 12], noise[0])), rp[k + 12:k + 16], noise[1])
        adv = adv.view(x.shape[0], n_act, N_ATOMS)
        return val.view(-1, 1, N_ATOMS) + (adv - adv.mean(dim=1, keepdim=True))
    for l in range(len(noise)):
        x = _noisy_dense(x, rp[k:k + 4], noise[l])
        x = x if l == len(noise) - 1 else F.relu(x)
        k += 4
    return x.view(x.shape[0], n_act, N_ATOMS)


def _device_logits(policy, out):
    """The policy's stored logits [B, head width] -> [B, A, N] after the dueling merge."""
    a, n = policy.n_act, policy.n_atoms
    blk = out.view(out.shape[0], policy._rows, policy._atom_stride)[:, :, :n].double()
    if policy._dueling:
        return blk[:, a:a + 1] + (blk[:, :a] - blk[:, :a].mean(dim=1, keepdim=True))
    return blk


def _tol(want, k_red):
    return 2e-5 * np.sqrt(k_red) * max(want.abs().max().item(), 1e-6)


# ------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("spec_no,n_act,dueling,common", CASES)
def test_forward_against_float64_reference_with_rebuilt_noise(spec_no, n_act, dueling, common):
    policy, spec = _make(n_act, spec_no, dueling=dueling, common_noise=common)
    rs = np.random.RandomState(spec_no + n_act)
    b = 37
    obs = _obs(rs, b)
    c0 = int(policy._noise_state[1])
    out, _, _ = policy._logits(policy._scaled(obs))
    got = _device_logits(policy, out)
    assert int(policy._noise_state[1]) == c0 + 1
    noise = _pass_noise(policy, c0, b, b if common else 1, 0, b)
    rp = _ref_params(policy, policy.flat_params)
    with torch.no_grad():
        want = _ref_logits(rp, spec, obs.double() / 255., noise, n_act, dueling)
    fan = policy._conv_out[0] * policy._conv_out[1] * policy._conv_out[2]
    assert (got - want).abs().max().item() <= _tol(want, 2 * fan), (got - want).abs().max().item()
    p_got, p_want = torch.softmax(got, dim=2), torch.softmax(want, dim=2)
    assert (p_got - p_want).abs().max().item() <= 1e-5
    z = policy.z.double()
    q_want = (p_want * z).sum(dim=2)
    top2 = torch.topk(q_want, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    policy._noise_state[1] = c0                                # the same draw again: greedy actions on the noisy Q
    greedy = policy.greedy_actions(obs).long()
    assert torch.equal(greedy[clear], q_want.argmax(dim=1)[clear]) and clear.any()
    if common:
        assert torch.equal(noise[0][0][0], noise[0][0][-1])
    else:
        assert not torch.equal(noise[0][0][0], noise[0][0][1])


# ------------------------------------------------------------------------------------- one update
def _batch(rs, b, n_act):
    act = torch.from_numpy(rs.randint(0, n_act, size=b).astype(np.uint8)).to(DEV)
    ret = torch.from_numpy((rs.randn(b) * 3).astype(np.float32)).to(DEV)
    term = torch.from_numpy((rs.rand(b) < 0.2).astype(np.uint8)).to(DEV)
    isw = torch.from_numpy((rs.rand(b) + 0.2).astype(np.float32)).to(DEV)
    return act, ret, term, isw


def _pair(rs, b):
    both = _obs(rs, 2 * b)            # obs and next_obs adjacent, as the replay memory hands them out
    return both[:b], both[b:]


@pytest.mark.parametrize("spec_no,n_act,dueling,common", CASES)
def test_update_matches_float64_autograd_with_the_pass_noise(spec_no, n_act, dueling, common):
    policy, spec = _make(n_act, spec_no, dueling=dueling, common_noise=common)
    policy.loss_folds_heads = bool(common)             # both loss paths (they agree bit for bit: the test below)
    rs = np.random.RandomState(3)
    b = 32
    obs, nxt = _pair(rs, b)
    act, ret, term, isw = _batch(rs, b, n_act)
    policy.flat_target.copy_(policy.flat_params * 0.9)
    gamma_n = float(np.float32(0.99 ** 3))
    c0 = int(policy._noise_state[1])
    rows, kl = policy.cat_loss_and_grads(obs, nxt, act, ret, term, isw, -10., 10., gamma_n, double_dqn=True)
    assert int(policy._noise_state[1]) == c0 + 2
    got = policy.bucket_to_reference(policy.flat_grads)
    rpd = b if common else 1
    tgt_noise = _pass_noise(policy, c0, b, rpd, 0, b)
    on_noise = _pass_noise(policy, c0 + 1, 2 * b, rpd, 0, b)            # the online obs + next_obs pass: 2B rows
    nx_noise = _pass_noise(policy, c0 + 1, 2 * b, rpd, b, b)
    rp, rt = _ref_params(policy, policy.flat_params), _ref_params(policy, policy.flat_target)
    pred = _ref_logits(rp, spec, obs.double() / 255., on_noise, n_act, dueling)
    with torch.no_grad():
        tgt = _ref_logits(rt, spec, nxt.double() / 255., tgt_noise, n_act, dueling)
        pol = _ref_logits(rp, spec, nxt.double() / 255., nx_noise, n_act, dueling)
    loss, kl_ref = ref_cat_loss(pred, tgt, pol, policy.z.double(), act, ret.double(), term, isw.double(), -10., 10.,
                                gamma_n)
    grads = torch.autograd.grad(loss, rp)
    want = np.concatenate([g.detach().cpu().numpy().reshape(-1) for g in grads])
    assert abs(rows.sum().item() - loss.item()) <= 1e-4 * abs(loss.item())
    assert torch.allclose(kl.double(), kl_ref, rtol=2e-3, atol=1e-6)
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * max(np.abs(want).max(), 1e-3)), np.abs(got - want).max()
    pos = np.cumsum([0] + [int(np.prod(s)) for s in policy._ref_shapes])
    for i, nm in enumerate(policy.param_short_names):
        if "sigma" in nm:
            assert np.abs(got[pos[i]:pos[i + 1]]).max() > 0, nm                # every sigma learns
    n, s, a = policy.n_atoms, policy._atom_stride, n_act
    for k in (policy._k_head, policy._k_out_sigma):                            # padding and off-blocks: exactly zero
        g3 = policy.grads[k].reshape(policy._rows, s, -1)
        assert not g3[:, n:].any() and not policy.grads[k + 1].reshape(policy._rows, s)[:, n:].any()
        if dueling:
            hs = policy.hidden_sizes[0]
            assert not g3[:a, :, hs:].any() and not g3[a, :, :hs].any()


# ------------------------------------------------------------------------------------- fused loss launch
def _run_update(policy, batch, c0):
    policy._noise_state[1] = c0
    obs, nxt, act, ret, term, isw = batch
    rows, kl = policy.cat_loss_and_grads(obs, nxt, act, ret, term, isw, -10., 10., float(np.float32(0.99 ** 3)),
                                         double_dqn=True)
    torch.cuda.synchronize()
    return [t.clone() for t in (rows, kl, policy._scratch[("dlogits", obs.shape[0])], policy.flat_grads,
                                policy._noise_state)]


@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("common", [False, True])
def test_fused_loss_equals_unfused_pair_bit_for_bit(dueling, common):
    """The policy's update through arl_noisy_catdqn_loss_parts, through the fallback past its split limit, and through
    the unfused path (the default: combine per pass, then arl_catdqn_loss): dlogits, loss rows, KL, every
    gradient and the device noise state identical to the last bit."""
    policy, _ = _make(6, 0, dueling=dueling, common_noise=common)
    rs = np.random.RandomState(8)
    b = 32
    obs, nxt = _pair(rs, b)
    batch = (obs, nxt) + _batch(rs, b, 6)
    policy.flat_target.copy_(policy.flat_params * 0.9)
    c0 = int(policy._noise_state[1])
    policy.loss_folds_heads = True
    fused = _run_update(policy, batch, c0)
    limit = policy.fused_max_splits
    policy.fused_max_splits = -1                               # every product past the limit: the fallback
    fallback = _run_update(policy, batch, c0)
    policy.fused_max_splits = limit
    policy.loss_folds_heads = False
    unfused = _run_update(policy, batch, c0)
    assert int(fused[4][1]) == c0 + 2
    assert torch.isfinite(fused[2]).all() and fused[3].abs().max() > 0
    for x, y, z in zip(fused, fallback, unfused):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("splits", [(0, 0), (1, 1), (4, 3), (16, 16), (17, 5), (40, 128)])
@pytest.mark.parametrize("dueling", [False, True])
def test_fused_loss_kernel_folds_like_the_combine_launch(splits, dueling):
    """arl_noisy_catdqn_loss_parts at the kernel level on synthetic products of 0 (finished) .. 128 splits (W, W_sigma):
    bit for bit against arl_noisy_dense_combine per source, then arl_catdqn_loss; 129 splits are refused."""
    from accel_rl_amd import _lib
    n_act, batch = 6, 19
    stride, rows = 52, n_act + int(dueling)
    r = rows * stride
    gen = torch.Generator(device=DEV).manual_seed(sum(splits) + int(dueling))
    srcs, logits, keep = [], [], []
    for _ in range(3):                                           # pred, tgt_next, pol_next
        items, biases = [], []
        for sp in splits:
            parts = torch.randn(max(sp, 1), batch * r, device=DEV, generator=gen)
            it = _lib.ArlFoldItem()
            it.part, it.out, it.total, it.splits, it.valid = parts.data_ptr(), parts.data_ptr(), batch * r, sp, 0
            items.append(it)
            biases.append(torch.randn(r, device=DEV, generator=gen) * 0.1)
            keep.append(parts)
        feout = torch.randn(batch, r, device=DEV, generator=gen)
        out = torch.empty(batch, r, device=DEV)
        _lib.noisy_dense_combine(items[0], biases[0], items[1], biases[1], feout, out, False)
        logits.append(out)
        srcs.append(_lib.noisy_logit_src(items[0], biases[0], items[1], biases[1], feout))
        keep += biases + [feout]
    z = torch.linspace(-10, 10, N_ATOMS, device=DEV)
    act = torch.randint(0, n_act, (batch,), device=DEV, generator=gen).to(torch.uint8)
    ret = torch.randn(batch, device=DEV, generator=gen) * 6
    term = (torch.rand(batch, device=DEV, generator=gen) < 0.3).to(torch.uint8)
    isw = torch.rand(batch, device=DEV, generator=gen) + 0.1
    gamma_n = float(np.float32(0.99 ** 3))
    outs = []
    for fused in (False, True):
        dl = torch.full((batch, r), float("nan"), device=DEV)
        lr, kl = torch.empty(batch, device=DEV), torch.empty(batch, device=DEV)
        if fused:
            _lib.noisy_catdqn_loss_parts(srcs[0], srcs[1], srcs[2], z, act, ret, term, isw, n_act, N_ATOMS, stride,
                                         -10., 10., gamma_n, dl, lr, kl, dueling=dueling)
        else:
            _lib.catdqn_loss(logits[0], logits[1], logits[2], z, act, ret, term, isw, n_act, N_ATOMS, -10., 10.,
                             gamma_n, dl, lr, kl, dueling=dueling)
        torch.cuda.synchronize()
        outs.append((dl, lr, kl))
    assert torch.isfinite(outs[0][0]).all()
    for x, y in zip(*outs):
        assert torch.equal(x, y), splits
    srcs[1].s_splits = 129
    with pytest.raises(RuntimeError, match="splits"):
        _lib.noisy_catdqn_loss_parts(srcs[0], srcs[1], srcs[2], z, act, ret, term, isw, n_act, N_ATOMS, stride, -10.,
                                     10., gamma_n, outs[1][0], outs[1][1], outs[1][2], dueling=dueling)


# ------------------------------------------------------------------------------------- sigma = 0 limit
@pytest.mark.parametrize("dueling", [False, True])
def test_zero_sigma_equals_cat_dqn_policy(dueling):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_cat_dqn_policy import AtariCatDqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    policy, spec = _make(dueling=dueling)
    flat = policy.get_param_values()
    pos = np.cumsum([0] + [int(np.prod(s)) for s in policy._ref_shapes])
    keep = []
    for i, nm in enumerate(policy.param_short_names):
        if "sigma" in nm:
            flat[pos[i]:pos[i + 1]] = 0
        else:
            keep.append(flat[pos[i]:pos[i + 1]])
    policy.set_param_values(flat)
    policy.update_target()
    plain = AtariCatDqnPolicy(epsilon=0, n_atoms=N_ATOMS, dueling=dueling, **cnn_specs[0])
    plain.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)), device=DEV)
    plain.set_param_values(np.concatenate(keep))
    plain.update_target()
    plain.incorporate_z(np.linspace(-10, 10, N_ATOMS, dtype=np.float32))
    assert plain._atom_stride == policy._atom_stride
    rs = np.random.RandomState(4)
    obs = _obs(rs, 37)
    z = policy.z.double()
    for w_n, w_p, tag in ((None, None, ""), (policy._w_target, plain._w_target, "t")):
        a = _device_logits(policy, policy._logits(policy._scaled(obs), w=w_n, tag=tag)[0])
        p = _device_logits(plain, plain._logits(plain._scaled(obs), w=w_p, tag=tag)[0])
        qa, qp = (torch.softmax(a, dim=2) * z).sum(dim=2), (torch.softmax(p, dim=2) * z).sum(dim=2)
        assert torch.allclose(qa, qp, rtol=1e-5, atol=1e-6), (qa - qp).abs().max()
    np.testing.assert_array_equal(policy.greedy_actions(obs).cpu().numpy(), plain.greedy_actions(obs).cpu().numpy())
    policy.host_draws(1, 37)
    policy.set_step(0)
    onehot, _ = policy.prob_value(obs)
    np.testing.assert_array_equal(onehot.argmax(dim=1).cpu().numpy(), plain.greedy_actions(obs).cpu().numpy())


# ------------------------------------------------------------------------------------- graphs and acting
@pytest.mark.parametrize("dueling", [False, True])
def test_graph_replay_draws_fresh_noise_in_the_eager_sequence_and_acting_draws_no_host_randomness(dueling):
    policy, _ = _make(dueling=dueling)
    rs = np.random.RandomState(0)
    obs = _obs(rs, 8)

    def fwd():
        return policy._logits(policy._scaled(obs))[0]
    fwd()                                                                   # warm (scratch buffers) before capture
    c0 = int(policy._noise_state[1])
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph):
            out = fwd()
    torch.cuda.current_stream().wait_stream(s)
    assert int(policy._noise_state[1]) == c0
    graph.replay()
    y1 = out.clone()
    graph.replay()
    y2 = out.clone()
    assert int(policy._noise_state[1]) == c0 + 2 and not torch.equal(y1, y2)
    policy._noise_state[1] = c0
    assert torch.equal(fwd(), y1)
    assert torch.equal(fwd(), y2)
    # acting: no epsilon, no np.random draw, and the noise explores
    assert policy.get_epsilon() == 0
    policy.set_epsilon(0.5)
    assert policy.get_epsilon() == 0
    flat = policy.get_param_values()
    pos = np.cumsum([0] + [int(np.prod(s)) for s in policy._ref_shapes])
    for i, nm in enumerate(policy.param_short_names):
        if "sigma" in nm:
            flat[pos[i]:pos[i + 1]] *= 10
    policy.set_param_values(flat)
    obs = _obs(rs, 64)
    np.random.seed(3)
    before = np.random.get_state()
    draws = policy.host_draws(4, 64)
    policy.set_step(0)
    a1 = policy.prob_value(obs)[0].argmax(dim=1).cpu().numpy()
    a2 = policy.prob_value(obs)[0].argmax(dim=1).cpu().numpy()
    acts, _ = policy.get_actions(obs)
    policy.get_action(obs[0])
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert draws.shape == (4 * 64,) and acts.shape == (64,)
    assert (a1 != a2).any()


# ------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("algo_kind,common", [("rainbow", False), ("rainbow", True), ("cat_dqn", False)])
def test_rainbow_trains_with_prioritized_replay_and_eval(algo_kind, common):
    """As test_noisy_net_gpu.test_noisy_dqn_trains_with_prioritized_replay_and_eval: captured rollout and update graphs,
    prioritized replay, 3-step returns; losses finite, the sigmas move, the dueling masks hold, two seeded runs agree bit
    for bit.  cat_dqn: CategoricalDQN (single DQN, no dueling) with the same policy class."""
    from accel_rl_amd.algos.dqn.cat_dqn import CategoricalDQN
    from accel_rl_amd.algos.dqn.rainbow import Rainbow
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_noisy_net_cat_dqn_policy import AtariNoisyNetCatDqnPolicy
    from accel_rl_amd.runners.accel_rl import AccelRLEval
    from accel_rl_amd.sampler.gpu_sampler_with_eval import GpuVecEvalSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    dueling = algo_kind == "rainbow"
    finals = []
    for _ in range(2):
        sampler = GpuVecEvalSampler(eval_steps=8 * 40, eval_envs_per=1, EnvCls=SynthAtariEnv,
                                    env_args=dict(game="seaquest"), horizon=4, n_parallel=4, envs_per=2,
                                    max_path_length=25, max_decorrelation_steps=0, device=DEV)
        args = dict(batch_size=32, min_steps_learn=64 * 4, replay_size=64 * 60, training_intensity=8,
                    target_update_steps=64 * 3)
        if dueling:
            algo = Rainbow(**args)
        else:
            algo = CategoricalDQN(reward_horizon=3, prioritized_replay=True, **args)
        policy = AtariNoisyNetCatDqnPolicy(dueling=dueling, common_noise=common, **cnn_specs[0])
        runner = AccelRLEval(algo=algo, policy=policy, sampler=sampler, n_steps=64 * 24, seed=9,
                             eval_interval_steps=64 * 8)
        runner.train()
        tab = runner.last_tabular
        assert np.isfinite(tab["LossAverage"]) and tab["LossAverage"] > 0 and tab["TrajsInEval"] > 0
        assert policy.get_epsilon() == 0
        flat = policy.get_param_values()
        pos = np.cumsum([0] + [int(np.prod(s)) for s in policy._ref_shapes])
        for nm in ("FC0Wsigma", "OutputWsigma") + (("FCVal0Wsigma", "ValWsigma") if dueling else ()):
            i = policy.param_short_names.index(nm)
            fan = policy._ref_shapes[i][0]
            assert (flat[pos[i]:pos[i + 1]] != np.float32(0.4 / np.sqrt(fan))).any(), nm
        if dueling:
            for k in (policy._k_head, policy._k_out_sigma):
                assert not (policy.params[k].detach() * (1 - policy._duel_mask)).any()
        finals.append(flat)
    np.testing.assert_array_equal(finals[0], finals[1])
