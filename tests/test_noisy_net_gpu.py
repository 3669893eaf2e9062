"""Noisy-net DQN on the device (csrc/noisy.hip, accel_rl_amd/policies/dqn/atari_noisy_net_dqn_policy.py) against
restatements of the reference (policies/dqn/layers/noisy_layer.py:15-147, networks/noisy_net_dqn_cnn.py:11-137,
atari_noisy_net_dqn_policy.py:20-148): the generator against its numpy statement, one noisy dense layer forward and
backward against float64 autograd with the noise read back, the parameter layout and initial draws, a training step
against autograd through a plain-torch noisy network fed with the noise the passes used, the sigma = 0 limit against
AtariDqnPolicy, exploration without epsilon, and end-to-end training under captured graphs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_dqn_gpu import ref_q_loss
from test_noisy_net_host import noisy_words_normals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tol(want, k_red):                  # tests/test_mfma_conv_gpu.py's tolerance for the dense contractions
    return 2e-5 * np.sqrt(k_red) * max(want.abs().max().item(), 1e-6)


def _make(n_act=6, spec_no=0, seed=5, **kw):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_noisy_net_dqn_policy import AtariNoisyNetDqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(seed)
    spec = dict(cnn_specs[spec_no])
    policy = AtariNoisyNetDqnPolicy(**spec, **kw)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(n_act)), device=DEV)
    return policy, spec


def _obs(rs, b):
    return torch.from_numpy(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)).to(DEV)


# ---------------------------------------------------------------------------------------------- generator
def test_device_generator_equals_numpy_statement():
    from accel_rl_amd import _lib
    _lib.load()
    for seed, counter, layer, which, rows, width, rpd in ((1234, 5, 1, 0, 7, 37, 1), (99, 2 ** 33 + 7, 0, 1, 9, 6, 4),
                                                          (123455, 0, 3, 0, 3, 3136, 3)):
        e = torch.empty((rows, width), dtype=torch.float32, device=DEV)
        f = torch.empty_like(e)
        w = torch.empty((rows, width), dtype=torch.int32, device=DEV)
        _lib.noisy_normals(seed, counter, layer, which, rows, width, rpd, e=e, f=f, words=w)
        words, e_np, f_np = noisy_words_normals(seed, counter, layer, which, rows, width, rpd)
        np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), words)
        e_d = e.cpu().numpy()
        assert (np.abs(e_d - e_np) <= 1e-6 * np.maximum(1, np.abs(e_np))).all()
        np.testing.assert_allclose(f.cpu().numpy(), f_np, rtol=1e-6, atol=1e-6)


def test_generator_statistics_and_keys():
    from accel_rl_amd import _lib
    _lib.load()
    n_r, n_c = 1000, 1024
    e = torch.empty((n_r, n_c), dtype=torch.float32, device=DEV)
    _lib.noisy_normals(42, 0, 0, 0, n_r, n_c, 1, e=e)
    x = e.double().cpu().numpy().ravel()
    n = x.size
    assert abs(x.mean()) < 5 / np.sqrt(n)
    assert abs(x.var() - 1) < 5 * np.sqrt(2. / n)

    def draw(seed=42, counter=0, layer=0, which=0, rows=4, width=16, rpd=1):
        out = torch.empty((rows, width), dtype=torch.float32, device=DEV)
        _lib.noisy_normals(seed, counter, layer, which, rows, width, rpd, e=out)
        return out.cpu().numpy()
    base = draw()
    assert not np.array_equal(base[0], base[1])                              # rows
    for other in (draw(layer=1), draw(which=1), draw(counter=1), draw(seed=43)):
        assert not np.isclose(base, other).any()
    grouped = draw(rows=6, rpd=3)
    np.testing.assert_array_equal(grouped[0], grouped[2])                    # a group shares its draw
    assert not np.array_equal(grouped[2], grouped[3])


def test_counter_advances_once_per_pass_and_graph_replays_draw_fresh_noise():
    policy, _ = _make()
    rs = np.random.RandomState(0)
    obs, nxt = _obs(rs, 8), _obs(rs, 8)
    assert policy._noise_state.cpu().tolist() == [policy.noise_seed, 0]
    policy.q(obs)
    assert int(policy._noise_state[1]) == 1
    z = torch.zeros(8, dtype=torch.float32, device=DEV)
    act = torch.zeros(8, dtype=torch.uint8, device=DEV)
    policy.q_loss_and_grads(obs, nxt, act, z, act, None, 0.99, 1.0, double_dqn=True)        # target + one 2B pass
    assert int(policy._noise_state[1]) == 3
    policy.q_loss_and_grads(obs, nxt, act, z, act, None, 0.99, 1.0, double_dqn=False)       # target + online
    assert int(policy._noise_state[1]) == 5
    policy.q(obs)                                                            # warm (scratch buffers) before capture
    c0 = int(policy._noise_state[1])
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph):
            out = policy.q(obs)
    torch.cuda.current_stream().wait_stream(s)
    assert int(policy._noise_state[1]) == c0                                  # capturing launches nothing
    graph.replay()
    y1 = out.clone()
    graph.replay()
    y2 = out.clone()
    assert int(policy._noise_state[1]) == c0 + 2
    assert not torch.equal(y1, y2)
    policy._noise_state[1] = c0
    assert torch.equal(policy.q(obs), y1)
    assert torch.equal(policy.q(obs), y2)


# ------------------------------------------------------------------------------------- one noisy dense layer
def _layer_case(fan, units, stride, relu, b, rpd, route, seed):
    from accel_rl_amd import _lib
    gen = torch.Generator(device="cpu").manual_seed(seed)

    def rnd(*shape, scale=1.):
        return (torch.randn(*shape, generator=gen) * scale).to(DEV)
    w, ws = rnd(stride, fan, scale=fan ** -0.5), rnd(stride, fan, scale=0.4 * fan ** -0.5)
    bias, bs = rnd(stride, scale=0.1), rnd(stride, scale=0.1)
    for t in (w, ws, bias, bs):
        t[units:] = 0
    x = torch.relu(rnd(b, fan))
    state = torch.tensor([seed + 17, 3], dtype=torch.int64, device=DEV)
    fein, feout, xs = (torch.empty((b, n), device=DEV) for n in (fan, stride, fan))
    _lib.noisy_noise(state, [(fein, feout, x, xs, fan, units, stride, 2)], b, rpd)
    geom = _lib.dense_geom(b, fan, stride, route)
    ws1, ws2 = _lib.conv_workspace(DEV), _lib.conv_workspace(DEV)
    yw, ys, y = (torch.empty((b, stride), device=DEV) for _ in range(3))
    it_w = _lib.conv2d_fwd_parts(x, w, bias, yw, geom, False, ws1)
    it_s = _lib.conv2d_fwd_parts(xs, ws, bs, ys, geom, False, ws2)
    _lib.noisy_dense_combine(it_w, bias, it_s, bs, feout, y, relu, state=state)
    assert int(state[1]) == 4
    g = rnd(b, stride)
    g[:, units:] = 0
    if relu:
        g *= (y > 0).float()
    g2, dxw, dxs = torch.empty_like(g), torch.empty_like(x), torch.empty_like(x)
    dw, dws = torch.zeros_like(w), torch.zeros_like(ws)
    db, dbs = torch.empty(stride, device=DEV), torch.empty(stride, device=DEV)
    folds = _lib.FoldList()
    fws = (_lib.conv_workspace(DEV), _lib.conv_workspace(DEV))       # the partials stay live until folds.run()
    _lib.noisy_dense_bwd_prep(g, feout, g2, db, dbs)
    folds.conv2d_bwd_pair(g, w, x, dxw, x, dw, geom, fws[0])
    folds.conv2d_bwd_pair(g2, ws, x, dxs, xs, dws, geom, fws[1])
    _lib.noisy_dense_bwd_dx(dxw, dxs, fein, dxw)
    folds.run()
    torch.cuda.synchronize()
    # float64 autograd with the noise the launch drew
    fe_i, fe_o = fein.double(), feout.double()
    np.testing.assert_array_equal(fe_o[:, units:].cpu().numpy(), 0)
    if rpd > 1:
        assert torch.equal(fe_i[0], fe_i[min(rpd, b) - 1]) and torch.equal(fe_o[0], fe_o[min(rpd, b) - 1])
    P = [t.double().requires_grad_() for t in (w, bias, ws, bs, x)]
    z = P[4] @ P[0].T + P[1] + fe_o * ((P[4] * fe_i) @ P[2].T + P[3])
    want_y = torch.relu(z) if relu else z
    gw, gb, gws, gbs, gx = torch.autograd.grad(z, P, grad_outputs=g.double())
    gx = gx * (x > 0).double()
    assert (y.double() - want_y).abs().max().item() <= _tol(want_y, 2 * fan)
    assert (dw.double() - gw).abs().max().item() <= _tol(gw, b)
    assert (dws.double() - gws).abs().max().item() <= _tol(gws, b)
    assert (db.double() - gb).abs().max().item() <= _tol(gb, b)
    assert (dbs.double() - gbs).abs().max().item() <= _tol(gbs, b)
    assert (dxw.double() - gx).abs().max().item() <= _tol(gx, 2 * stride)
    for t in (dws, dbs, dw, db):                               # the output layer's padding rows: exactly zero
        assert not t[units:].any()


@pytest.mark.parametrize("route", ["default", "fp32"])
@pytest.mark.parametrize("common", [False, True])
@pytest.mark.parametrize("shape", [(2592, 256, 256, True), (3136, 512, 512, True), (512, 6, 32, False)])
def test_noisy_dense_forward_backward_against_float64_autograd(shape, common, route):
    from accel_rl_amd import _lib
    _lib.load()
    fan, units, stride, relu = shape
    r = _lib.default_route if route == "default" else _lib.ROUTE_FP32
    for i, b in enumerate((1, 5, 32, 37, 64, 256)):
        _layer_case(fan, units, stride, relu, b, b if common else 1, r, seed=fan + units + i)


# ------------------------------------------------------------------------------------- layout and init
@pytest.mark.parametrize("mu_init", [True, False])
def test_layout_init_order_and_round_trip(mu_init):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_noisy_net_dqn_policy import AtariNoisyNetDqnPolicy
    policy, spec = _make(use_mu_init=mu_init, seed=11)
    # restatement: seed draw (np.random), Glorot conv weights (Lasagne's RNG), per noisy layer NormCInit (np.random) then
    # -- mu init -- uniform W, uniform b (Lasagne's RNG); sigmas sigma_0 / sqrt(fan_in)
    np.random.seed(11)
    lrng = np.random.RandomState(11)
    noise_seed = np.random.randint(1, 123456)
    ref, c, h, w = [], 4, 104, 80
    for nf, sz, st, pad in zip(spec["conv_filters"], spec["conv_filter_sizes"], spec["conv_strides"], spec["conv_pads"]):
        fan_in, fan_out = c * sz * sz, nf * sz * sz
        a = np.sqrt(6. / (fan_in + fan_out))
        ref += [lrng.uniform(-a, a, (nf, c, sz, sz)).astype(np.float32), np.zeros(nf, np.float32)]
        h, w, c = (h + 2 * pad[0] - sz) // st + 1, (w + 2 * pad[1] - sz) // st + 1, nf
    fan, count = c * h * w, sum(x.size for x in ref)
    for units, norm in [(hs, 1.0) for hs in spec["hidden_sizes"]] + [(6, 0.01)]:
        wn = np.random.randn(fan, units).astype(np.float32)
        wn *= norm / np.sqrt(np.square(wn).sum(axis=0, keepdims=True))
        bb = np.zeros(units, np.float32)
        if mu_init:
            v = np.sqrt(1 / fan)
            wn = lrng.uniform(-v, v, (fan, units)).astype(np.float32)
            bb = lrng.uniform(-v, v, units).astype(np.float32)
        s = np.float32(0.4 / np.sqrt(fan))
        ref += [wn, bb, np.full((fan, units), s, np.float32), np.full(units, s, np.float32)]
        count += 2 * (fan * units + units)
        fan = units
    assert policy.noise_seed == noise_seed and int(policy._noise_state[0]) == noise_seed
    assert policy.n_params == count
    flat = policy.get_param_values()
    np.testing.assert_array_equal(flat, np.concatenate([x.ravel() for x in ref]))
    assert policy.param_short_names[-8:] == ["FC0W", "FC0b", "FC0Wsigma", "FC0bsigma", "OutputW", "Outputb",
                                             "OutputWsigma", "Outputbsigma"]
    scaled = flat * np.float32(1.5) + np.float32(0.25)
    policy.set_param_values(scaled)
    np.testing.assert_array_equal(policy.get_param_values(), scaled)
    wq = policy._shapes[policy._k_head]                       # the padded output rows stay zero
    assert wq[0] == 32 and not policy.params[policy._k_out_sigma][6:].any() and not policy.params[policy._k_head][6:].any()
    with pytest.raises(NotImplementedError):
        AtariNoisyNetDqnPolicy(factorized=False, **cnn_specs[0])


# ------------------------------------------------------------------------------------- a training step
def _ref_noisy(rp, spec, x, noise, n_conv):
    """Reference-layout noisy network in plain torch; noise: per noisy layer (f(e_in) in the reference's input order,
    f(e_out))."""
    k = 0
    for i in range(n_conv):
        x = F.relu(F.conv2d(x, rp[k].flip(2, 3), rp[k + 1], stride=spec["conv_strides"][i],
                            padding=tuple(spec["conv_pads"][i])))
        k += 2
    x = x.flatten(1)
    for l, (fi, fo) in enumerate(noise):
        z = x @ rp[k] + rp[k + 1] + fo * ((x * fi) @ rp[k + 2] + rp[k + 3])
        x = z if l == len(noise) - 1 else F.relu(z)
        k += 4
    return x


def _pass_noise(policy, counter, rows, rpd, first, count):
    """The noise a pass of `rows` rows at `counter` used, rows [first, first + count), in the reference's input order."""
    from accel_rl_amd import _lib
    co, ho, wo = policy._conv_out
    out = []
    dims = [(fan_in, hs) for hs, fan_in in policy._hid_geom] + [(policy._hid_geom[-1][0], policy.n_act)]
    for l, (fan_in, units) in enumerate(dims):
        fi = torch.empty((rows, fan_in), device=DEV)
        fo = torch.empty((rows, units), device=DEV)
        _lib.noisy_normals(policy.noise_seed, counter, l, 0, rows, fan_in, rpd, f=fi)
        _lib.noisy_normals(policy.noise_seed, counter, l, 1, rows, units, rpd, f=fo)
        fi, fo = fi[first:first + count], fo[first:first + count]
        if l == 0:                                                            # internal (h, w, c) -> (c, h, w)
            fi = fi.reshape(count, ho, wo, co).permute(0, 3, 1, 2).reshape(count, -1)
        out.append((fi, fo))
    return out


def _ref_params(policy, flat_bucket):
    flat = policy.bucket_to_reference(flat_bucket)
    out, pos = [], 0
    for shape in policy._ref_shapes:
        n = int(np.prod(shape))
        out.append(torch.from_numpy(flat[pos:pos + n].reshape(shape).copy()).to(DEV).requires_grad_())
        pos += n
    return out


@pytest.mark.parametrize("common", [False, True])
@pytest.mark.parametrize("double", [False, True])
def test_training_step_matches_autograd_with_the_pass_noise(double, common):
    policy, spec = _make(common_noise=common)
    rs = np.random.RandomState(3)
    b = 32
    obs, nxt = _obs(rs, b), _obs(rs, b)
    act = torch.from_numpy(rs.randint(0, 6, size=b).astype(np.uint8)).to(DEV)
    ret = torch.from_numpy((rs.randn(b) * 0.02).astype(np.float32)).to(DEV)
    term = torch.from_numpy((rs.rand(b) < 0.2).astype(np.uint8)).to(DEV)
    isw = torch.from_numpy((rs.rand(b) + 0.2).astype(np.float32)).to(DEV)
    policy.flat_target.copy_(policy.flat_params * 0.9)
    gamma_n = float(np.float32(0.99))
    c0 = int(policy._noise_state[1])
    rows, td = policy.q_loss_and_grads(obs, nxt, act, ret, term, isw, gamma_n, 0.01, double_dqn=double)
    got = policy.bucket_to_reference(policy.flat_grads)
    n_conv = len(spec["conv_filters"])
    tgt_noise = _pass_noise(policy, c0, b, b if common else 1, 0, b)
    if double:                                    # the online network's obs + next_obs pass: 2B rows, two calls
        on_noise = _pass_noise(policy, c0 + 1, 2 * b, b if common else 1, 0, b)
        nx_noise = _pass_noise(policy, c0 + 1, 2 * b, b if common else 1, b, b)
    else:
        on_noise = _pass_noise(policy, c0 + 1, b, b if common else 1, 0, b)
    rp, rt = _ref_params(policy, policy.flat_params), _ref_params(policy, policy.flat_target)
    scale = np.float32(1. / 255)
    q = _ref_noisy(rp, spec, obs.float() * scale, on_noise, n_conv)
    with torch.no_grad():
        tgt = _ref_noisy(rt, spec, nxt.float() * scale, tgt_noise, n_conv)
        pol = _ref_noisy(rp, spec, nxt.float() * scale, nx_noise, n_conv) if double else None
    loss, td_ref = ref_q_loss(q, tgt, pol, act, ret, term, isw, gamma_n, 0.01)
    grads = torch.autograd.grad(loss, rp)
    want = np.concatenate([g.detach().cpu().numpy().reshape(-1) for g in grads])
    assert abs(rows.sum().item() - loss.item()) <= 1e-4 * abs(loss.item())
    assert torch.allclose(td, td_ref, rtol=2e-3, atol=1e-6)
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * max(np.abs(want).max(), 1e-3)), np.abs(got - want).max()
    n_sig = [i for i, nm in enumerate(policy.param_short_names) if "sigma" in nm]
    pos = np.cumsum([0] + [int(np.prod(s)) for s in policy._ref_shapes])
    assert all(np.abs(got[pos[i]:pos[i + 1]]).max() > 0 for i in n_sig)           # the sigmas learn


# ------------------------------------------------------------------------------------- sigma = 0 limit
def test_zero_sigma_equals_plain_dqn_policy():
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    policy, spec = _make()
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
    plain = AtariDqnPolicy(epsilon=0, **cnn_specs[0])
    plain.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)), device=DEV)
    plain.set_param_values(np.concatenate(keep))
    plain.update_target()
    rs = np.random.RandomState(4)
    obs = _obs(rs, 37)
    for a, b in ((policy.q(obs), plain.q(obs)), (policy.target_q(obs), plain.target_q(obs))):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), (a - b).abs().max()
    np.testing.assert_array_equal(policy.greedy_actions(obs).cpu().numpy(), plain.greedy_actions(obs).cpu().numpy())
    policy.host_draws(1, 37)
    policy.set_step(0)
    onehot, _ = policy.prob_value(obs)
    np.testing.assert_array_equal(onehot.argmax(dim=1).cpu().numpy(), plain.greedy_actions(obs).cpu().numpy())


# ------------------------------------------------------------------------------------- exploration
def test_exploration_without_epsilon():
    policy, _ = _make()
    assert policy.get_epsilon() == 0
    policy.set_epsilon(0.5)
    assert policy.get_epsilon() == 0
    flat = policy.get_param_values()
    pos = np.cumsum([0] + [int(np.prod(s)) for s in policy._ref_shapes])
    for i, nm in enumerate(policy.param_short_names):
        if "sigma" in nm:
            flat[pos[i]:pos[i + 1]] *= 10
    policy.set_param_values(flat)
    rs = np.random.RandomState(5)
    obs = _obs(rs, 64)
    np.random.seed(3)
    before = np.random.get_state()
    draws = policy.host_draws(4, 64)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert draws.shape == (4 * 64,)
    policy.set_step(0)
    a1 = policy.prob_value(obs)[0].argmax(dim=1).cpu().numpy()
    a2 = policy.prob_value(obs)[0].argmax(dim=1).cpu().numpy()
    assert (a1 != a2).any()
    acts, _ = policy.get_actions(obs)
    assert np.array_equal(np.random.get_state()[1], after[1])
    assert acts.shape == (64,)


# ------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("common", [False, True])
def test_noisy_dqn_trains_with_prioritized_replay_and_eval(common):
    """As test_dqn_gpu.test_dqn_trains_with_prioritized_replay_and_eval, with the noisy-net policy: captured rollout and
    update graphs; the sigmas move; two seeded runs agree bit for bit."""
    from accel_rl_amd.algos.dqn.dqn import DQN
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_noisy_net_dqn_policy import AtariNoisyNetDqnPolicy
    from accel_rl_amd.runners.accel_rl import AccelRLEval
    from accel_rl_amd.sampler.gpu_sampler_with_eval import GpuVecEvalSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    finals = []
    for _ in range(2):
        sampler = GpuVecEvalSampler(eval_steps=8 * 40, eval_envs_per=1, EnvCls=SynthAtariEnv,
                                    env_args=dict(game="seaquest"), horizon=4, n_parallel=4, envs_per=2,
                                    max_path_length=25, max_decorrelation_steps=0, device=DEV)
        algo = DQN(batch_size=32, min_steps_learn=64 * 4, replay_size=64 * 60, training_intensity=8,
                   target_update_steps=64 * 3, reward_horizon=3, prioritized_replay=True, double_dqn=True,
                   eps_greedy_args=dict(anneal_steps=64 * 10))
        policy = AtariNoisyNetDqnPolicy(common_noise=common, **cnn_specs[0])
        runner = AccelRLEval(algo=algo, policy=policy, sampler=sampler, n_steps=64 * 24, seed=9,
                             eval_interval_steps=64 * 8)
        runner.train()
        tab = runner.last_tabular
        assert np.isfinite(tab["LossAverage"]) and tab["LossAverage"] > 0 and tab["TrajsInEval"] > 0
        assert policy.get_epsilon() == 0
        flat = policy.get_param_values()
        i = policy.param_short_names.index("FC0Wsigma")
        pos = np.cumsum([0] + [int(np.prod(s)) for s in policy._ref_shapes])
        fan = policy._ref_shapes[i][0]
        assert (flat[pos[i]:pos[i + 1]] != np.float32(0.4 / np.sqrt(fan))).any()
        finals.append(flat)
    np.testing.assert_array_equal(finals[0], finals[1])
