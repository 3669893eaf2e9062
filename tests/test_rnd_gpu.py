"""RND on the device: the four entry points of csrc/rnd.hip against the restatements of tests/rnd_ref.py (bit for bit,
inside NaN guard bands; refusals leave the fill), RndNetwork's predictor gradient against float64 autograd of the same
graph, and RndPPO / RndA2C on the synthetic env -- replayed against eager, passes against one pass, the bonus switched
off against plain PPO."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rnd_ref
import test_resnet_gpu as trg
from test_head_limits_gpu import _nan, _untouched
from test_ppg_gpu import _assert_same_run, _whole_step_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan64(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


def _rollout(rs, n, t, c, h, w):
    """observations and extra_observations that disagree everywhere, every plane different; 0 and 255 present"""
    obs = rs.randint(0, 256, size=(n * t, c, h, w), dtype=np.uint8)
    extra = rs.randint(0, 256, size=(n, c, h, w), dtype=np.uint8)
    obs[-1, c - 1].flat[0], extra[0, c - 1].flat[0] = 255, 0
    obs[-1, c - 1].flat[-1], extra[0, c - 1].flat[-1] = 0, 255
    return obs, extra


# ---- arl_rnd_obs_stats ---------------------------------------------------------------------------------------------------

STATS_SHAPES = [(1, 1, 1, 1, 1), (3, 2, 4, 5, 7), (5, 3, 2, 104, 80)]


@pytest.mark.parametrize("shape", STATS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_obs_stats_two_calls_bit_for_bit(L, shape):
    n, t, c, h, w = shape
    rs = np.random.RandomState(sum(shape))
    hw = h * w
    ws = L.rnd_obs_stats_workspace(h, w, DEV)
    count, mean, m2 = _nan64(3), _nan64(hw + 2), _nan64(hw + 2)
    count[1], mean[1:hw + 1], m2[1:hw + 1] = 0., 0., 0.
    ref = (0., np.zeros(hw), np.zeros(hw))
    for call in range(2):
        obs, extra = _rollout(rs, n, t, c, h, w)
        if hw > 2:
            obs[:, :, 0, 1], extra[:, :, 0, 1] = 9, 9                    # a constant pixel
        L.rnd_obs_stats(_dev(obs), _dev(extra), n, t, count[1:2], mean[1:hw + 1], m2[1:hw + 1], ws)
        torch.cuda.synchronize()
        frames = rnd_ref.next_frames(obs, extra, n, t)
        if t > 1 and c > 1:     # the NEXT observation's NEWEST plane: neither this row's frame nor an older plane
            assert not np.array_equal(frames[0], obs[0, c - 1]) and not np.array_equal(frames[0], obs[1, 0])
            assert np.array_equal(frames[0], obs[1, c - 1]) and np.array_equal(frames[t - 1], extra[0, c - 1])
        ref = rnd_ref.obs_stats(frames, *ref)
        _same_bits(count[1:2].cpu().numpy(), np.array([ref[0]]), "count %d" % call)
        _same_bits(mean[1:hw + 1].cpu().numpy(), ref[1], "mean %d" % call)
        _same_bits(m2[1:hw + 1].cpu().numpy(), ref[2], "m2 %d" % call)
        assert all(_untouched(x[:1]) and _untouched(x[-1:]) for x in (count, mean, m2))
    assert ref[0] == 2 * n * t
    if hw > 2:
        assert ref[2][1] == 0 and ref[1][1] == 9


def test_obs_stats_and_prepare_refusals_leave_the_fill(L):
    lib = L.load()
    obs, extra = (_dev(a) for a in _rollout(np.random.RandomState(0), 2, 3, 4, 5, 6))
    ws = L.rnd_obs_stats_workspace(5, 6, DEV)
    count, mean, m2, out = _nan64(1), _nan64(30), _nan64(30), _nan(6, 5, 6, 4)
    s = L.stream_ptr()
    a = lambda x: x.data_ptr()                                                                  # noqa: E731
    assert lib.arl_rnd_obs_stats(a(obs), a(extra), 0, 3, 4, 5, 6, a(count), a(mean), a(m2), a(ws), s) == -2
    assert lib.arl_rnd_obs_stats(a(obs), a(extra), 2, 4097, 4, 5, 6, a(count), a(mean), a(m2), a(ws), s) == -2
    assert lib.arl_rnd_obs_stats(a(obs), None, 2, 3, 4, 5, 6, a(count), a(mean), a(m2), a(ws), s) == -1
    assert lib.arl_rnd_obs_stats(a(obs), a(extra), 2, 3, 4, 5, 6, a(count), a(mean) + 4, a(m2), a(ws), s) == -3
    assert lib.arl_rnd_obs_prepare(a(obs), a(extra), None, 7, 2, 3, 4, 5, 6, a(count), a(mean), a(m2), a(out), s) == -2
    assert lib.arl_rnd_obs_prepare(a(obs), a(extra), None, 6, 2, 3, 4, 5, 6, a(count), None, a(m2), a(out), s) == -1
    assert lib.arl_rnd_obs_prepare(a(obs), a(extra), None, 6, 2, 3, 4, 5, 6, a(count), a(mean), a(m2), a(out) + 4, s) == -3
    torch.cuda.synchronize()
    assert all(_untouched(x) for x in (count, mean, m2, out))


# ---- arl_rnd_obs_prepare -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "rows"])
@pytest.mark.parametrize("shape", STATS_SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_obs_prepare_bit_for_bit(L, shape, with_idx):
    n, t, c, h, w = shape
    rs = np.random.RandomState(sum(shape) + with_idx)
    hw = h * w
    obs, extra = _rollout(rs, n, t, c, h, w)
    obs[:, :, 0, 1], extra[:, :, 0, 1] = 9, 9                            # zero variance -> exactly 0
    frames = rnd_ref.next_frames(obs, extra, n, t)
    count, mean, m2 = rnd_ref.obs_stats(frames, 0., np.zeros(hw), np.zeros(hw))
    more = rs.randint(0, 256, size=(7, h, w), dtype=np.uint8)               # a second batch: a merged state
    more[:, 0, 1] = 9
    count, mean, m2 = rnd_ref.obs_stats(more, count, mean, m2)
    # pixel (0, 2): a tight state around 100, so that 255 lands beyond +5 and 0 beyond -5
    mean[2], m2[2] = 100.25, 4.0 * count
    obs[:, c - 1, 0, 2], extra[:, c - 1, 0, 2] = 255, 0
    frames = rnd_ref.next_frames(obs, extra, n, t)
    rows = rs.permutation(n * t)[:max(n * t - 2, 1)].astype(np.int32) if with_idx else np.arange(n * t, dtype=np.int32)
    want = rnd_ref.obs_prepare(frames[rows], count, mean, m2)
    z = (frames[rows][:, 0, 2].astype(F64) - mean[2]) / np.sqrt(m2[2] / count + 1e-8)
    assert (z > 5).any() and (z < -5).any() and set(np.unique(want[:, 0, 2, 0])) == {-5., 5.}
    assert (want[:, 0, 1, 0] == 0).all() and np.abs(want[..., 0]).max() == 5
    b = rows.size
    out = _nan(b + 2, h, w, 4)
    L.rnd_obs_prepare(_dev(obs), _dev(extra), _dev(rows) if with_idx else None, n, t, _dev(np.array([count])), _dev(mean),
                      _dev(m2), out[1:b + 1])
    torch.cuda.synchronize()
    got = out[1:b + 1].cpu().numpy()
    assert _untouched(out[0]) and _untouched(out[-1])
    assert (got[..., 1:] == 0).all() and not np.signbit(got[..., 1:]).any()
    _same_bits(got[..., 0], want[..., 0], "channel 0")


# ---- arl_rnd_error -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("e", [4, 64, 512, 1024])
@pytest.mark.parametrize("b", [1, 3, 4, 5, 257])
def test_error_bit_for_bit(L, b, e):
    rs = np.random.RandomState(1000 * b + e)
    pred, targ = rs.randn(b, e).astype(F32), rs.randn(b, e).astype(F32)
    pred[0, 0] = targ[0, 0]                                              # a zero difference
    pd, td = _dev(pred), _dev(targ)
    want_err, want_d, want_loss = rnd_ref.error(pred, targ, True)
    runs = []
    for _ in range(2):
        err, dpred, loss = _nan(b + 2), _nan(b + 2, e), _nan(3)
        L.rnd_error(pd, td, err[1:b + 1], dpred[1:b + 1], loss[1:2])
        torch.cuda.synchronize()
        assert all(_untouched(x[:1]) and _untouched(x[-1:]) for x in (err, dpred, loss))
        runs.append((err[1:b + 1].cpu().numpy(), dpred[1:b + 1].cpu().numpy(), loss[1:2].cpu().numpy()))
    for k, what in enumerate(("err", "dpred", "loss")):
        _same_bits(runs[0][k], runs[1][k], what + " twice")
    _same_bits(runs[0][0], want_err, "err")
    _same_bits(runs[0][1], want_d, "dpred")
    _same_bits(runs[0][2], np.array([want_loss]), "loss")
    # without the gradient: err alone, dpred and loss untouched
    err, dpred, loss = _nan(b + 2), _nan(b, e), _nan(1)
    assert L.load().arl_rnd_error(pd.data_ptr(), td.data_ptr(), b, e, 0, err[1:].data_ptr(), dpred.data_ptr(),
                                  loss.data_ptr(), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    _same_bits(err[1:b + 1].cpu().numpy(), want_err, "err alone")
    assert _untouched(dpred) and _untouched(loss) and _untouched(err[:1]) and _untouched(err[-1:])


def test_error_and_mix_refusals_leave_the_fill(L):
    lib = L.load()
    pred, targ = torch.randn(3, 64, device=DEV), torch.randn(3, 64, device=DEV)
    err, dpred, loss = _nan(4), _nan(3, 64), _nan(1)
    s = L.stream_ptr()
    a = lambda x: x.data_ptr()                                                                  # noqa: E731
    assert lib.arl_rnd_error(a(pred), a(targ), 3, 62, 1, a(err), a(dpred), a(loss), s) == -2
    assert lib.arl_rnd_error(a(pred), a(targ), 0, 64, 1, a(err), a(dpred), a(loss), s) == -2
    assert lib.arl_rnd_error(a(pred), a(targ), 3, 64, 1, a(err), None, a(loss), s) == -1
    assert lib.arl_rnd_error(a(pred) + 4, a(targ), 3, 64, 1, a(err), a(dpred), a(loss), s) == -3
    r_ext, r_mix, diag = torch.randn(4, device=DEV), _nan(4), _nan(2)
    rho, mom, ws = _nan64(2), _nan64(3), _nan64(4)
    mix = lambda *x: lib.arl_rnd_reward_mix(*x)                                                 # noqa: E731
    assert mix(a(err), a(r_ext), 2, 2, a(rho), a(mom), 1.5, 1., 1., a(r_mix), a(diag), a(ws), s) == -1
    assert mix(a(err), a(r_ext), 2, 2, a(rho), a(mom), 0.99, 1., 1., a(r_ext), a(diag), a(ws), s) == -1
    assert mix(a(err), a(r_ext), 0, 2, a(rho), a(mom), 0.99, 1., 1., a(r_mix), a(diag), a(ws), s) == -2
    assert mix(a(err), a(r_ext), 2, 4097, a(rho), a(mom), 0.99, 1., 1., a(r_mix), a(diag), a(ws), s) == -2
    assert mix(a(err), a(r_ext), 2, 2, a(rho) + 4, a(mom), 0.99, 1., 1., a(r_mix), a(diag), a(ws), s) == -3
    torch.cuda.synchronize()
    assert all(_untouched(x) for x in (err, dpred, loss, r_mix, diag, rho, mom, ws))


# ---- arl_rnd_reward_mix --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (256, 5), (1024, 20)], ids=lambda s: "%dx%d" % s)
def test_reward_mix_three_calls_bit_for_bit(L, shape):
    """The first call has every error equal (variance 0 for T = 1: the 1e-8 decides); calls two and three carry rho and
    the moments; the last has the bonus switched off and returns r_ext's bits."""
    n, t = shape
    rs = np.random.RandomState(n + t)
    rho, mom, ws = _nan64(n + 2), _nan64(5), torch.zeros(n * t, dtype=torch.float64, device=DEV)
    rho[1:n + 1], mom[1:4] = 0., 0.
    ref_rho, ref_mom = np.zeros(n), np.zeros(3)
    for call, (gamma, c_ext, c_int) in enumerate(((0., 2., 1.), (0.99, 2., 0.5), (0.99, 1., 0.))):
        err = np.full((n, t), 0.375, F32) if call == 0 else (rs.rand(n, t) * 2).astype(F32)
        r_ext = rs.randn(n, t).astype(F32)
        r_ext.flat[0] = F32(-0.0)
        r_mix, diag = _nan(n * t + 2), _nan(4)
        L.rnd_reward_mix(_dev(err), _dev(r_ext), n, t, rho[1:n + 1], mom[1:4], gamma, c_ext, c_int, r_mix[1:n * t + 1],
                         diag[1:3], ws)
        torch.cuda.synchronize()
        want, ref_rho, ref_mom, want_diag = rnd_ref.reward_mix(err, r_ext, ref_rho, ref_mom, gamma, c_ext, c_int)
        if call == 0:
            assert ref_mom[2] == 0 and want_diag[1] == F32(1e-4)        # gamma 0, equal errors: the 1e-8 alone
        _same_bits(r_mix[1:n * t + 1].cpu().numpy(), want.reshape(-1), "r_mix %d" % call)
        _same_bits(rho[1:n + 1].cpu().numpy(), ref_rho, "rho %d" % call)
        _same_bits(mom[1:4].cpu().numpy(), ref_mom, "moments %d" % call)
        _same_bits(diag[1:3].cpu().numpy(), want_diag, "diag %d" % call)
        assert all(_untouched(x[:1]) and _untouched(x[-1:]) for x in (r_mix, diag, rho, mom))
        if call == 2:
            _same_bits(r_mix[1:n * t + 1].cpu().numpy(), r_ext.reshape(-1), "the bonus switched off")
    assert ref_mom[0] == 3 * n * t


# ---- RndNetwork ------------------------------------------------------------------------------------------------------------

N_ENV, HORIZON = 4, 2


@functools.lru_cache(maxsize=None)
def _net_setup():
    from accel_rl_amd.policies.rnd_network import RndNetwork
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    net = RndNetwork(embedding_size=64, predictor_hidden=(64,), rnd_seed=4)
    net.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)), N_ENV, device=DEV)
    obs, extra = (_dev(a) for a in _rollout(np.random.RandomState(12), N_ENV, HORIZON, 4, 104, 80))
    net.update_obs_stats(obs, extra)
    return net, obs, extra


def _embed64(trunk, params, x):
    """The trunk as a float64 autograd graph on host copies of its internal parameter views; x f64 [B, 4, H, W]."""
    for i, (nf, ci, sz, st, pad, ho, wo) in enumerate(trunk._conv_geom):
        x = F.relu(F.conv2d(x, params[2 * i], params[2 * i + 1], stride=st, padding=pad))
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    k = 2 * trunk._n_conv
    for j in range(trunk._n_hid):
        x = F.linear(x, params[k], params[k + 1])
        x = F.relu(x) if j + 1 < trunk._n_hid else x
        k += 2
    return x


@pytest.mark.parametrize("b", [3, 8])
def test_predictor_gradient_matches_float64_autograd(b):
    net, obs, extra = _net_setup()
    idx = None if b == 8 else _dev(np.array([5, 0, 6], dtype=np.int32))
    pred_t = net.predictor
    pred_t.flat_grads.fill_(float("nan"))
    loss = net.loss_and_grads(obs, extra, idx).cpu().numpy()
    got = [g.detach().cpu().numpy().copy() for g in pred_t.grads]
    x = net._input(obs, extra, idx, b).clone()
    emb = pred_t._trunk(x)[1][-1].cpu().numpy()
    assert (emb > 0).any() and (emb < 0).any()          # both signs: a rectifier-masked bias sum would show
    frames = rnd_ref.next_frames(obs.cpu().numpy(), extra.cpu().numpy(), N_ENV, HORIZON)
    rows = np.arange(8) if idx is None else idx.cpu().numpy()
    state = net.rnd_state()
    _same_bits(x.cpu().numpy(), rnd_ref.obs_prepare(frames[rows], state["obs_count"][0], state["obs_mean"],
                                                     state["obs_m2"]), "the network's input")
    x64 = x.cpu().double().permute(0, 3, 1, 2)
    params = [p.detach().cpu().double().requires_grad_() for p in pred_t.params]
    with torch.no_grad():
        targ = _embed64(net.target, [p.detach().cpu().double() for p in net.target.params], x64)
    want_loss = ((_embed64(pred_t, params, x64) - targ) ** 2).mean()
    want = [g.numpy() for g in torch.autograd.grad(want_loss, params)]
    assert abs(loss[0] - want_loss.item()) <= 2e-3 * want_loss.item()
    scale = max(max(np.abs(g).max() for g in want), 1e-3)
    assert all(np.isfinite(g).all() for g in got)
    for k, (g, wv) in enumerate(zip(got, want)):
        assert np.abs(wv).max() > 0, k
        _whole_step_close(g, wv, scale, "B %d param %d" % (b, k))
    _whole_step_close(got[-1], want[-1], np.abs(want[-1]).max(), "the linear layer's bias gradient")


def test_predictor_learns_a_fixed_batch_and_the_target_stays():
    from accel_rl_amd.algos.pg.rnd import PredictorOptimizer
    from accel_rl_amd.optimizers import update_methods
    net, obs, extra = _net_setup()
    start = net.rnd_state()
    opt = PredictorOptimizer(1e-3, update_methods.adam)
    opt.initialize(net, 1)
    losses = []
    for k in range(40):
        losses.append(net.loss_and_grads(obs, extra).clone())
        opt.step()
        if k == 4:
            assert np.array_equal(_bits(net.rnd_state()["target"]), _bits(start["target"]))
    losses = torch.cat(losses).cpu().numpy()
    print("RndLoss first %.6g after 40 updates %.6g ratio %.4g" % (losses[0], losses[-1], losses[-1] / losses[0]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    end = net.rnd_state()
    assert np.array_equal(_bits(end["target"]), _bits(start["target"]))
    assert not np.array_equal(end["predictor"], start["predictor"]) and opt._step_count.item() == 40
    net.set_rnd_state(start)                                # (the cached network goes back as it came)


# ---- the algorithms --------------------------------------------------------------------------------------------------------

RND_ARGS = dict(embedding_size=64, predictor_hidden=(64,), rnd_seed=3)


def _train(cls, use_graph, n_itr, wrap=None, **kwargs):
    """`cls` on the synthetic pong, 8 envs x horizon 5, spec 0 with a 64-wide hidden layer.  wrap(algo, policy): called
    once initialize has run."""
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="pong"), horizon=5, n_parallel=2, envs_per=2,
                            max_path_length=25, max_decorrelation_steps=0, device=DEV)
    algo = cls(use_graph=use_graph, **kwargs)
    policy = AtariCnnPolicy(**dict(cnn_specs[0], hidden_sizes=[64]))
    log = dict(infos=[])
    initialize, optimize = algo.initialize, algo.optimize_policy

    def watching_initialize(*a, **kw):
        initialize(*a, **kw)
        log["first"] = policy.get_param_values()
        if wrap is not None:
            wrap(algo, policy)

    def recording_optimize(itr, samples):
        log["samples"] = samples
        out = optimize(itr, samples)
        log["infos"].append(out[1])
        return out
    algo.initialize, algo.optimize_policy = watching_initialize, recording_optimize
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=40 * (n_itr - 1), seed=9, log_interval_steps=40)
    runner.train()
    torch.cuda.synchronize()
    log["infos"] = [{k: trg._host(v).copy() for k, v in info.items()} for info in log["infos"]]
    return algo, policy, log


PPO_ARGS = dict(optimizer_args=dict(epochs=2, minibatch_size=20))


def test_rnd_ppo_trains_and_replayed_iterations_equal_eager_ones():
    """Six iterations: two eager, one captured, three replayed.  The same seeded run made eagerly ends in the same policy
    and predictor parameters, the same statistics, and returned the same diagnostics, bit for bit."""
    kw = dict(rnd_args=RND_ARGS, rnd_rows_per_pass=16, **PPO_ARGS)
    algo, policy, log = _train(_rnd_ppo(), True, 6, **kw)
    assert algo._graph is not None and len(log["infos"]) == 6
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, log["first"])
    assert algo._rnd_rows == 5 and algo._rnd_opt._step_count.item() == 6 * 4
    for info in log["infos"]:
        assert sorted(info) == ["GradNorm", "IntRewMean", "IntRewStd", "RndLoss"] and info["GradNorm"].shape == (4,)
        assert all(np.isfinite(v).all() for v in info.values())
        assert info["RndLoss"][0] > 0 and info["IntRewMean"][0] > 0 and info["IntRewStd"][0] > 0
    algo_e, policy_e, log_e = _train(_rnd_ppo(), False, 6, **kw)
    assert algo_e._graph is None
    _assert_same_run(log, policy, log_e, policy_e)
    state, state_e = algo.rnd.rnd_state(), algo_e.rnd.rnd_state()
    for k in state:
        assert np.array_equal(_bits(state[k]), _bits(state_e[k])), k
    assert state["obs_count"][0] == 6 * 40 and state["rew_moments"][0] == 6 * 40


def _rnd_ppo():
    from accel_rl_amd.algos.pg import RndPPO
    return RndPPO


@functools.lru_cache(maxsize=None)
def _watched_eager_run():
    """Two eager iterations of RndPPO with process_samples watched: what went in, what came out."""
    seen = []

    def wrap(algo, policy):
        inner = algo.process_samples

        def watched(itr, samples):
            before = dict(rewards=samples["rewards"].clone(), rho=algo.rnd.rho.clone(), mom=algo.rnd.rew_moments.clone())
            out = inner(itr, samples)
            seen.append(dict(before, err=algo._rnd_err.clone(), r_mix=algo._r_mix.clone(), diag=algo._rnd_diag.clone(),
                             rewards_after=samples["rewards"].clone(), rho_after=algo.rnd.rho.clone(),
                             mom_after=algo.rnd.rew_moments.clone()))
            return out
        algo.process_samples = watched
    algo, policy, log = _train(_rnd_ppo(), False, 2, wrap=wrap, rnd_args=RND_ARGS, **PPO_ARGS)
    return algo, log, seen


def test_bonus_pass_in_passes_of_two_rows_equals_one_pass():
    algo, log, _ = _watched_eager_run()
    one = algo.bonus_pass(log["samples"], None).clone()
    two = algo.bonus_pass(log["samples"], 2).clone()
    torch.cuda.synchronize()
    assert one.shape == (40,) and bool((one > 0).all())
    _same_bits(two.cpu().numpy(), one.cpu().numpy(), "passes of 2 rows")


def test_process_samples_mixes_by_the_restatement_and_leaves_the_rollout_alone():
    algo, log, seen = _watched_eager_run()
    assert len(seen) == 2
    for s in seen:
        h = {k: v.cpu().numpy() for k, v in s.items()}
        _same_bits(h["rewards_after"], h["rewards"], "the rollout's rewards")
        want, rho, mom, diag = rnd_ref.reward_mix(h["err"].reshape(8, 5), h["rewards"].reshape(8, 5), h["rho"], h["mom"],
                                                  algo.int_discount, algo.ext_coeff, algo.int_coeff)
        _same_bits(h["r_mix"], want.reshape(-1), "r_mix")
        _same_bits(h["rho_after"], rho, "rho")
        _same_bits(h["mom_after"], mom, "moments")
        _same_bits(h["diag"], diag, "diagnostics")
        assert (h["err"] > 0).all() and not np.array_equal(h["r_mix"], h["rewards"])


def test_rnd_ppo_with_the_bonus_switched_off_is_plain_ppo():
    from accel_rl_amd.algos.pg.ppo import PPO
    algo, policy, log = _train(_rnd_ppo(), True, 4, int_coeff=0., ext_coeff=1., rnd_args=RND_ARGS, **PPO_ARGS)
    algo_p, policy_p, log_p = _train(PPO, True, 4, **PPO_ARGS)
    assert np.array_equal(log["first"], log_p["first"])
    _same_bits(policy.get_param_values(), policy_p.get_param_values(), "policy parameters")
    for a, b in zip(log["infos"], log_p["infos"]):
        _same_bits(a["GradNorm"], b["GradNorm"], "GradNorm")
    assert not np.array_equal(policy.get_param_values(), log["first"])


def test_rnd_a2c_runs_on_the_whole_batch():
    from accel_rl_amd.algos.pg import RndA2C
    with pytest.raises(ValueError, match="update_proportion must be 1"):
        RndA2C(update_proportion=0.5)
    algo, policy, log = _train(RndA2C, True, 3, rnd_args=RND_ARGS)
    assert algo._rnd_rows == 40 and algo._rnd_opt._step_count.item() == 3 and len(log["infos"]) == 3
    assert not np.array_equal(policy.get_param_values(), log["first"])
    for info in log["infos"]:
        assert all(np.isfinite(v).all() for v in info.values()) and info["RndLoss"][0] > 0
