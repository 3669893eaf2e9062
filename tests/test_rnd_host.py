"""RND without a GPU: the restatements of tests/rnd_ref.py against plain NumPy, the constructors' and initialize's
refusals, the entry points' argument checks (they come back before any HIP call), the state round trip and the private
random stream of RndNetwork."""
import ctypes

import numpy as np
import pytest

import rnd_ref

F32, F64 = np.float32, np.float64


def _rollout(rs, n, t, c, h, w):
    obs = rs.randint(0, 256, size=(n * t, c, h, w), dtype=np.uint8)
    extra = rs.randint(0, 256, size=(n, c, h, w), dtype=np.uint8)
    return obs, extra


def test_next_frames_are_the_newest_plane_of_the_following_observation():
    rs = np.random.RandomState(0)
    n, t, c = 3, 4, 2
    obs, extra = _rollout(rs, n, t, c, 5, 6)
    f = rnd_ref.next_frames(obs, extra, n, t)
    for e in range(n):
        for s in range(t):
            want = obs[e * t + s + 1, c - 1] if s + 1 < t else extra[e, c - 1]
            assert np.array_equal(f[e * t + s], want)


def test_chan_merges_of_three_batches_equal_the_moments_of_the_concatenation():
    rs = np.random.RandomState(1)
    h, w = 6, 7
    count, mean, m2 = 0., np.zeros(h * w), np.zeros(h * w)
    seen = []
    for r in (5, 1, 11):
        frames = rs.randint(0, 256, size=(r, h, w), dtype=np.uint8)
        frames[:, 0, 0] = 255                       # a constant pixel
        frames[:, 0, 1] = 0
        seen.append(frames)
        count, mean, m2 = rnd_ref.obs_stats(frames, count, mean, m2)
    everything = np.concatenate(seen).reshape(17, -1).astype(F64)
    assert count == 17
    assert np.allclose(mean, everything.mean(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(m2 / count, everything.var(axis=0), rtol=1e-12, atol=0)
    assert m2[0] == 0 and m2[1] == 0 and mean[0] == 255 and mean[1] == 0


def test_reward_moments_over_three_calls_and_the_mix_equal_the_closed_formula():
    rs = np.random.RandomState(2)
    n, t, gamma = 7, 5, 0.99
    rho, moments = np.zeros(n), np.zeros(3)
    carried, values = np.zeros(n), []
    for call in range(3):
        err = (rs.rand(n, t) * 3).astype(F32)
        r_ext = rs.randn(n, t).astype(F32)
        r_mix, rho, moments, diag = rnd_ref.reward_mix(err, r_ext, rho, moments, gamma, 2.0, 0.5)
        for s in range(t):                          # the discounted running sums, by the textbook loop
            carried = gamma * carried + err[:, s]
            values.append(carried.copy())
        every = np.concatenate(values)
        assert moments[0] == every.size
        assert np.isclose(moments[1], every.mean(), rtol=1e-12, atol=0)
        assert np.isclose(moments[2] / moments[0], every.var(), rtol=1e-12, atol=0)
        sd = np.sqrt(every.var() + 1e-8)
        assert np.allclose(r_mix, 2.0 * r_ext.astype(F64) + 0.5 * err.astype(F64) / sd, rtol=1e-6, atol=1e-7)
        assert np.allclose(rho, carried, rtol=1e-13) and np.allclose(diag, [err.mean(dtype=F64), sd], rtol=1e-6)
    # the bonus switched off returns the extrinsic reward's bits, the sign of a zero included
    r_ext[0, 0], r_ext[0, 1] = F32(-0.0), F32(0.0)
    r_mix = rnd_ref.reward_mix(err, r_ext, rho, moments, gamma, 1.0, 0.0)[0]
    assert np.array_equal(r_mix.view(np.uint32), r_ext.view(np.uint32))


def test_prepare_clips_and_a_constant_pixel_gives_zero():
    h, w = 2, 2
    frames = np.zeros((50, h, w), np.uint8)
    frames[:, 0, 0] = 7                             # constant
    frames[:, 0, 1] = 100
    frames[0, 0, 1], frames[1, 0, 1] = 255, 0       # two outliers around a tight cluster
    frames[:, 1, :] = np.random.RandomState(3).randint(0, 256, size=(50, 2))
    count, mean, m2 = rnd_ref.obs_stats(frames, 0., np.zeros(4), np.zeros(4))
    z = (frames[:, 0, 1].astype(F64) - mean[1]) / np.sqrt(m2[1] / count + 1e-8)
    assert z[0] > 5 and -5 < z[1] < 0               # +5 clips here; -5 below, with another set of values
    out = rnd_ref.obs_prepare(frames, count, mean, m2)
    assert out.shape == (50, h, w, 4) and (out[..., 1:] == 0).all()
    assert (out[:, 0, 0, 0] == 0).all() and out[0, 0, 1, 0] == 5
    low = frames.copy()
    low[:, 0, 1] = 100
    low[0, 0, 1], low[1, 0, 1], low[2, 0, 1] = 0, 103, 103
    count, mean, m2 = rnd_ref.obs_stats(low, 0., np.zeros(4), np.zeros(4))
    out = rnd_ref.obs_prepare(low, count, mean, m2)
    assert out[0, 0, 1, 0] == -5 and -5 < out[3, 0, 1, 0] < 5


def test_error_against_plain_numpy():
    rs = np.random.RandomState(4)
    for b, e in ((1, 4), (3, 64), (5, 1024)):
        pred, targ = rs.randn(b, e).astype(F32), rs.randn(b, e).astype(F32)
        err, dpred, loss = rnd_ref.error(pred, targ, True)
        d = pred.astype(F64) - targ.astype(F64)
        assert np.allclose(err, (d * d).mean(axis=1), rtol=1e-6) and np.isclose(loss, (d * d).mean(), rtol=1e-6)
        assert np.allclose(dpred, 2 * d / (e * b), rtol=1e-6, atol=0)
        assert np.array_equal(rnd_ref.error(pred, targ, False), err)


# ---- constructors and initialize ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kwargs,match", [
    (dict(int_coeff=float("nan")), "int_coeff"), (dict(ext_coeff=float("inf")), "ext_coeff"),
    (dict(ext_coeff="2"), "ext_coeff"), (dict(int_discount=1.5), "int_discount"), (dict(int_discount=-0.1), "int_discount"),
    (dict(update_proportion=0), "update_proportion"), (dict(update_proportion=1.01), "update_proportion"),
    (dict(rnd_rows_per_pass=0), "rnd_rows_per_pass"), (dict(rnd_args=dict(momentum=1)), "rnd_args"),
    (dict(rnd_args=dict(embedding_size=6)), "embedding_size"), (dict(rnd_args=dict(predictor_hidden=(30,))), "predictor_hidden"),
    (dict(rnd_args=dict(rnd_seed=-1)), "rnd_seed")])
def test_constructor_refusals(kwargs, match):
    from accel_rl_amd.algos.pg import RndA2C, RndPPO
    for cls in (RndPPO, RndA2C):
        if cls is RndA2C and "update_proportion" in kwargs:
            continue
        with pytest.raises(ValueError, match=match):
            cls(**kwargs)


class _Policy(object):
    recurrent = False


def test_defaults_and_initialize_refusals():
    from accel_rl_amd.algos.pg import RndA2C, RndPPO
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.algos.pg.ppo import PPO
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.single import PpoOptimizer
    algo = RndPPO()
    assert isinstance(algo, PPO) and (algo.int_coeff, algo.ext_coeff, algo.int_discount, algo.update_proportion) == \
        (1.0, 2.0, 0.99, 0.25)
    assert algo.opt_info_keys == ["GradNorm", "RndLoss", "IntRewMean", "IntRewStd"] and algo.loss_kind == 1
    assert algo.rnd.embedding_size == 512 and algo.rnd.predictor_hidden == (512, 512)
    # the predictor's optimiser takes the policy optimizer's rule and rate unless rnd_args says otherwise
    assert algo._rnd_opt._learning_rate == algo.optimizer._learning_rate == 1e-3
    assert algo._rnd_opt._update_method is update_methods.adam and algo._rnd_opt._update_args["epsilon"] == 1e-5
    other = RndPPO(rnd_args=dict(learning_rate=3e-4, update_method=update_methods.rmsprop))
    assert other._rnd_opt._learning_rate == 3e-4 and other._rnd_opt._update_args == dict(rho=0.9, epsilon=1e-6)
    a2c = RndA2C()
    assert isinstance(a2c, A2C) and a2c.update_proportion == 1 and a2c.loss_kind == 0
    with pytest.raises(ValueError, match="update_proportion must be 1"):
        RndA2C(update_proportion=0.25)

    class Recurrent(object):
        recurrent = True

    class Sync(PpoOptimizer):
        parallelism_tag = "synchronous"
    for cls in (RndPPO, RndA2C):
        with pytest.raises(NotImplementedError, match=r"recurrent.*section E"):
            cls().initialize(Recurrent(), None, 40, 5, True)
        with pytest.raises(NotImplementedError, match=r"mid_batch_reset=False.*section E"):
            cls().initialize(_Policy(), None, 40, 5, False)
    with pytest.raises(NotImplementedError, match=r"single GPU only.*section E"):
        RndPPO(OptimizerCls=Sync).initialize(_Policy(), None, 40, 5, True)
    with pytest.raises(ValueError, match="arl_rnd_reward_mix"):
        RndPPO().initialize(_Policy(), None, (1 << 22) + 1, 1, True)


# ---- RndNetwork on the host ----------------------------------------------------------------------------------------------

def _network(seed=5, device="cpu"):
    from accel_rl_amd.policies.rnd_network import RndNetwork
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    net = RndNetwork(embedding_size=64, predictor_hidden=(64,), rnd_seed=seed)
    net.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)), 4, device=device)
    return net


def test_constructing_rnd_moves_nobody_else_s_random_numbers():
    from accel_rl_amd.util import seed
    seed.set_seed(7)
    before, layer_before = np.random.get_state(), seed.layer_rng().get_state()
    a = _network()
    after, layer_after = np.random.get_state(), seed.layer_rng().get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert np.array_equal(layer_before[1], layer_after[1]) and layer_before[2:] == layer_after[2:]
    # its own stream: the same seed gives the same buckets, another seed others; the two networks differ
    b, c = _network(), _network(seed=6)
    sa, sb, sc = a.rnd_state(), b.rnd_state(), c.rnd_state()
    assert np.array_equal(sa["target"], sb["target"]) and np.array_equal(sa["predictor"], sb["predictor"])
    assert not np.array_equal(sa["target"], sc["target"])
    n = a.target._offsets[2]
    assert not np.array_equal(sa["target"][:n], sa["predictor"][:n]) and np.abs(sa["target"][:n]).max() > 0


def test_layout_and_state_round_trip():
    from accel_rl_amd.policies import rnd_network
    net = _network()
    assert net.target._hid_geom == [(64, 9 * 6 * 64)] and net.predictor._hid_geom == [(64, 9 * 6 * 64), (64, 64)]
    assert net.target._conv_geom[0][1] == 4 and not net.target._u8       # one plane, padded to four channels
    w1 = net.target._w[0].view(32, 8, 8, 4)
    assert (w1[..., 1:] == 0).all() and w1[..., 0].abs().max() > 0
    state = net.rnd_state()
    assert sorted(state) == sorted(rnd_network.STATE_KEYS)
    assert state["obs_mean"].shape == (104 * 80,) and state["rho"].shape == (4,) and state["rew_moments"].shape == (3,)
    assert all(state[k].dtype == np.float64 for k in ("obs_count", "obs_mean", "obs_m2", "rew_moments", "rho"))
    rs = np.random.RandomState(8)
    moved = {k: (rs.rand(*v.shape) + 0.5).astype(v.dtype) for k, v in state.items()}
    other = _network(seed=9)
    other.set_rnd_state(moved)
    back = other.rnd_state()
    assert all(np.array_equal(back[k], moved[k]) for k in moved)
    back["rho"][0] = -1                              # a copy: the network keeps its own
    assert other.rnd_state()["rho"][0] == moved["rho"][0]
    with pytest.raises(ValueError, match="keys"):
        other.set_rnd_state({k: v for k, v in moved.items() if k != "rho"})
    with pytest.raises(ValueError, match="rho"):
        other.set_rnd_state(dict(moved, rho=np.zeros(5)))
    with pytest.raises(ValueError, match="obs_mean"):
        other.set_rnd_state(dict(moved, obs_mean=moved["obs_mean"].astype(np.float32)))


# ---- the entry points' argument checks -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


def _buf(nbytes, offset=0):
    """An aligned host address (never dereferenced: every call below is refused before any HIP call)."""
    raw = ctypes.create_string_buffer(nbytes + 64)
    base = (ctypes.addressof(raw) + 15) // 16 * 16
    return raw, base + offset


def test_argument_errors_come_back_before_any_launch(lib):
    from accel_rl_amd import _lib
    assert _lib.ARL_ABI_VERSION == 5 and lib.arl_abi_version() == 5
    keep, p = _buf(64)
    _, odd = _buf(64, 4)
    ws_bytes = lib.arl_rnd_obs_stats_workspace_bytes
    assert ws_bytes(104, 80) == (2 * 32 * 8320 + 2) * 8 and ws_bytes(0, 80) == 0 and ws_bytes(4096, 4097) == 0
    stats = lambda **kw: lib.arl_rnd_obs_stats(*[kw.get(k, d) for k, d in (                    # noqa: E731
        ("obs", p), ("extra", p), ("n", 2), ("t", 3), ("c", 4), ("h", 5), ("w", 6), ("count", p), ("mean", p), ("m2", p),
        ("ws", p), ("stream", None))])
    for kw, code in ((dict(obs=None), -1), (dict(extra=None), -1), (dict(count=None), -1), (dict(mean=None), -1),
                     (dict(m2=None), -1), (dict(ws=None), -1), (dict(n=0), -2), (dict(t=0), -2), (dict(t=4097), -2),
                     (dict(n=1 << 23, t=3), -2), (dict(c=0), -2), (dict(c=1025), -2), (dict(h=0), -2), (dict(w=0), -2),
                     (dict(h=4096, w=4097), -2), (dict(count=odd), -3), (dict(mean=odd), -3), (dict(m2=odd), -3),
                     (dict(ws=odd), -3)):
        assert stats(**kw) == code, kw
    prep = lambda **kw: lib.arl_rnd_obs_prepare(*[kw.get(k, d) for k, d in (                   # noqa: E731
        ("obs", p), ("extra", p), ("idx", None), ("b", 6), ("n", 2), ("t", 3), ("c", 4), ("h", 5), ("w", 6), ("count", p),
        ("mean", p), ("m2", p), ("out", p), ("stream", None))])
    _, odd8 = _buf(64, 8)
    _, odd2 = _buf(64, 2)
    for kw, code in ((dict(obs=None), -1), (dict(extra=None), -1), (dict(count=None), -1), (dict(mean=None), -1),
                     (dict(m2=None), -1), (dict(out=None), -1), (dict(b=0), -2), (dict(b=7), -2),
                     (dict(b=(1 << 24) + 1, idx=p), -2), (dict(n=0), -2), (dict(t=0), -2), (dict(c=0), -2), (dict(h=0), -2),
                     (dict(out=odd8), -3), (dict(idx=odd2), -3), (dict(mean=odd), -3)):
        assert prep(**kw) == code, kw
    err = lambda **kw: lib.arl_rnd_error(*[kw.get(k, d) for k, d in (                           # noqa: E731
        ("pred", p), ("targ", p), ("b", 3), ("e", 64), ("grad", 1), ("err", p), ("dpred", p), ("loss", p),
        ("stream", None))])
    for kw, code in ((dict(pred=None), -1), (dict(targ=None), -1), (dict(err=None), -1), (dict(dpred=None), -1),
                     (dict(loss=None), -1), (dict(b=0), -2), (dict(b=(1 << 24) + 1), -2), (dict(e=0), -2), (dict(e=6), -2),
                     (dict(e=65540), -2), (dict(pred=odd), -3), (dict(targ=odd8), -3), (dict(dpred=odd), -3),
                     (dict(err=odd2), -3), (dict(loss=odd2), -3)):
        assert err(**kw) == code, kw
    mix = lambda **kw: lib.arl_rnd_reward_mix(*[kw.get(k, d) for k, d in (                      # noqa: E731
        ("err", p), ("r", p + 16), ("n", 2), ("t", 3), ("rho", p), ("mom", p), ("g", 0.99), ("ce", 2.0), ("ci", 1.0),
        ("mix", p + 32), ("diag", p), ("ws", p), ("stream", None))])
    nan, inf = float("nan"), float("inf")
    for kw, code in ((dict(err=None), -1), (dict(r=None), -1), (dict(rho=None), -1), (dict(mom=None), -1),
                     (dict(mix=None), -1), (dict(diag=None), -1), (dict(ws=None), -1), (dict(g=nan), -1), (dict(g=1.01), -1),
                     (dict(g=-0.01), -1), (dict(ce=inf), -1), (dict(ci=nan), -1), (dict(mix=p), -1), (dict(mix=p + 16), -1),
                     (dict(n=0), -2), (dict(t=0), -2), (dict(t=4097), -2), (dict(n=(1 << 20) + 1, t=1), -2),
                     (dict(n=1 << 20, t=5), -2), (dict(err=odd2), -3), (dict(rho=odd), -3), (dict(mom=odd), -3),
                     (dict(ws=odd), -3)):
        assert mix(**kw) == code, kw
    assert b"arl_rnd_reward_mix" in lib.arl_last_error()
    del keep
