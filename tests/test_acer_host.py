"""ACER without a GPU: the restatements of tests/acer_ref.py against float64 autograd and against the plain discounted
return, the trust-region projection's two properties, the replay schedule, the binding, and every refusal."""
import ctypes

import numpy as np
import pytest
import torch

import acer_ref as ar

INF = float("inf")


def _core_inputs(seed, batch, n_act):
    rs = np.random.RandomState(seed)
    pi, lp, _ = ar.soft64(rs.randn(batch, n_act) * 1.5)
    pibar, _, _ = ar.soft64(rs.randn(batch, n_act) * 1.5)
    mu, _, _ = ar.soft64(rs.randn(batch, n_act))
    return dict(pi=pi, lp=lp, pibar=pibar, Q=rs.randn(batch, n_act) * 2, mu=mu, act=rs.randint(0, n_act, batch),
                qret=rs.randn(batch) * 2)


@pytest.mark.parametrize("c,delta", [(10.0, 1.0), (0.7, 0.05), (INF, INF), (1.3, 0.0)])
def test_loss_gradient_equals_autograd_taken_the_long_way(c, delta):
    """Probabilities as a leaf; g from autograd of the objective (truncated term + bias correction + entropy, Q, V and the
    weights constants); then the projection; then soft-max backward through autograd of sum(p(z) * zstar)."""
    B, A, q_coeff, ent = 7, 6, 0.5, 0.01
    d = _core_inputs(3, B, A)
    want = ar.loss_core(np, d["pi"], d["lp"], d["pibar"], d["Q"], d["mu"], d["act"], d["qret"], c, delta, q_coeff, ent,
                        float(B))
    t = lambda x: torch.tensor(x, dtype=torch.float64)              # noqa: E731
    z = torch.log(t(d["pi"])).requires_grad_(True)                  # logits whose soft-max is pi
    p = torch.softmax(z, dim=1)
    leaf = p.detach().clone().requires_grad_(True)
    Q, mu, act, qret = t(d["Q"]), t(d["mu"]), torch.from_numpy(d["act"]), t(d["qret"])
    with torch.no_grad():
        V = (leaf * Q).sum(1)
        rho = leaf / (mu + ar.AC_EPS)
        rho_t = rho.gather(1, act[:, None])[:, 0]
        w = torch.clamp(1 - c / (rho + ar.AC_EPS), min=0) if c != INF else torch.zeros_like(rho)
        f = torch.minimum(rho_t, torch.tensor(c, dtype=torch.float64)) * (qret - V)
    objective = (f * torch.log(leaf.gather(1, act[:, None])[:, 0] + ar.AC_EPS)).sum() \
        + (w * (Q - V[:, None]) * leaf).sum() - ent * (leaf * torch.log(leaf)).sum()
    g, = torch.autograd.grad(objective, leaf)
    np.testing.assert_allclose(g.numpy(), want["g"], rtol=1e-9, atol=1e-12)
    k = -t(d["pibar"]) / (leaf.detach() + ar.AC_EPS)
    s = torch.clamp(((k * g).sum(1) - delta) / (k * k).sum(1), min=0) if delta != INF else torch.zeros(B, dtype=torch.float64)
    zstar = g - s[:, None] * k
    dz, = torch.autograd.grad(-(p * zstar).sum() / B, z)
    np.testing.assert_allclose(dz.numpy(), want["dz"], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(want["dq"], q_coeff * (d["Q"][np.arange(B), d["act"]] - d["qret"]) / B, rtol=1e-12)


def test_on_policy_flat_q_scan_is_the_plain_discounted_return():
    """mu = pi and Q constant across actions (Q(a) == V): at lambda = 1 the carried value is cbar (qret - V) + V with
    cbar = rho = pi / (pi + eps), short of 1 by at most eps / min pi, so qret is the discounted bootstrapped return up to
    T steps of that relative shortfall on |qret - V|; at lambda = 0 it is the one-step target r + discount V_next."""
    n_env, T, A = 5, 9, 6
    c = ar.scan_case(1, n_env, T, A, 8, done_at=3)
    c["old_prob"] = c["prob"].copy()
    c["q"][:, :A] = c["q"][:, :1]
    c["q_last"][:, :A] = c["q_last"][:, :1]
    args = (c["prob"], c["prob_last"], c["q"], c["q_last"], c["old_prob"], c["actions"], c["rewards"], c["dones"], 0.99)
    qret, v, stats = ar.retrace(*args, 1.0, n_env, T)
    want = ar.discounted_return(c["rewards"], c["dones"], c["q_last"][:, 0], 0.99, n_env, T)
    spread = np.abs(want).max() + np.abs(c["q"][:, 0]).max()
    np.testing.assert_allclose(qret, want, rtol=2e-6, atol=T * (ar.AC_EPS / c["prob"].min()) * spread + 1e-6)
    assert (stats[:, 1] == 0).all() and np.allclose(stats[:, 0], T, rtol=1e-4)
    one_step, _, _ = ar.retrace(*args, 0.0, n_env, T)
    v_next = np.concatenate([c["q"][:, 0].reshape(n_env, T)[:, 1:], c["q_last"][:, :1]], axis=1).reshape(-1)
    keep = 1.0 - c["dones"].astype(np.float64)
    np.testing.assert_allclose(one_step, c["rewards"] + keep * 0.99 * v_next, rtol=2e-6, atol=1e-6)


def test_projection_holds_the_trust_region_when_active_and_is_the_identity_otherwise():
    d = _core_inputs(8, 200, 6)
    for delta in (0.0, 0.3, 1.0, 30.0):
        r = ar.loss_core(np, d["pi"], d["lp"], d["pibar"], d["Q"], d["mu"], d["act"], d["qret"], 10.0, delta, 0.5, 0.01,
                         200.0)
        kz = (r["k"] * r["zs"]).sum(axis=1)
        active = r["s"] > 0
        assert (kz[active] <= delta + 1e-9 * (1 + np.abs(r["kg"][active]))).all()
        assert np.array_equal(r["zs"][~active], r["g"][~active]) and (r["kg"][~active] <= delta).all()
        assert (r["kg"][active] > delta).all()
    assert active.sum() == 0 or delta == 30.0
    r0 = ar.loss_core(np, d["pi"], d["lp"], d["pibar"], d["Q"], d["mu"], d["act"], d["qret"], 10.0, 0.0, 0.5, 0.01, 200.0)
    assert (r0["s"] > 0).any() and (r0["s"] == 0).any()
    off = ar.loss_core(np, d["pi"], d["lp"], d["pibar"], d["Q"], d["mu"], d["act"], d["qret"], 10.0, INF, 0.5, 0.01, 200.0)
    assert (off["s"] == 0).all() and np.array_equal(off["zs"], off["g"])
    zero = ar.loss_core(np, d["pi"], d["lp"], 0 * d["pibar"], d["Q"], d["mu"], d["act"], d["qret"], 10.0, 0.0, 0.5, 0.01,
                        200.0)
    assert (zero["s"] == 0).all() and np.isfinite(zero["dz"]).all()             # kk == 0: no projection, no NaN


def test_an_fma_would_change_the_average_step():
    rs = np.random.RandomState(5)
    avg, params = rs.randn(4096).astype(np.float32), rs.randn(4096).astype(np.float32)
    mask = ar.fma_differs(avg, params, 0.99)
    assert mask.any() and not mask.all()
    assert np.array_equal(ar.avg_step(avg, params, 1.0), avg) and np.array_equal(ar.avg_step(avg, params, 0.0), params)


def test_replay_schedule():
    from accel_rl_amd.algos.pg.acer import draw_trajectories, replay_count, rollouts_of
    assert [rollouts_of(s, 40) for s in (1, 40, 41, 50000)] == [1, 1, 2, 1250]
    np.random.seed(0)
    state = np.random.get_state()[1].copy()
    assert replay_count(4, 2, 3, 16) == 0 and replay_count(0, 5, 3, 16) == 0
    assert np.array_equal(np.random.get_state()[1], state)                      # nothing drawn before the start
    np.random.seed(0)
    want = np.random.poisson(4, size=200)
    np.random.seed(0)
    got = [replay_count(4, 3, 3, 6) for _ in range(200)]
    assert got == [min(int(w), 6) for w in want] and max(got) == 6 and want.max() > 6 and min(got) < 6
    idx = draw_trajectories(5, 8, 3)
    assert idx.shape == (5, 8) and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < 24 and len(set(idx.ravel())) > 8


def test_binding_and_arg_errors():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    lib = _lib.load()
    assert "acer.hip" in _build.SOURCES and lib.arl_abi_version() == 5
    for name in ("arl_acer_retrace_scan", "arl_acer_loss", "arl_acer_avg_step", "arl_gather_segments"):
        assert name in _lib.EXPORTED_SYMBOLS and callable(getattr(_lib, name[4:]))
        assert getattr(lib, name).restype is ctypes.c_int32
    assert lib.arl_acer_retrace_scan(*([None] * 4), 4, *([None] * 4), 0.99, 1.0, 1, 1, 1, None, None, None, None) == -1
    assert b"null" in lib.arl_last_error()
    assert lib.arl_acer_loss(*([None] * 6), 1, 1, 4, 10.0, 1.0, 0.5, 0.01, None, None, None) == -1
    assert lib.arl_acer_avg_step(None, None, 1, 0.99, None) == -1
    assert lib.arl_gather_segments(None, None, 1, 1, 1, None, None) == -1


def _policy_cls():
    from accel_rl_amd.policies.dqn.atari_acer_policy import AtariAcerPolicy
    return AtariAcerPolicy


def _spec():
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    return dict(cnn_specs[0], hidden_sizes=[64])


def test_policy_refusals_and_head_layout_round_trip():
    cls = _policy_cls()
    for kw in (dict(dueling=True), dict(shared_last_bias=True), dict(recurrent=True)):
        with pytest.raises(NotImplementedError, match="section E"):
            cls(**dict(_spec(), **kw))
    pol = cls(**_spec())
    with pytest.raises(NotImplementedError, match="ONE-HOT.*section E"):       # the host sampler's grouped serving
        pol.serve_group(None, 0, 8)
    from accel_rl_amd.policies.dqn.atari_sac_discrete_policy import AtariSacDiscretePolicy
    from accel_rl_amd.policies.dqn.q_policy_base import SoftmaxServeMixin
    for name in ("_serve", "host_draws", "get_actions", "get_action", "set_deterministic", "get_epsilon"):
        assert getattr(cls, name) is getattr(SoftmaxServeMixin, name) is getattr(AtariSacDiscretePolicy, name), name
    pol.n_act = 6
    ref, names = pol._head_reference_init(64, 6)
    assert names == ["OutputW", "Outputb", "QW", "Qb"] and pol.half_stride == 32 and pol._head_width == 64
    assert pol._head_internal_shapes(64, 6) == [(64, 64), (64,)]
    rs = np.random.RandomState(0)
    ref = [rs.randn(*a.shape).astype(np.float32) for a in ref]
    w, b = pol._head_to_internal(ref)
    assert w.shape == (64, 64) and (w[6:32] == 0).all() and (w[38:] == 0).all() and (b[6:32] == 0).all()
    back = pol._head_to_reference(w, b)
    assert all(np.array_equal(x, y) for x, y in zip(back, ref))
    with pytest.raises(NotImplementedError, match="section E"):
        pol.n_act = 19
        pol._head_reference_init(64, 19)
    with pytest.raises(NotImplementedError, match="acer_loss_and_grads"):
        pol.loss_and_grads(dict(), 0, 0., 0.5, 0.01, None)
    assert pol.serve_supported() is False and pol.get_epsilon() == 0.
    pol.set_deterministic(True)
    assert pol.get_deterministic() is True


class _FakePolicy(object):
    recurrent = False


def test_algorithm_refusals_and_defaults():
    from accel_rl_amd.algos.pg import ACER
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.single import AcerOptimizer, PpoOptimizer
    algo = ACER()
    opt = algo.optimizer
    assert isinstance(opt, AcerOptimizer) and opt._learning_rate == 7e-4 and opt._update_method is update_methods.rmsprop
    assert opt._grad_norm_clip == 10 and opt._epochs == 1 and opt.avg_alpha == 0.99
    assert (algo.discount, algo.retrace_lambda, algo.c, algo.delta, algo.q_coeff, algo.ent_loss_coeff) == \
        (0.99, 1.0, 10.0, 1.0, 0.5, 0.01)
    assert algo.replay_ratio == 4 and algo.opt_info_keys == ["GradNorm", "QLoss", "Entropy", "RhoMean", "TrustScaleMean",
                                                             "ReplayUpdates"]
    with pytest.raises(NotImplementedError, match="AtariAcerPolicy.*section E"):
        algo.initialize(_FakePolicy(), None, 40, 5, True)
    pol = _policy_cls()(**_spec())
    with pytest.raises(NotImplementedError, match="mid_batch_reset.*section E"):
        algo.initialize(pol, None, 40, 5, False)

    class Recurrent(_policy_cls()):
        recurrent = True
    with pytest.raises(NotImplementedError, match="recurrent.*section E"):
        algo.initialize(Recurrent(**_spec()), None, 40, 5, True)

    class Sync(AcerOptimizer):
        parallelism_tag = "synchronous"
    with pytest.raises(NotImplementedError, match="single GPU.*section E"):
        ACER(OptimizerCls=Sync).initialize(pol, None, 40, 5, True)
    with pytest.raises(TypeError, match="AcerOptimizer"):
        ACER(OptimizerCls=PpoOptimizer).initialize(pol, None, 40, 5, True)
    for kw in (dict(discount=1.1), dict(retrace_lambda=-0.1), dict(c=0.0), dict(delta=-1.0), dict(alpha=1.5),
               dict(replay_ratio=-1), dict(r_max=0), dict(replay_steps=0), dict(q_coeff=INF)):
        with pytest.raises(ValueError):
            ACER(**kw)
    assert ACER(c=INF, delta=INF).c == INF
    with pytest.raises(ValueError, match="grad_norm_clip.*section E"):
        ACER(optimizer_args=dict(grad_norm_clip=None))
    bare = AcerOptimizer(7e-4, update_methods.rmsprop, dict(), 1, None, grad_norm_clip=None)
    with pytest.raises(NotImplementedError, match="grad_norm_clip"):
        bare.whole_batch_update(())
