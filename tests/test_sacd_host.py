"""SAC-Discrete without a GPU: constructor and algorithm refusals, the defaults table, the parameter vector's
actor | q1 | q2 | log_alpha order, SacOptimizer's argument checks, the three exported entry points and their argument
errors, and the float64 yardstick of tests/sacd_ref.py against autograd."""
import numpy as np
import pytest
import torch

import sacd_ref as sr


@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


def _spec(**kw):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    return dict(dict(cnn_specs[0], hidden_sizes=[64]), **kw)


def test_policy_constructor_and_refusals():
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.policies.dqn.atari_sac_discrete_policy import AtariSacDiscretePolicy
    from accel_rl_amd.policies.dqn.q_policy_base import QPolicyBase
    for kw in (dict(dueling=True), dict(shared_last_bias=True)):
        with pytest.raises(NotImplementedError, match="section E"):
            AtariSacDiscretePolicy(**_spec(**kw))
    with pytest.raises(TypeError):                              # there is no epsilon to give
        AtariSacDiscretePolicy(epsilon=0.1, **_spec())
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="initial_alpha"):
            AtariSacDiscretePolicy(initial_alpha=bad, **_spec())
    p = AtariSacDiscretePolicy(**_spec())
    assert isinstance(p, QPolicyBase) and not isinstance(p, AtariDqnPolicy)
    assert type(p.q1) is AtariDqnPolicy and type(p.q2) is AtariDqnPolicy and p.q1 is not p.q2
    assert p.initial_alpha == 1.0 and p.get_deterministic() is False and p.serve_supported() is False
    assert p.serves_rows is False and not p._dueling
    p.set_epsilon(0.7)                                          # inert
    assert p.get_epsilon() == 0.0
    p.set_deterministic(1)
    assert p.get_deterministic() is True
    assert AtariSacDiscretePolicy(initial_alpha=0.2, deterministic=True, **_spec()).get_deterministic() is True


def test_parameter_vector_order_and_round_trip():
    """actor | q1 | q2 | log_alpha: split_param_vector cuts exactly there, and set / get through stand-ins for the three
    networks keep every entry in its place (the device round trip: tests/test_sacd_gpu.py)."""
    from accel_rl_amd.policies.dqn import atari_sac_discrete_policy as mod
    sizes = [5, 3, 3, 1]
    flat = np.arange(12, dtype=np.float32)
    parts = mod.split_param_vector(flat, sizes)
    assert [p.tolist() for p in parts] == [[0, 1, 2, 3, 4], [5, 6, 7], [8, 9, 10], [11]]
    for bad in (flat[:-1], np.concatenate([flat, flat[:1]])):
        with pytest.raises(ValueError, match="actor \\| q1 \\| q2 \\| log_alpha"):
            mod.split_param_vector(bad, sizes)

    class Net(object):
        def __init__(self, n):
            self.n_params, self.v = n, np.zeros(n, np.float32)

        def get_param_values(self):
            return self.v

        def set_param_values(self, v):
            self.v = np.array(v, np.float32)

    p = mod.AtariSacDiscretePolicy(**_spec())
    p.q1, p.q2 = Net(3), Net(3)
    p._actor_n_params, p._ref_shapes = 5, [(5,)]
    p.log_alpha = torch.zeros(4)
    seen = {}
    p._set_from_reference_arrays = lambda ref: seen.update(actor=np.concatenate([r.reshape(-1) for r in ref]))
    p.bucket_to_reference = lambda flat_bucket: seen["actor"]
    p.flat_params = None
    p.set_param_values(flat)
    assert seen["actor"].tolist() == [0, 1, 2, 3, 4] and p.q1.v.tolist() == [5, 6, 7] and p.q2.v.tolist() == [8, 9, 10]
    assert p.log_alpha.tolist() == [11, 0, 0, 0]
    np.testing.assert_array_equal(p.get_param_values(), flat)


def test_algorithm_refusals_and_defaults():
    from accel_rl_amd.algos.dqn.dqn import DQN
    from accel_rl_amd.algos.dqn.sac_discrete import SacDiscrete
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.dqn import DqnOptimizer, SacOptimizer
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.policies.dqn.atari_sac_discrete_policy import AtariSacDiscretePolicy
    for kw in (dict(double_dqn=True), dict(dueling_dqn=True), dict(reward_horizon=3)):
        with pytest.raises(NotImplementedError, match="section E"):
            SacDiscrete(**kw)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="target_entropy_scale"):
            SacDiscrete(target_entropy_scale=bad)
    with pytest.raises(TypeError, match="SacOptimizer"):
        SacDiscrete(OptimizerCls=DqnOptimizer)
    with pytest.raises(TypeError, match="augment_args"):
        SacDiscrete(augment_args=dict(shift=3))
    with pytest.raises(NotImplementedError):                    # one shifted view per observation, as every DQN but DrQ
        SacDiscrete(augment_args=dict(m_online=2))

    class Sub(AtariSacDiscretePolicy):
        pass
    for policy in (AtariDqnPolicy(**_spec()), Sub(**_spec())):
        with pytest.raises(TypeError, match="AtariSacDiscretePolicy"):
            SacDiscrete().build_loss(None, policy)
    a = SacDiscrete()
    assert isinstance(a, DQN) and type(a.optimizer) is SacOptimizer
    assert (a.batch_size, a.min_steps_learn, a.target_update_steps, a.training_intensity) == (64, 20000, 8000, 16)
    assert (a.delta_clip, a.target_entropy_scale, a.eval_deterministic, a.reward_horizon) == (None, 0.89, True, 1)
    assert a.opt_info_keys == ["Priority", "Loss", "PiLoss", "Entropy", "Alpha"]
    opt = a.optimizer
    assert (opt._learning_rate, opt._update_method, opt._grad_norm_clip) == (3e-4, update_methods.adam, None)
    assert opt._update_args["epsilon"] == 1e-4 and opt._alpha_learning_rate == 3e-4
    assert opt._alpha_method is update_methods.adam and opt._alpha_kernel_args == (0.9, 0.999, 1e-4)
    assert SacDiscrete(augment_args=dict(pad=4))._replay_augment["pad"] == 4

    class FakePolicy(object):
        det, eps = False, "untouched"

        def set_deterministic(self, v):
            self.det = bool(v)

        def get_deterministic(self):
            return self.det
    a.policy = FakePolicy()
    a.update_epsilon(5)                                         # a no-op
    a.prep_eval(0)
    assert a.policy.det is True
    a.post_eval(0)
    assert a.policy.det is False and a.policy.eps == "untouched"
    b = SacDiscrete(eval_deterministic=False)
    b.policy = FakePolicy()
    b.prep_eval(3)
    assert b.policy.det is False


def test_sac_optimizer_argument_checks():
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.dqn import SacOptimizer
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    with pytest.raises(TypeError, match="alpha_args"):
        SacOptimizer(3e-4, update_methods.adam, alpha_args=dict(lr=1e-3))
    with pytest.raises(TypeError, match="update_method_args"):
        SacOptimizer(3e-4, update_methods.adam, alpha_args=dict(update_method=update_methods.rmsprop,
                                                                update_method_args=dict(beta1=0.5)))
    with pytest.raises(NotImplementedError):
        SacOptimizer(3e-4, update_methods.adam, scale_conv_grads=True)
    opt = SacOptimizer(3e-4, update_methods.adam, update_method_args=dict(epsilon=1e-4),
                       alpha_args=dict(learning_rate=1e-3, update_method=update_methods.rmsprop))
    assert opt._alpha_learning_rate == 1e-3 and opt._alpha_kernel_args == (0.9, 0.0, 1e-6)
    with pytest.raises(TypeError, match="AtariSacDiscretePolicy"):
        opt._setup_bucket(AtariDqnPolicy(**_spec()), 1)


def test_the_library_exports_the_three_entry_points_and_refuses_null_pointers(lib):
    from accel_rl_amd import _lib
    for name in ("arl_sacd_act", "arl_sacd_loss", "arl_sacd_alpha_grad"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None and callable(getattr(_lib, name[4:]))
    # no device is touched: the argument checks come first
    assert lib.arl_sacd_act(None, None, 1, 4, 4, 0, None, None, None) == -1 and b"null" in lib.arl_last_error()
    assert lib.arl_sacd_loss(*([None] * 11), 1, 4, 4, 0.99, 1.0, None, None, None, None, None) == -1
    assert b"arl_sacd_loss" in lib.arl_last_error() and b"null" in lib.arl_last_error()
    assert lib.arl_sacd_alpha_grad(None, 1, None, 0.5, None, None) == -1 and b"null" in lib.arl_last_error()


# ---- the yardstick itself -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip", [None, 1.0])
def test_ref_loss_gradients_equal_float64_autograd(clip):
    c = sr.case(5, 6, 32, 14, True, shift=2)
    assert set(c["kinds"].tolist()) == set(range(sr.N_KINDS))
    ref = sr.ref_loss(c, sr.GAMMA, clip)
    A, B = 6, 14
    t = lambda x: torch.from_numpy(np.asarray(x[:, :A], np.float64))            # noqa: E731
    q1, q2, lo = t(c["q1"]).requires_grad_(), t(c["q2"]).requires_grad_(), t(c["lo"]).requires_grad_()
    alpha = float(np.exp(np.float64(c["log_alpha"])))
    lpn = torch.log_softmax(t(c["ln"]), dim=1)
    soft = (lpn.exp() * (torch.minimum(t(c["t1"]), t(c["t2"])) - alpha * lpn)).sum(dim=1)
    y = torch.from_numpy(c["ret"]).double() + (1. - torch.from_numpy(c["term"]).double()) * sr.GAMMA * soft
    act = torch.from_numpy(ref["act"])
    w = torch.from_numpy(ref["w"])
    q_loss = 0.
    for q in (q1, q2):
        d = y - q[torch.arange(B), act]
        ad = d.abs()
        q_loss = q_loss + (w * (torch.where(ad <= clip, 0.5 * d * d, clip * (ad - clip / 2.)) if clip else 0.5 * d * d)).sum()
    lp = torch.log_softmax(lo, dim=1)
    pi_loss = (lp.exp() * (alpha * lp - torch.minimum(q1, q2).detach())).sum(dim=1).mean()
    g1, g2 = torch.autograd.grad(q_loss, (q1, q2))
    gl, = torch.autograd.grad(pi_loss, lo)
    for got, want in ((ref["dq1"], g1), (ref["dq2"], g2), (ref["dlogits"], gl)):
        assert np.abs(got - want.numpy()).max() <= 1e-12 * max(1.0, np.abs(want.numpy()).max())
    assert abs(ref["rows"].sum() - q_loss.item()) <= 1e-12 * abs(q_loss.item())
    assert abs(ref["pi_rows"].sum() - pi_loss.item()) <= 1e-12 * max(1.0, abs(pi_loss.item()))
    eq = c["kinds"] == sr.ALL_EQUAL
    np.testing.assert_allclose(ref["ent"][eq], np.log(A), rtol=1e-12)
    hot = c["kinds"] == sr.ONE_HOT
    assert np.isfinite(ref["dlogits"]).all() and (ref["pi"][hot].max(axis=1) == 1.0).all() and (ref["ent"][hot] < 1e-30).all()


def test_ref_alpha_grad_signs():
    ent = np.full(7, 1.2)
    above, _ = sr.ref_alpha_grad(ent, 0.3, 1.0)                 # entropy above the target: a positive gradient lowers alpha
    below, _ = sr.ref_alpha_grad(ent, 0.3, 1.5)
    assert above > 0 > below and abs(above - np.exp(0.3) * 0.2) < 1e-12
