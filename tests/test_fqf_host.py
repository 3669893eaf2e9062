"""CPU-only: the host side of FQF -- constructor and algorithm refusals and defaults, the parameter names and flat order
(the fraction layer last), the reference-layout conversion of the fraction layer, FqfOptimizer's argument handling, the
three exported entry points' argument checks, and the float64 restatement of tests/fqf_ref.py checked against autograd
through a numerically integrated 1-Wasserstein distance."""
import numpy as np
import pytest
import torch

import fqf_ref as R


@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


def _spec(**kw):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    spec = dict(cnn_specs[0])
    spec.update(kw)
    return spec


def test_constructor_refusals_and_defaults():
    from accel_rl_amd.policies.dqn.atari_fqf_policy import AtariFqfPolicy
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    for bad in (0, 65, -1):
        with pytest.raises(NotImplementedError, match="n_quantiles"):
            AtariFqfPolicy(**_spec(n_quantiles=bad))
    for ok, stride in ((1, 32), (32, 32), (33, 64), (64, 64)):
        p = AtariFqfPolicy(**_spec(n_quantiles=ok))
        assert (p.n_quantiles, p.n_target_quantiles, p.n_policy_quantiles, p._n_stride) == (ok, ok, ok, stride)
    with pytest.raises(NotImplementedError, match="dueling"):
        AtariFqfPolicy(dueling=True, **_spec())
    for gone in ("n_target_quantiles", "n_policy_quantiles"):
        with pytest.raises(TypeError):
            AtariFqfPolicy(**_spec(**{gone: 8}))
    p = AtariFqfPolicy(epsilon=0.25, **_spec())
    assert isinstance(p, AtariIqnPolicy) and p.n_quantiles == 32 and p.get_epsilon() == 0.25 and not p._dueling
    assert p.frac_rows is None and p.entropy is None
    for method in (p.iqn_loss_and_grads, p.munchausen_loss_and_grads):
        with pytest.raises(NotImplementedError, match="train it with FQF"):
            method(None, None, None, None, None, None, 0.99, 1.0)


def test_algorithm_refusals_and_defaults():
    from accel_rl_amd.algos.dqn.fqf import FQF
    from accel_rl_amd.algos.dqn.iqn import ImplicitQuantileDQN
    from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.dqn import DqnOptimizer, FqfOptimizer
    from accel_rl_amd.policies.dqn.atari_fqf_policy import AtariFqfPolicy
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    a = FQF()
    assert isinstance(a, ImplicitQuantileDQN) and (a.kappa, a.ent_coef, a.batch_size) == (1.0, 0.0, 32)
    assert a._get_default_sub_args() == QuantileDQN()._get_default_sub_args()        # main defaults: QuantileDQN's
    paper = dict(learning_rate=2.5e-9, update_method=update_methods.rmsprop, update_method_args=dict(rho=0.95, epsilon=1e-5))
    assert a.fraction_optimizer_args == paper
    o = a.optimizer
    assert isinstance(o, FqfOptimizer) and isinstance(o, DqnOptimizer)
    assert (o._learning_rate, o._update_method, o._grad_norm_clip) == (5e-5, update_methods.adam, None)
    assert (o._frac_learning_rate, o._frac_method, o._frac_args) == (2.5e-9, update_methods.rmsprop, dict(rho=0.95, epsilon=1e-5))
    o = FQF(fraction_optimizer_args=dict(learning_rate=1e-6, update_method=update_methods.adam, update_method_args=None),
            optimizer_args=dict(learning_rate=1e-4)).optimizer
    assert (o._learning_rate, o._frac_learning_rate, o._frac_method) == (1e-4, 1e-6, update_methods.adam)
    assert o._frac_args == dict(beta1=0.9, beta2=0.999, epsilon=1e-8)
    assert FqfOptimizer(1e-4, update_methods.adam)._frac_args == dict(rho=0.95, epsilon=1e-5)   # the paper's, by default
    with pytest.raises(TypeError, match="fraction_args"):
        FqfOptimizer(1e-4, update_methods.adam, fraction_args=dict(lr=1.))
    with pytest.raises(TypeError, match="FqfOptimizer"):
        FQF(OptimizerCls=DqnOptimizer)
    assert FQF(kappa=0., ent_coef=0.01).ent_coef == 0.01
    for bad in (-1., float("inf"), float("nan")):
        with pytest.raises(ValueError, match="kappa"):
            FQF(kappa=bad)
        with pytest.raises(ValueError, match="ent_coef"):
            FQF(ent_coef=bad)
    with pytest.raises(NotImplementedError, match="dueling"):
        FQF(dueling_dqn=True)
    with pytest.raises(TypeError, match="AtariFqfPolicy"):
        FQF().build_loss(None, AtariIqnPolicy(**_spec()))
    base = ["obs", "next_obs", "act", "disc_n_return", "terminal"]
    inputs, loss = FQF().build_loss(None, AtariFqfPolicy(**_spec()))
    assert inputs == base and callable(loss)
    inputs, _ = FQF(prioritized_replay=True, double_dqn=True, reward_horizon=3).build_loss(None, AtariFqfPolicy(**_spec()))
    assert inputs == base + ["importance_sample_weights"]
    # the parents refuse the class where they would call the methods it does not have
    _, loss = ImplicitQuantileDQN().build_loss(None, AtariFqfPolicy(**_spec()))
    with pytest.raises(NotImplementedError, match="train it with FQF"):
        loss((None, None, None, None, torch.zeros(1, dtype=torch.uint8)))


def test_parameter_names_order_and_fraction_layer_layout():
    """The layout hooks need no device: names and reference shapes in flat order, the fraction layer last, stored
    (n_stride, F) with zero rows in the padding and its fan-in axis converted like the first dense layer's."""
    from accel_rl_amd.policies.dqn.atari_fqf_policy import AtariFqfPolicy
    n = 5
    p = AtariFqfPolicy(**_spec(hidden_sizes=(32,), n_quantiles=n))
    co, ho, wo = p._conv_out = (8, 3, 5)
    f = co * ho * wo
    p.n_act = 6
    hid, hid_names, fan = p._hidden_reference_init(f)
    head, head_names = p._head_reference_init(fan, 6)
    assert (hid_names + head_names)[-4:] == ["OutputW", "Outputb", "FracW", "Fracb"]
    assert hid_names + head_names == ["EmbW", "Embb", "FC0W", "FC0b", "OutputW", "Outputb", "FracW", "Fracb"]
    assert [a.shape for a in head] == [(32, 6), (6,), (f, n), (n,)]
    assert p._head_internal_shapes(32, 6) == [(32, 32), (32,), (32, f), (32,)]
    np.testing.assert_allclose(np.square(head[2]).sum(axis=0), 0.01 ** 2, rtol=1e-5)       # NormC(0.01): near-uniform fractions
    assert not head[3].any()
    rs = np.random.RandomState(0)
    ref = [rs.randn(*a.shape).astype(np.float32) for a in head]
    internal = p._head_to_internal(ref)
    assert [a.shape for a in internal] == p._head_internal_shapes(32, 6)
    assert not internal[2][n:].any() and not internal[3][n:].any() and internal[2][:n].all()   # zero rows in the padding
    back = p._head_to_reference(internal[0], internal[1]) + p._frac_to_reference(internal[2], internal[3])
    for a, b in zip(ref, back):
        np.testing.assert_array_equal(a, b)
    c, h, w = 5, 2, 3                       # unit (c, h, w) of the reference is unit (h, w, c) inside, as FC0's fan-in
    u_ref, u_int = (c * ho + h) * wo + w, (h * wo + w) * co + c
    np.testing.assert_array_equal(internal[2][:n, u_int], ref[2][u_ref])


def test_the_library_exports_the_entry_points_and_refuses_bad_arguments(lib):
    from accel_rl_amd import _lib
    for name in ("arl_fqf_fractions", "arl_fqf_act", "arl_fqf_loss"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    for fn in ("fqf_fractions", "fqf_act", "fqf_loss"):
        assert callable(getattr(_lib, fn))
    assert lib.arl_abi_version() == 5
    p = 4096                                                    # any aligned non-null address (never dereferenced)

    def frac(lg=p, b=1, n=8, s=8, tau=p, hat=p):
        return lib.arl_fqf_fractions(lg, b, n, s, tau, hat, None, None, None, None, None)

    def act(th=p, tau=p, b=1, a=4, k=8, s=4, out=p):
        return lib.arl_fqf_act(th, tau, None, b, a, k, s, out, None, None)

    def loss(pred=p, mid=p, b=1, a=4, n=8, s=4, ns=8, kappa=1.0, ent=0.0, dl=p, fr=p, tau=p, q=p):
        return lib.arl_fqf_loss(pred, mid, tau, p, q, p, p, p, None, p, p, p, None, b, a, n, s, ns, 0.99, kappa, ent, p, p, p,
                                dl, fr, None)

    assert frac(lg=None) == -1 and b"null" in lib.arl_last_error()
    assert frac(tau=None) == -1 and frac(hat=None) == -1
    assert act(th=None) == -1 and act(tau=None) == -1 and act(out=None) == -1
    assert loss(pred=None) == -1 and b"null" in lib.arl_last_error()
    assert loss(dl=None) == -1 and loss(fr=None) == -1 and loss(tau=None) == -1 and loss(q=None) == -1
    assert loss(mid=None) == -1                                 # N > 1 needs the pass at the inner fractions
    for n in (0, 65):
        assert frac(n=n, s=68) == -1 and b"fractions" in lib.arl_last_error()
        assert act(k=n) == -1 and loss(n=n, ns=68) == -1
    assert frac(b=0) == -1 and act(b=0) == -1 and loss(b=0) == -1
    assert frac(b=2 ** 31) == -1 and frac(b=2 ** 31 - 1, n=1, s=4) == -1        # batch x (N + 1) would pass 2^31
    assert act(b=2 ** 31 - 1, k=1) == -1 and loss(b=2 ** 31 - 1, n=1, ns=4) == -1
    for a, s in ((6, 10), (6, 4), (65, 68), (0, 4)):            # stride % 4, stride < n_actions, n_actions > 64, < 1
        assert act(a=a, s=s) == -1 and loss(a=a, s=s) == -1
    for ns in (4, 10, 2 ** 20 + 4):                             # n_stride < N, % 4, > 2^20
        assert frac(s=ns) == -1 and b"n_stride" in lib.arl_last_error()
        assert loss(ns=ns) == -1 and b"n_stride" in lib.arl_last_error()
    for bad in (-1.0, float("inf"), float("nan")):
        assert loss(kappa=bad) == -1 and b"kappa" in lib.arl_last_error()
        assert loss(ent=bad) == -1 and b"ent_coef" in lib.arl_last_error()
    assert frac(lg=p + 4) == -3 and b"alignment" in lib.arl_last_error()        # ARL_E_ALIGN
    assert loss(dl=p + 4) == -3 and b"alignment" in lib.arl_last_error()


def _smooth_quantile(omega):
    """A smooth, strictly increasing quantile function on [0, 1]."""
    return 2.0 * omega + 0.5 * torch.sin(3.0 * omega) + omega ** 3


@pytest.mark.parametrize("n,ent_coef", [(1, 0.01), (2, 0.0), (8, 0.0), (8, 0.01), (32, 0.01)])
def test_closed_form_dlogits_equal_autograd_through_the_integrated_w1(n, ent_coef):
    """d (W1 - ent_coef H) / d logits by autograd through 20 001-point trapezoids of the real 1-Wasserstein integral against
    ref_dlogits with g_i = 2 F^-1(tau_i) - F^-1(tau_hat_i) - F^-1(tau_hat_{i-1}): within 1e-8 of the largest entry."""
    rs = np.random.RandomState(n)
    logits = torch.from_numpy(rs.uniform(-1.5, 1.5, size=(1, n))).requires_grad_()
    fr = R.ref_fractions(logits)
    objective = R.wasserstein_1(_smooth_quantile, fr["tau"][0]) - ent_coef * fr["H"][0]
    want, = torch.autograd.grad(objective, logits)
    with torch.no_grad():
        tau, hat = fr["tau"], fr["tau_hat"]
        g = (2. * _smooth_quantile(tau[:, 1:n]) - _smooth_quantile(hat[:, 1:])) - _smooth_quantile(hat[:, :-1])
        got, frac = R.ref_dlogits(fr["q"], fr["logq"], fr["H"], tau, g, torch.ones(1, dtype=torch.float64), ent_coef)
    # ... and the surrogate w G - ent_coef H has the same gradient (g held fixed), though not W1's value
    fr2 = R.ref_fractions(logits)
    surrogate = (g[0] * fr2["tau"][0, 1:n]).sum() - ent_coef * fr2["H"][0]
    want2, = torch.autograd.grad(surrogate, logits)
    scale = max(want.abs().max().item(), 1e-300)
    print("N %d: max |closed form - autograd(W1)| %.3g, - autograd(surrogate) %.3g, of %.3g" % (
        n, (got - want).abs().max().item(), (got - want2).abs().max().item(), scale))
    if n == 1:
        assert not got.any() and not want.any()                 # one fraction: nothing to propose
        return
    assert (got - want).abs().max().item() <= 1e-8 * scale
    assert (got - want2).abs().max().item() <= 1e-13 * scale
    assert abs(got.sum().item()) <= 1e-14 * scale * n           # analytically sum_k dlogit_k = 0
    assert abs(frac.item() - (g[0] * tau[0, 1:n]).sum().item()) <= 1e-15 * max(abs(frac.item()), 1.)
