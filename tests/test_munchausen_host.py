"""CPU-only: the host side of Munchausen DQN / IQN -- constructor defaults, refusals and ValueErrors, the build_loss
type checks, the two exported entry points' argument checks, and a NumPy fp32 emulation of both target computations in
the kernels' stated order against float64, on the shapes of tests/test_munchausen_gpu.py: the derived bounds of
tests/munchausen_ref.py must hold for correctly rounded exp / log (they do with room to spare: the largest error is
0.20 of the M-DQN bound and 0.09 of the M-IQN bound), which keeps the bounds honest without a GPU."""
import numpy as np
import pytest

import munchausen_ref as mr


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


def _classes():
    from accel_rl_amd.algos.dqn.munchausen import MunchausenDQN, MunchausenIQN
    return MunchausenDQN, MunchausenIQN


def test_constructor_defaults():
    from accel_rl_amd.algos.dqn.dqn import DQN
    from accel_rl_amd.algos.dqn.iqn import ImplicitQuantileDQN
    from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
    from accel_rl_amd.optimizers import update_methods
    mdqn, miqn = _classes()
    a, i = mdqn(), miqn()
    assert isinstance(a, DQN) and not isinstance(a, QuantileDQN) and isinstance(i, ImplicitQuantileDQN)
    for algo in (a, i):
        assert (algo.entropy_tau, algo.munchausen_alpha, algo.munchausen_clip) == (0.03, 0.9, -1.0)
        assert algo.batch_size == 32 and algo.reward_horizon == 1 and not algo.double_dqn
        assert algo._get_default_sub_args() == QuantileDQN()._get_default_sub_args()
        opt, eps, pri = algo._get_default_sub_args()
        assert opt == dict(learning_rate=5e-5, update_method=update_methods.adam, grad_norm_clip=None,
                           update_method_args=dict(epsilon=0.01 / 32), scale_conv_grads=False)
        assert eps == dict(initial=1., final=0.01, eval=0.001, anneal_steps=int(1e6))
        assert pri == dict(alpha=0.6, beta_initial=0.4, beta_final=1., beta_anneal_steps=50e6, default_priority=1.)
    assert a.delta_clip == 1 and i.kappa == 1.0
    b = mdqn(entropy_tau=1., munchausen_alpha=0., munchausen_clip=0., batch_size=64, dueling_dqn=True)
    assert (b.entropy_tau, b.munchausen_alpha, b.munchausen_clip) == (1., 0., 0.)
    assert b._get_default_sub_args()[0]["update_method_args"] == dict(epsilon=0.01 / 64)
    assert b._get_default_sub_args()[0]["grad_norm_clip"] == 10
    assert miqn(kappa=0.).kappa == 0.


@pytest.mark.parametrize("which", [0, 1], ids=["mdqn", "miqn"])
def test_refusals_and_value_errors(which):
    cls = _classes()[which]
    with pytest.raises(NotImplementedError, match="double-DQN"):
        cls(double_dqn=True)
    for horizon in (0, 2, 3):
        with pytest.raises(NotImplementedError, match="n-step"):
            cls(reward_horizon=horizon)
    assert cls(reward_horizon=1, double_dqn=False).reward_horizon == 1
    for bad in (0., -0.03, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="entropy_tau"):
            cls(entropy_tau=bad)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="munchausen_alpha"):
            cls(munchausen_alpha=bad)
    for bad in (0.5, float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="munchausen_clip"):
            cls(munchausen_clip=bad)
    if which == 1:
        with pytest.raises(NotImplementedError, match="dueling"):
            cls(dueling_dqn=True)
        with pytest.raises(ValueError, match="kappa"):
            cls(kappa=-1.)


def test_build_loss_checks_the_policy_type():
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    from accel_rl_amd.policies.dqn.atari_noisy_net_dqn_policy import AtariNoisyNetDqnPolicy
    from accel_rl_amd.policies.dqn.atari_qr_dqn_policy import AtariQrDqnPolicy
    mdqn, miqn = _classes()
    base = ["obs", "next_obs", "act", "disc_n_return", "terminal"]
    inputs, loss = mdqn().build_loss(None, AtariDqnPolicy(**_spec()))
    assert inputs == base and callable(loss)
    inputs, loss = mdqn(dueling_dqn=True, prioritized_replay=True).build_loss(None, AtariDqnPolicy(dueling=True, **_spec()))
    assert inputs == base + ["importance_sample_weights"] and callable(loss)
    noisy = AtariNoisyNetDqnPolicy(**_spec())
    for other in (noisy, AtariQrDqnPolicy(**_spec()), AtariIqnPolicy(**_spec())):
        with pytest.raises(TypeError, match="AtariDqnPolicy"):
            mdqn().build_loss(None, other)
    with pytest.raises(NotImplementedError, match="noisy Munchausen"):
        noisy.munchausen_loss_and_grads(None, None, None, None, None, None, 0.99, 1., 0.03, 0.9, -1.)
    inputs, loss = miqn().build_loss(None, AtariIqnPolicy(**_spec()))
    assert inputs == base and callable(loss)
    inputs, _ = miqn(prioritized_replay=True).build_loss(None, AtariIqnPolicy(**_spec()))
    assert inputs == base + ["importance_sample_weights"]
    for other in (AtariDqnPolicy(**_spec()), AtariQrDqnPolicy(**_spec())):
        with pytest.raises(TypeError, match="AtariIqnPolicy"):
            miqn().build_loss(None, other)


def test_the_library_exports_the_entry_points_and_refuses_bad_arguments(lib):
    from accel_rl_amd import _lib
    for name in ("arl_mdqn_loss", "arl_miqn_loss"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert callable(_lib.mdqn_loss) and callable(_lib.miqn_loss)
    assert lib.arl_abi_version() == 5
    # refused before any HIP call is made (no device here): nulls, then sizes and constants (nothing is dereferenced)
    assert lib.arl_mdqn_loss(None, None, None, None, None, None, None, 1, 4, 4, 0, 0.99, 1.0, 0.03, 0.9, -1.0, None, None,
                             None, None) == -1 and b"null" in lib.arl_last_error()
    assert lib.arl_miqn_loss(None, None, None, None, None, None, None, None, 1, 4, 8, 8, 4, 0.99, 1.0, 0.03, 0.9, -1.0,
                             None, None, None, None, 0, None) == -1 and b"null" in lib.arl_last_error()
    p = 4096                                                    # any aligned non-null address

    def mdqn(cur=p, b=1, a=4, s=4, duel=0, te=0.03, al=0.9, l0=-1.0):
        return lib.arl_mdqn_loss(p, p, cur, p, p, p, None, b, a, s, duel, 0.99, 1.0, te, al, l0, p, p, p, None)

    def miqn(cur=p, b=1, a=4, n=8, m=8, s=4, kappa=1.0, te=0.03, al=0.9, l0=-1.0):
        return lib.arl_miqn_loss(p, p, p, cur, p, p, p, None, b, a, n, m, s, 0.99, kappa, te, al, l0, p, p, p, None, 0, None)

    assert mdqn(cur=None) == -1 and miqn(cur=None) == -1        # the target net on obs is mandatory
    for kw in (dict(b=0), dict(a=0), dict(a=256, s=256), dict(s=6), dict(a=5, s=4), dict(a=4, s=4, duel=1)):
        assert mdqn(**kw) == -2, kw                             # arl_dqn_loss's limits and code (ARL_E_RANGE)
    for kw in (dict(b=0), dict(a=0), dict(a=65, s=68), dict(s=6), dict(a=5, s=4), dict(n=0), dict(n=65), dict(m=0),
               dict(m=65), dict(kappa=-1.0), dict(kappa=float("nan"))):
        assert miqn(**kw) == -1, kw
    for call in (mdqn, miqn):
        for te in (0., -1., float("inf"), float("nan")):
            assert call(te=te) == -1 and b"tau_e" in lib.arl_last_error()
        for al in (-0.5, float("inf"), float("nan")):
            assert call(al=al) == -1 and b"alpha" in lib.arl_last_error()
        for l0 in (0.5, float("-inf"), float("nan")):
            assert call(l0=l0) == -1 and b"l0" in lib.arl_last_error()


@pytest.mark.parametrize("tau_e", mr.TAUS_E)
def test_fp32_emulation_of_the_mdqn_target_stays_within_the_bound(tau_e):
    worst = 0.
    seen = set()
    for n_act in mr.MDQN_ACTIONS:
        for batch in mr.MDQN_BATCHES:
            for dueling in ((False, True) if n_act <= 18 else (False,)):
                for scale in ((2.0,) if dueling else (2.0, 1e4)):   # (the bound knows the merged q, not val and adv)
                    c = mr.mdqn_case(mr.mdqn_seed(n_act, batch, dueling, True), n_act, batch, dueling, True, scale=scale,
                                     shift=n_act + int(dueling))
                    ref = mr.ref_mdqn(c, mr.GAMMA, 1.0, tau_e)
                    y = mr.emu_mdqn_y(c, mr.GAMMA, tau_e)
                    assert np.isfinite(y).all()
                    ratio = (np.abs(y.astype(np.float64) - ref["y"].numpy()) / ref["atol"].numpy()).max()
                    worst = max(worst, ratio)
                    seen.update(c["kinds"].tolist())
    print("M-DQN emulation, tau_e %g: largest error / bound %.3f" % (tau_e, worst))
    assert seen == set(range(mr.N_KINDS))
    assert worst <= 1., worst


@pytest.mark.parametrize("tau_e", mr.TAUS_E)
def test_fp32_emulation_of_the_miqn_targets_stays_within_the_bound(tau_e):
    worst = 0.
    seen = set()
    for k, shape in enumerate(mr.MIQN_SHAPES):
        n, m, n_act, stride = shape
        for batch in mr.MIQN_BATCHES:
            for weighted in (False, True):
                for scale in (2.0, 1e4):
                    c = mr.miqn_case(mr.miqn_seed(shape, batch, weighted), n, m, n_act, stride, batch, weighted,
                                     scale=scale, shift=k + 3 * int(weighted))
                    ref = mr.ref_miqn_targets(c, mr.GAMMA, tau_e)
                    T = mr.emu_miqn_targets(c, mr.GAMMA, tau_e)
                    assert np.isfinite(T).all()
                    ratio = (np.abs(T.astype(np.float64) - ref["T"].numpy()) / ref["atol"].numpy()).max()
                    worst = max(worst, ratio)
                    seen.update(c["kinds"].tolist())
    print("M-IQN emulation, tau_e %g: largest error / bound %.3f" % (tau_e, worst))
    assert seen == set(range(mr.N_KINDS))
    assert worst <= 1., worst


def test_the_reference_restates_the_two_exact_consequences():
    """alpha == 0 and a maximum unique by a wide gap: the float64 targets are the hard-max ones (the GPU file's bit-for-bit
    test rests on the same reduction); an all-equal row has lp = -tau_e ln A."""
    c = mr.mdqn_case(3, 6, 12, False, False)
    c["nxt"][:, :6] = np.clip(np.round(c["nxt"][:, :6]), -7, 7)
    c["nxt"][np.arange(12), c["act"]] = 9.
    ref = mr.ref_mdqn(c, 0.5, 0., 2.0 ** -10, alpha=0.)
    want = c["ret"].astype(np.float64) + (1. - c["term"]) * 0.5 * 9.
    np.testing.assert_allclose(ref["y"].numpy(), want, rtol=0, atol=1e-12)
    c = mr.mdqn_case(4, 18, 12, False, False)
    ref = mr.ref_mdqn(c, mr.GAMMA, 1., 0.03)
    rows = c["kinds"] == mr.ALL_EQUAL
    np.testing.assert_allclose(ref["lp_act"].numpy()[rows], -0.03 * np.log(18), rtol=1e-12)
    assert (ref["lp_act"].numpy()[c["kinds"] == mr.LP_ZERO] == 0).all()
    assert (ref["lp_act"].numpy()[c["kinds"] == mr.CLIPPED] < mr.L0).all()
    close = ref["lp_act"].numpy()[c["kinds"] == mr.CLOSE]
    assert ((close > mr.L0) & (close < 0)).all()
