"""CPU-only: the host side of quantile-regression DQN -- constructor refusals, QuantileDQN's defaults and loss inputs,
the dueling-mismatch assertion, and the two exported entry points."""
import pytest


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


def test_constructor_refusals():
    from accel_rl_amd.policies.dqn.atari_qr_dqn_policy import AtariQrDqnPolicy
    for kw in (dict(n_quantiles=1), dict(n_quantiles=65), dict(n_quantiles=0), dict(dueling=True, hidden_sizes=(256, 256)),
               dict(dueling=True, hidden_sizes=())):
        with pytest.raises(NotImplementedError):
            AtariQrDqnPolicy(**_spec(**kw))
    with pytest.raises(NotImplementedError, match="n_quantiles"):
        AtariQrDqnPolicy(n_quantiles=65, **_spec())
    for n in (2, 64):
        p = AtariQrDqnPolicy(n_quantiles=n, dueling=True, epsilon=0.25, **_spec())
        assert p.n_quantiles == n and p._dueling and p.get_epsilon() == 0.25
    p = AtariQrDqnPolicy(**_spec())
    assert p.n_quantiles == 64 and not p._dueling and p.get_epsilon() == 1
    with pytest.raises(NotImplementedError):                    # no support, no categorical loss
        p.incorporate_z([0.] * 64)
    with pytest.raises(NotImplementedError):
        p.cat_loss_and_grads()


def test_quantile_dqn_defaults():
    from accel_rl_amd.algos.dqn.dqn import DQN
    from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
    from accel_rl_amd.optimizers import update_methods
    a = QuantileDQN()
    assert isinstance(a, DQN) and a.kappa == 1.0 and a.batch_size == 32
    opt, eps, pri = a._get_default_sub_args()
    assert opt == dict(learning_rate=5e-5, update_method=update_methods.adam, grad_norm_clip=None,
                       update_method_args=dict(epsilon=0.01 / 32), scale_conv_grads=False)
    assert eps == dict(initial=1., final=0.01, eval=0.001, anneal_steps=int(1e6))
    assert pri == dict(alpha=0.6, beta_initial=0.4, beta_final=1., beta_anneal_steps=50e6, default_priority=1.)
    assert (a._eps_initial, a._eps_final, a._eps_eval) == (1., 0.01, 0.001)
    d = QuantileDQN(dueling_dqn=True, batch_size=64, kappa=0.)
    opt, _, _ = d._get_default_sub_args()
    assert opt["grad_norm_clip"] == 10 and opt["scale_conv_grads"] is True and d.kappa == 0.
    assert opt["update_method_args"] == dict(epsilon=0.01 / 64)
    for bad in (-1., float("inf"), float("nan")):
        with pytest.raises(ValueError, match="kappa"):
            QuantileDQN(kappa=bad)


def test_build_loss_inputs_and_dueling_mismatch():
    from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
    from accel_rl_amd.policies.dqn.atari_qr_dqn_policy import AtariQrDqnPolicy
    base = ["obs", "next_obs", "act", "disc_n_return", "terminal"]
    inputs, loss = QuantileDQN().build_loss(None, AtariQrDqnPolicy(**_spec()))
    assert inputs == base and callable(loss)
    inputs, _ = QuantileDQN(prioritized_replay=True, double_dqn=True, reward_horizon=3).build_loss(
        None, AtariQrDqnPolicy(**_spec()))
    assert inputs == base + ["importance_sample_weights"]
    inputs, _ = QuantileDQN(dueling_dqn=True).build_loss(None, AtariQrDqnPolicy(dueling=True, **_spec()))
    assert inputs == base
    with pytest.raises(AssertionError, match="dueling"):
        QuantileDQN().build_loss(None, AtariQrDqnPolicy(dueling=True, **_spec()))
    with pytest.raises(AssertionError, match="dueling"):
        QuantileDQN(dueling_dqn=True).build_loss(None, AtariQrDqnPolicy(**_spec()))


def test_the_library_exports_both_entry_points(lib):
    from accel_rl_amd import _lib
    for name in ("arl_qrdqn_act", "arl_qrdqn_loss"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert callable(_lib.qrdqn_act) and callable(_lib.qrdqn_loss)
    assert lib.arl_abi_version() == 5
    # null pointers are refused before any HIP call is made
    assert lib.arl_qrdqn_act(None, None, 1, 4, 8, 8, 0, None, None, None) == -1
    assert b"null" in lib.arl_last_error()
    assert lib.arl_qrdqn_loss(None, None, None, None, None, None, None, 1, 4, 8, 8, 0, 0.99, 1.0, None, None, None,
                              None) == -1
