"""CPU-only: the host side of implicit quantile networks -- constructor refusals, ImplicitQuantileDQN's refusals,
defaults and loss inputs, the parameter names and flat order (embedding between the conv and hidden layers), the
reference-layout conversion of the embedding layer, and the five exported entry points' argument checks."""
import numpy as np
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


def test_constructor_refusals_and_defaults():
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy, SERVE_PAIR_ROWS
    from accel_rl_amd.policies.dqn.q_policy_base import QPolicyBase
    for name in ("n_quantiles", "n_target_quantiles", "n_policy_quantiles"):
        for bad in (0, 65, -1):
            with pytest.raises(NotImplementedError, match=name):
                AtariIqnPolicy(**_spec(**{name: bad}))
        for ok in (1, 64):
            assert getattr(AtariIqnPolicy(**_spec(**{name: ok})), name) == ok
    with pytest.raises(NotImplementedError, match="dueling"):
        AtariIqnPolicy(dueling=True, **_spec())
    with pytest.raises(NotImplementedError):
        AtariIqnPolicy(**_spec(hidden_sizes=()))
    p = AtariIqnPolicy(epsilon=0.25, **_spec())
    assert isinstance(p, QPolicyBase) and not p._dueling and p.get_epsilon() == 0.25
    assert (p.n_quantiles, p.n_target_quantiles, p.n_policy_quantiles) == (8, 8, 32)
    assert p.serve_pair_rows == SERVE_PAIR_ROWS == 8192
    assert AtariIqnPolicy(**_spec()).get_epsilon() == 1


def test_algorithm_refusals_and_defaults():
    from accel_rl_amd.algos.dqn.dqn import DQN
    from accel_rl_amd.algos.dqn.iqn import ImplicitQuantileDQN
    from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    from accel_rl_amd.policies.dqn.atari_qr_dqn_policy import AtariQrDqnPolicy
    a = ImplicitQuantileDQN()
    assert isinstance(a, DQN) and a.kappa == 1.0 and a.batch_size == 32
    assert a._get_default_sub_args() == QuantileDQN()._get_default_sub_args()
    opt, eps, pri = a._get_default_sub_args()
    assert opt == dict(learning_rate=5e-5, update_method=update_methods.adam, grad_norm_clip=None,
                       update_method_args=dict(epsilon=0.01 / 32), scale_conv_grads=False)
    assert eps == dict(initial=1., final=0.01, eval=0.001, anneal_steps=int(1e6))
    assert pri == dict(alpha=0.6, beta_initial=0.4, beta_final=1., beta_anneal_steps=50e6, default_priority=1.)
    assert ImplicitQuantileDQN(kappa=0., batch_size=64).kappa == 0.
    for bad in (-1., float("inf"), float("nan")):
        with pytest.raises(ValueError, match="kappa"):
            ImplicitQuantileDQN(kappa=bad)
    with pytest.raises(NotImplementedError, match="dueling"):
        ImplicitQuantileDQN(dueling_dqn=True)
    with pytest.raises(TypeError, match="AtariIqnPolicy"):
        ImplicitQuantileDQN().build_loss(None, AtariQrDqnPolicy(**_spec()))
    base = ["obs", "next_obs", "act", "disc_n_return", "terminal"]
    inputs, loss = ImplicitQuantileDQN().build_loss(None, AtariIqnPolicy(**_spec()))
    assert inputs == base and callable(loss)
    inputs, _ = ImplicitQuantileDQN(prioritized_replay=True, double_dqn=True, reward_horizon=3).build_loss(
        None, AtariIqnPolicy(**_spec()))
    assert inputs == base + ["importance_sample_weights"]


def test_parameter_names_order_and_embedding_layout():
    """The layout hooks need no device: names and reference shapes in flat order, and the embedding layer's unit axis
    converted like the first dense layer's fan-in axis (NHWC-flatten inside, the reference's (c, h, w) outside)."""
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    p = AtariIqnPolicy(**_spec(hidden_sizes=(32, 16)))
    co, ho, wo = p._conv_out = (8, 3, 5)
    f = co * ho * wo
    p.n_act = 6
    ref, names, fan = p._hidden_reference_init(f)
    assert names == ["EmbW", "Embb", "FC0W", "FC0b", "FC1W", "FC1b"] and fan == 16
    assert [a.shape for a in ref] == [(64, f), (f,), (f, 32), (32,), (32, 16), (16,)]
    assert p._hidden_internal_shapes() == [(f, 64), (f,), (32, f), (32,), (16, 32), (16,)]
    np.testing.assert_allclose(np.square(ref[0]).sum(axis=0), 1., rtol=1e-5)         # the hidden layers' rule: NormC(1)
    rs = np.random.RandomState(0)
    ref = [rs.randn(*a.shape).astype(np.float32) for a in ref]
    internal = p._hidden_to_internal(ref)
    assert [a.shape for a in internal] == p._hidden_internal_shapes()
    back = p._hidden_to_reference(internal)
    for a, b in zip(ref, back):
        np.testing.assert_array_equal(a, b)
    # unit (c, h, w) of the reference is unit (h, w, c) inside -- for W_emb, b_emb and FC0's fan-in alike
    c, h, w = 5, 2, 3
    u_ref, u_int = (c * ho + h) * wo + w, (h * wo + w) * co + c
    np.testing.assert_array_equal(internal[0][u_int], ref[0][:, u_ref])
    assert internal[1][u_int] == ref[1][u_ref]
    np.testing.assert_array_equal(internal[2][:, u_int], ref[2][u_ref])
    head, head_names = p._head_reference_init(16, 6)
    assert head_names == ["OutputW", "Outputb"] and [a.shape for a in head] == [(16, 6), (6,)]
    assert p._head_width == 32 and p._head_internal_shapes(16, 6) == [(32, 16), (32,)]
    wi, bi = p._head_to_internal([rs.randn(16, 6).astype(np.float32), rs.randn(6).astype(np.float32)])
    assert not wi[6:].any() and not bi[6:].any()                                     # zero weights in the padding
    with pytest.raises(NotImplementedError, match="64 actions"):
        p._head_reference_init(16, 65)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        p._hidden_reference_init(30)


def test_the_library_exports_the_entry_points_and_refuses_bad_arguments(lib):
    from accel_rl_amd import _lib
    names = ("arl_iqn_embed", "arl_iqn_merge_fwd", "arl_iqn_merge_bwd", "arl_iqn_act", "arl_iqn_loss")
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    for fn in ("iqn_embed", "iqn_merge_fwd", "iqn_merge_bwd", "iqn_act", "iqn_loss"):
        assert callable(getattr(_lib, fn))
    assert lib.arl_abi_version() == 5
    # refused before any HIP call is made (no device here): nulls, then sizes (the pointers are never dereferenced)
    assert lib.arl_iqn_embed(None, None, 0, 0, 1, 1, None, None, None) == -1 and b"null" in lib.arl_last_error()
    assert lib.arl_iqn_merge_fwd(None, None, 1, 1, 4, None, None) == -1
    assert lib.arl_iqn_merge_bwd(None, None, None, 1, 1, 4, None, None, None) == -1
    assert lib.arl_iqn_act(None, None, 1, 4, 8, 4, None, None, None, 0, None) == -1
    assert lib.arl_iqn_loss(None, None, None, None, None, None, None, None, 1, 4, 8, 8, 4, 0.99, 1.0, None, None, None,
                            None, 0, None) == -1
    p = 4096                                                    # any aligned non-null address
    assert lib.arl_iqn_embed(None, None, 0, 0, 1, 1, p, p, None) == -1 and b"exactly one" in lib.arl_last_error()
    assert lib.arl_iqn_embed(p, p, 0, 0, 1, 1, p, p, None) == -1
    for r in (0, 65):
        assert lib.arl_iqn_embed(p, None, 0, 0, 1, r, p, p, None) == -1
        assert lib.arl_iqn_merge_fwd(p, p, 1, r, 4, p, None) == -1
        assert lib.arl_iqn_merge_bwd(p, p, p, 1, r, 4, p, p, None) == -1
        assert lib.arl_iqn_act(p, None, 1, 4, r, 4, p, None, None, 0, None) == -1
        assert lib.arl_iqn_loss(p, p, p, None, p, p, p, None, 1, 4, r, 8, 4, 0.99, 1.0, p, p, p, None, 0, None) == -1
        assert lib.arl_iqn_loss(p, p, p, None, p, p, p, None, 1, 4, 8, r, 4, 0.99, 1.0, p, p, p, None, 0, None) == -1
    assert lib.arl_iqn_embed(p, None, -1, 0, 1, 1, p, p, None) == -1
    assert lib.arl_iqn_embed(p, None, 2 ** 31 - 1, 0, 1, 2, p, p, None) == -1       # the pair index would pass 2^31
    assert lib.arl_iqn_merge_fwd(p, p, 1, 1, 6, p, None) == -1                      # f not a multiple of 4
    assert lib.arl_iqn_merge_fwd(p, p, 0, 1, 4, p, None) == -1
    for a, s in ((6, 10), (6, 4), (65, 68), (0, 4)):            # stride % 4, stride < n_actions, n_actions > 64, < 1
        assert lib.arl_iqn_act(p, None, 1, a, 8, s, p, None, None, 0, None) == -1
        assert lib.arl_iqn_loss(p, p, p, None, p, p, p, None, 1, a, 8, 8, s, 0.99, 1.0, p, p, p, None, 0, None) == -1
    for kappa in (-1.0, float("inf"), float("nan")):
        assert lib.arl_iqn_loss(p, p, p, None, p, p, p, None, 1, 4, 8, 8, 4, 0.99, kappa, p, p, p, None, 0, None) == -1
        assert b"kappa" in lib.arl_last_error()
