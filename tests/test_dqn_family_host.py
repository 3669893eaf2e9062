"""CPU-only: what the six value-based algorithms' `build_loss` hands to their policy.  The policy's `*_loss_and_grads`
is replaced by a recorder; the `inputs` list, the unpacked minibatch (the same tensors, bool terminals as a uint8 view
of the same storage, host importance weights as a float32 tensor, None when replay is uniform), the algorithm's
scalars in their positional order, `double_dqn` as a keyword where it is one, and the order of the returned pair."""
import numpy as np
import pytest
import torch

BASE = ["obs", "next_obs", "act", "disc_n_return", "terminal"]
B = 5


def _spec():
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    return dict(cnn_specs[0])


def _cases():
    """name -> (algorithm class, its arguments, policy factory, recorded method, scalars(algo), keywords(algo))"""
    from accel_rl_amd.algos.dqn.cat_dqn import CategoricalDQN
    from accel_rl_amd.algos.dqn.dqn import DQN
    from accel_rl_amd.algos.dqn.iqn import ImplicitQuantileDQN
    from accel_rl_amd.algos.dqn.munchausen import MunchausenDQN, MunchausenIQN
    from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
    from accel_rl_amd.policies.dqn.atari_cat_dqn_policy import AtariCatDqnPolicy
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    from accel_rl_amd.policies.dqn.atari_qr_dqn_policy import AtariQrDqnPolicy

    def g_n(a):
        return float(np.float32(a.discount ** a.reward_horizon))

    def g_1(a):
        return float(np.float32(a.discount))

    def dbl(a):
        return dict(double_dqn=a.double_dqn)

    n_step = dict(discount=0.97, reward_horizon=3, double_dqn=True)
    return dict(
        dqn=(DQN, dict(delta_clip=0.5, **n_step), AtariDqnPolicy, "q_loss_and_grads",
             lambda a: (g_n(a), a.delta_clip), dbl),
        cat=(CategoricalDQN, dict(V_min=-3, V_max=7, **n_step), AtariCatDqnPolicy, "cat_loss_and_grads",
             lambda a: (a.V_min, a.V_max, g_n(a)), dbl),
        qr=(QuantileDQN, dict(kappa=0.25, **n_step), AtariQrDqnPolicy, "qr_loss_and_grads",
            lambda a: (g_n(a), a.kappa), dbl),
        iqn=(ImplicitQuantileDQN, dict(kappa=0.25, **n_step), AtariIqnPolicy, "iqn_loss_and_grads",
             lambda a: (g_n(a), a.kappa), dbl),
        mdqn=(MunchausenDQN, dict(discount=0.97, delta_clip=0.5, entropy_tau=0.05, munchausen_alpha=0.8,
                                  munchausen_clip=-2.), AtariDqnPolicy, "munchausen_loss_and_grads",
              lambda a: (g_1(a), a.delta_clip, a.entropy_tau, a.munchausen_alpha, a.munchausen_clip), lambda a: dict()),
        miqn=(MunchausenIQN, dict(discount=0.97, kappa=0.25, entropy_tau=0.05, munchausen_alpha=0.8,
                                  munchausen_clip=-2.), AtariIqnPolicy, "munchausen_loss_and_grads",
              lambda a: (g_1(a), a.kappa, a.entropy_tau, a.munchausen_alpha, a.munchausen_clip), lambda a: dict()),
    )


def _minibatch(prioritized):
    obs = torch.zeros((B, 4, 8, 8), dtype=torch.uint8)
    next_obs = torch.ones((B, 4, 8, 8), dtype=torch.uint8)
    act = torch.arange(B, dtype=torch.uint8)
    ret = torch.linspace(-1., 1., B)
    term = torch.tensor([False, True, False, False, True])
    mb = [obs, next_obs, act, ret, term]
    if prioritized:
        mb.append(np.linspace(0.25, 1., B))                     # float64 on the host, as a NumPy replay hands them out
    return mb


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
@pytest.mark.parametrize("name", ["dqn", "cat", "qr", "iqn", "mdqn", "miqn"])
def test_build_loss_hands_the_policy_the_unpacked_minibatch(name, prioritized):
    algo_cls, algo_kw, policy_cls, method, scalars, keywords = _cases()[name]
    algo = algo_cls(prioritized_replay=prioritized, **algo_kw)
    policy = policy_cls(**_spec())
    policy.device = "cpu"
    calls = []
    first, second = torch.full((B,), 1.), torch.full((B,), 2.)

    def recorder(*args, **kwargs):
        calls.append((args, kwargs))
        return first, second                    # (loss_rows, priorities) as every *_loss_and_grads returns them

    setattr(policy, method, recorder)
    inputs, loss = algo.build_loss(None, policy)
    assert inputs == BASE + (["importance_sample_weights"] if prioritized else [])
    if name == "cat":
        np.testing.assert_array_equal(policy.z.numpy(), np.linspace(-3, 7, policy.n_atoms, dtype=np.float32))
    mb = _minibatch(prioritized)
    out = loss(mb)
    (args, kwargs), = calls
    for got, want in zip(args[:4], mb[:4]):
        assert got is want
    term_u8 = args[4]
    assert term_u8.dtype == torch.uint8 and term_u8.data_ptr() == mb[4].data_ptr()
    assert term_u8.tolist() == [0, 1, 0, 0, 1]
    isw = args[5]
    if prioritized:
        assert isinstance(isw, torch.Tensor) and isw.dtype == torch.float32 and isw.device.type == "cpu"
        np.testing.assert_array_equal(isw.numpy(), np.linspace(0.25, 1., B).astype(np.float32))
    else:
        assert isw is None
    want_scalars = scalars(algo)
    assert args[6:] == want_scalars and [type(v) for v in args[6:]] == [type(v) for v in want_scalars]
    assert kwargs == keywords(algo)
    assert out[0] is second and out[1] is first                 # (priorities, loss_rows)
    # a device tensor of weights and uint8 terminals pass through as they are
    if prioritized:
        mb2 = _minibatch(True)
        mb2[4] = mb2[4].view(torch.uint8)
        mb2[5] = torch.linspace(0.5, 1., B)
        loss(mb2)
        args2 = calls[-1][0]
        assert args2[4] is mb2[4] and args2[5] is mb2[5]
