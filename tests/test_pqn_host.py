"""PQN without a GPU: the yardsticks of tests/pqn_ref.py against autograd and against the identities of Q(lambda), the
constructor refusals of AtariPqnPolicy / PQN and the defaults table."""
import numpy as np
import pytest
import torch

import pqn_ref as pr


# ---- the LayerNorm yardstick ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,width", [(1, 4), (3, 32), (7, 100), (5, 1024)])
def test_analytic_ln_backward_equals_float64_autograd(rows, width):
    rs = np.random.RandomState(rows * 1000 + width)
    z = rs.randn(rows, width).astype(np.float32)
    z[0, 0] = 40.0                                              # a row with one large entry
    gamma = (1.0 + 0.5 * rs.randn(width)).astype(np.float32)
    beta = (0.3 * rs.randn(width)).astype(np.float32)
    dy = rs.randn(rows, width).astype(np.float32)
    eps = 1e-5
    zt, gt, bt = (torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in (z, gamma, beta))
    y = pr._ln_relu_torch(zt, gt, bt, float(np.float32(eps)), 1)
    want = torch.autograd.grad((y * torch.from_numpy(dy.astype(np.float64))).sum(), (zt, gt, bt))
    y64, mean, rstd = pr.ln_relu_fwd64(z, gamma, beta, eps)
    np.testing.assert_allclose(y64, y.detach().numpy(), rtol=1e-12, atol=0)
    got = pr.ln_relu_bwd64(dy, y64 > 0, z, gamma, eps)
    assert (y64 > 0).any() and not (y64 > 0).all()
    for g, w in zip(got, want):
        w = w.numpy()
        assert np.abs(g - w).max() <= 1e-12 * np.abs(w).max()


def test_ln_constant_row():
    """var = 0: finite output, xhat = 0 (y = max(0, beta)); dz = rstd (h - mean h), which is 0 where h is constant over
    the row."""
    z = np.full((2, 8), 0.75, np.float32)
    gamma, beta = np.full(8, 2.0, np.float32), np.linspace(-1, 1, 8).astype(np.float32)
    y, mean, rstd = pr.ln_relu_fwd64(z, gamma, beta, 1e-5)
    np.testing.assert_array_equal(y, np.maximum(beta.astype(np.float64), 0)[None].repeat(2, 0))
    assert np.isfinite(rstd).all()
    dz, _, _ = pr.ln_relu_bwd64(np.ones((2, 8), np.float32), np.ones((2, 8), bool), z, gamma, 1e-5)
    np.testing.assert_array_equal(dz, 0.0)


def test_ln_shape_restates_the_dispatch_table():
    assert pr.ln_shape(1031, 32)[:4] == (8, 1, 33, 1) and pr.ln_shape(1031, 64)[:4] == (16, 1, 65, 1)
    assert pr.ln_shape(1031, 100)[:4] == (64, 1, 256, 2) and pr.ln_shape(3, 512)[:3] == (64, 2, 1)
    assert pr.ln_shape(65, 1024)[:3] == (64, 4, 17) and pr.ln_shape(1, 4)[4] == 7 and pr.ln_shape(1, 1024)[4] == 22


# ---- Q(lambda) identities -----------------------------------------------------------------------------------------------

def _rollout(seed, n_env, horizon, n_act, stride=8, p_done=0.0):
    rs = np.random.RandomState(seed)
    return dict(q=rs.randn(n_env, horizon, stride).astype(np.float32), q_last=rs.randn(n_env, stride).astype(np.float32),
                r=rs.randn(n_env, horizon).astype(np.float32), d=(rs.rand(n_env, horizon) < p_done).astype(np.uint8),
                n_act=n_act)


def _boot(c):
    a = c["n_act"]
    return np.concatenate([c["q"][:, 1:, :a].max(axis=2), c["q_last"][:, None, :a].max(axis=2)], axis=1).astype(np.float64)


def test_scan_lambda_0_is_the_one_step_target():
    c = _rollout(1, 5, 7, 3, p_done=0.3)
    got = pr.qlambda_scan64(c["q"], c["q_last"], 3, c["r"], c["d"], 0.9, 0.0)
    keep = (c["d"] == 0).astype(np.float64)
    want = c["r"].astype(np.float64) + keep * (0.9 * _boot(c))          # b_t + 0 * (R - b_t) = b_t exactly
    np.testing.assert_array_equal(got, want.astype(np.float32))
    assert c["d"].any() and not c["d"].all()


def test_scan_lambda_1_without_dones_is_the_discounted_sum():
    c = _rollout(2, 4, 9, 4)
    got = pr.qlambda_scan64(c["q"], c["q_last"], 4, c["r"], c["d"], 0.95, 1.0).astype(np.float64)
    t = np.arange(9)
    for e in range(4):
        for s in range(9):
            want = (0.95 ** (t[s:] - s) * c["r"][e, s:]).sum() + 0.95 ** (9 - s) * c["q_last"][e, :4].max()
            assert abs(got[e, s] - want) <= 1e-6 * max(1.0, abs(want))       # (float32 storage of the result)


def test_scan_done_cuts_the_return():
    c = _rollout(3, 3, 8, 2)
    c["d"][:, 4] = 1
    got = pr.qlambda_scan64(c["q"], c["q_last"], 2, c["r"], c["d"], 0.99, 0.65)
    np.testing.assert_array_equal(got[:, 4], c["r"][:, 4])
    other = dict(c, q=c["q"].copy(), q_last=c["q_last"] + 5, r=c["r"].copy())
    other["q"][:, 5:] += 3.0                                    # everything after t = 4, and its bootstrap row (t + 1 = 5)
    other["r"][:, 5:] -= 2.0
    got2 = pr.qlambda_scan64(other["q"], other["q_last"], 2, other["r"], other["d"], 0.99, 0.65)
    np.testing.assert_array_equal(got2[:, :5], got[:, :5])
    assert not np.array_equal(got2[:, 5:], got[:, 5:])


def test_scan_reads_only_the_first_n_actions_and_ties_do_not_matter():
    c = _rollout(4, 2, 3, 3)
    c["q"][:, :, 3:] = 100.0                                    # padding columns
    c["q"][0, 1, :3] = [0.5, 0.5, -1.0]                         # two equal maxima
    got = pr.qlambda_scan64(c["q"], c["q_last"], 3, c["r"], c["d"], 0.9, 0.5)
    assert np.abs(got).max() < 50


# ---- regression loss yardsticks agree with one another ----------------------------------------------------------------

@pytest.mark.parametrize("clip", [None, 1.0, 0.25])
def test_regress32_within_the_float64_bound(clip):
    rs = np.random.RandomState(7)
    q = rs.randn(64, 8).astype(np.float32)
    act, ret = rs.randint(0, 6, 100).astype(np.uint8), rs.randn(100).astype(np.float32)
    idx = rs.permutation(100)[:64].astype(np.int32)
    dq, rows, td = pr.q_regress32(q, idx, act, ret, 6, clip)
    ref = pr.q_regress64(q, idx, act, ret, 6, clip)
    ok = ref["ok"]
    assert ok.sum() >= 60
    assert (np.abs(rows - ref["rows"])[ok] <= ref["rows_tol"][ok]).all()
    assert (np.abs(td - ref["td"])[ok] <= ref["td_tol"][ok]).all()
    assert (np.abs(dq[:, :6] - ref["dq"]).max(axis=1)[ok] <= ref["dq_tol"][ok]).all()
    assert (dq[:, 6:] == 0).all()


# ---- refusals and defaults ----------------------------------------------------------------------------------------------

def _spec(**kw):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    return dict(dict(cnn_specs[0], hidden_sizes=[64]), **kw)


@pytest.mark.parametrize("kw", [dict(dueling=True), dict(shared_last_bias=True), dict(hidden_sizes=[]),
                                dict(hidden_sizes=[1028]), dict(hidden_sizes=[62]), dict(conv_filters=[16, 30]),
                                dict(conv_filters=[2048, 32])])
def test_policy_refusals(kw):
    from accel_rl_amd.policies.dqn.atari_pqn_policy import AtariPqnPolicy
    with pytest.raises(NotImplementedError, match="section E"):
        AtariPqnPolicy(**_spec(**kw))
    AtariPqnPolicy(**_spec())                                   # the plain network is taken
    with pytest.raises(ValueError):
        AtariPqnPolicy(ln_eps=0.0, **_spec())


def test_policy_refuses_the_replay_losses():
    from accel_rl_amd.policies.dqn.atari_pqn_policy import AtariPqnPolicy
    policy = AtariPqnPolicy(**_spec())
    for name in ("q_loss_and_grads", "drq_loss_and_grads", "munchausen_loss_and_grads"):
        with pytest.raises(NotImplementedError, match="pqn_loss_and_grads"):
            getattr(policy, name)(None, None)
    assert policy.serves_rows is False


def test_algo_refusals():
    from accel_rl_amd.algos.dqn.pqn import PQN
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.policies.dqn.atari_pqn_policy import AtariPqnPolicy

    class Sub(AtariPqnPolicy):
        pass
    for policy in (AtariDqnPolicy(**_spec()), Sub(**_spec())):
        with pytest.raises(TypeError, match="AtariPqnPolicy"):
            PQN().initialize(policy, None, 128, 8, True)
    with pytest.raises(NotImplementedError, match="mid_batch_reset"):
        PQN().initialize(AtariPqnPolicy(**_spec()), None, 128, 8, False)
    for kw in (dict(discount=1.5), dict(q_lambda=-0.1), dict(q_lambda=float("nan")), dict(delta_clip=0.0),
               dict(delta_clip=float("inf"))):
        with pytest.raises(ValueError):
            PQN(**kw)
    with pytest.raises(TypeError):
        PQN(eps_greedy_args=dict(anneal=3))
    with pytest.raises(ValueError):
        PQN(lr_schedule="cosine")


def test_defaults_table():
    from accel_rl_amd.algos.dqn.pqn import PQN, MINIBATCHES_PER_EPOCH
    from accel_rl_amd.optimizers.single import PpoOptimizer
    algo = PQN()
    opt = algo.optimizer
    assert type(opt) is PpoOptimizer and opt.parallelism_tag == "single"
    assert (algo.discount, algo.q_lambda, algo.delta_clip, algo.lr_schedule) == (0.99, 0.65, None, "linear")
    assert (opt._epochs, opt._minibatch_size, opt._learning_rate, opt._grad_norm_clip) == (2, None, 2.5e-4, 10)
    assert opt._update_method.name == "adam" and opt._update_args["epsilon"] == 1e-5 and MINIBATCHES_PER_EPOCH == 32
    assert (algo._eps_initial, algo._eps_final, algo._eps_eval) == (1.0, 0.001, 0.0)
    assert algo._eps_anneal_steps is None and algo._eps_anneal_fraction == 0.1
    assert algo.need_extra_obs is True and algo.opt_info_keys == ["Loss", "TdAbs", "GradNorm"]

    class FakePolicy(object):
        eps = None

        def set_epsilon(self, v):
            self.eps = v

        def get_epsilon(self):
            return self.eps
    algo.policy = FakePolicy()
    algo.set_n_itr(200)                                         # epsilon 1 -> 0.001 over the first 10 % of the run
    assert algo._eps_anneal_itr == 20
    for itr, want in ((0, 1.0), (10, 0.5005), (20, 0.001), (150, 0.001)):
        algo.update_epsilon(itr)
        assert abs(algo.policy.eps - want) < 1e-12
    algo.prep_eval(5)
    assert algo.policy.eps == 0.0
    algo.post_eval(5)
    assert algo.policy.eps == 0.001
    custom = PQN(optimizer_args=dict(minibatch_size=64, epochs=3), eps_greedy_args=dict(anneal_steps=1000, final=0.05))
    assert (custom.optimizer._minibatch_size, custom.optimizer._epochs, custom._eps_final) == (64, 3, 0.05)
