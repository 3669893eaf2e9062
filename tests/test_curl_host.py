"""CURL without a GPU: the two entry points' refusals (before any HIP call), CURL's defaults and its refusals."""
import pytest

E_ARG, E_RANGE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    return _lib.load()


def test_the_entry_points_are_bound_and_refuse_before_any_hip_call(lib):
    from accel_rl_amd import _lib
    assert lib.arl_abi_version() == 5
    assert {"arl_curl_loss_parts", "arl_curl_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    for width, want in ((4, 64 * 4 * (16 + 4)), (128, 64 * 4 * (128 * 128 + 4)), (0, 0), (6, 0), (132, 0), (-4, 0)):
        assert lib.arl_curl_workspace_bytes(width) == want, width
    p = 4096                                    # any aligned non-null address: a refused call reads none of them

    def call(zq=p, zk=p, w=p, batch=8, width=8, coef=1.0, dzq=p, dw=p, loss2=p, ws=p):
        return lib.arl_curl_loss_parts(zq, zk, w, batch, width, coef, dzq, dw, loss2, ws, None, None)

    for name in ("zq", "zk", "w", "dzq", "dw", "loss2", "ws"):
        assert call(**{name: None}) == E_ARG and b"null" in lib.arl_last_error(), name
    assert call(coef=float("nan")) == E_ARG and call(coef=float("inf")) == E_ARG
    for kw in (dict(batch=0), dict(batch=4097), dict(batch=-1), dict(width=0), dict(width=2), dict(width=6),
               dict(width=132)):
        assert call(**kw) == E_RANGE, kw


def test_curl_defaults_and_refusals():
    from accel_rl_amd.algos.dqn import CURL
    from accel_rl_amd.algos.dqn.drq import DrQ
    from accel_rl_amd.optimizers.dqn import CurlOptimizer, DqnOptimizer
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn import AtariCurlDqnPolicy
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    algo, drq = CURL(), DrQ()
    assert (algo.curl_coef, algo.latent, algo.momentum_tau) == (1.0, 128, 0.001)
    assert algo._replay_augment == dict(pad=4, seed=0, m_obs=2, k_next=1) and isinstance(algo.optimizer, CurlOptimizer)
    for name in ("double_dqn", "dueling_dqn", "reward_horizon", "batch_size", "replay_size", "min_steps_learn",
                 "training_intensity", "target_update_steps"):
        assert getattr(algo, name) == getattr(drq, name), name
    assert algo._get_default_sub_args() == drq._get_default_sub_args()
    assert CURL(prioritized_replay=True).prioritized_replay
    with pytest.raises(TypeError, match="augment_args"):
        CURL(augment_args=dict(pad=4))
    with pytest.raises(TypeError, match="CurlOptimizer"):
        CURL(OptimizerCls=DqnOptimizer)
    for latent in (0, 2, 6, 132, 64.0):
        with pytest.raises(ValueError, match="latent"):
            CURL(latent=latent)
        with pytest.raises(ValueError, match="latent"):
            AtariCurlDqnPolicy(latent=latent, **cnn_specs[0])
    for kw in (dict(curl_coef=-1.), dict(curl_coef=float("nan")), dict(momentum_tau=1.5), dict(pad=65)):
        with pytest.raises(ValueError):
            CURL(**kw)
    with pytest.raises(TypeError, match="AtariCurlDqnPolicy"):
        algo.build_loss(None, AtariDqnPolicy(dueling=True, **cnn_specs[0]))
    with pytest.raises(ValueError, match="latent"):
        algo.build_loss(None, AtariCurlDqnPolicy(dueling=True, latent=64, **cnn_specs[0]))
