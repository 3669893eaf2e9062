"""PopArt without a GPU: the entry points' argument checks (they come back before any HIP call), the mixin's argument
validation and initialize's refusals, and properties of the restatements of tests/popart_ref.py in float64."""
import ctypes

import numpy as np
import pytest
import torch

import popart_ref

F32, F64 = np.float32, np.float64


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
    assert (_lib.POPART_MAX_ROWS, _lib.POPART_MAX_HID) == (1 << 22, 65536)
    assert "arl_popart_denorm" in _lib.EXPORTED_SYMBOLS and "arl_popart_step" in _lib.EXPORTED_SYMBOLS
    keep, p = _buf(4096)
    odd2, odd4 = p + 2, p + 4
    nan, inf = float("nan"), float("inf")
    # value_n [8] at p, last_n [2] at p + 64, stats at p + 128, value [8] at p + 256, last_value [2] at p + 512
    denorm = lambda **kw: lib.arl_popart_denorm(*[kw.get(k, d) for k, d in (                    # noqa: E731
        ("vn", p), ("rows", 8), ("ln", p + 64), ("n_last", 2), ("stats", p + 128), ("v", p + 256), ("lv", p + 512),
        ("stream", None))])
    for kw, code in ((dict(vn=None), -1), (dict(ln=None), -1), (dict(stats=None), -1), (dict(v=None), -1),
                     (dict(lv=None), -1), (dict(rows=0), -2), (dict(rows=(1 << 22) + 1), -2), (dict(n_last=0), -2),
                     (dict(n_last=9), -2),
                     # aliased outputs: the input itself, a partial overlap, the other input, the other output
                     (dict(v=p), -1), (dict(v=p + 28), -1), (dict(v=p + 60), -1), (dict(lv=p + 64), -1), (dict(lv=p), -1),
                     (dict(lv=p + 256 + 28), -1),
                     (dict(stats=p + 128 + 4), -3), (dict(vn=odd2), -3), (dict(ln=p + 64 + 2), -3), (dict(v=p + 256 + 2), -3),
                     (dict(lv=p + 512 + 2), -3)):
        assert denorm(**kw) == code, kw
        assert b"arl_popart_denorm" in lib.arl_last_error(), kw
    # returns [8] at p, advantages [8] at p + 64, valids at p + 128, stats at p + 256, w_value [4] at p + 512 + 4 (only
    # 4-byte aligned, as row A of W_head is for odd A * hid), b_value at p + 600, diag2 at p + 640
    step = lambda **kw: lib.arl_popart_step(*[kw.get(k, d) for k, d in (                        # noqa: E731
        ("ret", p), ("adv", p + 64), ("valids", p + 128), ("rows", 8), ("beta", 3e-4), ("smin", 1e-4), ("smax", 1e6),
        ("stats", p + 256), ("w", p + 512 + 4), ("b", p + 600 + 4), ("hid", 4), ("diag", p + 640), ("stream", None))])
    for kw, code in ((dict(ret=None), -1), (dict(stats=None), -1), (dict(w=None), -1), (dict(b=None), -1),
                     (dict(diag=None), -1),
                     (dict(beta=-0.1), -1), (dict(beta=1.1), -1), (dict(beta=nan), -1),
                     (dict(smin=0.), -1), (dict(smin=-1.), -1), (dict(smin=nan), -1), (dict(smax=inf), -1),
                     (dict(smax=nan), -1), (dict(smin=2., smax=1.), -1), (dict(adv=p), -1), (dict(adv=p + 28), -1),
                     (dict(rows=0), -2), (dict(rows=(1 << 22) + 1), -2), (dict(hid=0), -2), (dict(hid=65537), -2),
                     (dict(stats=p + 256 + 4), -3), (dict(ret=odd2), -3), (dict(adv=p + 64 + 2), -3),
                     (dict(w=p + 512 + 2), -3), (dict(b=p + 600 + 2), -3), (dict(diag=p + 640 + 2), -3)):
        assert step(**kw) == code, kw
        assert b"arl_popart_step" in lib.arl_last_error(), kw
    assert odd4 % 8 == 4
    del keep


# ---- constructors and initialize ---------------------------------------------------------------------------------------

def _classes():
    from accel_rl_amd.algos.pg import PopArtA2C, PopArtIMPALA, PopArtPPO, PopArtVMPO
    return PopArtA2C, PopArtPPO, PopArtVMPO, PopArtIMPALA


@pytest.mark.parametrize("kwargs,match", [
    (dict(beta=-0.1), "beta"), (dict(beta=1.1), "beta"), (dict(beta=float("nan")), "beta"), (dict(beta="0.1"), "beta"),
    (dict(beta=True), "beta"), (dict(sigma_min=0.), "sigma_min"), (dict(sigma_min=2., sigma_max=1.), "sigma_min"),
    (dict(sigma_max=float("inf")), "sigma_max"), (dict(popart_init=1.0), "popart_init"),
    (dict(popart_init=(0., float("nan"))), "popart_init"), (dict(popart_init=(0., 0.)), "popart_init"),
    (dict(popart_init=(0., 1e7)), "popart_init"), (dict(popart_init=(0., 1., 2.)), "popart_init")])
def test_constructor_refusals(kwargs, match):
    for cls in _classes():
        with pytest.raises(ValueError, match=match):
            cls(**kwargs)


class _Policy(object):
    """no value_head()"""
    recurrent = False


class _Headed(_Policy):
    def value_head(self):
        return torch.zeros(64), torch.zeros(1)


def test_defaults_and_initialize_refusals():
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.algos.pg.impala import IMPALA
    from accel_rl_amd.algos.pg.ppo import PPO
    from accel_rl_amd.algos.pg.vmpo import VMPO
    from accel_rl_amd.optimizers.single import A2cOptimizer, PpoOptimizer
    from accel_rl_amd.policies.dqn.atari_acer_policy import AtariAcerPolicy
    a2c_cls, ppo_cls, vmpo_cls, impala_cls = _classes()
    for cls, parent, keys in ((a2c_cls, A2C, ["GradNorm"]), (ppo_cls, PPO, ["GradNorm"]),
                              (vmpo_cls, VMPO, ["GradNorm", "Eta", "Alpha", "MeanKL"]),
                              (impala_cls, IMPALA, ["GradNorm", "RhoMean", "RhoClipFrac"])):
        algo = cls()
        assert isinstance(algo, parent) and algo.loss_kind == parent.loss_kind
        assert (algo.beta, algo.sigma_min, algo.sigma_max, algo.popart_init) == (3e-4, 1e-4, 1e6, (0., 1.))
        assert algo.opt_info_keys == keys + ["PopArtMu", "PopArtSigma"]
        assert algo._reuse_granted(dict()) is False
        with pytest.raises(RuntimeError, match="initialize"):
            algo.popart_state()
        with pytest.raises(RuntimeError, match="initialize"):
            algo.set_popart_state(0., 1., 1., 0.)

    class Recurrent(object):
        recurrent = True

    class SyncPpo(PpoOptimizer):
        parallelism_tag = "synchronous"

    class SyncA2c(A2cOptimizer):
        parallelism_tag = "synchronous"
    for cls in _classes():
        with pytest.raises(NotImplementedError, match=r"recurrent.*section E"):
            cls().initialize(Recurrent(), None, 40, 5, True)
        with pytest.raises(NotImplementedError, match=r"value_head.*section E"):
            cls().initialize(_Policy(), None, 40, 5, True)
        with pytest.raises(NotImplementedError, match=r"value_head.*section E"):
            cls().initialize(AtariAcerPolicy.__new__(AtariAcerPolicy), None, 40, 5, True)
        with pytest.raises(ValueError, match=r"arl_popart_step.*section E"):
            cls().initialize(_Headed(), None, (1 << 22) + 1, 1, True)
    with pytest.raises(NotImplementedError, match=r"single GPU only.*diverge.*section E"):
        ppo_cls(OptimizerCls=SyncPpo).initialize(_Headed(), None, 40, 5, True)
    with pytest.raises(NotImplementedError, match=r"single GPU only.*diverge.*section E"):
        a2c_cls(OptimizerCls=SyncA2c).initialize(_Headed(), None, 40, 5, True)
    # mid_batch_reset=False: A2C and PPO take it (valids); V-MPO's and IMPALA's own refusals stand
    for cls in (vmpo_cls, impala_cls):
        with pytest.raises(NotImplementedError, match=r"mid_batch_reset=False.*section E"):
            cls().initialize(_Headed(), None, 40, 5, False)


def test_value_head_is_refused_where_the_output_layers_differ():
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.dqn.atari_acer_policy import AtariAcerPolicy
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    for cls in (AtariAcerPolicy, AtariDqnPolicy):
        assert issubclass(cls, AtariCnnPolicy)
        with pytest.raises(NotImplementedError, match="value row"):
            cls.__new__(cls).value_head()


# ---- the restatements --------------------------------------------------------------------------------------------------------

def test_preservation_is_exact_where_the_arithmetic_is_and_within_rounding_elsewhere():
    # returns -1 and 3 in equal numbers, beta 1: mu' = 1, nu' = 5, sigma' = 2 -- every operation below is exact
    ret = np.array([3., -1.] * 6, F32)
    w, b = np.array([0.5, -1.25, 2., 0.75], F64), np.array([0.375], F64)
    h = np.array([[1., 2., 0.5, 4.], [0., 0., 0., 0.], [-3., 0.25, 8., 1.]], F64)
    before = popart_ref.unnormalized_head(h, w, b, popart_ref.INIT_STATS)
    ret_n, adv_n, stats, w_n, b_n, diag = popart_ref.step(ret, ret.copy(), None, 1.0, 1e-4, 1e6, popart_ref.INIT_STATS, w, b)
    assert stats.tolist() == [1., 5., 2., 1.] and diag.tolist() == [1., 2.]
    assert np.array_equal(w_n, w / 2) and b_n[0] == (0.375 - 1.) / 2
    assert np.array_equal(popart_ref.unnormalized_head(h, w_n, b_n, stats), before)
    assert np.array_equal(ret_n, np.array([1., -1.] * 6, F32)) and np.array_equal(adv_n, ret / 2)
    # random float64 weights, three consecutive steps from a state that is not the initial one: a few roundings
    rs = np.random.RandomState(0)
    w, b = rs.randn(64), rs.randn(1)
    h = np.maximum(rs.randn(16, 64), 0)
    stats = np.array([0.7, 0.7 * 0.7 + 9., 3., 5.])
    before = popart_ref.unnormalized_head(h, w, b, stats)
    for k in range(3):
        ret = (rs.randn(100) * 10. ** k + 5.).astype(F32)
        _, _, stats, w, b, _ = popart_ref.step(ret, None, None, 0.3, 1e-4, 1e6, stats, w, b)
        after = popart_ref.unnormalized_head(h, w, b, stats)
        assert np.abs(after - before).max() <= 1e-13 * np.abs(before).max()
    assert stats[3] == 8 and stats[2] > 3.


def test_the_clamps_engage_and_the_skipped_update_keeps_every_bit():
    w, b = np.array([1., -2.], F32), np.array([0.5], F32)
    # all returns equal, beta 1: nu' - mu'^2 = 0 exactly, sigma_min decides
    ret = np.full(50, 3.5, F32)
    ret_n, _, stats, w_n, b_n, diag = popart_ref.step(ret, None, None, 1.0, 1e-4, 1e6, popart_ref.INIT_STATS, w, b)
    assert stats.tolist() == [3.5, 12.25, 1e-4, 1.] and diag[1] == F32(1e-4) and (ret_n == 0).all()
    assert np.allclose(w_n, w * 1e4, rtol=1e-7) and np.isclose(b_n[0], (0.5 - 3.5) * 1e4, rtol=1e-7)
    # 1e6 with the smallest float32 spread around it: the difference of two numbers near 1e12 cancels to something >= 0
    ret = np.array([1e6, np.nextafter(F32(1e6), F32(2e6))] * 10, F32)
    _, _, stats, _, _, _ = popart_ref.step(ret, None, None, 1.0, 1e-4, 1e6, popart_ref.INIT_STATS, w, b)
    assert 1e-4 <= stats[2] <= 0.1 and stats[1] - stats[0] * stats[0] >= 0
    # sigma_max
    _, _, stats, _, _, _ = popart_ref.step((ret * 1e3 * np.array([1, -1] * 10)).astype(F32), None, None, 1.0, 1e-4, 100.,
                                           popart_ref.INIT_STATS, w, b)
    assert stats[2] == 100.
    # no valid row, and one infinite return: statistics and head keep their bits; the targets go by the old statistics
    old = np.array([2., 13., 3., 7.])
    ret = np.array([5., -1., 8., 2.], F32)
    for valids, rets in ((np.zeros(4, np.int8), ret), (None, np.array([5., np.inf, 8., 2.], F32)),
                         (np.array([1, 0, 1, 1], np.int8), np.array([np.inf, 4., 8., 2.], F32))):
        ret_n, adv_n, stats, w_n, b_n, diag = popart_ref.step(rets, ret.copy(), valids, 0.5, 1e-4, 1e6, old, w, b)
        assert np.array_equal(stats, old) and np.array_equal(w_n, w) and np.array_equal(b_n, b)
        assert diag.tolist() == [2., 3.]
        if valids is not None and not valids.any():
            assert (ret_n == 0).all() and (adv_n == 0).all()
    # an infinite return in a row that valids masks out does not reach the sums
    ret_n, _, stats, _, _, _ = popart_ref.step(np.array([5., np.inf, 8., 2.], F32), None, np.array([1, 0, 1, 1], np.int8),
                                               0.5, 1e-4, 1e6, old, w, b)
    assert stats[3] == 8 and stats[0] == 0.5 * 2. + 0.5 * 5. and ret_n[1] == 0 and np.isfinite(ret_n).all()


def test_beta_zero_from_the_initial_statistics_is_the_identity_and_denorm_inverts_the_targets():
    rs = np.random.RandomState(1)
    ret, adv = rs.randn(70).astype(F32) * 30, rs.randn(70).astype(F32)
    w, b = rs.randn(8).astype(F32), rs.randn(1).astype(F32)
    ret_n, adv_n, stats, w_n, b_n, diag = popart_ref.step(ret, adv, None, 0., 1e-4, 1e6, popart_ref.INIT_STATS, w, b)
    bits = lambda a: a.view(np.uint32)                                                          # noqa: E731
    assert all(np.array_equal(bits(x), bits(y)) for x, y in ((ret_n, ret), (adv_n, adv), (w_n, w), (b_n, b)))
    assert stats.tolist() == [0., 1., 1., 1.]
    v, lv = popart_ref.denorm(ret, ret[:3], popart_ref.INIT_STATS)
    assert np.array_equal(bits(v), bits(ret)) and np.array_equal(bits(lv), bits(ret[:3]))
    # denorm under the new statistics takes the normalised targets back to the returns (two float32 roundings)
    ret_n, _, stats, _, _, _ = popart_ref.step(ret, None, None, 0.5, 1e-4, 1e6, popart_ref.INIT_STATS, w, b)
    back, _ = popart_ref.denorm(ret_n, ret_n[:1], stats)
    assert np.allclose(back, ret, rtol=0, atol=2. ** -22 * (np.abs(ret).max() + abs(stats[0])))
