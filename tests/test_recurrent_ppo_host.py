"""CPU-only: the host side of recurrent PPO.  TrajPpoOptimizer draws exactly the segments of the reference's
iterate_traj_idxs (optimizers/util.py:21-32; its stream is pinned by fixture G15), refuses sizes that do not divide
before the first update, and arl_traj_minibatch reports argument errors without a device."""
import ctypes
import types

import numpy as np
import pytest

from conftest import load_golden


def _sizes():
    g = load_golden("g15_trajidx")
    cases = [tuple(int(x) for x in g["c%d_cfg" % c]) for c in range(int(g["n_cases"]))]
    # (config 2's own sizes -- minibatch 512 of 1280 rows, horizon 5 -- do not divide: iterate_traj_idxs itself
    #  refuses them, see test_sizes_that_do_not_divide_are_refused_at_initialize; 640 is the nearest size that does)
    return cases + [(640, 1280, 5, 11)]


def _optimizer(minibatch_size, horizon, epochs, shuffle=True):
    """A TrajPpoOptimizer as far as `initialize` gets without a device (the bucket set-up needs the policy's)."""
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.single import TrajPpoOptimizer
    opt = TrajPpoOptimizer(learning_rate=1e-3, update_method=update_methods.adam, update_method_args=dict(epsilon=1e-5),
                           epochs=epochs, minibatch_size=minibatch_size, shuffle=shuffle)
    opt._horizon, opt._idx_host, opt._n_updates = horizon, None, 0
    opt._opt_state = types.SimpleNamespace(norm_log_len=1)
    return opt


@pytest.mark.parametrize("shuffle", [True, False])
def test_prepare_host_draws_the_reference_segments(shuffle):
    from accel_rl_amd.optimizers.base import iterate_traj_idxs
    epochs = 3
    for bs, n, horizon, seed in _sizes():
        np.random.seed(seed)
        want = [[segs for _, segs in iterate_traj_idxs(bs, n, horizon=horizon, shuffle=shuffle)] for _ in range(epochs)]
        after_ref = np.random.randint(0, 2 ** 31 - 1, size=2)
        opt = _optimizer(bs, horizon, epochs, shuffle)
        np.random.seed(seed)
        for call in range(2):                                   # the second call re-uses the buffer
            if call:
                np.random.seed(seed)
            opt.prepare_host(n)
            after = np.random.randint(0, 2 ** 31 - 1, size=2)
            np.testing.assert_array_equal(after, after_ref)    # same amount of the stream consumed
            got = opt._idx_host.numpy()
            per_epoch = n // bs
            assert got.dtype == np.int32 and got.shape == (epochs * per_epoch, bs // horizon)
            assert opt._n_minibatches == epochs * per_epoch
            for e in range(epochs):
                np.testing.assert_array_equal(got[e * per_epoch:(e + 1) * per_epoch], np.stack(want[e]))
        assert opt._opt_state.norm_log_len == min(epochs * per_epoch, 64)


@pytest.mark.parametrize("bs,n,horizon", [(12, 20, 5), (10, 25, 5), (10, 22, 5), (3, 20, 5), (512, 1280, 7), (512, 1280, 5)])
def test_sizes_that_do_not_divide_are_refused_at_initialize(bs, n, horizon):
    from accel_rl_amd.optimizers.base import iterate_traj_idxs
    with pytest.raises(AssertionError):                         # the reference function's own condition
        list(iterate_traj_idxs(bs, n, horizon=horizon, shuffle=False))
    opt = _optimizer(bs, horizon, 1)
    with pytest.raises(ValueError) as e:
        # (refused before the target is touched: no device needed)
        opt.initialize(inputs=[], losses=None, constraints=None, target=None, horizon=horizon, data_length=n)
    for number in (bs, n, horizon):
        assert str(number) in str(e.value)
    with pytest.raises(TypeError, match="horizon"):
        opt.initialize(inputs=[], losses=None, constraints=None, target=None)


def test_trajectory_optimizer_declares_itself():
    from accel_rl_amd.algos.pg.ppo import PPO, RecurrentPPO
    from accel_rl_amd.optimizers.single import PpoOptimizer, TrajPpoOptimizer
    assert TrajPpoOptimizer.trajectory_minibatches and not getattr(PpoOptimizer, "trajectory_minibatches", False)
    assert issubclass(TrajPpoOptimizer, PpoOptimizer)
    algo = RecurrentPPO(optimizer_args=dict(minibatch_size=40))
    assert isinstance(algo.optimizer, TrajPpoOptimizer) and algo.optimizer.parallelism_tag == "single"
    assert algo.optimizer._minibatch_size == 40 and algo.loss_kind == 1
    assert type(PPO().optimizer) is PpoOptimizer
    assert isinstance(PPO(OptimizerCls=TrajPpoOptimizer).optimizer, TrajPpoOptimizer)


class _FeedForward:
    recurrent = False
    state_info_keys = []
    device = "cpu"
    distribution = types.SimpleNamespace(dist_info_keys=["prob"])


def test_feed_forward_policy_is_refused_with_a_clear_message():
    from accel_rl_amd.algos.pg.ppo import RecurrentPPO
    algo = RecurrentPPO(optimizer_args=dict(minibatch_size=40))
    with pytest.raises(NotImplementedError, match="feed-forward"):
        algo.initialize(_FeedForward(), None, sample_size=80, horizon=5, mid_batch_reset=False)


def test_traj_minibatch_argument_errors_without_a_device():
    from accel_rl_amd import _build, _lib
    _build.build_extension()
    lib = _lib.load()
    assert "arl_traj_minibatch" in _lib.EXPORTED_SYMBOLS and callable(_lib.traj_minibatch)
    E_ARG, E_RANGE, E_ALIGN = -1, -2, -3
    # host memory stands in for the device pointers: every call below returns before anything is launched
    mem = (ctypes.c_char * 256)()
    p = ctypes.addressof(mem) + (-ctypes.addressof(mem)) % 16
    ptrs = (ctypes.c_void_p * 2)(p, p)
    nulls = (ctypes.c_void_p * 2)(None, None)

    def call(seg=p, n_seg=4, horizon=5, n_traj=8, state_in=ptrs, n_state=2, hidden=256, valids=p, idx=p,
             state_out=ptrs, inv=p):
        return lib.arl_traj_minibatch(seg, n_seg, horizon, n_traj, state_in, n_state, hidden, valids, idx, state_out,
                                      inv, None)
    assert call(seg=None) == E_ARG and b"null" in lib.arl_last_error()
    assert call(idx=None) == E_ARG
    assert call(state_in=None) == E_ARG and call(state_out=None) == E_ARG
    assert call(state_in=nulls) == E_ARG and call(state_out=nulls) == E_ARG
    for kw in (dict(n_seg=0), dict(horizon=0), dict(n_traj=0), dict(hidden=6), dict(hidden=1028), dict(n_state=3),
               dict(n_state=-1), dict(n_seg=65536, horizon=32768), dict(n_traj=2 ** 31 // 5 + 1)):
        assert call(**kw) == E_RANGE, kw
    odd = (ctypes.c_void_p * 2)(p + 4, p + 4)
    assert call(state_in=odd) == E_ALIGN and call(state_out=odd) == E_ALIGN
