"""Two properties every captured graph of the package relies on:

  util.misc.capture_graph   the cyclic garbage collector runs BEFORE the capture and not during it.  A dead reference
                            cycle that still holds an earlier torch.cuda.CUDAGraph would otherwise be destroyed by
                            whichever allocation of the capture body trips the collector, and on ROCm that destructor
                            synchronises the device, which a global-mode capture forbids (the process aborts).
  QPolicyBase override tables   one (pinned host, device) table per (env count, horizon), never replaced: a captured
                            rollout graph holds the device address, and training and evaluation may serve the same
                            number of envs over different horizons.

The host tests need no device (the capture itself is replaced by a recording stand-in); the GPU test runs the real
host_draws of the epsilon-greedy and the noisy policy."""
import contextlib
import gc
import weakref

import numpy as np
import pytest
import torch


class _Node(object):
    pass


def _dead_cycle():
    a, b = _Node(), _Node()
    a.other, b.other = b, a
    return weakref.ref(a)


@pytest.fixture
def recorded_capture(monkeypatch):
    """torch.cuda.graph replaced by a context manager that records what it was given and the collector's state."""
    seen = []

    @contextlib.contextmanager
    def fake_graph(graph, capture_error_mode=None):
        seen.append(dict(graph=graph, mode=capture_error_mode, gc_enabled_at_begin=gc.isenabled()))
        yield
        seen[-1]["gc_enabled_at_end"] = gc.isenabled()

    monkeypatch.setattr(torch.cuda, "graph", fake_graph)
    return seen


def test_capture_graph_collects_first_and_holds_the_collector_off(recorded_capture):
    from accel_rl_amd.util.misc import capture_graph, graph_capture_mode
    assert gc.isenabled()
    gc.disable()                                # (so that the cycle below is certainly still there when the helper starts)
    try:
        dead = _dead_cycle()
        assert dead() is not None
        gc.enable()
        token = object()
        with capture_graph(token):
            assert dead() is None               # collected before the capture began
            assert not gc.isenabled()
            inside = _dead_cycle()
            for _ in range(20000):              # far beyond the collector's thresholds: nothing is collected in here
                _Node()
            assert inside() is not None
        assert gc.isenabled()
        (rec,) = recorded_capture
        assert rec["graph"] is token and rec["mode"] == graph_capture_mode()
        assert rec["gc_enabled_at_begin"] is False and rec["gc_enabled_at_end"] is False
    finally:
        gc.enable()


def test_capture_graph_restores_the_collector_after_a_failed_body_and_leaves_a_disabled_one_disabled(recorded_capture):
    from accel_rl_amd.util.misc import capture_graph
    with pytest.raises(ZeroDivisionError):
        with capture_graph(object()):
            1 / 0
    assert gc.isenabled()
    gc.disable()
    try:
        with capture_graph(object()):
            pass
        assert not gc.isenabled()               # the caller's own setting (e.g. a frozen sampler parent) is kept
    finally:
        gc.enable()


def test_every_capture_of_the_package_goes_through_capture_graph():
    """The three capture sites (rollout graph, DQN-family update, A2C / PPO update) use the helper, not torch's own."""
    import inspect
    from accel_rl_amd.algos.pg import aac_base
    from accel_rl_amd.optimizers import dqn
    from accel_rl_amd.sampler import gpu_sampler
    for mod in (aac_base, dqn, gpu_sampler):
        src = inspect.getsource(mod)
        assert "with capture_graph(" in src and "torch.cuda.graph(" not in src, mod.__name__


def _bare_policy():
    from accel_rl_amd.policies.dqn.q_policy_base import QPolicyBase
    p = QPolicyBase.__new__(QPolicyBase)
    p._overrides, p._override_tables = dict(), dict()
    return p


def test_override_tables_are_made_once_per_env_count_and_horizon():
    p = _bare_policy()
    made = []

    def make(shape):
        def f():
            made.append(shape)
            return torch.zeros(shape, dtype=torch.int32), torch.zeros(shape, dtype=torch.int32)
        return f

    host4, dev4 = p._select_overrides(4, 8, make((4, 8)))
    assert p._overrides[8][1] is dev4
    ptr_h, ptr_d = host4.data_ptr(), dev4.data_ptr()
    host30, dev30 = p._select_overrides(30, 8, make((30, 8)))           # evaluation: the same 8 envs over 30 steps
    assert dev30.shape == (30, 8) and p._overrides[8][1] is dev30 and dev30.data_ptr() != ptr_d
    again_h, again_d = p._select_overrides(4, 8, make((4, 8)))          # back to training
    assert again_h is host4 and again_d is dev4 and p._overrides[8][1] is dev4
    assert (again_h.data_ptr(), again_d.data_ptr()) == (ptr_h, ptr_d)
    assert p._select_overrides(30, 8, make((30, 8)))[1] is dev30
    other = p._select_overrides(4, 16, make((4, 16)))[1]                # another env count: its own table and its own slot
    assert other.shape == (4, 16) and p._overrides[16][1] is other and p._overrides[8][1] is dev30
    assert made == [(4, 8), (30, 8), (4, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["epsilon_greedy", "noisy"])
def test_host_draws_keeps_the_table_a_captured_graph_reads(kind):
    """Training (horizon 4) and evaluation (horizon 30) on the SAME env count, alternating as AAOEvalSampler does: the
    training table's device address never changes, its contents are the latest draws, and serving selects the table
    that was drawn last."""
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    if kind == "noisy":
        from accel_rl_amd.policies.dqn.atari_noisy_net_dqn_policy import AtariNoisyNetDqnPolicy
        policy = AtariNoisyNetDqnPolicy(**cnn_specs[0])
    else:
        from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
        policy = AtariDqnPolicy(epsilon=0.5, **cnn_specs[0])
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(6)), device="cuda:0")
    np.random.seed(3)
    policy.host_draws(4, 8)
    train = policy._overrides[8][1]
    ptr = train.data_ptr()
    assert train.shape == (4, 8) and train.is_cuda
    for _ in range(3):
        policy.host_draws(30, 8)
        assert policy._overrides[8][1].shape == (30, 8) and policy._overrides[8][1].data_ptr() != ptr
        junk = [torch.zeros(32, dtype=torch.int32, device="cuda:0") for _ in range(8)]      # takes any block a replaced table freed
        state = np.random.get_state()
        policy.host_draws(4, 8)
        assert policy._overrides[8][1] is train and train.data_ptr() == ptr
        del junk
        if kind == "epsilon_greedy":            # the table holds THIS call's draws (the reference's order: rand, then sample_n)
            np.random.set_state(state)
            want = np.full((4, 8), -1, np.int32)
            for s in range(4):
                for j in range(2):
                    idx = np.where(np.random.rand(4) < 0.5)[0]
                    want[s, j * 4 + idx] = np.random.randint(low=0, high=6, size=len(idx), dtype=np.uint8)
            torch.cuda.synchronize()
            assert np.array_equal(train.cpu().numpy(), want) and (want >= 0).any()
        else:
            assert (train == -1).all()
