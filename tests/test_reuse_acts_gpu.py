"""The learner's first minibatch takes its trunk activations from the rollout instead of computing them again
(AtariCnnPolicy.serve_store / stored_acts_for / _trunk_from_store, arl_gather_rows_many, arl_serve_head.hidden_out).
Everything here is bit for bit (torch.equal): the stored rows against the learner's own forward at its batch size, the
losses and gradients with and without reuse, whole training runs with the switch on and off, the gather kernel against
torch.index_select, and the refusals -- stale parameters, bad arguments -- which must leave the full forward / no launch.

Shapes: the smallest at which the paths still differ, both on the spec-1 network and the synthetic env's 104 x 80
frames.  8 envs x horizon 2 with minibatches of 8 rows: 16 rows, 8 images take the fast weight-gradient kernels.
6 envs x horizon 3 with minibatches of 5 rows: the generic kernels and row counts that are no multiple of 8 (the
sampler's env count is 2 x n_parallel x envs_per, so an odd count of envs cannot be built; the odd count is the
minibatch's).  The layer-equality case also runs at the benchmark's own sizes (256 envs x 5, minibatch 512), where the
dense layer's reduction is split 24 ways in the rollout and 12 ways in the learner and must NOT be offered.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = {"8x2_mb8": (2, 2, 2, 8), "6x3_mb5": (1, 3, 3, 5)}        # n_parallel, envs_per, horizon, minibatch rows


def build(kind, n_parallel, envs_per, horizon, minibatch, reuse=True, max_path_length=int(27e3), use_graph=True, seed=5):
    """sampler + algorithm + policy wired by the runner, as bench.py wires them; reuse False = ARL_REUSE_ACTS=0."""
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.algos.pg.ppo import PPO
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="breakout"), horizon=horizon, n_parallel=n_parallel,
                            envs_per=envs_per, max_path_length=max_path_length, mid_batch_reset=True,
                            max_decorrelation_steps=0, device=DEV, use_graph=use_graph)
    if kind == "ppo":
        algo = PPO(discount=0.99, gae_lambda=0.95, optimizer_args=dict(minibatch_size=minibatch, epochs=2), use_graph=use_graph)
    else:
        algo = A2C(discount=0.99, gae_lambda=1, use_graph=use_graph)
    policy = AtariCnnPolicy(**cnn_specs[1])
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=seed, log_interval_steps=1e8)
    old = os.environ.get("ARL_REUSE_ACTS")
    os.environ["ARL_REUSE_ACTS"] = "1" if reuse else "0"
    try:
        runner.startup()
    finally:
        if old is None:
            del os.environ["ARL_REUSE_ACTS"]
        else:
            os.environ["ARL_REUSE_ACTS"] = old
    assert sampler._serve_fused and (sampler._act_store is not None) == reuse
    with torch.no_grad():       # sharpen the heads (a fresh one is almost uniform) and move every bias off zero
        policy.flat_params[policy._offsets[policy._k_head]:].mul_(40.0)
        for k in range(1, 2 * (policy._n_conv + policy._n_hid), 2):
            policy._w[k].add_(0.01 * torch.randn(policy._w[k].shape, device=DEV,
                                                 generator=torch.Generator(DEV).manual_seed(k)))
    return runner, sampler, algo, policy


def minibatch_of(algo, samples, idx):
    """The dict the optimiser hands to `_losses` for rows idx of this batch (advantages and returns from process_samples)."""
    opt = algo.process_samples(0, samples)
    mb = dict(zip(algo.optimizer._input_names, algo.prep_opt_inputs(0, samples, opt)))
    mb["idx"] = idx
    return mb


def losses(algo, mb, reuse):
    """algo._losses on the call's first minibatch -> clones of (loss4, flat_grads, dout, dh)."""
    policy = algo.policy
    algo._reuse_now, algo._mb_no = reuse, 0
    algo._losses(mb)                # (returns the summed loss only; the four sums live in the policy's scratch)
    b = mb["observations"].shape[0] if mb["idx"] is None else mb["idx"].shape[0]
    torch.cuda.synchronize()
    return tuple(policy._scratch[(key, b)].clone() if key else policy.flat_grads.clone() for key in ("loss", None, "dout", "dh"))


class LaunchSpy(object):
    """What a call launched, from the library's launch log: every forward entry point's launches (family names) and
    the gather calls."""

    def __init__(self, monkeypatch):
        from accel_rl_amd import _lib
        self.forward, self.gathers = [], 0
        real = {n: getattr(_lib, n) for n in ("conv2d_fwd", "conv2d_u8_fwd", "gather_rows_many")}

        def logged(name):
            def call(*args, **kwargs):
                out = real[name](*args, **kwargs)
                self.forward.append((name, [rec.family for rec in _lib.conv_launch_log()]))
                return out
            return call

        def gather(*args, **kwargs):
            self.gathers += 1
            return real["gather_rows_many"](*args, **kwargs)
        monkeypatch.setattr(_lib, "conv2d_fwd", logged("conv2d_fwd"))
        monkeypatch.setattr(_lib, "conv2d_u8_fwd", logged("conv2d_u8_fwd"))
        monkeypatch.setattr(_lib, "gather_rows_many", gather)

    def clear(self):
        self.forward, self.gathers = [], 0


def random_idx(rows, b, seed):
    """b row numbers with repeats, the first and the last row among them when there is room."""
    idx = np.random.RandomState(seed).randint(0, rows, size=b)
    if b >= 4:
        idx[0], idx[1], idx[2] = 0, rows - 1, idx[3]
    return torch.from_numpy(idx.astype(np.int32)).to(DEV)


# ---- layer equality: what may be reused at all

@pytest.mark.parametrize("n_parallel,envs_per,horizon,b,depth", [
    (2, 2, 2, 8, 4), (1, 3, 3, 5, 4),
    (16, 8, 5, 512, 3),         # the benchmark's sizes: the dense layer is split 24 / 12 ways -- conv layers only
], ids=["8x2_mb8", "6x3_mb5", "256x5_mb512"])
def test_stored_layers_are_the_learners_forward(n_parallel, envs_per, horizon, b, depth):
    """After one rollout every stored layer, gathered by a random idx with repeats, is bit for bit what _trunk computes on
    the same rows at the minibatch size -- for the layers _reuse_depth offers; and a layer it does not offer (the dense
    layer at the benchmark's sizes) is indeed not the same bits, so the rule is not merely cautious."""
    from accel_rl_amd import _lib
    runner, sampler, algo, policy = build("ppo", n_parallel, envs_per, horizon, b, use_graph=False)
    samples, _ = sampler.obtain_samples(0)
    store = policy.stored_acts_for(samples.observations)
    assert store is not None and store is sampler._act_store
    n = 2 * n_parallel * envs_per
    idx = random_idx(n * horizon, b, 1)
    acts, hids = policy._trunk(policy._scaled(samples.observations, idx))
    want = [t.clone() for t in acts + hids]
    assert policy._reuse_depth(store, b) == depth
    stored = [t.flatten(0, 1) for t in store.acts + store.hids]
    got = [torch.full_like(t, -3.0) for t in want]
    _lib.gather_rows_many(list(zip(stored, got)), idx, step_major=(horizon, n))
    torch.cuda.synchronize()
    same = [torch.equal(g, w) for g, w in zip(got, want)]
    print("layers equal:", same, "plans:", [(_lib.conv2d_fwd_plan(ga), _lib.conv2d_fwd_plan(gb)) for ga, gb in
                                             zip(sum(policy._layer_geoms(n), []), sum(policy._layer_geoms(b), []))])
    assert all(same[:depth]), same
    assert all(float(w.abs().sum()) > 0 for w in want)
    if depth < len(same):
        assert not any(same[depth:]), same
    # and the trunk built from the store is the trunk
    acts2, hids2 = policy._trunk_from_store(policy._scaled(samples.observations, idx), store, idx)
    torch.cuda.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(acts2 + hids2, want))
    sampler.shutdown()


# ---- losses and gradients with and without reuse

@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", ["ppo", "a2c"])
def test_reuse_gives_the_full_forwards_losses_and_gradients(kind, shape, monkeypatch):
    n_parallel, envs_per, horizon, b = SHAPES[shape]
    runner, sampler, algo, policy = build(kind, n_parallel, envs_per, horizon, b, use_graph=False)
    spy = LaunchSpy(monkeypatch)
    samples, _ = sampler.obtain_samples(0)
    rows = 2 * n_parallel * envs_per * horizon
    mb = minibatch_of(algo, samples, random_idx(rows, b, 2) if kind == "ppo" else None)     # A2C: the whole batch
    spy.clear()
    got = losses(algo, mb, True)
    assert spy.gathers == 1 and not spy.forward, spy.forward           # every layer came from the store
    monkeypatch.setenv("ARL_REUSE_ACTS", "0")
    spy.clear()
    want = losses(algo, mb, True)
    assert spy.gathers == 0 and len(spy.forward) == policy._n_conv + policy._n_hid
    for g, w, name in zip(got, want, ("loss4", "flat_grads", "dout", "dh")):
        assert torch.equal(g, w), name
    assert float(want[1].abs().sum()) > 0 and torch.isfinite(want[0]).all()
    sampler.shutdown()


@pytest.mark.parametrize("writer", ["set_param_values", "optimizer_update", "tensor_write"])
def test_stale_parameters_withdraw_the_offer(writer, monkeypatch):
    """A write to the parameters between the rollout and the call -- set_param_values, one optimiser update, an in-place
    write to flat_params -- and the first minibatch runs the full forward (its launches are in the library's launch log)
    with the full forward's results."""
    n_parallel, envs_per, horizon, b = SHAPES["8x2_mb8"]
    runner, sampler, algo, policy = build("ppo", n_parallel, envs_per, horizon, b, use_graph=False)
    spy = LaunchSpy(monkeypatch)
    samples, _ = sampler.obtain_samples(0)
    mb = minibatch_of(algo, samples, random_idx(16, b, 3))
    assert policy.stored_acts_for(samples.observations) is not None
    if writer == "set_param_values":
        policy.set_param_values(policy.get_param_values() * np.float32(1.01))
    elif writer == "optimizer_update":
        algo.optimize_policy(0, samples)            # (an eager warm-up call: its own updates move the parameters)
    else:
        with torch.no_grad():
            policy.flat_params.mul_(1.01)
    assert policy.stored_acts_for(samples.observations) is None
    spy.clear()
    got = losses(algo, mb, True)
    families = [fam for _, fams in spy.forward for fam in fams]
    assert spy.gathers == 0 and len(spy.forward) == policy._n_conv + policy._n_hid
    assert "conv1_img" in families and any(f.startswith("igemm") for f in families), families
    monkeypatch.setenv("ARL_REUSE_ACTS", "0")
    want = losses(algo, mb, True)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # the next rollout's offer stands again
    monkeypatch.delenv("ARL_REUSE_ACTS")
    samples, _ = sampler.obtain_samples(1)
    assert policy.stored_acts_for(samples.observations) is not None
    sampler.shutdown()


def test_a_batch_with_mid_batch_resets(monkeypatch):
    """Envs that reset in the middle of a batch (a short max_path_length): the rows after the reset are the new
    episode's observations, and their stored activations are those observations' forward."""
    n_parallel, envs_per, horizon, b = SHAPES["6x3_mb5"]
    runner, sampler, algo, policy = build("ppo", n_parallel, envs_per, horizon, b, max_path_length=3, use_graph=False)
    spy = LaunchSpy(monkeypatch)
    n, found = 2 * n_parallel * envs_per, 0
    for k in range(4):
        samples, _ = sampler.obtain_samples(k)
        torch.cuda.synchronize()
        mid = samples.env_infos["need_reset"].view(n, horizon)[:, :-1].bool() | samples.dones.view(n, horizon)[:, :-1].bool()
        if not bool(mid.any()):
            continue
        found += 1
        mb = minibatch_of(algo, samples, random_idx(n * horizon, b, 10 + k))
        all_rows = minibatch_of(algo, samples, torch.arange(n * horizon, dtype=torch.int32, device=DEV))
        for m in (mb, all_rows):
            monkeypatch.delenv("ARL_REUSE_ACTS", raising=False)
            spy.clear()
            got = losses(algo, m, True)
            assert spy.gathers == 1 and not spy.forward
            monkeypatch.setenv("ARL_REUSE_ACTS", "0")
            want = losses(algo, m, True)
            for g, w in zip(got, want):
                assert torch.equal(g, w)
        monkeypatch.delenv("ARL_REUSE_ACTS", raising=False)
    assert found >= 1
    sampler.shutdown()


# ---- whole runs: rollout graphs, the learner's captured graphs of both flavours, the stamp across replays

@pytest.mark.parametrize("kind,shape", [("ppo", "8x2_mb8"), ("ppo", "6x3_mb5"), ("a2c", "8x2_mb8")])
def test_training_runs_are_the_same_with_and_without_reuse(kind, shape):
    """Seven iterations (the learner's graphs are captured in the third), one of them followed by a second update on the
    same batch (the parameters have moved: the full-forward graph) and one by an in-place write to the parameters:
    parameters, optimiser slots and the rollout buffer bit for bit those of a run with ARL_REUSE_ACTS=0."""
    n_parallel, envs_per, horizon, b = SHAPES[shape]
    outs = []
    for reuse in (True, False):
        runner, sampler, algo, policy = build(kind, n_parallel, envs_per, horizon, b, reuse=reuse)
        np.random.seed(77)
        granted = []
        for itr in range(7):
            samples, _ = sampler.obtain_samples(itr)
            if itr == 5:
                with torch.no_grad():
                    policy.flat_params.mul_(1.001)
            granted.append(algo._reuse_granted(samples))
            algo.optimize_policy(itr, samples)
            if itr == 4:
                granted.append(algo._reuse_granted(samples))
                algo.optimize_policy(itr, samples)
        torch.cuda.synchronize()
        assert granted == [reuse, reuse, reuse, reuse, reuse, False, False, reuse]
        assert sorted(algo._graphs) == ([False, True] if reuse else [False])
        outs.append((policy.flat_params.clone(), algo.optimizer._slot0.clone(), samples.observations.clone(),
                     samples.agent_infos["prob"].clone(), samples.agent_infos["value"].clone()))
        algo._graph = None
        sampler.shutdown()
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    assert torch.isfinite(outs[0][0]).all()


# ---- the served step's hidden_out

def test_served_step_leaves_the_hidden_row_and_nothing_else_changes():
    """hidden_out = the fold of the same partial sums + bias + rectifier as arl_conv2d_fwd's own fold kernel computes them
    (the learner-side forward on the step's rows), every step; and a sampler without the store (hidden_out NULL, one
    reused set of buffers) fills the rollout buffer with the same bits."""
    from accel_rl_amd import _lib
    n_parallel, envs_per, horizon = 2, 2, 3
    n = 2 * n_parallel * envs_per
    bufs = []
    for reuse in (True, False):
        runner, sampler, algo, policy = build("ppo", n_parallel, envs_per, horizon, 8, reuse=reuse, use_graph=False)
        np.random.seed(9)
        samples, _ = sampler.obtain_samples(0)
        torch.cuda.synchronize()
        bufs.append([t.clone() for t in (samples.observations, samples.actions, samples.rewards, samples.dones,
                                         samples.agent_infos["prob"], samples.agent_infos["value"])])
        if reuse:
            store = sampler._act_store
            _, dense_g = policy._layer_geoms(n)
            assert _lib.conv2d_fwd_plan(dense_g[-1])[0] > 1         # split partials: the row exists nowhere else
            for s in range(horizon):
                acts, hids = policy._trunk(policy._scaled(samples.observations, sampler._step_rows[s]))
                torch.cuda.synchronize()
                assert torch.equal(store.hids[-1][s], hids[-1]) and float(hids[-1].abs().sum()) > 0
                for i, a in enumerate(acts):
                    assert torch.equal(store.acts[i][s], a), (s, i)
        sampler.shutdown()
    for a, c in zip(*bufs):
        assert torch.equal(a, c)


# ---- the gather kernel alone

def _gather_case(n_src, widths, idx, step_major=None, dtype=torch.float32):
    from accel_rl_amd import _lib
    g = torch.Generator(DEV).manual_seed(len(widths) * 1000 + n_src)
    srcs = [torch.randn(n_src, w, device=DEV, generator=g).to(dtype) if dtype.is_floating_point else
            torch.randint(0, 255, (n_src, w), device=DEV, generator=g).to(dtype) for w in widths]
    n_rows = n_src if idx is None else idx.numel()
    dsts = [torch.zeros(n_rows, w, device=DEV, dtype=dtype) for w in widths]
    _lib.gather_rows_many(list(zip(srcs, dsts)), idx, step_major=step_major)
    torch.cuda.synchronize()
    rows = torch.arange(n_rows, device=DEV) if idx is None else idx.long()
    if step_major is not None:
        t, n = step_major
        rows = (rows % t) * n + rows // t
    for s, d in zip(srcs, dsts):
        assert torch.equal(d, s.index_select(0, rows))


def test_gather_rows_many_against_index_select():
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)      # noqa: E731
    _gather_case(7, [4], i32([3]))                                      # one row of 16 bytes
    _gather_case(7, [15200], i32([6]))                                  # one row of conv 1's size (four chunks, a tail)
    _gather_case(600, [8, 1028], random_idx(600, 513, 4))               # 513 rows: a grid tail; first, last, repeats
    _gather_case(40, [12], i32([0, 39, 39, 0, 0, 39, 17, 17]))          # repeated indices, first and last source row
    _gather_case(24, [260], None)                                       # identity without idx
    _gather_case(24, [260], None, step_major=(3, 8))                    # whole batch through the step-major map
    _gather_case(15, [1024, 4], random_idx(15, 9, 5), step_major=(3, 5))
    _gather_case(15, [1024, 4], random_idx(15, 9, 5), step_major=(5, 3))
    # 8 items of different row sizes in one call (below, at and above one chunk of 1024 vectors)
    _gather_case(33, [4, 8, 4096, 4100, 12, 8192, 20, 516], random_idx(33, 50, 6))
    _gather_case(12, [16, 32], random_idx(12, 20, 7), dtype=torch.uint8)        # bytes: any dtype, row sizes in bytes
    # indices outside the source (device-side: cannot be refused) read row 0, never memory outside it
    from accel_rl_amd import _lib
    src, dst = torch.randn(10, 8, device=DEV), torch.zeros(4, 8, device=DEV)
    _lib.gather_rows_many([(src, dst)], i32([-1, 10, 2 ** 31 - 1, 9]))
    torch.cuda.synchronize()
    assert torch.equal(dst, src[[0, 0, 0, 9]])
    dst.zero_()
    _lib.gather_rows_many([(src, dst)], i32([-1, -7, 57, 7]), step_major=(5, 2))       # 57 -> 15, outside; 7 -> 2 * 2 + 1
    torch.cuda.synchronize()
    assert torch.equal(dst, src[[0, 0, 0, 5]])


def test_gather_rows_many_refusals_launch_nothing():
    from accel_rl_amd import _lib
    lib = _lib.load()
    src, dst = torch.randn(10, 8, device=DEV), torch.full((6, 8), 5.0, device=DEV)
    idx = torch.arange(6, dtype=torch.int32, device=DEV)

    def call(items, n_items, idx_ptr, n_rows, row_map=None):
        arr = (_lib.ArlGatherItem * 9)(*items)
        return lib.arl_gather_rows_many(arr, n_items, idx_ptr, n_rows, None if row_map is None else C.byref(row_map),
                                        _lib.stream_ptr())

    def item(s=None, d=None, row_bytes=32, src_rows=10):
        return _lib.ArlGatherItem(src.data_ptr() if s is None else s, dst.data_ptr() if d is None else d, row_bytes, src_rows)
    E_ARG, E_RANGE, E_ALIGN = -1, -2, -3
    assert call([item(row_bytes=24)], 1, idx.data_ptr(), 6) == E_RANGE              # row_bytes % 16 != 0
    assert call([item(row_bytes=0)], 1, idx.data_ptr(), 6) == E_RANGE
    assert call([item(s=src.data_ptr() + 4)], 1, idx.data_ptr(), 6) == E_ALIGN      # a misaligned pointer
    assert call([item(d=dst.data_ptr() + 8)], 1, idx.data_ptr(), 6) == E_ALIGN
    assert call([item()], 1, idx.data_ptr() + 2, 6) == E_ALIGN
    assert call([item()], 0, idx.data_ptr(), 6) == E_RANGE                          # 0 or more than 8 items
    assert call([item()] * 9, 9, idx.data_ptr(), 6) == E_RANGE
    assert call([item()], 1, idx.data_ptr(), 0) == E_RANGE                          # n_rows <= 0
    assert call([item()], 1, idx.data_ptr(), -3) == E_RANGE
    assert call([item(s=0)], 1, idx.data_ptr(), 6) == E_ARG                         # NULL pointers
    assert lib.arl_gather_rows_many(None, 1, idx.data_ptr(), 6, None, _lib.stream_ptr()) == E_ARG
    assert call([item(src_rows=0)], 1, idx.data_ptr(), 6) == E_ARG
    assert call([item(src_rows=4)], 1, None, 6) == E_RANGE                          # host-known rows outside the source
    assert call([item()], 1, None, 6, _lib.ArlRowMap(1, 3, 4, 0)) == E_RANGE        # 3 x 4 rows mapped into 10
    assert call([item()], 1, idx.data_ptr(), 6, _lib.ArlRowMap(2, 3, 2, 0)) == E_RANGE
    assert call([item()], 1, idx.data_ptr(), 6, _lib.ArlRowMap(1, 0, 2, 0)) == E_RANGE
    assert b"arl_gather_rows_many" in lib.arl_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 5.0).all())                                                 # nothing was launched
    assert call([item()], 1, idx.data_ptr(), 6) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, src[:6])
