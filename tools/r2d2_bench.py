"""The measurements of DESIGN.md 28 (R2D2; recorded, no bar).  `python tools/r2d2_bench.py [count] [update]`:
  count   the library's entry points called by one eager update (sample a sequence minibatch, loss, backward, optimiser
          step, priorities written back) at the small size
  update  the captured update alone (DqnOptimizer's graph: both unrolls, arl_r2d2_loss, BPTT, the optimiser step) at the
          default sizes (batch 64, burn-in 40, train 80, n 5, LSTM 512) and at one small size (batch 8, 4 + 8 + 2 steps,
          LSTM 64): device events around 3 graph replays on static inputs, 9 windows after 3 warm-up replays
The replay memory is filled with random frames, states and flags (no sampler, no environment): what is timed does not
depend on their values.  One process; medians (min / max) are printed as JSON."""
import collections
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from accel_rl_amd import _lib                           # noqa: E402

DEV = torch.device("cuda", 0)
SIZES = dict(
    default=dict(algo=dict(), hidden=512, n_env=32, horizon=40, ring=400),
    small=dict(algo=dict(burn_in=4, train_len=8, seq_stride=4, reward_horizon=2, batch_size=8), hidden=64, n_env=8,
               horizon=8, ring=64))
result = dict()


def save():
    print(json.dumps(result), flush=True)


def build(size, use_graph):
    """(algo, policy) with a replay memory filled over one lap and a half of random sampler batches."""
    from accel_rl_amd.algos.dqn.r2d2 import R2D2
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_r2d2_policy import AtariR2d2Policy
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    from accel_rl_amd.util import logger
    from accel_rl_amd.util.seed import set_seed
    logger.set_quiet(True)
    set_seed(0)
    s = SIZES[size]
    n_env, horizon, hidden = s["n_env"], s["horizon"], s["hidden"]
    env_spec = EnvSpec(UintBox((4, 104, 80)), Discrete(6))
    policy = AtariR2d2Policy(**dict(cnn_specs[0], hidden_sizes=[hidden]))
    policy.initialize(env_spec, device=DEV)
    algo = R2D2(replay_size=n_env * s["ring"], min_steps_learn=0, training_intensity=1,
                optimizer_args=dict(use_graph=use_graph), **s["algo"])
    per_update = algo.batch_size * algo.train_len
    algo.training_intensity = per_update // np.gcd(per_update, n_env * horizon)      # (an integer number of updates)
    algo.initialize(policy, env_spec, n_env * horizon, horizon, True)
    rs = np.random.RandomState(0)
    rows = n_env * horizon
    dev = lambda a: torch.from_numpy(a).to(DEV)                                          # noqa: E731
    for _ in range(3 * s["ring"] // (2 * horizon)):
        algo.replay_buffer.append_data(dict(
            observations=dev(rs.randint(0, 256, size=(rows, 4, 104, 80), dtype=np.uint8)),
            actions=dev(rs.randint(0, 6, size=rows).astype(np.uint8)), rewards=dev(rs.randn(rows).astype(np.float32)),
            dones=dev((rs.rand(rows) < 0.02).astype(np.uint8)),
            agent_infos={k: dev((rs.randn(rows, hidden) * 0.3).astype(np.float32)) for k in policy.state_info_keys}))
    return algo, policy


def one_update(algo):
    mb = algo.replay_buffer.sample_batch(algo.batch_size)
    priority, loss = algo.optimizer.optimize(mb)
    algo.replay_buffer.update_batch_priorities(priority)


def launch_count():
    algo, policy = build("small", use_graph=False)
    lib = _lib.load()
    for _ in range(2):
        one_update(algo)
    torch.cuda.synchronize()
    counts, originals = collections.Counter(), dict()
    for name in _lib.EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        originals[name] = fn

        def counting(*a, _fn=fn, _name=name):
            counts[_name] += 1
            return _fn(*a)
        setattr(lib, name, counting)
    try:
        one_update(algo)
        torch.cuda.synchronize()
    finally:
        for name, fn in originals.items():
            setattr(lib, name, fn)
    result["library_calls_one_update_small"] = dict(counts, total=sum(counts.values()))
    print("library calls, one eager update (small size):", result["library_calls_one_update_small"], flush=True)
    save()


def update_times():
    replays, windows = 3, 9
    out = dict()
    for size in ("small", "default"):
        algo, policy = build(size, use_graph=True)
        for _ in range(4):                                       # two eager calls, the capture, one replay
            one_update(algo)
        graph = algo.optimizer._graph
        assert graph is not None and bool(torch.isfinite(policy.flat_params).all())
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        times = []
        for _ in range(windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                graph.replay()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / replays)
        rb = algo.replay_buffer
        out[size] = dict(batch=algo.batch_size, burn_in=algo.burn_in, train_len=algo.train_len, n=algo.reward_horizon,
                         rows=algo.batch_size * rb.seq_len, hidden=SIZES[size]["hidden"],
                         median_us=round(float(np.median(times)), 1), min_us=round(min(times), 1),
                         max_us=round(max(times), 1), replays_per_window=replays, windows=windows)
        print("captured update, %s:" % size, out[size], flush=True)
        assert bool(torch.isfinite(policy.flat_params).all())
        del algo, policy, graph
        torch.cuda.empty_cache()
    result["captured_update"] = out
    save()


if __name__ == "__main__":
    what = sys.argv[1:] or ["count", "update"]
    if "count" in what:
        launch_count()
    if "update" in what:
        update_times()
