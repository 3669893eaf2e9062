"""The measurements of DESIGN.md 24 (IMPALA; recorded, no bar).  `python tools/vtrace_bench.py [scan] [count] [iter]`:
  scan   arl_vtrace_scan next to arl_gae_scan (promo nep50, the sequential walk) on the same rollouts: each a captured
         graph of 50 back-to-back launches, the two taking turns, device events around 4 replays, 15 windows
  count  the library's entry points called by the learner of one eager iteration (epochs = 1) at config 2's sizes
  iter   whole iterations (rollout + learner, captured graphs) of IMPALA at epochs 1 and 4, A2C and PPO at config 2's
         sizes, taking turns in windows of 150 iterations after 40 warm-up iterations each, host clock around windows
         that end in a device synchronise, 5 windows
One process; medians (min / max) are printed as JSON."""
import collections
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench                                            # noqa: E402
import vtrace_ref as vr                                 # noqa: E402
from accel_rl_amd import _lib                           # noqa: E402
from accel_rl_amd.util.misc import capture_graph        # noqa: E402

DEV = torch.device("cuda", 0)
result = dict()


def save():
    print(json.dumps(result), flush=True)


def scan_times():
    per_graph, replays, windows = 50, 4, 15
    out = dict()
    for n_env, horizon in ((256, 5), (128, 32), (1024, 128)):
        c = vr.rollout(1, n_env, horizon, 6)
        d = {k: torch.from_numpy(np.ascontiguousarray(v.reshape((-1, 6)) if v.ndim == 3 else v.reshape(-1))).to(DEV)
             for k, v in c.items()}
        ret, adv = (torch.zeros(n_env * horizon, device=DEV) for _ in range(2))
        stats = torch.zeros(n_env, 2, device=DEV)

        def vtrace():
            _lib.vtrace_scan(d["prob"], d["old_prob"], d["actions"], d["values"], d["last_values"], d["rewards"],
                             d["dones"], 0.99, 0.95, 1.0, 1.0, 1.0, n_env, horizon, ret, adv, stats=stats)

        def gae():
            _lib.gae_scan(d["rewards"], d["values"], d["dones"], d["last_values"], 0.99, 0.95, n_env, horizon, adv, ret)
        graphs = dict()
        for name, fn in (("vtrace", vtrace), ("gae", gae)):
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with capture_graph(g):
                for _ in range(per_graph):
                    fn()
            for _ in range(3):
                g.replay()
            graphs[name] = g
        torch.cuda.synchronize()
        times = collections.defaultdict(list)
        for _ in range(windows):
            for name, g in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(replays):
                    g.replay()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3 / (per_graph * replays))
        out["%dx%d" % (n_env, horizon)] = {k: dict(median_us=round(float(np.median(v)), 3), min_us=round(min(v), 3),
                                                   max_us=round(max(v), 3)) for k, v in times.items()}
        print("scan %4d x %3d:" % (n_env, horizon), out["%dx%d" % (n_env, horizon)], flush=True)
    result["scan_us_per_launch"] = out
    save()


def build_impala(epochs, use_graph=True):
    from accel_rl_amd.algos.pg import IMPALA
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game=bench.GAME), horizon=bench.HORIZON, n_parallel=16,
                            envs_per=bench.N_ENVS // 32, max_path_length=int(27e3), mid_batch_reset=True,
                            max_decorrelation_steps=2000, device=DEV, use_graph=use_graph)
    policy = AtariCnnPolicy(**cnn_specs[bench.CNN_SPEC])
    algo = IMPALA(optimizer_args=dict(epochs=epochs), use_graph=use_graph)
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=0, affinities=dict(gpu=0),
                     log_interval_steps=1e8)
    runner.startup()
    return runner, sampler, algo, policy


def launch_count():
    """Calls into the library during one eager iteration's learner at config 2's sizes, epochs = 1."""
    runner, sampler, algo, policy = build_impala(1, use_graph=False)
    lib = _lib.load()
    counts = collections.Counter()
    originals = dict()
    samples, _ = sampler.obtain_samples(0)
    algo.optimize_policy(0, samples)
    samples, _ = sampler.obtain_samples(1)
    torch.cuda.synchronize()
    for name in _lib.EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        originals[name] = fn

        def counting(*a, _fn=fn, _name=name):
            counts[_name] += 1
            return _fn(*a)
        setattr(lib, name, counting)
    try:
        algo.optimize_policy(1, samples)
        torch.cuda.synchronize()
    finally:
        for name, fn in originals.items():
            setattr(lib, name, fn)
    result["library_calls_one_iteration_epochs1"] = dict(counts)
    print("library calls, learner of one iteration (epochs 1):", dict(counts), flush=True)
    save()
    sampler.shutdown()


def iterations():
    warm, window, windows = 40, 150, 5
    variants = collections.OrderedDict()
    variants["impala_e1"] = build_impala(1)
    variants["impala_e4"] = build_impala(4)
    variants["a2c"] = bench.build_workload(DEV, 0, 0, 1, bench.GAME, True, kind="a2c")
    variants["ppo"] = bench.build_workload(DEV, 0, 0, 1, bench.GAME, True, kind="ppo")
    itr = {k: 0 for k in variants}
    per = bench.N_ENVS * bench.HORIZON

    def run(name, n):
        runner, sampler, algo, policy = variants[name]
        for _ in range(n):
            bench.one_step(itr[name], sampler, algo)
            itr[name] += 1
        torch.cuda.synchronize()
    for name in variants:
        run(name, warm)
        print("warmed", name, flush=True)
    rates = collections.defaultdict(list)
    for _ in range(windows):
        for name in variants:
            t0 = time.perf_counter()
            run(name, window)
            rates[name].append(window * per / (time.perf_counter() - t0))
    result["env_steps_per_s"] = {k: dict(median=round(float(np.median(v))), min=round(min(v)), max=round(max(v)))
                                 for k, v in rates.items()}
    result["iteration_sizes"] = dict(n_env=bench.N_ENVS, horizon=bench.HORIZON, spec=bench.CNN_SPEC, game=bench.GAME,
                                     warmup_iterations=warm, window_iterations=window, windows=windows)
    for name, (runner, sampler, algo, policy) in variants.items():
        assert torch.isfinite(policy.flat_params).all(), name
        if name.startswith("impala"):
            assert algo._graph is not None
    print("env-steps/s:", result["env_steps_per_s"], flush=True)
    save()


if __name__ == "__main__":
    what = sys.argv[1:] or ["scan", "count", "iter"]
    if "scan" in what:
        scan_times()
    if "count" in what:
        launch_count()
    if "iter" in what:
        iterations()
