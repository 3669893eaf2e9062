"""The measurements of DESIGN.md 25 (the IMPALA residual network; recorded, no bar).
`python tools/resnet_bench.py [count] [kern] [iter]`:
  count  the library's entry points called by the learner of one eager A2C iteration with AtariResnetPolicy at config 2's
         sizes (256 envs x 5 steps)
  kern   arl_maxpool3s2_fwd / _bwd and arl_add_relu (with and without its rectifier) at the network's own shapes for
         1280 rows: each a captured graph of 20 back-to-back launches, device events around 4 replays, 15 windows; the
         bytes a launch must move over its time, next to the 6.29 TB/s a float4 copy reaches on this chip
  iter   whole iterations (rollout + learner, captured graphs) of A2C with AtariResnetPolicy and with the spec-1 conv stack
         at config 2's sizes, taking turns in windows of 60 iterations after 25 warm-up iterations each, host clock
         around windows that end in a device synchronise, 5 windows
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

import bench                                            # noqa: E402
from accel_rl_amd import _lib                           # noqa: E402
from accel_rl_amd.util.misc import capture_graph        # noqa: E402

DEV = torch.device("cuda", 0)
HBM_COPY_TBPS = 6.29                                    # float4 copy, measured
ROWS = bench.N_ENVS * bench.HORIZON
result = dict()


def save():
    print(json.dumps(result), flush=True)


def build_a2c(resnet, use_graph=True):
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.atari_resnet_policy import AtariResnetPolicy
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game=bench.GAME), horizon=bench.HORIZON, n_parallel=16,
                            envs_per=bench.N_ENVS // 32, max_path_length=int(27e3), mid_batch_reset=True,
                            max_decorrelation_steps=2000, device=DEV, use_graph=use_graph)
    policy = AtariResnetPolicy() if resnet else AtariCnnPolicy(**cnn_specs[bench.CNN_SPEC])
    algo = A2C(discount=0.99, gae_lambda=1, use_graph=use_graph)
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=0, affinities=dict(gpu=0),
                     log_interval_steps=1e8)
    runner.startup()
    return runner, sampler, algo, policy


def launch_count():
    runner, sampler, algo, policy = build_a2c(True, use_graph=False)
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
    result["library_calls_one_a2c_iteration"] = dict(counts, total=sum(counts.values()))
    print("library calls, learner of one A2C iteration:", result["library_calls_one_a2c_iteration"], flush=True)
    save()
    sampler.shutdown()


def kernel_times():
    per_graph, replays, windows = 20, 4, 15
    out = dict()
    for h, w, c in ((104, 80, 16), (52, 40, 32), (26, 20, 32)):          # the three sections' pool inputs
        oh, ow = _lib.maxpool3s2_out_hw(h, w)
        z = torch.randn(ROWS, h, w, c, device=DEV)
        y, r, dy, t = (torch.randn(ROWS, oh, ow, c, device=DEV) for _ in range(4))
        arg = torch.zeros(ROWS, oh, ow, c, dtype=torch.uint8, device=DEV)
        dz, s = torch.empty_like(z), torch.empty_like(y)
        n_in, n_out = z.numel(), y.numel()
        cases = collections.OrderedDict()
        cases["maxpool3s2_fwd"] = (lambda: _lib.maxpool3s2_fwd(z, y, r, arg), 4 * n_in + 9 * n_out)
        cases["maxpool3s2_bwd"] = (lambda: _lib.maxpool3s2_bwd(dy, arg, dz), 4 * n_in + 5 * n_out)
        cases["add_relu"] = (lambda: _lib.add_relu(y, t, s, r), 16 * n_out)
        cases["add"] = (lambda: _lib.add_relu(y, t, s), 12 * n_out)
        graphs = dict()
        for name, (fn, _) in cases.items():
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
        key = "%dx%dx%dx%d" % (ROWS, h, w, c)
        out[key] = dict()
        for name, v in times.items():
            med = float(np.median(v))
            out[key][name] = dict(median_us=round(med, 2), min_us=round(min(v), 2), max_us=round(max(v), 2),
                                  mbytes=round(cases[name][1] / 1e6, 1), tbytes_per_s=round(cases[name][1] / med / 1e6, 2),
                                  share_of_copy_rate=round(cases[name][1] / med / 1e6 / HBM_COPY_TBPS, 2))
        print(key, out[key], flush=True)
        del z, y, r, dy, t, arg, dz, s, graphs
        torch.cuda.empty_cache()
    result["kernel_us_per_launch"] = out
    save()


def iterations():
    warm, window, windows = 25, 60, 5
    variants = collections.OrderedDict()
    variants["a2c_resnet"] = build_a2c(True)
    variants["a2c_spec1"] = build_a2c(False)
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
        assert torch.isfinite(policy.flat_params).all() and algo._graph is not None, name
    print("env-steps/s:", result["env_steps_per_s"], flush=True)
    save()


if __name__ == "__main__":
    what = sys.argv[1:] or ["count", "kern", "iter"]
    if "count" in what:
        launch_count()
    if "kern" in what:
        kernel_times()
    if "iter" in what:
        iterations()
