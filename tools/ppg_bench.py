"""The measurements of DESIGN.md 26 (PPG; recorded, no bar).  `python tools/ppg_bench.py [kern] [count] [iter]`:
  kern   both phases of arl_ppg_head_loss_parts next to arl_pg_head_loss_parts (kind 1, no weight-copy items) from the
         same build on the same inputs: each a captured graph of 50 back-to-back launches, the three taking turns, device
         events around 4 replays, 15 windows (the method of DESIGN.md 24)
  count  the library's entry points called by one eager policy-phase iteration and by one eager auxiliary phase at
         config 2's sizes
  iter   whole iterations (rollout + learner, captured graphs) of PPG -- auxiliary phases included, windows of whole n_pi
         cycles --, PPO and A2C at config 2's sizes, taking turns, host clock around windows that end in a device
         synchronise, 5 windows.  The three do different amounts of learning per environment step.
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
N_PI, E_AUX = 32, 6
result = dict()


def save():
    print(json.dumps(result), flush=True)


def kernel_times():
    per_graph, replays, windows = 50, 4, 15
    out = dict()
    for batch, hid, n_act in ((512, 512, 6), (1280, 512, 6), (1280, 256, 6)):
        gen = torch.Generator(device=DEV).manual_seed(batch + hid)
        K, n_rows = n_act + 1, 4 * batch
        h = torch.relu(torch.randn(batch, hid, device=DEV, generator=gen))
        w = torch.randn(K, hid, device=DEV, generator=gen) * (0.8 / np.sqrt(hid))
        b = torch.randn(K, device=DEV, generator=gen) * 0.1
        act = torch.randint(0, n_act, (n_rows,), device=DEV, generator=gen).to(torch.uint8)
        adv, ret = (torch.randn(n_rows, device=DEV, generator=gen) for _ in range(2))
        old = torch.softmax(torch.randn(n_rows, n_act, device=DEV, generator=gen), 1)
        idx = torch.randperm(n_rows, device=DEV, generator=gen)[:batch].to(torch.int32)
        lr_mult = torch.ones(1, device=DEV)
        dout, dh = torch.empty(batch, K, device=DEV), torch.empty(batch, hid, device=DEV)
        dw, db, loss4 = torch.empty(K, hid, device=DEV), torch.empty(K + 3, device=DEV), torch.empty(4, device=DEV)
        ws = _lib.pg_head_workspace(DEV)
        folds = _lib.FoldList()

        def ppg(phase):
            folds.ppg_head_loss(h, w, b, act, adv, ret, old, idx, lr_mult, None, n_act, phase, 0.2, 0.5, 0.01, 1.0,
                                dout, dh, dw, db[:K], loss4, ws, relu_mask_dh=True)
            folds._n = 0                                # (the launches alone: the fold is the same for all three)

        def ppo():
            folds.pg_head_loss(h, w, b, act, adv, ret, old, None, idx, lr_mult, None, n_act, 1, 0.2, 0.5, 0.01,
                               dout, dh, dw, db[:K], loss4, ws, relu_mask_dh=True)
            folds._n = 0
        graphs = dict()
        for name, fn in (("pg_head_ppo", ppo), ("ppg_policy", lambda: ppg(_lib.PPG_POLICY)),
                         ("ppg_aux", lambda: ppg(_lib.PPG_AUX))):
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
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(replays):
                    g.replay()
                e.record()
                e.synchronize()
                times[name].append(a.elapsed_time(e) * 1e3 / (per_graph * replays))
        key = "B%d-hid%d-A%d" % (batch, hid, n_act)
        out[key] = {k: dict(median_us=round(float(np.median(v)), 3), min_us=round(min(v), 3), max_us=round(max(v), 3))
                    for k, v in times.items()}
        print("kern %s:" % key, out[key], flush=True)
    result["head_us_per_launch"] = out
    save()


def build_ppg(use_graph=True):
    from accel_rl_amd.algos.pg import PPG
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
    algo = PPG(n_pi=N_PI, e_aux=E_AUX, optimizer_args=dict(minibatch_size=bench.MINIBATCH), use_graph=use_graph)
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=0, affinities=dict(gpu=0),
                     log_interval_steps=1e8)
    runner.startup()
    return runner, sampler, algo, policy


def call_counts():
    """Calls into the library during one eager policy-phase iteration's learner and during one eager auxiliary phase."""
    runner, sampler, algo, policy = build_ppg(use_graph=False)
    lib = _lib.load()
    for itr in range(N_PI - 1):                         # the next iteration is the first with an auxiliary phase
        bench.one_step(itr, sampler, algo)
    samples, _ = sampler.obtain_samples(N_PI - 1)
    torch.cuda.synchronize()
    counts = dict(policy_phase_iteration=collections.Counter(), auxiliary_phase=collections.Counter())
    current = ["policy_phase_iteration"]
    originals = dict()
    for name in _lib.EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        originals[name] = fn

        def counting(*a, _fn=fn, _name=name):
            counts[current[0]][_name] += 1
            return _fn(*a)
        setattr(lib, name, counting)
    enqueue_aux = algo._enqueue_aux

    def counted_aux():
        current[0] = "auxiliary_phase"
        enqueue_aux()
    algo._enqueue_aux = counted_aux
    try:
        algo.optimize_policy(N_PI - 1, samples)
        torch.cuda.synchronize()
    finally:
        for name, fn in originals.items():
            setattr(lib, name, fn)
    assert algo._aux_phases == 1
    result["library_calls"] = {k: dict(v, total=sum(v.values())) for k, v in counts.items()}
    result["library_calls_sizes"] = dict(n_pi=N_PI, e_aux=E_AUX, policy_updates=algo.optimizer._n_minibatches,
                                         aux_updates=algo._aux_opt._n_minibatches, aux_minibatch=algo._aux_opt._minibatch_size,
                                         stored_rows=algo._mem_rows)
    print("library calls:", result["library_calls"], result["library_calls_sizes"], flush=True)
    save()
    sampler.shutdown()


def iterations():
    cycles_warm, cycles_window, windows = 4, 2, 5
    warm, window = cycles_warm * N_PI, cycles_window * N_PI
    variants = collections.OrderedDict()
    variants["ppg"] = build_ppg()
    variants["ppo"] = bench.build_workload(DEV, 0, 0, 1, bench.GAME, True, kind="ppo")
    variants["a2c"] = bench.build_workload(DEV, 0, 0, 1, bench.GAME, True, kind="a2c")
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
    algo = variants["ppg"][2]
    assert algo._graph is not None and algo._aux_graph is not None and algo._aux_phases == cycles_warm
    rates = collections.defaultdict(list)
    for _ in range(windows):
        for name in variants:
            t0 = time.perf_counter()
            run(name, window)
            rates[name].append(window * per / (time.perf_counter() - t0))
    result["env_steps_per_s"] = {k: dict(median=round(float(np.median(v))), min=round(min(v)), max=round(max(v)))
                                 for k, v in rates.items()}
    result["iteration_sizes"] = dict(n_env=bench.N_ENVS, horizon=bench.HORIZON, spec=bench.CNN_SPEC, game=bench.GAME,
                                     n_pi=N_PI, e_aux=E_AUX, aux_minibatch=algo._aux_opt._minibatch_size,
                                     warmup_iterations=warm, window_iterations=window, windows=windows)
    for name, (runner, sampler, algo, policy) in variants.items():
        assert torch.isfinite(policy.flat_params).all(), name
    print("env-steps/s:", result["env_steps_per_s"], flush=True)
    save()


if __name__ == "__main__":
    what = sys.argv[1:] or ["kern", "count", "iter"]
    if "kern" in what:
        kernel_times()
    if "count" in what:
        call_counts()
    if "iter" in what:
        iterations()
