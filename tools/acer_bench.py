"""The measurements of DESIGN.md 34 (ACER; recorded, no bar).  `python tools/acer_bench.py [iter] [parts]`:
  iter   iteration time (rollout + update(s), captured graphs) of IMPALA next to ACER at replay_ratio 0 and 4, at config
         2's shape -- 256 envs, horizon 5, spec 1, the defaults of each (ACER's memory cut to 10 rollouts, replay from 2
         on) -- from the same build in one process, the three taking turns: device events around 20 iterations, 9 windows
         each.  At replay_ratio 4 an iteration holds 1 + r updates, r ~ Poisson(4): the mean r of the windows is printed.
  parts  every new launch by itself at the same shape, each a captured graph of 10 launches replayed under device events:
         arl_acer_retrace_scan, arl_acer_loss (whole batch), arl_acer_avg_step (the flat bucket), and the six
         arl_gather_segments that stage one replay batch
One process; medians (min / max) are printed as JSON."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                            # noqa: E402
from accel_rl_amd.util.misc import capture_graph        # noqa: E402

DEV = torch.device("cuda", 0)
ITERS, WINDOWS = 20, 9
result = dict()


def save():
    print(json.dumps(result), flush=True)


def _stats(v):
    return dict(median_us=round(float(np.median(v)), 1), min_us=round(min(v), 1), max_us=round(max(v), 1))


def build(cls, policy_cls, **kwargs):
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game=bench.GAME), horizon=bench.HORIZON, n_parallel=16,
                            envs_per=bench.N_ENVS // 32, max_path_length=int(27e3), mid_batch_reset=True,
                            max_decorrelation_steps=2000, device=DEV, use_graph=True)
    policy = policy_cls(**cnn_specs[bench.CNN_SPEC])
    algo = cls(use_graph=True, **kwargs)
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=0, affinities=dict(gpu=0),
                     log_interval_steps=1e8)
    runner.startup()
    return sampler, algo


def _window(sampler, algo, itr):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(ITERS):
        bench.one_step(itr + k, sampler, algo)
    e.record()
    e.synchronize()
    return a.elapsed_time(e) * 1e3 / ITERS


def iteration_times():
    from accel_rl_amd.algos.pg import ACER, IMPALA
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.dqn.atari_acer_policy import AtariAcerPolicy
    rows = bench.N_ENVS * bench.HORIZON
    rigs = dict(impala=build(IMPALA, AtariCnnPolicy),
                acer_r0=build(ACER, AtariAcerPolicy, replay_ratio=0),
                acer_r4=build(ACER, AtariAcerPolicy, replay_ratio=4, replay_steps=10 * rows, replay_start_steps=2 * rows))
    for sampler, algo in rigs.values():                 # warm-up and capture (ACER: the replay graph too)
        for k in range(8):
            bench.one_step(k, sampler, algo)
    torch.cuda.synchronize()
    itr = 8
    times = {k: [] for k in rigs}
    replays0 = rigs["acer_r4"][1]._replays
    for _ in range(WINDOWS):
        for name, (sampler, algo) in rigs.items():
            times[name].append(_window(sampler, algo, itr))
        itr += ITERS
    result["iteration_us"] = {k: _stats(v) for k, v in times.items()}
    result["iteration_sizes"] = dict(n_env=bench.N_ENVS, horizon=bench.HORIZON, spec=bench.CNN_SPEC,
                                     mean_replay_updates=round((rigs["acer_r4"][1]._replays - replays0) /
                                                               float(WINDOWS * ITERS), 2))
    print("iteration:", result["iteration_us"], result["iteration_sizes"], flush=True)
    save()
    return rigs


def _graph_time(fn, per_graph=10):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture_graph(g):
        for _ in range(per_graph):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        e.record()
        e.synchronize()
        out.append(a.elapsed_time(e) * 1e3 / per_graph)
    return _stats(out)


def part_times(rigs):
    from accel_rl_amd import _lib
    sampler, algo = rigs["acer_r4"]
    pol, s = algo.policy, algo._fields_of(sampler.samples_buf)
    torch.cuda.synchronize()
    rows, half = algo._batch_size, pol.half_stride
    prob, out = (t.clone() for t in pol.pi_q_rows(s["observations"], None, tag="bench_rows"))
    prob_last, out_last = (t.clone() for t in pol.pi_q_rows(s["extra_observations"], None, tag="bench_last"))
    qret = torch.zeros(rows, device=DEV)
    stats2 = torch.zeros((algo._n_env, 2), device=DEV)
    dout, stats5 = torch.zeros_like(out), torch.zeros((5, rows), device=DEV)
    avg, params = pol.flat_avg.clone(), pol.flat_params.clone()

    def scan():
        _lib.acer_retrace_scan(prob, prob_last, out[:, half:], out_last[:, half:], s["prob"], s["actions"].reshape(-1),
                               s["rewards"].reshape(-1), s["dones"].reshape(-1), algo.discount, algo.retrace_lambda,
                               algo._n_env, algo._horizon, qret, stats=stats2)

    def loss():
        _lib.acer_loss(out, out, s["prob"], s["actions"].reshape(-1), qret, None, pol.n_act, algo.c, algo.delta,
                       algo.q_coeff, algo.ent_loss_coeff, dout, stats5)

    def stage():
        from accel_rl_amd.algos.pg.acer import STORED_FIELDS
        for name in STORED_FIELDS:
            _lib.gather_segments(algo._mem[name], algo._idx_now, algo._staged[name])
    parts = dict(retrace_scan=_graph_time(scan), acer_loss=_graph_time(loss),
                 avg_step=_graph_time(lambda: _lib.acer_avg_step(avg, params, algo.alpha)),
                 stage_six_gathers=_graph_time(stage))
    parts["bucket_floats"] = int(avg.numel())
    parts["staged_bytes"] = int(sum(t.numel() * t.element_size() for t in algo._staged.values()))
    result["parts_us"] = parts
    print("parts:", parts, flush=True)
    save()


if __name__ == "__main__":
    what = sys.argv[1:] or ["iter", "parts"]
    rigs = iteration_times()
    if "parts" in what:
        part_times(rigs)
    for sampler, _ in rigs.values():
        sampler.shutdown()
