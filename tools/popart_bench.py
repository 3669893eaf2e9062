"""The measurements of DESIGN.md 36 (PopArt; recorded, no bar).  `python tools/popart_bench.py [iter] [parts]`:
  iter   iteration time (rollout + update, captured graphs) at config 2's shape -- 256 envs, horizon 5, spec 1, bench.py's
         arguments of A2C and PPO -- of the plain learner, the plain learner WITHOUT the rollout's stored activations
         (_reuse_granted False: what PopArt gives up) and the PopArt learner, from the same build in one process, the
         rigs taking turns: device events around 20 iterations, 9 windows each.  PopArt's added time per update is the
         third minus the first; the second splits it into the reuse given up and the two launches.
  parts  the two launches by themselves at the same shape (1 280 rows, 256 bootstrap values, a 512-wide value row), as a
         captured graph of 20 pairs replayed under device events
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


def build(cls, **kwargs):
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game=bench.GAME), horizon=bench.HORIZON, n_parallel=16,
                            envs_per=bench.N_ENVS // 32, max_path_length=int(27e3), mid_batch_reset=True,
                            max_decorrelation_steps=2000, device=DEV, use_graph=True)
    policy = AtariCnnPolicy(**cnn_specs[bench.CNN_SPEC])
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
    from accel_rl_amd.algos.pg import PopArtA2C, PopArtPPO
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.algos.pg.ppo import PPO

    class FullForwardA2C(A2C):
        def _reuse_granted(self, samples_data):
            return False

    class FullForwardPPO(PPO):
        def _reuse_granted(self, samples_data):
            return False
    a2c = dict(discount=0.99, gae_lambda=1)
    ppo = dict(discount=0.99, gae_lambda=0.95, optimizer_args=dict(minibatch_size=bench.MINIBATCH))
    rigs = dict(a2c=build(A2C, **a2c), a2c_full_forward=build(FullForwardA2C, **a2c), popart_a2c=build(PopArtA2C, **a2c),
                ppo=build(PPO, **ppo), ppo_full_forward=build(FullForwardPPO, **ppo), popart_ppo=build(PopArtPPO, **ppo))
    for sampler, algo in rigs.values():                 # warm-up and capture
        for k in range(6):
            bench.one_step(k, sampler, algo)
    torch.cuda.synchronize()
    itr = 6
    times = {name: [] for name in rigs}
    for _ in range(WINDOWS):
        for name, (sampler, algo) in rigs.items():
            times[name].append(_window(sampler, algo, itr))
        itr += ITERS
    result["iteration_us"] = {k: _stats(v) for k, v in times.items()}
    med = {k: v["median_us"] for k, v in result["iteration_us"].items()}
    result["added_us"] = {
        kind: dict(popart_minus_plain=round(med["popart_" + kind] - med[kind], 1),
                   reuse_given_up=round(med[kind + "_full_forward"] - med[kind], 1),
                   popart_minus_full_forward=round(med["popart_" + kind] - med[kind + "_full_forward"], 1))
        for kind in ("a2c", "ppo")}
    result["iteration_sizes"] = dict(n_env=bench.N_ENVS, horizon=bench.HORIZON, spec=bench.CNN_SPEC,
                                     reusing_graphs={k: sorted(algo._graphs) for k, (_, algo) in rigs.items()})
    print("iteration:", result["iteration_us"], result["added_us"], flush=True)
    save()
    return rigs


def _graph_time(fn, per_graph):
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


def part_times():
    """The two launches on arrays of their own (no learner is touched): returns that stay finite under repetition --
    every pair of launches normalises them, so they are put back from a copy first (one more small copy in the pair)."""
    from accel_rl_amd import _lib
    rows, n_env, hid = bench.N_ENVS * bench.HORIZON, bench.N_ENVS, 512
    f32 = lambda n: torch.randn(n, device=DEV)                                                  # noqa: E731
    value_n, last_n, value, last_value = f32(rows), f32(n_env), f32(rows), f32(n_env)
    ret0, ret, adv, w, b, diag = f32(rows) * 30, f32(rows), f32(rows), f32(hid), f32(1), f32(2)
    stats = torch.tensor([0., 1., 1., 0.], dtype=torch.float64, device=DEV)

    def pair():
        ret.copy_(ret0)
        _lib.popart_denorm(value_n, last_n, stats, value, last_value)
        _lib.popart_step(ret, adv, None, 3e-4, 1e-4, 1e6, stats, w, b, diag)

    def copy_alone():
        ret.copy_(ret0)
    both, copy = _graph_time(pair, 20), _graph_time(copy_alone, 20)
    result["parts_us"] = dict(copy_denorm_step=both, copy_alone=copy, rows=rows, n_last=n_env, hid=hid,
                              denorm_plus_step_median_us=round(both["median_us"] - copy["median_us"], 1))
    print("parts:", result["parts_us"], flush=True)
    save()


if __name__ == "__main__":
    what = sys.argv[1:] or ["iter", "parts"]
    if "parts" in what:
        part_times()
    if "iter" in what:
        for sampler, _ in iteration_times().values():
            sampler.shutdown()
