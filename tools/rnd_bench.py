"""The measurements of DESIGN.md 32 (RND; recorded, no bar).  `python tools/rnd_bench.py [iter] [parts]`:
  iter   iteration time (rollout + update, captured graphs) of PPO next to RndPPO at config 2's shape -- 256 envs,
         horizon 5, spec 1, the defaults of both -- from the same build in one process, the two taking turns: device
         events around 20 iterations, 9 windows each
  parts  RndPPO's additions by themselves at the same shape, each a captured graph replayed under device events: the
         bonus pass (arl_rnd_obs_stats, prepare -> both trunks -> arl_rnd_error over all 1 280 rows, arl_rnd_reward_mix)
         and one predictor update (prepare, both forwards, arl_rnd_error with gradient, predictor backward, optimiser
         step) on the 128 leading rows of a 512-row minibatch; "rest" = RndPPO's iteration minus the bonus pass minus its
         updates' predictor updates
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
    from accel_rl_amd.algos.pg import RndPPO
    from accel_rl_amd.algos.pg.ppo import PPO
    rigs = dict(ppo=build(PPO), rnd_ppo=build(RndPPO))
    itr = 0
    for sampler, algo in rigs.values():                 # warm-up and capture
        for k in range(6):
            bench.one_step(k, sampler, algo)
    torch.cuda.synchronize()
    itr = 6
    times = dict(ppo=[], rnd_ppo=[])
    for _ in range(WINDOWS):
        for name, (sampler, algo) in rigs.items():
            times[name].append(_window(sampler, algo, itr))
        itr += ITERS
    result["iteration_us"] = {k: _stats(v) for k, v in times.items()}
    result["iteration_sizes"] = dict(n_env=bench.N_ENVS, horizon=bench.HORIZON, spec=bench.CNN_SPEC,
                                     updates=rigs["rnd_ppo"][1].optimizer._n_minibatches,
                                     minibatch=rigs["rnd_ppo"][1].optimizer._minibatch_size,
                                     predictor_rows=rigs["rnd_ppo"][1]._rnd_rows)
    print("iteration:", result["iteration_us"], result["iteration_sizes"], flush=True)
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


def part_times(rigs):
    sampler, algo = rigs["rnd_ppo"]
    samples = sampler.samples_buf
    torch.cuda.synchronize()
    state = algo.rnd.rnd_state()
    from accel_rl_amd import _lib

    def bonus():
        algo.rnd.update_obs_stats(samples["observations"], samples["extra_observations"])
        algo.bonus_pass(samples, algo.rnd_rows_per_pass)
        _lib.rnd_reward_mix(algo._rnd_err, samples["rewards"].reshape(-1), algo._n_env, algo._horizon, algo.rnd.rho,
                            algo.rnd.rew_moments, algo.int_discount, algo.ext_coeff, algo.int_coeff, algo._r_mix,
                            algo._rnd_diag, algo._mix_ws)
    idx = torch.randperm(algo._batch_size, device=DEV)[:algo._rnd_rows].to(torch.int32)

    def update():
        algo.rnd.loss_and_grads(samples["observations"], samples["extra_observations"], idx)
        algo._rnd_opt.step()
    parts = dict(bonus_pass=_graph_time(bonus, 10), predictor_update=_graph_time(update, 10))
    algo.rnd.set_rnd_state(state)
    n_upd = algo.optimizer._n_minibatches
    it = result["iteration_us"]["rnd_ppo"]["median_us"]
    parts["updates_per_iteration"] = n_upd
    parts["rest_us"] = round(it - parts["bonus_pass"]["median_us"] - n_upd * parts["predictor_update"]["median_us"], 1)
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
