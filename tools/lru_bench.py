"""The measurements of DESIGN.md 42 (the LRU policy; recorded, no bar), by tools/tattn_bench.py's method.
`python tools/lru_bench.py [kern] [update]`:
  kern    arl_lru_fwd, arl_lru_bwd and (apart) arl_lru_param_fold at N = 128, T = 5, 20, 128 (n_seg = 256) and 1024
          (n_seg = 64), no resets, the serial recurrence and the four-chunk reduce-then-scan each forced
          (arl_dev_lru_force_path: both are legal at every T), each a captured graph of 50 calls replayed under device
          events, the candidates taking turns; medians (min / max) of 9 windows.  `default` names the path that
          ARL_LRU_CHUNK_MIN picks at that T.
  update  one RecurrentPPO update (4 epochs x 4 trajectory minibatches, captured) on a fixed batch at
          tools/recurrent_bench.py's sizes (256 envs, horizon 5, spec-0 trunk, width 256) with AtariLruPolicy
          (state_size 128) and with AtariLstmPolicy in one process, taking turns in windows of 10 updates
One JSON line per part."""
import collections
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from accel_rl_amd import _lib                           # noqa: E402
from attn_bench import DEV, PER, WINDOWS, _graph, _stats, _timed     # noqa: E402

SERIAL, CHUNKED = 1, 2                                  # arl_dev_lru_force_path


def kernel_times(s, t, n=128):
    rs = np.random.RandomState(t)
    dev = lambda *shape: torch.from_numpy(rs.randn(*shape).astype(np.float32)).to(DEV)        # noqa: E731
    u, h0, dh = dev(s, t, 2 * n), dev(s, 2 * n), dev(s, t, 2 * n)
    nu = torch.from_numpy(np.log(-np.log(rs.uniform(0.9, 0.999, size=n))).astype(np.float32)).to(DEV)
    theta = torch.from_numpy(rs.uniform(0, np.pi / 10, size=n).astype(np.float32)).to(DEV)
    lam, gam = torch.empty((n, 2), device=DEV), torch.empty(n, device=DEV)
    _lib.lru_params(nu, theta, lam, gam)
    dlam, dgam, dnu, dtheta = torch.empty((s, n, 2), device=DEV), torch.empty((s, n), device=DEV), torch.empty_like(nu), torch.empty_like(nu)
    outs = {p: (torch.empty_like(u), torch.empty_like(u)) for p in (SERIAL, CHUNKED)}          # (h_all, du) per path
    lib = _lib.load()

    graphs = collections.OrderedDict()
    for path, name in ((SERIAL, "serial"), (CHUNKED, "chunked")):      # the path is a launch argument: captured with it
        lib.arl_dev_lru_force_path(path)
        graphs[name + "_fwd"] = _graph(lambda: _lib.lru_fwd(u, lam, gam, h0, outs[path][0]))
        graphs[name + "_bwd"] = _graph(lambda: _lib.lru_bwd(u, outs[path][0], h0, lam, gam, dh, outs[path][1], dlam, dgam))
    lib.arl_dev_lru_force_path(0)
    graphs["param_fold"] = _graph(lambda: _lib.lru_param_fold(dlam, dgam, nu, theta, dnu, dtheta))
    torch.cuda.synchronize()
    for a, b in zip(outs[SERIAL], outs[CHUNKED]):       # two orders of rounding of one sum
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-4 * float(a.abs().max()))
    times = {k: [] for k in graphs}
    for _ in range(WINDOWS):
        for k, g in graphs.items():
            times[k].append(_timed(g.replay, PER))
    out = {k: _stats(v) for k, v in times.items()}
    out["default"] = "chunked" if t >= _lib.LRU_CHUNK_MIN else "serial"
    return out


def build_ppo(lru):
    from accel_rl_amd.algos.pg.ppo import RecurrentPPO
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies import AtariLruPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.atari_lstm_policy import AtariLstmPolicy
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    n_envs, horizon = 256, 5
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="breakout"), horizon=horizon, n_parallel=16,
                            envs_per=n_envs // 32, max_path_length=int(27e3), mid_batch_reset=False,
                            max_decorrelation_steps=200, device="cuda:0")
    spec = dict(cnn_specs[0], hidden_sizes=[256])
    policy = AtariLruPolicy(state_size=128, **spec) if lru else AtariLstmPolicy(**spec)
    algo = RecurrentPPO(optimizer_args=dict(minibatch_size=n_envs * horizon // 4, epochs=4))
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=0, affinities=dict(gpu=0),
                     log_interval_steps=1e8)
    runner.startup()
    for itr in range(5):                        # past the warm-up calls: the update replays from its graph
        samples, _ = sampler.obtain_samples(itr)
        algo.optimize_policy(itr, samples)
    torch.cuda.synchronize()
    assert algo._graph is not None
    return algo, samples, policy


def updates(window=10, windows=9):
    variants = collections.OrderedDict(ppo_lru=build_ppo(True), ppo_lstm=build_ppo(False))
    itr = [5]

    def run(name):
        algo, samples, _ = variants[name]
        for _ in range(window):
            algo.optimize_policy(itr[0], samples)
            itr[0] += 1
    times = collections.defaultdict(list)
    for _ in range(windows):
        for name in variants:
            times[name].append(_timed(lambda: run(name), window))
    for name, (_, _, policy) in variants.items():
        assert torch.isfinite(policy.flat_params).all(), name
    out = {k: _stats(v) for k, v in times.items()}
    out["sizes"] = dict(n_env=256, horizon=5, epochs=4, minibatch_rows=320, width=256, window_updates=window, windows=windows)
    return out


if __name__ == "__main__":
    what = sys.argv[1:] or ["kern", "update"]
    result = dict()
    if "kern" in what:
        result.update({"kernel_t%d" % t: kernel_times(64 if t == 1024 else 256, t) for t in (5, 20, 128, 1024)})
        print(json.dumps(result), flush=True)
    if "update" in what:
        result["update_us"] = updates()
        print(json.dumps(result), flush=True)
