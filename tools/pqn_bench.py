"""Measurements behind DESIGN.md 22 (PQN), one MI355X, one process; prints one JSON line per part.

  scan    arl_qlambda_scan at 128 x 32 (PQN's own batch), 1 024 x 128 and 16 384 x 32 (more blocks than stay resident at
          once), 18 actions at a stride of 32: a captured graph of 50 back-to-back launches, device events around 4
          replays, 15 windows; median / min / max per launch
  ln      arl_ln_relu_fwd / arl_ln_relu_bwd at the three training shapes next to arl_copy_bytes (a 16-byte-per-lane copy)
          of the SAME bytes: every variant a captured graph of 20 launches, the variants taking turns inside one process;
          median / min / p90 per launch over the rounds, and the kernels' rate as a share of the copy's
  update  one PQN minibatch (forward, regression loss, backward, adam step with the global-norm clip) at the default
          size of a 128-env x 32-step batch (128 rows) next to one double-DQN update (32 rows), both replayed from a
          captured graph and taking turns; library entry-point calls per update counted on the eager call
  steps   env-steps/s of whole PQN iterations (rollout + returns + 2 epochs x 32 minibatches), 128 envs x horizon 32

usage: python tools/pqn_bench.py [scan] [ln] [update] [steps]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from accel_rl_amd import _lib                                                                      # noqa: E402
from accel_rl_amd.policies.atari_cnn_specs import cnn_specs                                         # noqa: E402
from accel_rl_amd.util.misc import capture_graph                                                   # noqa: E402

DEV = "cuda:0"


def _stats(us):
    us = np.sort(np.asarray(us))
    return dict(median=round(float(np.median(us)), 2), min=round(float(us[0]), 2),
                p90=round(float(us[int(0.9 * (len(us) - 1))]), 2))


def _turns(variants, rounds=40, inner=20):
    """variants: name -> callable enqueuing ONE launch group.  -> name -> us per call (median / min / p90)."""
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / inner)
    return {k: _stats(v) for k, v in out.items()}


def bench_scan(per_graph=50, replays=4, windows=15, n_act=18, stride=32):
    out = dict()
    for n_env, horizon in ((128, 32), (1024, 128), (16384, 32)):
        steps = n_env * horizon
        q, q_last = torch.randn(steps, stride, device=DEV), torch.randn(n_env, stride, device=DEV)
        rewards, returns = torch.randn(steps, device=DEV), torch.zeros(steps, device=DEV)
        dones = (torch.rand(steps, device=DEV) < 0.02).to(torch.uint8)

        def many():
            for _ in range(per_graph):
                _lib.qlambda_scan(q, q_last, rewards, dones, 0.99, 0.65, n_env, horizon, n_act, returns)
        g = _graph_of(many)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                g.replay()
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / (per_graph * replays))
        out["%dx%d" % (n_env, horizon)] = dict(median_us=round(float(np.median(us)), 3), min_us=round(min(us), 3),
                                               max_us=round(max(us), 3))
    print(json.dumps(dict(part="scan", n_actions=n_act, q_stride=stride, us_per_launch=out)), flush=True)


def bench_ln(inner=20):
    """Each variant is a captured graph of `inner` launches (enqueued from Python a launch costs more host time than
    these kernels run); the buffers (<= 31 MB per variant) stay in the Infinity Cache, as the activations of a training
    pass do between the launch that writes them and the one that reads them."""
    for rows, width in ((128 * 25 * 19, 32), (128 * 11 * 8, 64), (128, 512)):
        n = rows * width
        z, dy = torch.randn(rows, width, device=DEV), torch.randn(rows, width, device=DEV)
        y, dz = torch.empty_like(z), torch.empty_like(z)
        gamma, beta = torch.rand(width, device=DEV) + 0.5, torch.randn(width, device=DEV)
        stats = torch.empty(rows, 2, device=DEV)
        dg, db = torch.empty(width, device=DEV), torch.empty(width, device=DEV)
        ws = _lib.ln_bwd_workspace(DEV)
        src, dst = torch.randn(2 * n, device=DEV), torch.empty(2 * n, device=DEV)
        s2, d2, s3, d3 = src[:n], dst[:n], src[:3 * n // 2], dst[:3 * n // 2]
        _lib.ln_relu_fwd(z, gamma, beta, 1e-5, y, stats)
        variants = dict(
            fwd=lambda: _lib.ln_relu_fwd(z, gamma, beta, 1e-5, y, stats),
            copy_2n=lambda: _lib.copy_bytes(d2, s2),                # reads n floats, writes n: the forward's bytes
            bwd_masked=lambda: _lib.ln_relu_bwd(dy, y, z, stats, gamma, True, dz, dg, db, ws),      # + its fold launch
            copy_3n=lambda: _lib.copy_bytes(d3, s3),                # 3 n floats moved: the masked backward's bytes
            bwd=lambda: _lib.ln_relu_bwd(dy, y, z, stats, gamma, False, dz, dg, db, ws),
            copy_4n=lambda: _lib.copy_bytes(dst, src))              # 4 n floats moved: the unmasked backward's

        def repeated(fn):
            def many():
                for _ in range(inner):
                    fn()
            return many
        graphs = {k: _graph_of(repeated(fn)) for k, fn in variants.items()}
        res = _turns({k: g.replay for k, g in graphs.items()}, rounds=30, inner=5)
        res = {k: {m: round(v / inner, 2) for m, v in st.items()} for k, st in res.items()}
        share = {k: round(res[c]["median"] / res[k]["median"], 3)
                 for k, c in (("fwd", "copy_2n"), ("bwd_masked", "copy_3n"), ("bwd", "copy_4n"))}
        gbs = {k: round(f * 4 * n / res[k]["median"] / 1e3, 1) for k, f in (("fwd", 2), ("bwd_masked", 3), ("bwd", 4),
                                                                            ("copy_2n", 2), ("copy_3n", 3), ("copy_4n", 4))}
        print(json.dumps(dict(part="ln", rows=rows, width=width, mbytes_fwd=round(8 * n / 1e6, 2), us=res, gb_per_s=gbs,
                              share_of_copy_rate=share)), flush=True)


class _CallCounter(object):
    """Counts the library's entry-point calls that enqueue device work (one launch each; a call that folds at once: two)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("arl_") and not name.endswith(("_bytes", "_plan", "last_error", "_supported")):
            def counted(*a, **kw):
                self.calls.append(name)
                return fn(*a, **kw)
            return counted
        return fn


def _count_calls(fn):
    lib = _lib.load()
    counter = _CallCounter(lib)
    _lib._lib = counter
    try:
        fn()
    finally:
        _lib._lib = lib
    torch.cuda.synchronize()
    return len(counter.calls), sorted(set(counter.calls))


def _graph_of(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture_graph(g):
        fn()
    return g


def bench_update(spec=1):
    from accel_rl_amd.optimizers import update_methods
    from accel_rl_amd.optimizers.single import A2cOptimizer
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.policies.dqn.atari_pqn_policy import AtariPqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(0)
    env_spec = EnvSpec(UintBox((4, 104, 80)), Discrete(18))
    n = 128 * 32
    obs = torch.randint(0, 256, (n, 4, 104, 80), dtype=torch.uint8, device=DEV)
    act = torch.randint(0, 18, (n,), dtype=torch.uint8, device=DEV)
    ret = torch.randn(n, device=DEV)
    term = torch.zeros(n, dtype=torch.uint8, device=DEV)

    def make(cls, clip):
        policy = cls(**cnn_specs[spec])
        policy.initialize(env_spec, device=DEV)
        opt = A2cOptimizer(2.5e-4, update_methods.adam, dict(epsilon=1e-5), grad_norm_clip=clip)
        opt._setup_bucket(policy, 1.0)
        return policy, opt
    pqn, pqn_opt = make(AtariPqnPolicy, 10)
    dqn, dqn_opt = make(AtariDqnPolicy, 10)
    idx = torch.randperm(n, device=DEV)[:n // 32].to(torch.int32)
    o32, n32 = obs[:32].contiguous(), obs[32:64].contiguous()

    def pqn_update():
        pqn.pqn_loss_and_grads(obs, idx, act, ret, None)
        pqn_opt._apply_update()

    def dqn_update():
        dqn.q_loss_and_grads(o32, n32, act[:32], ret[:32], term[:32], None, 0.99, 1.0, double_dqn=True)
        dqn_opt._apply_update()
    pqn_update(), dqn_update()
    calls = dict(pqn=_count_calls(pqn_update), dqn=_count_calls(dqn_update))
    graphs = dict(pqn_128_rows=_graph_of(pqn_update), double_dqn_32_rows=_graph_of(dqn_update))
    res = _turns({k: g.replay for k, g in graphs.items()}, rounds=40, inner=10)
    print(json.dumps(dict(part="update", spec=spec, us=res, entry_point_calls={k: v[0] for k, v in calls.items()},
                          entry_points={k: v[1] for k, v in calls.items()})), flush=True)


def bench_steps(spec=1, n_env=128, horizon=32, warmup=6, steps=20):
    from accel_rl_amd.algos.dqn.pqn import PQN
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.dqn.atari_pqn_policy import AtariPqnPolicy
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="seaquest"), horizon=horizon, n_parallel=16,
                            envs_per=n_env // 32, max_path_length=int(27e3), mid_batch_reset=True,
                            max_decorrelation_steps=0, device=torch.device(DEV))
    algo, policy = PQN(), AtariPqnPolicy(**cnn_specs[spec])
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=0, log_interval_steps=1e8)
    runner.startup()
    itr, windows = 0, []
    for _ in range(warmup):
        samples, _ = sampler.obtain_samples(itr)
        algo.optimize_policy(itr, samples)
        itr += 1
    for _ in range(3):                                          # three windows: the spread is part of the figure
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            samples, _ = sampler.obtain_samples(itr)
            info = algo.optimize_policy(itr, samples)[1]
            itr += 1
        torch.cuda.synchronize()
        windows.append(steps * n_env * horizon / (time.perf_counter() - t0))
    print(json.dumps(dict(part="steps", spec=spec, n_env=n_env, horizon=horizon, minibatch=algo.optimizer._minibatch_size,
                          updates_per_iteration=algo.optimizer._n_minibatches, graph=algo._graph is not None,
                          env_steps_per_s=[round(w, 1) for w in windows],
                          loss=float(info["Loss"].mean()), finite=bool(torch.isfinite(policy.flat_params).all()))),
          flush=True)
    runner.shutdown()


if __name__ == "__main__":
    parts = sys.argv[1:] or ["scan", "ln", "update", "steps"]
    _lib.load()
    if "scan" in parts:
        bench_scan()
    if "ln" in parts:
        bench_ln()
    if "update" in parts:
        bench_update()
    if "steps" in parts:
        bench_steps()
