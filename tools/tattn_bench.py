"""The measurements of DESIGN.md 41 (the attention-memory policy; recorded, no bar), by tools/attn_bench.py's method.
`python tools/tattn_bench.py [kern] [update]`:
  kern    arl_tattn_fwd and arl_tattn_bwd (with arl_tattn_rel_fold) at T = 20, M = 16, H = 2, d = 32, n_seg = 64 and 256,
          no resets, next to the same masked attention as PyTorch calls (a dense [T, M + T] band mask; the backward's five
          products written out), each a captured graph of 50 calls replayed under device events, the candidates taking
          turns; medians (min / max) of 9 windows
  update  one RecurrentPPO update (4 epochs x 4 trajectory minibatches, captured) on a fixed batch at
          tools/recurrent_bench.py's sizes (256 envs, horizon 5, spec-0 trunk, width 256) with AtariAttnMemoryPolicy
          (memory_len 4, 4 heads of 64) and with AtariLstmPolicy in one process, taking turns in windows of 10 updates
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


def kernel_times(s, t=20, m=16, h=2, d=32):
    rs = np.random.RandomState(s)
    dev = lambda *shape: torch.from_numpy(rs.randn(*shape).astype(np.float32)).to(DEV)        # noqa: E731
    q, kv, rel, dout = dev(s, t, h, d), dev(s, m + t, 2, h, d), dev(h, m + 1), dev(s, t, h * d)
    out, lse = torch.empty_like(dout), torch.empty((s, h, t), device=DEV)
    dq, dkv, parts, drel = torch.empty_like(q), torch.empty_like(kv), torch.empty((s, h, m + 1), device=DEV), torch.empty_like(rel)
    scale = d ** -0.5
    age = m + torch.arange(t, device=DEV)[:, None] - torch.arange(m + t, device=DEV)[None, :]
    outside, age_c = (age < 0) | (age > m), age.clamp(0, m)
    lib = dict()

    def lib_fwd():
        qq, k, v = q.transpose(1, 2), kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2)  # [S, H, ., d] views
        sc = (scale * (qq @ k.transpose(2, 3)) + rel[:, age_c]).masked_fill(outside, float("-inf"))
        lib["p"] = torch.softmax(sc, dim=3)
        lib["out"] = (lib["p"] @ v).transpose(1, 2).reshape(s, t, h * d)

    def lib_bwd():
        qq, k, v = q.transpose(1, 2), kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2)
        p, do = lib["p"], dout.view(s, t, h, d).transpose(1, 2)
        w = p * (do @ v.transpose(2, 3) - (do * lib["out"].view(s, t, h, d).transpose(1, 2)).sum(dim=3, keepdim=True))
        ds = scale * w
        lib["dq"] = (ds @ k).transpose(1, 2)
        lib["dkv"] = torch.stack([ds.transpose(2, 3) @ qq, p.transpose(2, 3) @ do], dim=1).permute(0, 3, 1, 2, 4)
        lib["drel"] = torch.zeros_like(rel).index_add_(1, age_c.reshape(-1), w.sum(dim=0).reshape(h, -1))

    def hip_bwd():
        _lib.tattn_bwd(q, kv, rel, out, lse, dout, dq, dkv, parts, None, None, scale)
        _lib.tattn_rel_fold(parts, drel)

    graphs = collections.OrderedDict()
    graphs["hip_fwd"] = _graph(lambda: _lib.tattn_fwd(q, kv, rel, out, lse, None, None, scale))
    graphs["pytorch_fwd"] = _graph(lib_fwd)
    graphs["hip_bwd"] = _graph(hip_bwd)
    graphs["pytorch_bwd"] = _graph(lib_bwd)
    torch.cuda.synchronize()
    for name, got in (("out", out), ("dq", dq), ("dkv", dkv), ("drel", drel)):
        assert torch.allclose(lib[name].reshape(got.shape), got, rtol=1e-3, atol=1e-4 * float(got.abs().max())), name
    times = {k: [] for k in graphs}
    for _ in range(WINDOWS):
        for k, g in graphs.items():
            times[k].append(_timed(g.replay, PER))
    return {k: _stats(v) for k, v in times.items()}


def build_ppo(memory):
    from accel_rl_amd.algos.pg.ppo import RecurrentPPO
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies import AtariAttnMemoryPolicy
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
    policy = AtariAttnMemoryPolicy(memory_len=4, n_heads=4, head_dim=64, **spec) if memory else AtariLstmPolicy(**spec)
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
    variants = collections.OrderedDict(ppo_attn_memory=build_ppo(True), ppo_lstm=build_ppo(False))
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
        result.update({"kernel_s%d" % s: kernel_times(s) for s in (64, 256)})
        print(json.dumps(result), flush=True)
    if "update" in what:
        result["update_us"] = updates()
        print(json.dumps(result), flush=True)
