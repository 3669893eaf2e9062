"""The measurements of DESIGN.md 39 and 40 (the relational policy; recorded, no bar).
`python tools/attn_bench.py [kern] [iter] [N ...]`:
  kern   the attention pair at B = 256 and 1280, H = 2, d = 32 and every position count N given (63 if none): arl_attn_fwd
         and arl_attn_bwd up to 64 positions, arl_attn_tiled_fwd and arl_attn_tiled_bwd above, next to the same
         mathematics as PyTorch calls (two batched matmuls and a soft-max forward; the five products of the backward
         written out), each a captured graph of 50 calls replayed under device events, the two taking turns; medians
         (min / max) of 9 windows
  iter   whole A2C iterations (rollout + captured update) at config 2's sizes with AtariRelationalPolicy(), with
         AtariRelationalPolicy(**spec 1's conv arguments, max_positions=128) and with AtariCnnPolicy(**cnn_specs[1]) in one
         process, taking turns in windows of 60 iterations after 25 warm-up iterations each, under device events
One JSON line per part."""
import collections
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                            # noqa: E402
from accel_rl_amd import _lib                           # noqa: E402
from accel_rl_amd.util.misc import capture_graph        # noqa: E402

DEV = torch.device("cuda", 0)
PER, WINDOWS = 50, 9
result = dict()


def _stats(v):
    return dict(median_us=round(float(np.median(v)), 1), min_us=round(min(v), 1), max_us=round(max(v), 1))


def _timed(fn, per):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e) * 1e3 / per


def _graph(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture_graph(g):
        for _ in range(PER):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def kernel_times(b, n=63, h=2, d=32):
    rs = np.random.RandomState(b)
    qkv = torch.from_numpy(rs.randn(b, n, 3, h, d).astype(np.float32)).to(DEV)
    dout = torch.from_numpy(rs.randn(b, n, h * d).astype(np.float32)).to(DEV)
    out, lse, dqkv = torch.empty_like(dout), torch.empty((b, h, n), device=DEV), torch.empty_like(qkv)
    scale = d ** -0.5
    lib = dict()

    def lib_fwd():
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))                             # [B, H, N, d] views
        lib["p"] = torch.softmax(scale * (q @ k.transpose(2, 3)), dim=3)
        lib["out"] = (lib["p"] @ v).transpose(1, 2).reshape(b, n, h * d)

    def lib_bwd():
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        p, do = lib["p"], dout.view(b, n, h, d).transpose(1, 2)
        dp = do @ v.transpose(2, 3)
        ds = scale * p * (dp - (do * lib["out"].view(b, n, h, d).transpose(1, 2)).sum(dim=3, keepdim=True))
        lib["dqkv"] = torch.stack([ds @ k, ds.transpose(2, 3) @ q, p.transpose(2, 3) @ do], dim=1).permute(0, 3, 1, 2, 4)

    graphs = collections.OrderedDict()
    fwd, bwd = (_lib.attn_tiled_fwd, _lib.attn_tiled_bwd) if n > _lib.ATTN_MAX_POS else (_lib.attn_fwd, _lib.attn_bwd)
    graphs["hip_fwd"] = _graph(lambda: fwd(qkv, out, lse, scale))
    graphs["pytorch_fwd"] = _graph(lib_fwd)
    graphs["hip_bwd"] = _graph(lambda: bwd(qkv, out, lse, dout, dqkv, scale))
    graphs["pytorch_bwd"] = _graph(lib_bwd)
    torch.cuda.synchronize()
    assert torch.allclose(lib["out"], out, rtol=1e-3, atol=1e-5) and torch.allclose(lib["dqkv"], dqkv, rtol=1e-3, atol=1e-5)
    times = {k: [] for k in graphs}
    for _ in range(WINDOWS):
        for k, g in graphs.items():
            times[k].append(_timed(g.replay, PER))
    return {k: _stats(v) for k, v in times.items()}


def build_a2c(relational):
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies import AtariRelationalPolicy
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game=bench.GAME), horizon=bench.HORIZON, n_parallel=16,
                            envs_per=bench.N_ENVS // 32, max_path_length=int(27e3), mid_batch_reset=True,
                            max_decorrelation_steps=2000, device=DEV, use_graph=True)
    spec1 = {k: v for k, v in cnn_specs[1].items() if k != "hidden_sizes"}
    policy = {"default": AtariRelationalPolicy, "spec1": lambda: AtariRelationalPolicy(**spec1, max_positions=128),
              None: lambda: AtariCnnPolicy(**cnn_specs[1])}[relational]()
    algo = A2C(discount=0.99, gae_lambda=1, use_graph=True)
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=0, affinities=dict(gpu=0),
                     log_interval_steps=1e8)
    runner.startup()
    return runner, sampler, algo, policy


def iterations(warm=25, window=60, windows=5):
    variants = collections.OrderedDict(a2c_relational=build_a2c("default"), a2c_relational_spec1=build_a2c("spec1"),
                                       a2c_spec1=build_a2c(None))
    itr = {k: 0 for k in variants}

    def run(name, n):
        runner, sampler, algo, policy = variants[name]
        for _ in range(n):
            bench.one_step(itr[name], sampler, algo)
            itr[name] += 1
    for name in variants:
        run(name, warm)
        torch.cuda.synchronize()
    times = collections.defaultdict(list)
    for _ in range(windows):
        for name in variants:
            times[name].append(_timed(lambda: run(name, window), window))
    for name, (runner, sampler, algo, policy) in variants.items():
        assert torch.isfinite(policy.flat_params).all() and algo._graph is not None, name
    out = {k: _stats(v) for k, v in times.items()}
    out["sizes"] = dict(n_env=bench.N_ENVS, horizon=bench.HORIZON, game=bench.GAME, warmup_iterations=warm,
                        window_iterations=window, windows=windows)
    return out


if __name__ == "__main__":
    counts = [int(a) for a in sys.argv[1:] if a.isdigit()] or [63]
    what = [a for a in sys.argv[1:] if not a.isdigit()] or ["kern", "iter"]
    if "kern" in what:
        for n in counts:
            result.update({"kernel_n%d_b%d" % (n, b): kernel_times(b, n) for b in (256, 1280)})
        print(json.dumps(result), flush=True)
    if "iter" in what:
        result["iteration_us"] = iterations()
        print(json.dumps(result), flush=True)
