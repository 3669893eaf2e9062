"""The measurements of DESIGN.md 29 (V-MPO; recorded, no bar).  `python tools/vmpo_bench.py [kern] [count]`:
  kern   arl_vmpo_head_loss_parts next to arl_ppg_head_loss_parts' auxiliary phase (the nearest existing launch: the same
         KL work, minus the weighted term) from the same build on the same inputs at 512 x 512, 1 280 x 512 and
         1 280 x 256: each a captured graph of 50 back-to-back launches, the two taking turns, device events around 4
         replays, 15 windows (the method of tools/ppg_bench.py kern); and arl_vmpo_weights alone at 512, 1 280 and 5 120
         rows, measured the same way
  count  the library's entry points called by the learner of one eager V-MPO iteration at config 2's sizes
One process; medians (min / max) are printed as JSON."""
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
PER_GRAPH, REPLAYS, WINDOWS = 50, 4, 15
result = dict()


def save():
    print(json.dumps(result), flush=True)


def _taking_turns(fns):
    """{name: [us per launch of each window]}: one captured graph of PER_GRAPH launches per fn, replayed in turns."""
    graphs = dict()
    for name, fn in fns:
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture_graph(g):
            for _ in range(PER_GRAPH):
                fn()
        for _ in range(3):
            g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    times = collections.defaultdict(list)
    for _ in range(WINDOWS):
        for name, g in graphs.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPLAYS):
                g.replay()
            e.record()
            e.synchronize()
            times[name].append(a.elapsed_time(e) * 1e3 / (PER_GRAPH * REPLAYS))
    return {k: dict(median_us=round(float(np.median(v)), 3), min_us=round(min(v), 3), max_us=round(max(v), 3))
            for k, v in times.items()}


def kernel_times():
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
        duals = torch.tensor([1.0, 5.0], device=DEV)
        psi, temp4 = torch.zeros(n_rows, device=DEV), torch.zeros(4, device=DEV)
        _lib.vmpo_weights(adv, idx, duals, 0.01, psi, temp4)
        dout, dh = torch.empty(batch, K, device=DEV), torch.empty(batch, hid, device=DEV)
        dw, db, loss4 = torch.empty(K, hid, device=DEV), torch.empty(K + 3, device=DEV), torch.empty(4, device=DEV)
        ws = _lib.pg_head_workspace(DEV)
        folds = _lib.FoldList()

        def vmpo():
            folds.vmpo_head_loss(h, w, b, act, psi, ret, old, idx, duals, None, n_act, 0.5, dout, dh, dw, db[:K], loss4,
                                 ws, relu_mask_dh=True)
            folds._n = 0                                # (the launches alone: the fold is the same for both)

        def ppg_aux():
            folds.ppg_head_loss(h, w, b, None, None, ret, old, idx, None, None, n_act, _lib.PPG_AUX, 0., 0.5, 0., 1.0,
                                dout, dh, dw, db[:K], loss4, ws, relu_mask_dh=True)
            folds._n = 0
        key = "B%d-hid%d-A%d" % (batch, hid, n_act)
        out[key] = _taking_turns((("ppg_aux", ppg_aux), ("vmpo_head", vmpo)))
        print("kern %s:" % key, out[key], flush=True)
    result["head_us_per_launch"] = out
    out = dict()
    for n in (512, 1280, 5120):
        gen = torch.Generator(device=DEV).manual_seed(n)
        adv = torch.randn(4 * n, device=DEV, generator=gen)
        idx = torch.randperm(4 * n, device=DEV, generator=gen)[:n].to(torch.int32)
        duals = torch.tensor([1.0, 5.0], device=DEV)
        psi, temp4 = torch.zeros(4 * n, device=DEV), torch.zeros(4, device=DEV)
        out["n%d" % n] = _taking_turns((("vmpo_weights", lambda: _lib.vmpo_weights(adv, idx, duals, 0.01, psi, temp4)),))
        print("weights n %d:" % n, out["n%d" % n], flush=True)
    result["weights_us_per_launch"] = out
    save()


def build_vmpo(use_graph=True):
    from accel_rl_amd.algos.pg import VMPO
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
    algo = VMPO(use_graph=use_graph)
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=1e9, seed=0, affinities=dict(gpu=0),
                     log_interval_steps=1e8)
    runner.startup()
    return runner, sampler, algo, policy


def call_counts():
    """Calls into the library during the learner of one eager iteration (the defaults: 4 epochs of 2 minibatches)."""
    runner, sampler, algo, policy = build_vmpo(use_graph=False)
    lib = _lib.load()
    for itr in range(2):
        bench.one_step(itr, sampler, algo)
    samples, _ = sampler.obtain_samples(2)
    torch.cuda.synchronize()
    counts = collections.Counter()
    originals = dict()
    for name in _lib.EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        originals[name] = fn

        def counting(*a, _fn=fn, _name=name):
            counts[_name] += 1
            return _fn(*a)
        setattr(lib, name, counting)
    try:
        algo.optimize_policy(2, samples)
        torch.cuda.synchronize()
    finally:
        for name, fn in originals.items():
            setattr(lib, name, fn)
    result["library_calls"] = dict(counts, total=sum(counts.values()))
    result["library_calls_sizes"] = dict(n_env=bench.N_ENVS, horizon=bench.HORIZON, spec=bench.CNN_SPEC,
                                         updates=algo.optimizer._n_minibatches,
                                         minibatch=algo.optimizer._minibatch_size)
    print("library calls:", result["library_calls"], result["library_calls_sizes"], flush=True)
    save()
    sampler.shutdown()


if __name__ == "__main__":
    what = sys.argv[1:] or ["kern", "count"]
    if "kern" in what:
        kernel_times()
    if "count" in what:
        call_counts()
