"""The measurements of DESIGN.md 38 (CURL; recorded, no bar).  `python tools/curl_bench.py`:
  kernel   arl_curl_loss_parts (launch + fold) at B = 32 and 512, D = 128, next to the same mathematics as PyTorch calls
           (five matmuls, soft-max, cross-entropy), each a captured graph of 50 calls replayed under device events, the
           two taking turns
  update   the captured CURL update (AtariCurlDqnPolicy, CurlOptimizer) next to the captured DrQ update (m = k = 1,
           AtariDqnPolicy, DqnOptimizer) at batch 32, spec 1, dueling + double: optimize() calls on seeded minibatches,
           50 per window under device events, the two taking turns
One process; medians (min / max) of 9 windows are printed as JSON."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from accel_rl_amd import _lib                           # noqa: E402
from accel_rl_amd.util.misc import capture_graph        # noqa: E402

DEV = torch.device("cuda", 0)
PER, WINDOWS = 50, 9


def _stats(v):
    return dict(median_us=round(float(np.median(v)), 1), min_us=round(min(v), 1), max_us=round(max(v), 1))


def _timed(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e) * 1e3 / PER


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


def kernel_times(b, d=128, coef=1.0):
    rs = np.random.RandomState(b)
    zq, zk = (torch.from_numpy(rs.randn(b, d).astype(np.float32)).to(DEV) for _ in range(2))
    w = torch.from_numpy((rs.randn(d, d) / d).astype(np.float32)).to(DEV)
    dzq, dw, loss2, ws = torch.empty_like(zq), torch.empty_like(w), torch.empty(4, device=DEV), _lib.curl_workspace(d, DEV)
    eye = torch.eye(b, device=DEV)
    out = dict()

    def fused():
        _lib.curl_loss(zq, zk, w, coef, dzq, dw, loss2, ws)

    def library():
        p = zq @ w
        s = p @ zk.T
        out["loss"] = coef * (torch.logsumexp(s, dim=1) - s.diagonal()).mean()
        g = (torch.softmax(s, dim=1) - eye) * (coef / b)
        dp = g @ zk
        out["dzq"], out["dw"] = dp @ w.T, zq.T @ dp

    graphs = dict(fused=_graph(fused), pytorch=_graph(library))
    torch.cuda.synchronize()
    assert torch.allclose(out["dzq"], dzq, rtol=1e-3, atol=1e-6) and torch.allclose(out["dw"], dw, rtol=1e-3, atol=1e-6)
    times = {k: [] for k in graphs}
    for _ in range(WINDOWS):
        for k, g in graphs.items():
            times[k].append(_timed(g.replay))
    return {k: _stats(v) for k, v in times.items()}


def update_times(b=32, n_act=6):
    from accel_rl_amd.algos.dqn import CURL
    from accel_rl_amd.algos.dqn.drq import DrQ
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn import AtariCurlDqnPolicy
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
    from accel_rl_amd.util.seed import set_seed
    set_seed(0)
    rs = np.random.RandomState(0)
    dev = lambda a: torch.from_numpy(a).to(DEV)                 # noqa: E731
    u8 = lambda n: dev(rs.randint(0, 256, size=(n, 4, 104, 80), dtype=np.uint8))       # noqa: E731
    tail = (u8(b), dev(rs.randint(0, n_act, size=b).astype(np.uint8)), dev((rs.randn(b) * 0.05).astype(np.float32)),
            dev((rs.rand(b) < 0.1).astype(np.uint8)))
    rigs = dict()
    for name, algo, cls, views in (("curl", CURL(), AtariCurlDqnPolicy, 2), ("drq", DrQ(), AtariDqnPolicy, 1)):
        policy = cls(dueling=True, **cnn_specs[1])
        policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(n_act)), device=DEV)
        algo.optimizer.initialize(*algo.build_loss(None, policy), target=policy)
        rigs[name] = (algo.optimizer, (u8(views * b),) + tail)
        for _ in range(4):                      # two eager calls, the capture, one replay
            algo.optimizer.optimize(rigs[name][1])
        assert algo.optimizer._graph is not None
    torch.cuda.synchronize()
    times = {k: [] for k in rigs}
    for _ in range(WINDOWS):
        for k, (opt, mb) in rigs.items():
            times[k].append(_timed(lambda: [opt.optimize(mb) for _ in range(PER)]))
    out = {k: _stats(v) for k, v in times.items()}
    out["ratio"] = round(out["curl"]["median_us"] / out["drq"]["median_us"], 3)
    return out


if __name__ == "__main__":
    result = dict(kernel_b32=kernel_times(32), kernel_b512=kernel_times(512))
    print(json.dumps(result), flush=True)
    result["update_b32"] = update_times()
    print(json.dumps(result), flush=True)
