"""Measurement behind DESIGN.md 23 (SAC-Discrete), one MI355X, one process; prints one JSON line per batch size.

arl_sacd_loss (+ arl_sacd_alpha_grad) next to arl_mdqn_loss and arl_dqn_loss at 18 actions in rows of 32 floats: every
variant a captured graph of 20 back-to-back launches (enqueued from Python a launch costs more host time than these
kernels run), the variants taking turns inside the process, device events around each replay; median / min / p90 per
launch over the rounds.  Random rows (not zeros), random actions and terminals, importance weights given.

usage: python tools/sacd_bench.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from accel_rl_amd import _lib                                                                      # noqa: E402
from accel_rl_amd.util.misc import capture_graph                                                   # noqa: E402

DEV = "cuda:0"
N_ACT, STRIDE, INNER = 18, 32, 20


def _stats(us):
    us = np.sort(np.asarray(us))
    return dict(median=round(float(np.median(us)), 2), min=round(float(us[0]), 2),
                p90=round(float(us[int(0.9 * (len(us) - 1))]), 2))


def _graph_of(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture_graph(g):
        for _ in range(INNER):
            fn()
    return g


def _turns(graphs, rounds=40, replays=5):
    for g in graphs.values():
        for _ in range(5):
            g.replay()
    torch.cuda.synchronize()
    out = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                g.replay()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / (replays * INNER))
    return {k: _stats(v) for k, v in out.items()}


def main():
    for batch in (32, 64, 256):
        rs = np.random.RandomState(batch)
        rows = [torch.from_numpy((rs.randn(batch, STRIDE) * 2).astype(np.float32)).to(DEV) for _ in range(6)]
        q1, q2, t1, t2, lo, ln = rows
        act = torch.from_numpy(rs.randint(0, N_ACT, size=batch).astype(np.uint8)).to(DEV)
        ret = torch.from_numpy(rs.randn(batch).astype(np.float32)).to(DEV)
        term = torch.from_numpy((rs.rand(batch) < 0.3).astype(np.uint8)).to(DEV)
        isw = torch.from_numpy((rs.rand(batch) + 0.1).astype(np.float32)).to(DEV)
        log_alpha = torch.tensor([-0.7, 0, 0, 0], dtype=torch.float32, device=DEV)
        dq1, dq2, dl = (torch.empty_like(q1) for _ in range(3))
        stats, grad = torch.empty(4, batch, device=DEV), torch.empty(4, device=DEV)
        pack = torch.empty(2, batch, device=DEV)

        def sacd():
            _lib.sacd_loss(q1, q2, t1, t2, lo, ln, act, ret, term, isw, log_alpha, N_ACT, 0.99, 1.0, dq1, dq2, dl, stats)

        def sacd_with_alpha():
            sacd()
            _lib.sacd_alpha_grad(stats[3], log_alpha, 2.5, grad)

        def mdqn():
            _lib.mdqn_loss(q1, t1, t2, act, ret, term, isw, N_ACT, 0.99, 1.0, 0.03, 0.9, -1.0, dq1, pack[0], pack[1])

        def dqn():
            _lib.dqn_loss(q1, t1, q2, act, ret, term, isw, N_ACT, 0.99, 1.0, dq1, pack[0], pack[1])

        graphs = {k: _graph_of(fn) for k, fn in (("sacd_loss", sacd), ("sacd_loss_and_alpha_grad", sacd_with_alpha),
                                                 ("mdqn_loss", mdqn), ("double_dqn_loss", dqn))}
        print(json.dumps(dict(part="sacd_loss", n_actions=N_ACT, stride=STRIDE, batch=batch, launches_per_graph=INNER,
                              us_per_launch=_turns(graphs))), flush=True)


if __name__ == "__main__":
    main()
