"""Noisy-net DQN against plain DQN on the device: one double-DQN update (forward of the three passes, loss, backward,
folds; no optimiser step) at batch 32 with the spec-1 CNN, and one served rollout step (the Q network + arl_dqn_act) at
256 environments, each captured in a hipGraph and replayed.  Prints one JSON line per case.
--net cat: the same for the categorical networks, dueling, 51 atoms -- AtariNoisyNetCatDqnPolicy (Rainbow's network;
its update through the fused loss launch, --unfused: through the combines and arl_catdqn_loss, the policy's default)
against AtariCatDqnPolicy (EpsRainbow's).

    python tools/noisy_bench.py [--iters 200] [--only update|serve] [--net q|cat] [--unfused]

Launches per update: run the update case under `rocprofv3 --kernel-trace --stats -- python tools/noisy_bench.py
--only update --iters N` and divide the kernel count by the replays (N + warm-up, printed as "replays")."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"


NET = "q"
UNFUSED = False


def _policy(noisy, n_act=6):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_cat_dqn_policy import AtariCatDqnPolicy
    from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
    from accel_rl_amd.policies.dqn.atari_noisy_net_cat_dqn_policy import AtariNoisyNetCatDqnPolicy
    from accel_rl_amd.policies.dqn.atari_noisy_net_dqn_policy import AtariNoisyNetDqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(1)
    if NET == "cat":
        p = (AtariNoisyNetCatDqnPolicy(n_atoms=51, dueling=True, **cnn_specs[1]) if noisy else
             AtariCatDqnPolicy(epsilon=0.1, n_atoms=51, dueling=True, **cnn_specs[1]))
    else:
        p = AtariNoisyNetDqnPolicy(**cnn_specs[1]) if noisy else AtariDqnPolicy(epsilon=0.1, **cnn_specs[1])
    p.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(n_act)), device=DEV)
    if NET == "cat":
        p.incorporate_z(np.linspace(-10, 10, 51, dtype=np.float32))
        if noisy:
            p.loss_folds_heads = not UNFUSED
    return p


def _time_graph(fn, iters, warm=3):
    for _ in range(2):
        fn()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(warm):
        graph.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / iters, iters + warm


def bench_update(noisy, iters):
    p = _policy(noisy)
    rs = np.random.RandomState(0)
    b = 32
    obs2 = torch.from_numpy(rs.randint(0, 256, size=(2 * b, 4, 104, 80), dtype=np.uint8)).to(DEV)
    obs, nxt = obs2[:b], obs2[b:]                       # adjacent, as the replay memory hands them out
    act = torch.from_numpy(rs.randint(0, 6, size=b).astype(np.uint8)).to(DEV)
    ret = torch.from_numpy(rs.randn(b).astype(np.float32)).to(DEV)
    term = torch.zeros(b, dtype=torch.uint8, device=DEV)
    isw = torch.ones(b, dtype=torch.float32, device=DEV)
    if NET == "cat":
        def step():
            return p.cat_loss_and_grads(obs, nxt, act, ret, term, isw, -10., 10., 0.97, double_dqn=True)
    else:
        def step():
            return p.q_loss_and_grads(obs, nxt, act, ret, term, isw, 0.99, 1.0, double_dqn=True)
    us, replays = _time_graph(step, iters)
    return dict(case="update", net=NET, policy=_name(noisy), batch=b, us=round(us, 2), replays=replays)


def bench_serve(noisy, iters, n_envs=256):
    p = _policy(noisy)
    rs = np.random.RandomState(1)
    obs = torch.from_numpy(rs.randint(0, 256, size=(n_envs, 4, 104, 80), dtype=np.uint8)).to(DEV)
    p.host_draws(1, n_envs)
    p.set_step(0)
    us, replays = _time_graph(lambda: p.prob_value(obs), iters)
    return dict(case="serve", net=NET, policy=_name(noisy), envs=n_envs, us=round(us, 2), replays=replays)


def _name(noisy):
    return ("noisy" + (("-unfused" if UNFUSED else "-fused") if NET == "cat" else "")) if noisy else "plain"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--only", choices=["update", "serve"], default=None)
    ap.add_argument("--policy", choices=["noisy", "plain", "both"], default="both")
    ap.add_argument("--net", choices=["q", "cat"], default="q")
    ap.add_argument("--unfused", action="store_true")
    a = ap.parse_args()
    global NET, UNFUSED
    NET, UNFUSED = a.net, a.unfused
    from accel_rl_amd import _lib
    _lib.load()
    kinds = [True, False] if a.policy == "both" else [a.policy == "noisy"]
    for noisy in kinds:
        if a.only in (None, "update"):
            print(json.dumps(bench_update(noisy, a.iters)), flush=True)
        if a.only in (None, "serve"):
            print(json.dumps(bench_serve(noisy, a.iters)), flush=True)


if __name__ == "__main__":
    main()
