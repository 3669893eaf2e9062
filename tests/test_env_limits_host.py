"""tests/env_ref.py -- the plain restatement of one agent step that the env and served-step kernels are tested against in
test_env_limits_gpu.py -- pinned to the oracle on the CPU: driven with CpuSamplerPort's own actions and start no-op draws
it reproduces the port's rollout arrays, env state and trajectory records bit for bit.  No GPU.
"""
import numpy as np
import pytest

from env_ref import EnvRef, RecordingTablePolicy, make_tables
from oracle import ref_port as P
from oracle import synth_ale

RING = 64


def _state_of_port(ora, ref, rngs):
    """env_ref state equal to a freshly initialised port: the envs' emulator fields, the current observations, fresh
    trajectories, and each worker stream's NEXT start no-op draws (from a copy of its RandomState) as the ring."""
    n = ora.n_envs
    ring = np.zeros((2 * ora.n_parallel, RING), np.uint8)
    for w, rng in enumerate(rngs):
        twin = np.random.RandomState()
        twin.set_state(rng.get_state())
        ring[w] = twin.randint(0, ref.max_start_noops + 1, size=RING)
    st = ref.new_state([env.phase for env in ora.envs], ring)
    for e, env in enumerate(ora.envs):
        st["tick"][e], st["emu_lives"][e], st["env_lives"][e], st["over"][e] = env.tick, env.emu_lives, env.env_lives, env.over
    st["obs"][:] = ora.step_obs
    return st


@pytest.mark.parametrize("game,n_parallel,envs_per,max_len,kw", [
    # frame_skip 40: tick 251 (the first life loss) falls into step 6, before the length limit ends the episode
    ("breakout", 2, 3, 8, dict(max_start_noops=30, frame_skip=40)),
    ("seaquest", 1, 5, 6, dict(max_start_noops=30, episodic_lives=False, clip_reward=False)),
    ("pong", 3, 2, 4, dict(max_start_noops=7, num_img_obs=2, frame_skip=1)),
    ("qbert", 2, 2, 5, dict(max_start_noops=0, num_img_obs=3)),
])
def test_env_ref_reproduces_the_oracle_sampler_port(game, n_parallel, envs_per, max_len, kw):
    horizon, seed, n_batches, discount = 5, 11, 3, 0.99
    ora = P.CpuSamplerPort(game, horizon, n_parallel, envs_per, max_path_length=max_len, mid_batch_reset=True, env_kwargs=kw)
    np.random.seed(seed)
    n_act, _ = ora.initialize(seed + 1, discount=discount)
    n, t = ora.n_envs, horizon
    ref = EnvRef(game, n, envs_per, n_stack=kw.get("num_img_obs", 4), frame_skip=kw.get("frame_skip", 4),
                 max_start_noops=kw["max_start_noops"], episodic_lives=kw.get("episodic_lives", True),
                 clip_reward=kw.get("clip_reward", True))
    rngs = [ora.envs[w * envs_per].rng for w in range(2 * n_parallel)]
    st = _state_of_port(ora, ref, rngs)
    policy = RecordingTablePolicy(*make_tables(n_act, 5))
    n_over_len, n_life_loss, n_resets = 0, 0, 0
    for b in range(n_batches):
        want, completed = ora.obtain_samples(policy)
        calls, policy.actions = policy.actions, []
        assert len(calls) == 2 * t
        records = []
        for s in range(t):
            actions = np.concatenate([calls[2 * s], calls[2 * s + 1]])           # (the port's two groups: env order)
            rows = np.arange(n) * t + s
            np.testing.assert_array_equal(want["actions"][rows], actions)
            np.testing.assert_array_equal(want["observations"][rows], st["obs"])
            res = ref.step(st, actions, max_len, discount)
            msg = "%s batch %d step %d" % (game, b, s)
            np.testing.assert_array_equal(res.row["reward"], want["rewards"][rows], err_msg=msg)
            np.testing.assert_array_equal(res.row["done"], want["dones"][rows], err_msg=msg)
            if ref.clip_reward:
                np.testing.assert_array_equal(res.row["raw_reward"], want["raw_reward"][rows], err_msg=msg)
            if ref.episodic_lives:
                np.testing.assert_array_equal(res.row["need_reset"], want["need_reset"][rows], err_msg=msg)
                n_life_loss += int((res.row["done"] & ~res.row["need_reset"]).sum())
            n_over_len += sum(1 for rec in res.records if rec[1] > max_len)
            n_resets += len(res.resets)
            assert sorted(res.resets) == res.resets == [rec[0] for rec in res.records]
            for w, info in enumerate(res.streams):                                # ranks: env order inside the stream
                assert sorted(info["rank"], key=info["rank"].get) == sorted(info["rank"])
                assert info["next_cursor"] - info["cursor"] == (len(info["rank"]) if ref.max_start_noops else 0)
            records += [rec[1:] for rec in res.records]
            st = res.state
        np.testing.assert_array_equal(want["extra_observations"], st["obs"])
        assert records == [ti.as_tuple() for ti in completed]                     # same (step, env) order, bit for bit
        # the port's own state behind the arrays: emulators, wrappers, trajectory accumulators
        for e, (env, traj) in enumerate(zip(ora.envs, ora.trajs)):
            got = (st["tick"][e], st["emu_lives"][e], st["env_lives"][e], bool(st["over"][e]), st["phase"][e])
            assert got == (env.tick, env.emu_lives, env.env_lives, bool(env.over), env.phase), (e, got)
            assert (st["traj_len"][e], st["traj_ret"][e], st["traj_raw"][e], st["traj_nonzero"][e], st["traj_disc"][e]) == \
                (traj["Length"], traj["Return"], traj["RawReturn"], traj["NonzeroRewards"], traj["DiscountedReturn"]), e
            assert float(st["traj_curdisc"][e]) == traj.cur_discount
        np.testing.assert_array_equal(st["obs"], ora.step_obs)
    assert n_over_len >= n, "every env must run over length"
    assert n_resets >= n_over_len
    if game == "breakout":
        assert n_life_loss >= n, "tick 251 within the run: every env loses a life"
    if ref.max_start_noops:                                                       # every stream consumed draws, none wrapped
        assert (st["noop_cursor"] > 0).all() and st["noop_cursor"].max() <= RING


def test_ragged_last_stream_and_rank_order():
    """What no sampler produces: 7 envs in streams of 3 (the last stream has one env), envs resetting at different times.
    The ranks count a stream's resetting envs in env order, the draws follow the cursor, the ring wraps."""
    ref = EnvRef("breakout", 7, 3, max_start_noops=30)
    assert ref.n_streams == 3
    ring = np.arange(3 * 4, dtype=np.uint8).reshape(3, 4) + 1
    st = ref.new_state(np.arange(7), ring)
    for e in range(7):
        ref.reset_env(st, e, 0)
    st["traj_len"][:] = [3, 0, 3, 3, 3, 0, 3]                                      # limit 3: envs 0, 2, 3, 4, 6 end now
    st["noop_cursor"][:] = [3, 0, 9]
    res = ref.step(st, np.zeros(7, np.int64), 3, 0.99)
    assert res.resets == [0, 2, 3, 4, 6] and res.straddled() and res.max_stream_resets() == 2
    assert [s["rank"] for s in res.streams] == [{0: 0, 2: 1}, {3: 0, 4: 1}, {6: 0}]
    assert [s["draw"] for s in res.streams] == [{0: 4, 2: 1}, {3: 5, 4: 6}, {6: 10}]      # (3, 4) % 4; 0, 1; 9 % 4
    np.testing.assert_array_equal(res.state["noop_cursor"], [5, 2, 10])
    for s in res.streams:
        for e, noops in s["draw"].items():
            assert res.state["tick"][e] == ref.tick_after_reset(noops) == 2 + noops
    assert res.state["tick"][1] == st["tick"][1] + 4 and st["tick"][1] == 2          # the caller's state is untouched
    assert (res.state["obs"][0, :3] == 0).all() and res.state["obs"][0, 3].any()     # a blank stack with one frame
    np.testing.assert_array_equal(res.state["obs"][1, 2], st["obs"][1, 3])           # a stack shift
    np.testing.assert_array_equal(
        res.state["obs"][1, 3], P.preprocess_pair(ref.bank[(1 + 5) % synth_ale.K_FRAMES], ref.bank[(1 + 6) % synth_ale.K_FRAMES]))
