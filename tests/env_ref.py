"""One agent step of n envs, restated in plain numpy / python on copies of the state arrays: the reference that the env
kernels (csrc/env.hip, env_dev.h, serve_step.hip) are tested against where the oracle's sampler port cannot be -- streams of
any length (a ragged last one included), env counts that no sampler produces, envs that reset at different times.

It follows oracle/synth_ale.py (the emulator), oracle/ref_port.py's PortedAtariEnv (AtariEnv.step / reset, atari_env.py:65-100,
151-191), PortedTrajInfo (sampler/util.py:75-101) and the ResetCollector's rules as CpuSamplerPort restates them
(overlap/worker.py:37-59), and is itself pinned to CpuSamplerPort bit for bit in tests/test_env_limits_host.py.

State (a dict of arrays, one entry per env unless noted): tick, emu_lives, env_lives, over, phase, traj_len, traj_nonzero,
traj_ret, traj_raw, traj_disc (f32), traj_curdisc (f64), obs (the current stacked observation, u8[n][F][104][80]),
noop_cursor (i64[n_streams]: start no-ops consumed so far), noop_ring (u8[n_streams][len]: each stream's pre-drawn start
no-ops, draw i at index i % len).  A stream is envs_per_stream consecutive envs sharing one worker's RNG: the envs of a
stream that reset in a step take the stream's next draws in env order (the worker loops over its envs, worker.py:38-50).
"""
import numpy as np

from oracle import ref_port as P
from oracle import synth_ale

F32, F64 = np.float32, np.float64

STATE_KEYS = ("tick", "emu_lives", "env_lives", "over", "phase", "traj_len", "traj_nonzero", "traj_ret", "traj_raw",
              "traj_disc", "traj_curdisc", "obs", "noop_cursor", "noop_ring")


class StepResult(object):
    """state: the new state; row: the rollout row of every env (reward, raw_reward, done, need_reset); resets: envs that
    reset, ascending; records: completed trajectories (env, Length, Return, RawReturn, NonzeroRewards, DiscountedReturn)
    in env order; streams: per stream dict(lo, hi, cursor, next_cursor, rank={env: rank}, draw={env: start no-ops})."""

    def __init__(self, state, row, resets, records, streams):
        self.state, self.row, self.resets, self.records, self.streams = state, row, resets, records, streams

    def max_stream_resets(self):
        return max(len(s["rank"]) for s in self.streams)

    def straddled(self):
        """Does some stream have resets both below and above an env of its own that does not reset?"""
        for s in self.streams:
            hit = sorted(s["rank"])
            if hit and any(e not in s["rank"] for e in range(hit[0], hit[-1])):
                return True
        return False


class EnvRef(object):

    def __init__(self, game, n_env, envs_per_stream, n_stack=4, frame_skip=4, max_start_noops=30, episodic_lives=True,
                 clip_reward=True, resample="box2x", action_set=None):
        self.game_id, minimal, self.start_lives = synth_ale.GAMES[game]
        self.action_set = list(minimal if action_set is None else action_set)
        self.bank = synth_ale.frame_bank(self.game_id)
        self.n_env, self.per = int(n_env), int(envs_per_stream)
        self.n_streams = (self.n_env + self.per - 1) // self.per            # (the last one may be shorter)
        self.n_stack, self.frame_skip, self.max_start_noops = n_stack, frame_skip, max_start_noops
        self.episodic_lives, self.clip_reward, self.resample = episodic_lives, clip_reward, resample
        self.has_fire, self.has_up = 1 in self.action_set, 2 in self.action_set

    # ---- emulator (synth_ale.SynthALE.act) on env e of the arrays
    def _act(self, st, e, code):
        if st["over"][e]:
            return 0
        st["tick"][e] += 1
        tick = int(st["tick"][e])
        r = synth_ale.reward_fn(tick, int(code))
        if self.start_lives > 0:
            if tick % synth_ale.LIFE_PERIOD == 0:
                st["emu_lives"][e] -= 1
                st["over"][e] = st["emu_lives"][e] == 0
        elif tick >= synth_ale.LIFE_PERIOD * 5:
            st["over"][e] = 1
        return r

    def _screen(self, st, e):
        return self.bank[(int(st["phase"][e]) + int(st["tick"][e])) % synth_ale.K_FRAMES]

    def _push(self, st, e, first):
        img = P.preprocess_pair(first, self._screen(st, e), self.resample)
        st["obs"][e] = np.concatenate([st["obs"][e][1:], img[None]])

    def _press_start(self, st, e):
        self._act(st, e, 0)
        if self.has_fire:
            self._act(st, e, 1)
        if self.has_up:
            self._act(st, e, 2)
        st["env_lives"][e] = st["emu_lives"][e]

    def reset_env(self, st, e, noops):
        """AtariEnv.reset with the start no-op draw made an input (atari_env.py:93-100)."""
        st["tick"][e], st["emu_lives"][e], st["over"][e] = 0, self.start_lives, 0
        st["obs"][e] = 0
        self._press_start(st, e)
        for _ in range(int(noops)):
            self._act(st, e, 0)
        self._push(st, e, None)

    def new_state(self, phases, noop_ring):
        """Every env constructed (phase given) with a fresh trajectory; nothing reset yet."""
        n = self.n_env
        st = dict(tick=np.zeros(n, np.int32), emu_lives=np.zeros(n, np.int32), env_lives=np.zeros(n, np.int32),
                  over=np.zeros(n, np.uint8), phase=np.asarray(phases, np.int32).copy(), traj_len=np.zeros(n, np.int32),
                  traj_nonzero=np.zeros(n, np.int32), traj_ret=np.zeros(n, F32), traj_raw=np.zeros(n, F32),
                  traj_disc=np.zeros(n, F32), traj_curdisc=np.ones(n, F64),
                  obs=np.zeros((n, self.n_stack, P.OBS_H, P.OBS_W), np.uint8),
                  noop_cursor=np.zeros(self.n_streams, np.int64), noop_ring=np.asarray(noop_ring, np.uint8).copy())
        assert st["phase"].shape == (n,) and st["noop_ring"].shape[0] >= self.n_streams
        return st

    def step(self, state, actions, max_path_length=np.inf, discount=1.):
        """One agent step of every env under the ResetCollector (mid-batch resets).  `state` is left untouched."""
        st = {k: np.array(v, copy=True) for k, v in state.items()}
        n = self.n_env
        row = dict(reward=np.zeros(n, F32), raw_reward=np.zeros(n, F32), done=np.zeros(n, bool),
                   need_reset=np.zeros(n, bool))
        resets, records = [], []
        for e in range(n):
            # ---- AtariEnv.step
            code = self.action_set[int(actions[e])]
            reward = F32(0.)
            for _ in range(self.frame_skip - 1):
                reward = F32(reward + F32(self._act(st, e, code)))
            first = self._screen(st, e).copy()
            reward = F32(reward + F32(self._act(st, e, code)))
            self._push(st, e, first)
            raw = reward
            if self.clip_reward:
                reward = F32(np.sign(reward))
            lost = bool(st["emu_lives"][e] < st["env_lives"][e] and st["emu_lives"][e] > 0)
            need_reset = bool(st["over"][e])
            if self.episodic_lives:
                if lost:
                    self._press_start(st, e)
                    st["obs"][e] = 0
                    self._push(st, e, None)
                done = lost or need_reset
            else:
                if lost:
                    self._press_start(st, e)
                done = need_reset
            # ---- TrajInfo.step: f32 accumulators, the running discount a python float
            st["traj_len"][e] += 1
            st["traj_ret"][e] = F32(st["traj_ret"][e] + reward)
            st["traj_raw"][e] = F32(st["traj_raw"][e] + (raw if self.clip_reward else reward))
            st["traj_nonzero"][e] += int(reward != 0)
            st["traj_disc"][e] = F32(st["traj_disc"][e] + F32(F32(st["traj_curdisc"][e]) * reward))
            st["traj_curdisc"][e] = float(st["traj_curdisc"][e]) * float(discount)
            # ---- collector (worker.py:42-50)
            over_len = int(st["traj_len"][e]) > max_path_length
            hit = over_len or (done and (need_reset if self.episodic_lives else True))
            if hit:
                done = True
                if over_len and self.episodic_lives:
                    need_reset = True
                records.append((e, int(st["traj_len"][e]), float(st["traj_ret"][e]), float(st["traj_raw"][e]),
                                int(st["traj_nonzero"][e]), float(st["traj_disc"][e])))
                for k in ("traj_len", "traj_nonzero", "traj_ret", "traj_raw", "traj_disc"):
                    st[k][e] = 0
                st["traj_curdisc"][e] = 1.
                resets.append(e)
            row["reward"][e], row["raw_reward"][e], row["done"][e] = reward, raw, done
            row["need_reset"][e] = need_reset and self.episodic_lives
        # ---- env.reset() of the envs that ended: each stream's draws in env order
        streams = []
        ring_len = st["noop_ring"].shape[1]
        for w in range(self.n_streams):
            lo, hi = w * self.per, min((w + 1) * self.per, n)
            cursor = int(st["noop_cursor"][w])
            info = dict(lo=lo, hi=hi, cursor=cursor, rank=dict(), draw=dict())
            for rank, e in enumerate(x for x in resets if lo <= x < hi):
                noops = int(st["noop_ring"][w, (cursor + rank) % ring_len]) if self.max_start_noops > 0 else 0
                info["rank"][e], info["draw"][e] = rank, noops
                self.reset_env(st, e, noops)
            info["next_cursor"] = cursor + (len(info["rank"]) if self.max_start_noops > 0 else 0)
            st["noop_cursor"][w] = info["next_cursor"]
            streams.append(info)
        return StepResult(st, row, resets, records, streams)

    def tick_after_reset(self, noops):
        """The emulator tick a reset with `noops` start no-ops leaves (press start + no-ops; no life is lost that early)."""
        return 1 + int(self.has_fire) + int(self.has_up) + int(noops)


class RecordingTablePolicy(object):
    """The fixtures' table policy for the oracle's sampler port (key = pixel sum mod 64; actions by the oracle's
    weighted_sample_n on numpy's global stream) that keeps every served action: actions[k] = the k-th call's."""

    def __init__(self, prob_table, value_table):
        self.prob_table, self.value_table, self.actions = prob_table, value_table, []

    def get_actions(self, obs):
        k = obs.reshape(obs.shape[0], -1).astype(np.int64).sum(axis=1) % 64
        prob, value = self.prob_table[k], self.value_table[k]
        acts = P.sample_actions(prob, np.random.rand(len(k)))
        self.actions.append(acts.copy())
        return acts, dict(prob=prob, value=value)


def make_tables(n_act, seed):
    rs = np.random.RandomState(seed)
    logits = rs.randn(64, n_act) * 1.5
    p = np.exp(logits - logits.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(F32), (rs.randn(64) * 2).astype(F32)
