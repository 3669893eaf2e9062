"""The env-step and served-step kernels (csrc/env.hip, env_dev.h, serve_step.hip: arl_env_step, arl_env_step_served) at the
limits their entry points accept, beyond what the samplers produce at the benchmark's shapes:

  (2) through the sampler, under a hipGraph, against the oracle's sampler port (oracle/ref_port.py CpuSamplerPort), bit for
      bit: streams of 65 and 257 envs (two rounds of the served kernel's 64-env ballots / of env_step_kernel's 256-env
      counts, ranks 0..256 across the round boundary), frame stacks of 1, 2, 3 and 5, frame_skip 1, no start no-ops,
      frozen envs without mid-batch resets;
  (3) launches driven by hand on twin allocations with n_env / envs_per_stream no sampler produces (1 .. 34 envs, ragged
      last streams, streams longer than n_env; the 16-shard arrival ticket at 1, 15, 16, 17, 33 envs), envs that reset at
      different times -- arl_env_step against arl_env_step_served against tests/env_ref.py after every launch;
  (4) the served head at its limits: hid 4 .. 1024, 0 .. 130 split partials (empty fold groups, the 16- and 64-way folds
      at exactly 64 KiB of scratch), bias / rectifier on and off, conv 1 of 16 and 32 filters riding along or not, the
      draw at u = 0 / a cumsum value / past the last one, saturated and all-equal logits -- against the separate launches
      bit for bit, a float64 head, and the oracle's weighted_sample_n; and every refusal as an argument error that launches
      nothing.

References: tests/env_ref.py (pinned to the oracle in test_env_limits_host.py), CpuSamplerPort, float64 numpy.  Everything
but the float64 comparison (tolerance: test_head_limits_gpu._tol) is bit-exact.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from env_ref import EnvRef, make_tables
from oracle import ref_port as P
from test_head_limits_gpu import _close
from test_sampler_gpu import DeviceTablePolicy, HostTablePolicy, make_gpu_sampler
from test_serve_step_gpu import EchoPolicy, env_state, host, make_sampler, traj_tuples

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, HORIZON = 17, 5


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_oracle_runs():
    yield
    _oracle_table_run.cache_clear()


# =====================================================================================================================
# (2) through the sampler against the oracle port
# =====================================================================================================================

@functools.lru_cache(maxsize=1)
def _oracle_table_run(game, n_parallel, envs_per, max_len, kw_items, mbr, n_batches):
    """The oracle port's batches under the table policy, computed once for the tests that share a configuration:
    (tables, [(numpy's global state before the batch, its arrays, its sorted trajectory tuples)])."""
    ora = P.CpuSamplerPort(game, HORIZON, n_parallel, envs_per, max_path_length=max_len, mid_batch_reset=mbr,
                           env_kwargs=dict(kw_items))
    np.random.seed(SEED)
    n_act, _ = ora.initialize(SEED + 1, discount=0.99)
    tables = make_tables(n_act, 77)
    policy = HostTablePolicy(*tables)
    np.random.seed(SEED + 5)
    runs = []
    for _ in range(n_batches):
        state = np.random.get_state()
        want, completed = ora.obtain_samples(policy)
        runs.append((state, {k: v.copy() for k, v in want.items()}, sorted(ti.as_tuple() for ti in completed)))
    return tables, runs


def _stream_resets(want, n, per):
    """Per (stream, step): how many of the stream's envs the port reset (episodic lives: need_reset marks exactly those)."""
    hits = want["need_reset"].reshape(n, HORIZON)
    return np.stack([hits[lo:lo + per].sum(axis=0) for lo in range(0, n, per)])


def _compare_batch(buf, want, mbr, msg):
    valid = np.ones(len(want["actions"]), bool)
    if not mbr:                                                  # NonResetCollector leaves stale rows behind an episode's end
        valid = P.valid_mask(want["need_reset"].reshape(-1, HORIZON)).reshape(-1).astype(bool)
    pairs = [("actions", buf.actions, False), ("prob", buf.agent_infos["prob"], False),
             ("value", buf.agent_infos["value"], False), ("rewards", buf.rewards, True), ("dones", buf.dones, True),
             ("observations", buf.observations, True)]
    pairs += [(k, buf.env_infos[k], True) for k in ("raw_reward", "need_reset") if k in buf.env_infos]
    for key, got, masked in pairs:
        got = got.cpu().numpy().astype(want[key].dtype)
        sel = valid if masked else slice(None)
        np.testing.assert_array_equal(got[sel], want[key][sel], err_msg="%s %s" % (key, msg))
    np.testing.assert_array_equal(buf.extra_observations.cpu().numpy(), want["extra_observations"], err_msg=msg)


def _table_sampler_against_the_port(game, n_parallel, envs_per, max_len, kw, serves_rows, mbr=True, n_batches=3,
                                    policy_cls=None):
    """GpuVecSampler under a hipGraph with the device table policy against the port's cached run.  Returns the sampler
    facts a caller asserts on: (max resets of one stream in one step, envs that reset at all, completed trajectories)."""
    tables, runs = _oracle_table_run(game, n_parallel, envs_per, max_len, tuple(sorted(kw.items())), mbr, n_batches)
    if policy_cls is None:
        smp = make_gpu_sampler(game, HORIZON, n_parallel, envs_per, SEED, mbr, max_len, kw, tables, 0.99, True,
                               serves_rows=serves_rows)
    else:
        from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
        from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
        from accel_rl_amd.util import logger
        logger.set_quiet(True)
        smp = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(kw, game=game), horizon=HORIZON, n_parallel=n_parallel,
                            envs_per=envs_per, mid_batch_reset=mbr, max_path_length=max_len, max_decorrelation_steps=0,
                            device=DEV, use_graph=True)
        np.random.seed(SEED)
        smp.initialize(seed=SEED + 1, affinities=dict(), discount=0.99, need_extra_obs=True)
        smp.policy_init(policy_cls(*tables, serves_rows=serves_rows))
    assert smp._single_write == (serves_rows and mbr) and not smp._serve_fused
    assert smp._game.n_stack == kw.get("num_img_obs", 4) and smp._game.frame_skip == kw.get("frame_skip", 4)
    n = 2 * n_parallel * envs_per
    most, n_traj, ever = 0, 0, np.zeros(n, bool)
    for b, (state, want, want_t) in enumerate(runs):
        np.random.set_state(state)
        buf, infos = smp.obtain_samples(b)
        got_t = sorted((ti.Length, ti.Return, ti.RawReturn, ti.NonzeroRewards, ti.DiscountedReturn) for ti in infos)
        _compare_batch(buf, want, mbr, "%s batch %d" % (game, b))
        assert got_t == want_t
        n_traj += len(want_t)
        most = max(most, int(_stream_resets(want, n, envs_per).max()))
        ever |= want["need_reset"].reshape(n, HORIZON).any(axis=1)
    assert int(smp._st.epoch[2].item()) == 0                     # no reset the forecast had not announced
    assert (smp.policy.row_calls > 0) == smp._single_write
    smp.shutdown()
    return most, int(ever.sum()), n_traj


def _cnn_sampler_against_the_port(game, n_parallel, envs_per, max_len, kw, n_batches=3, twin=True):
    """The real AtariCnnPolicy (spec 1): the served sampler (arl_env_step_served per step) under a hipGraph against the
    separate launches (every array, the env state, the records) and against the oracle port served the same network
    through EchoPolicy.  Returns (max resets of one stream in one step, the served sampler's conv-1-in-launch flag)."""
    from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    policy = AtariCnnPolicy(**cnn_specs[1])
    b = make_sampler(game, n_parallel, envs_per, HORIZON, SEED, max_len, kw, policy, True, served=True)
    a = make_sampler(game, n_parallel, envs_per, HORIZON, SEED, max_len, kw, policy, True, served=False) if twin else None
    assert b._serve_fused and b._single_write
    assert a is None or (not a._serve_fused and a._single_write)
    n = 2 * n_parallel * envs_per
    with_conv1 = policy.serve_conv1(b._game, n)[0] is not None
    with torch.no_grad():                                        # a sharp head: the softmax and the draw matter
        policy.flat_params[policy._offsets[policy._k_head]:].mul_(40.0)
    ora = P.CpuSamplerPort(game, HORIZON, n_parallel, envs_per, max_path_length=max_len, mid_batch_reset=True, env_kwargs=kw)
    np.random.seed(SEED)
    ora.initialize(SEED + 1, discount=0.99)
    echo = EchoPolicy(policy, n)
    state = np.random.get_state()
    most, n_traj = 0, 0
    for k in range(n_batches):
        np.random.set_state(state)
        buf_b, infos_b = b.obtain_samples(k)
        got_b, traj_b = host(buf_b), traj_tuples(infos_b)
        if a is not None:
            np.random.set_state(state)
            buf_a, infos_a = a.obtain_samples(k)
            got_a, traj_a = host(buf_a), traj_tuples(infos_a)
            for key in got_a:
                np.testing.assert_array_equal(got_b[key], got_a[key], err_msg="twins %s batch %d" % (key, k))
            sa, sb = env_state(a), env_state(b)
            for key in sa:
                np.testing.assert_array_equal(sb[key], sa[key], err_msg="twins state %s batch %d" % (key, k))
            assert traj_a == traj_b
        np.random.set_state(state)
        want, completed = ora.obtain_samples(echo)
        state = np.random.get_state()
        for key, wkey in (("actions", "actions"), ("rewards", "rewards"), ("dones", "dones"), ("env_raw_reward", "raw_reward"),
                          ("env_need_reset", "need_reset"), ("prob", "prob"), ("value", "value"),
                          ("observations", "observations"), ("extra_observations", "extra_observations")):
            np.testing.assert_array_equal(got_b[key].astype(want[wkey].dtype), want[wkey], err_msg="%s batch %d" % (key, k))
        assert sorted(t[1:] for t in traj_b) == sorted(ti.as_tuple() for ti in completed)
        n_traj += len(traj_b)
        most = max(most, int(_stream_resets(want, n, envs_per).max()))
    assert int(b._st.epoch[2].item()) == 0 and n_traj > 0
    assert len(np.unique(got_b["actions"])) > 1
    b.shutdown()
    if a is not None:
        a.shutdown()
    return most, with_conv1


# ---- long streams: the reset-rank loops beyond one round

@pytest.mark.parametrize("envs_per,serves_rows", [(65, False), (65, True), (257, False), (257, True)])
def test_long_streams_separate_launches(envs_per, serves_rows):
    """One stream of 65 / 257 envs per group: env_step_kernel counts a stream's resets 256 envs per round, so 257 takes a
    second round.  Length limit 4: every env of a stream runs over length in the same step -- ranks 0 .. envs_per - 1."""
    most, ever, n_traj = _table_sampler_against_the_port("breakout", 1, envs_per, 4, dict(max_start_noops=30), serves_rows)
    assert most == envs_per and ever == 2 * envs_per and n_traj >= 2 * envs_per * 2
    assert (envs_per + 255) // 256 == (2 if envs_per == 257 else 1)


@pytest.mark.parametrize("envs_per", [65, 257])
def test_long_streams_served(envs_per):
    """serve_step_kernel ranks with wave ballots, 64 envs per round: 2 rounds at 65, 5 at 257 (514 envs: inside both of
    _serve_in_step_max_envs).  The served sampler against the oracle port; at 65 also against the separate launches."""
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    assert 2 * envs_per <= GpuVecSampler._serve_in_step_max_envs[1]
    most, with_conv1 = _cnn_sampler_against_the_port("breakout", 1, envs_per, 4, dict(max_start_noops=30),
                                                     twin=envs_per == 65)
    assert most == envs_per and with_conv1 and (envs_per + 63) // 64 == (2 if envs_per == 65 else 5)


# ---- frame stacks other than 4

class _ServeOfferingTablePolicy(DeviceTablePolicy):
    """A table policy that OFFERS the served step: only the sampler's own frame-stack rule can decline it."""

    def serve_supported(self):
        return True

    def serve_forward(self, *args, **kwargs):
        raise AssertionError("the sampler handed a frame stack deeper than 4 to the served step")

    def serve_conv1(self, game, b):
        return None, None


@pytest.mark.parametrize("serves_rows", [False, True])
@pytest.mark.parametrize("n_stack", [1, 2, 3, 5])
def test_frame_stacks_separate_launches(n_stack, serves_rows):
    """FramePush keeps MAX_STACK - 1 older planes in registers: stacks of 1, 2 and 3 through the wide column copy
    (single_write) and the narrow one (two writes); 5 takes push_frame, and the served step must be declined."""
    kw = dict(max_start_noops=30, num_img_obs=n_stack)
    most, ever, n_traj = _table_sampler_against_the_port("pong", 2, 3, 6, kw, serves_rows,
                                                         policy_cls=_ServeOfferingTablePolicy if n_stack == 5 else None)
    assert most == 3 and ever == 12 and n_traj >= 12


@pytest.mark.parametrize("n_stack", [1, 2, 3])
def test_frame_stacks_served_with_conv1_in_the_launch(n_stack):
    most, with_conv1 = _cnn_sampler_against_the_port("pong", 2, 3, 6, dict(max_start_noops=30, num_img_obs=n_stack))
    assert most == 3 and with_conv1                              # conv 1 of depth n_stack rode in the step launch


# ---- frame_skip 1, no start no-ops

@pytest.mark.parametrize("form", ["two_writes", "single_write", "served"])
@pytest.mark.parametrize("kw", [dict(max_start_noops=30, frame_skip=1), dict(max_start_noops=0)], ids=["skip1", "noop0"])
def test_frame_skip_1_and_no_start_noops(form, kw):
    """frame_skip 1: no first-loop iterations, the two frames of a step one tick apart.  max_start_noops 0: no draws, no
    ranks, cursors that never move (asserted on the device)."""
    if form == "served":
        most, _ = _cnn_sampler_against_the_port("seaquest", 2, 3, 6, kw)
    else:
        most, ever, _ = _table_sampler_against_the_port("seaquest", 2, 3, 6, kw, form == "single_write")
        assert ever == 12
    assert most == 3


def test_no_start_noops_leaves_the_cursors_alone():
    tables = make_tables(4, 1)
    smp = make_gpu_sampler("breakout", HORIZON, 2, 3, SEED, True, 3, dict(max_start_noops=0), tables, 0.99, True,
                           serves_rows=True)
    for b in range(2):
        _, infos = smp.obtain_samples(b)
        assert len(infos) >= 12
    assert int(smp._st.noop_cursor.abs().sum().item()) == 0 and int(smp._st.epoch[2].item()) == 0
    smp.shutdown()


# ---- frozen envs

def test_long_stream_without_mid_batch_resets():
    """mid_batch_reset False at 65 envs per stream: envs freeze at their episode's end, the `active`-less step skips them,
    and the end-of-batch arl_env_reset ranks the 65 flagged envs of a stream."""
    most, ever, n_traj = _table_sampler_against_the_port("breakout", 1, 65, 4, dict(max_start_noops=30), False, mbr=False)
    assert ever == 130 and n_traj >= 130


# =====================================================================================================================
# (3) + (4) launches driven by hand on twin allocations
# =====================================================================================================================

N_ALLOC = 34
STATE_KEYS = ("tick", "emu_lives", "env_lives", "phase", "over", "traj_len", "traj_nonzero", "traj_ret", "traj_raw",
              "traj_disc", "traj_curdisc")


@pytest.fixture(scope="module")
def twins():
    """Two identically seeded 34-env samplers (34 streams of one env: room for any stream layout of <= 34 envs); only
    their device allocations, game and rollout descriptions are used -- every launch below is made by hand."""
    tables = make_tables(18, 3)
    pair = [make_gpu_sampler("seaquest", HORIZON, N_ALLOC // 2, 1, 9, True, 1000, dict(max_start_noops=30), tables, 0.99,
                             False, serves_rows=True) for _ in range(2)]
    yield pair
    for smp in pair:
        smp.shutdown()


def _snapshot(smp):
    torch.cuda.synchronize()
    out = {"st." + k: v.clone() for k, v in smp._st.items()}
    buf = smp.samples_buf
    out.update(observations=buf.observations.clone(), rewards=buf.rewards.clone(), dones=buf.dones.clone(),
               actions=buf.actions.clone(), prob=buf.agent_infos["prob"].clone(), value=buf.agent_infos["value"].clone(),
               step_obs=smp.step_obs.clone())
    out.update(("env_" + k, v.clone()) for k, v in buf.env_infos.items())
    return out


def _assert_same(got, want, skip=()):
    for k in want:
        if k not in skip:
            assert torch.equal(got[k], want[k]), k


class Harness(object):
    """n envs in streams of `per` on the first rows of both twins' allocations: twin A steps with the separate launches
    (arl_fold_many + arl_bias_relu + arl_pg_head_infer + arl_env_step(single_write)), twin B with arl_env_step_served;
    after every launch both are compared with each other and with env_ref's step."""

    def __init__(self, twins, n, per, n_act, max_len, seed, ring_len=8, max_start_noops=30):
        from accel_rl_amd import _lib
        self.lib, self.twins, self.n, self.per, self.A, self.L = _lib, twins, n, per, n_act, max_len
        self.noops, self.discount, self.t = max_start_noops, 0.99, HORIZON
        self.ref = EnvRef("seaquest", n, per, max_start_noops=max_start_noops, action_set=list(range(n_act)))
        rs = np.random.RandomState(seed)
        ns = self.ref.n_streams
        st = self.ref.new_state(rs.randint(0, 64, n), rs.randint(0, max_start_noops + 1, (ns, ring_len)))
        for e in range(n):
            self.ref.reset_env(st, e, rs.randint(0, max_start_noops + 1))
        # desynchronised, and nobody due at the first step: the zeroed forecast below is then the truth
        st["traj_len"][:] = rs.randint(0, max_len - 1, n)
        st["noop_cursor"][:] = rs.randint(0, 50, ns)
        self.st, self.rs, self.cursor0 = st, rs, int(st["noop_cursor"].sum())
        self.games, self.states = [], []
        for smp in twins:
            g = _lib.ArlGame.from_buffer_copy(smp._game)
            g.n_actions = n_act
            s = _lib.ArlEnvState.from_buffer_copy(smp._state)
            s.n_env, s.envs_per_stream, s.noop_ring_len = n, per, ring_len
            self.games.append(g)
            self.states.append(s)
            d = smp._st
            for k in STATE_KEYS:
                d[k].zero_()
                d[k][:n].copy_(torch.from_numpy(st[k]))
            for k in ("epoch", "launch_count", "frozen", "next_reset", "done_count", "reset_flag", "noop_ring", "noop_cursor", "done_int", "done_flt",
                      "frame_a", "frame_b", "frame_mode"):
                d[k].zero_()
            d.noop_ring.view(-1)[:ns * ring_len].copy_(torch.from_numpy(st["noop_ring"][:ns].reshape(-1)))
            d.noop_cursor.view(-1)[:2 * ns].copy_(torch.from_numpy(np.tile(st["noop_cursor"], 2)))
            smp.step_obs.zero_()
            smp.step_obs[:n].copy_(torch.from_numpy(st["obs"]))
            buf = smp.samples_buf
            for v in (buf.observations, buf.rewards, buf.dones, buf.actions, buf.agent_infos["prob"], buf.agent_infos["value"],
                      buf.env_infos["raw_reward"], buf.env_infos["need_reset"]):
                v.zero_()
        self.forecast, self.n_launches, self.batch_records = np.zeros(n, bool), 0, []
        self.rows = torch.arange(n, dtype=torch.int64, device=DEV) * self.t

    def begin_batch(self):
        for smp, g, s in zip(self.twins, self.games, self.states):
            self.lib.rollout_begin(g, s, smp._rollout)
        self.batch_records = []

    def current_obs(self, smp, step):
        return smp.samples_buf.observations[self.rows + step]

    def _ticket(self, smp):
        return int(smp._st.epoch[0].item()), int(smp._st.launch_count[0].item())

    def launch(self, step, spec, u_fn, conv=None, what=""):
        """spec: dict(part, splits, bias, relu, w, b) of device tensors -- the served head's input.  u_fn(prob of twin A's
        head, numpy) -> the uniforms.  conv: None or dict(geom, w, bias, y) for conv 1 riding in B's launch."""
        lib, n, A, t = self.lib, self.n, self.A, self.t
        a, b = self.twins
        hid = spec["w"].shape[1]
        before = [self._ticket(smp) for smp in self.twins]
        # ---- twin A: the separate launches
        if spec["splits"] > 0:
            h = torch.empty((n, hid), dtype=torch.float32, device=DEV)
            fl = lib.FoldList()
            it = fl._items[0]
            it.part, it.out, it.total, it.splits, it.valid = spec["part"].data_ptr(), h.data_ptr(), n * hid, spec["splits"], 0
            fl._n = 1
            fl.run()
            if spec["relu"]:
                lib.bias_relu(h, spec["bias"] if spec["bias"] is not None else torch.zeros(hid, device=DEV), n, hid)
            elif spec["bias"] is not None:
                h.add_(spec["bias"])
        else:
            h = spec["part"]
        prob = torch.empty((n, A), dtype=torch.float32, device=DEV)
        value = torch.empty(n, dtype=torch.float32, device=DEV)
        lib.pg_head_infer(h, spec["w"], spec["b"], prob, value)
        prob_np = prob.cpu().numpy()
        assert np.isfinite(prob_np).all() and np.isfinite(value.cpu().numpy()).all(), what
        u_np = np.asarray(u_fn(prob_np), np.float64)
        u = torch.from_numpy(u_np).to(DEV)
        lib.env_step(self.games[0], self.states[0], a._rollout, prob, value, u, step, True, self.L, self.discount, self.noops,
                     single_write=True)
        # ---- twin B: one launch
        head = lib.ArlServeHead()
        head.hidden.part, head.hidden.total, head.hidden.splits = spec["part"].data_ptr(), n * hid, spec["splits"]
        head.hidden_bias = None if spec["bias"] is None else spec["bias"].data_ptr()
        head.hidden_relu, head.hid = int(spec["relu"]), hid
        head.w_head, head.b_head = spec["w"].data_ptr(), spec["b"].data_ptr()
        c1 = None
        if conv is not None:
            c1 = lib.ArlServeConv1()
            c1.geom = C.pointer(conv["geom"])
            c1.w, c1.bias, c1.y = conv["w"].data_ptr(), conv["bias"].data_ptr(), conv["y"].data_ptr()
            c1.scale, c1.relu = 1. / 255, 1
            conv["y"].fill_(-7.0)
        lib.env_step_served(self.games[1], self.states[1], b._rollout, head, c1, u, step, self.L, self.discount, self.noops)
        torch.cuda.synchronize()
        self.n_launches += 1
        # ---- (a) the twins, bit for bit (the completed-trajectory slots are handed out in arrival order: compared below)
        sa, sb = _snapshot(a), _snapshot(b)
        _assert_same(sb, sa, skip=("st.done_int", "st.done_flt"))
        # ---- the ticket
        for smp, (e0, l0) in zip(self.twins, before):
            ep = smp._st.epoch.cpu().numpy()
            assert (int(ep[0]), int(smp._st.launch_count[0].item())) == (e0 + 1, l0 + 1), what
            assert ep[1] == 0 and ep[2] == 0 and not ep[32::32].any(), (what, ep[:3], ep[32::32])
        # ---- env_ref's step, given the device's actions
        rows = (np.arange(n) * t + step)
        got = {k: v.cpu().numpy() for k, v in sb.items()}
        flat_prob = got["prob"].reshape(-1)[:n * t * A].reshape(n * t, A)
        actions = got["actions"][rows]
        np.testing.assert_array_equal(flat_prob[rows], prob_np, err_msg=what)
        np.testing.assert_array_equal(got["value"][rows], value.cpu().numpy(), err_msg=what)
        np.testing.assert_array_equal(actions, P.sample_actions(flat_prob[rows], u_np), err_msg=what)       # (c) the draw
        res = self.ref.step(self.st, actions, self.L, self.discount)
        np.testing.assert_array_equal(np.flatnonzero(self.forecast), res.resets, err_msg=what)
        for k in STATE_KEYS:
            np.testing.assert_array_equal(got["st." + k][:n], res.state[k], err_msg="%s %s" % (k, what))
        np.testing.assert_array_equal(got["rewards"][rows], res.row["reward"], err_msg=what)
        np.testing.assert_array_equal(got["dones"][rows].astype(bool), res.row["done"], err_msg=what)
        np.testing.assert_array_equal(got["env_raw_reward"][rows], res.row["raw_reward"], err_msg=what)
        np.testing.assert_array_equal(got["env_need_reset"][rows].astype(bool), res.row["need_reset"], err_msg=what)
        new_obs = got["observations"][rows + 1] if step + 1 < t else got["step_obs"][:n]
        np.testing.assert_array_equal(new_obs, res.state["obs"], err_msg=what)
        ns = self.ref.n_streams
        par = int(got["st.epoch"][0]) & 1
        np.testing.assert_array_equal(got["st.noop_cursor"].reshape(-1)[par * ns:(par + 1) * ns], res.state["noop_cursor"])
        for s in res.streams:
            for e, noops in s["draw"].items():                   # the draw of the env's rank in its stream
                assert got["st.tick"][e] == self.ref.tick_after_reset(noops), (what, e, s)
        np.testing.assert_array_equal(got["st.reset_flag"][:n].astype(bool), np.isin(np.arange(n), res.resets))
        lpar = int(got["st.launch_count"][0]) & 1
        self.forecast = got["st.next_reset"].reshape(-1)[lpar * n:(lpar + 1) * n].astype(bool)
        self.batch_records += res.records
        count = int(got["st.done_count"][0])
        assert count == len(self.batch_records)
        for smp in self.twins:
            ints, flts = smp._st.done_int[:count].cpu().numpy(), smp._st.done_flt[:count].cpu().numpy()
            recs = sorted((int(i[0]), int(i[1]), float(f[0]), float(f[1]), int(i[2]), float(f[2])) for i, f in zip(ints, flts))
            assert recs == sorted(self.batch_records), what
        # ---- conv 1 of the observation just written
        if conv is not None:
            want_y = torch.empty_like(conv["y"])
            if step + 1 < t:
                lib.conv2d_u8_fwd(b.samples_buf.observations, (self.rows + step + 1).to(torch.int32), 1. / 255, conv["w"],
                                  conv["bias"], want_y, conv["geom"], True)
            else:
                lib.conv2d_u8_fwd(b.step_obs[:n].contiguous(), None, 1. / 255, conv["w"], conv["bias"], want_y, conv["geom"], True)
            torch.cuda.synchronize()
            assert torch.equal(conv["y"], want_y) and float(want_y.abs().sum()) > 0, what
        self.st = res.state
        return res, prob_np, value.cpu().numpy()


def _onehot_spec(h, step, w, b):
    """Finished activations (splits 0): one-hot of the observation's table key -- a policy that depends on the pixels."""
    obs = h.current_obs(h.twins[0], step)
    keys = obs.reshape(obs.shape[0], -1).sum(dim=1, dtype=torch.int64) % 64
    part = torch.nn.functional.one_hot(keys, 64).to(torch.float32).contiguous()
    return dict(part=part, splits=0, bias=None, relu=0, w=w, b=b)


@pytest.mark.parametrize("n,per,straddle", [(1, 1, False), (15, 4, True), (16, 16, True), (17, 5, True), (33, 7, True),
                                            (34, 64, True), (33, 33, True)])
def test_env_counts_streams_and_the_ticket(twins, n, per, straddle):
    """n_env / envs_per_stream the sampler cannot produce: a ragged last stream (15 / 4, 17 / 5, 33 / 7), a stream longer
    than n_env (34 / 64), the ticket's 16 shards at 1, 15, 16, 17, 33 and 34 arrivals; envs that run over length at
    different steps, so that a stream's resets sit between envs that go on (asserted for the longer streams)."""
    A, L = 6, 6
    h = Harness(twins, n, per, A, L, seed=100 + n)
    g = torch.Generator(device="cpu").manual_seed(n)
    w = (torch.randn(A + 1, 64, generator=g) * 2).to(DEV)
    b = torch.zeros(A + 1, device=DEV)
    n_resets, straddled = 0, False
    for batch in range(3):                                      # 15 steps >= L + 2: every env ends an episode twice
        h.begin_batch()
        for step in range(HORIZON):
            res, _, _ = h.launch(step, _onehot_spec(h, step, w, b), lambda p: h.rs.rand(n), what="n %d per %d batch %d step %d" %
                                 (n, per, batch, step))
            n_resets += len(res.resets)
            straddled |= res.straddled()
            assert len(res.resets) < n or n == 1                 # desynchronised: never everybody at once
    assert n_resets >= 2 * n and straddled == straddle
    assert h.ref.n_streams == (n + per - 1) // per
    assert int(h.st["noop_cursor"].sum()) - h.cursor0 == n_resets                              # (the ring holds 8 draws)


COMBOS = list(itertools.product([None, 16, 32], [False, True], [0, 1]))     # (conv 1 filters, hidden bias, rectifier)


@pytest.mark.parametrize("A,hid,splits,wide_from", [
    (1, 4, 0, 0), (2, 4, 1, 0), (6, 68, 15, 0), (18, 100, 16, 0), (18, 1024, 17, 0),
    (18, 1024, 127, 0),          # zgn 16 at exactly 64 KiB of fold scratch
    (4, 256, 128, 0),            # the 64-way fold at exactly 64 KiB
    (4, 256, 130, 0),            # ... with groups of 3 and 2 splits
    (9, 256, 3, 2),              # the 64-way fold made cheap: 61 empty groups
])
def test_served_head_fold_and_draw(twins, A, hid, splits, wide_from):
    """17 envs in streams of 5 (a ragged last one).  Every launch: (a) twins bit for bit, (b) prob / value against a
    float64 fold + bias + rectifier + heads + softmax, (c) the draw against weighted_sample_n -- over the 12 combinations
    of (conv 1: none, 16, 32 filters) x (hidden bias) x (rectifier), steps horizon - 1 with conv 1 included."""
    from accel_rl_amd import _lib
    n, L = 17, 4
    zgn = 64 if splits >= (wide_from or 128) else 16
    assert splits == 0 or zgn * hid * 4 <= 64 * 1024
    h = Harness(twins, n, 5, A, L, seed=7 * hid + splits)
    g = torch.Generator(device="cpu").manual_seed(hid + splits)
    rnd = lambda *s: torch.randn(*s, generator=g)                # noqa: E731
    w, b, bias = (rnd(A + 1, hid) * (2 / np.sqrt(hid))).to(DEV), (rnd(A + 1) * 0.5).to(DEV), (rnd(hid) * 0.5).to(DEV)
    convs = dict()
    for nf in (16, 32):
        geom = _lib.conv_geom(n, 104, 80, 4, nf, 8, 8, 4, 0, 0)
        assert _lib.serve_conv1_supported(h.games[1], geom)
        convs[nf] = dict(geom=geom, w=(rnd(nf, 4, 8, 8) * 0.05).to(DEV), bias=(rnd(nf) * 0.1).to(DEV),
                         y=torch.empty((n, 25, 19, nf), device=DEV))
    _lib.load().arl_dev_fold_wide_from(wide_from)
    try:
        k, n_neg, last_step_conv = 0, 0, 0
        for batch in range(3):
            h.begin_batch()
            for step in range(HORIZON):
                nf, use_bias, relu = COMBOS[k % len(COMBOS)]
                k += 1
                if splits > 0:                                   # partial sums of O(1) activations, half of them negative
                    part = (rnd(splits, n, hid) / np.sqrt(splits)).to(DEV)
                else:
                    part = rnd(n, hid).relu_().to(DEV)
                spec = dict(part=part, splits=splits, bias=bias if use_bias else None, relu=relu, w=w, b=b)
                what = "A %d hid %d splits %d conv %s bias %s relu %d step %d" % (A, hid, splits, nf, use_bias, relu, step)
                res, prob, value = h.launch(step, spec, lambda p: h.rs.rand(n), conv=convs.get(nf), what=what)
                want_p, want_v, act = _head_f64(spec)
                n_neg += int((act < 0).sum()) if splits > 0 else 0
                _close(torch.from_numpy(prob), want_p, hid, "prob " + what)
                _close(torch.from_numpy(value), want_v, hid, "value " + what)
                last_step_conv += int(step == HORIZON - 1 and nf is not None)
        assert last_step_conv >= 2 and (splits == 0 or n_neg > n * hid)       # the rectifier mattered
    finally:
        _lib.load().arl_dev_fold_wide_from(0)


def _head_f64(spec):
    """float64 fold + bias + rectifier + heads + softmax of float64 copies of the inputs (CPU); also the pre-rectifier
    activations."""
    part = spec["part"].double().cpu()
    act = part.sum(dim=0) if spec["splits"] > 0 else part
    hcur = act
    if spec["splits"] > 0:
        if spec["bias"] is not None:
            hcur = hcur + spec["bias"].double().cpu()
        act = hcur
        if spec["relu"]:
            hcur = hcur.clamp_min(0)
    out = hcur @ spec["w"].double().cpu().t() + spec["b"].double().cpu()
    return torch.softmax(out[:, :-1], dim=1), out[:, -1], act


def _edge_uniforms(prob, rs):
    """Per env one edge of the draw, from the fp32 sequential cumsum the kernels build: u = 0; u equal to a cumsum value
    (the compare is strict: that entry is not counted) and the next double above it; u = 1 and the double below 1, where
    the last cumsum can sit below u and the clamp to A - 1 applies."""
    n, A = prob.shape
    cs = np.cumsum(prob, axis=1, dtype=np.float32).astype(np.float64)
    picks = [0, A // 2, max(A - 2, 0), A - 1]
    edges = [lambda e: 0.0, lambda e: 1.0, lambda e: np.nextafter(1.0, 0.0)]
    for j in picks:
        edges += [lambda e, j=j: cs[e, j], lambda e, j=j: np.nextafter(cs[e, j], np.inf), lambda e, j=j: np.nextafter(cs[e, j], -np.inf)]
    u = np.array([edges[e % len(edges)](e) for e in range(n)])
    return u


@pytest.mark.parametrize("A", [18, 1])
def test_draw_and_softmax_edges(twins, A):
    """Softmax rows: ordinary, all-equal logits, one logit larger by 1e4 (probability exactly 1, the rest 0), logits near
    +-80; per env one edge of the draw (_edge_uniforms).  (a), (b), (c) of the head test on every launch, no NaN."""
    n, L, hid, splits = 17, 4, 68, 15
    h = Harness(twins, n, 5, A, L, seed=A)
    g = torch.Generator(device="cpu").manual_seed(A)
    rnd = lambda *s: torch.randn(*s, generator=g)                # noqa: E731
    small_w = rnd(A + 1, hid) * (0.5 / np.sqrt(hid))
    flat_w = small_w.clone()
    flat_w[:A] = 0
    big = torch.zeros(A + 1)
    big[A // 3] = 1e4
    pm80 = torch.tensor([80.0 if j % 2 == 0 else -80.0 for j in range(A)] + [0.5])
    kinds = [("ordinary", small_w * 4, rnd(A + 1) * 0.5), ("all_equal", flat_w, torch.full((A + 1,), 0.25)),
             ("one_hot_1e4", small_w, big), ("pm80", small_w, pm80)]
    bias = (rnd(hid) * 0.5).to(DEV)
    seen = set()
    for batch in range(3):
        h.begin_batch()
        for step in range(HORIZON):
            name, w, b = kinds[(batch * HORIZON + step) % len(kinds)]
            part = (rnd(splits, n, hid) / np.sqrt(splits)).to(DEV)
            spec = dict(part=part, splits=splits, bias=bias, relu=1, w=w.to(DEV), b=b.to(DEV))
            shift = batch * HORIZON + step                       # every env meets every edge over the launches
            u_fn = lambda p: np.roll(_edge_uniforms(p, h.rs), shift)          # noqa: E731
            res, prob, value = h.launch(step, spec, u_fn, what="%s A %d batch %d step %d" % (name, A, batch, step))
            want_p, want_v, _ = _head_f64(spec)
            _close(torch.from_numpy(prob), want_p, hid, "prob " + name)
            _close(torch.from_numpy(value), want_v, hid, "value " + name)
            if name == "all_equal":
                assert (prob == prob[0, 0]).all()
            if name == "one_hot_1e4":
                assert (prob[:, A // 3] == 1).all() and prob.sum() == n
            rows = np.arange(n) * HORIZON + step
            seen |= set(h.twins[1].samples_buf.actions.cpu().numpy()[rows].tolist())
    assert seen == set(range(A)) if A == 1 else {0, A - 1} <= seen


# ---- refusals: argument errors that launch nothing

def _served_args(twins, n=17, A=6, hid=64):
    from accel_rl_amd import _lib
    h = Harness(twins, n, 5, A, 4, seed=1)
    h.begin_batch()
    scratch = torch.zeros(128 * n * 1028 + 16, dtype=torch.float32, device=DEV)     # room for every shape named below
    w, b = torch.zeros(A + 1, 1028, device=DEV), torch.zeros(A + 1, device=DEV)
    u = torch.rand(n, dtype=torch.float64, device=DEV)

    def head(hid=hid, splits=4, total=None, offset=0):
        hd = _lib.ArlServeHead()
        hd.hidden.part, hd.hidden.splits = scratch.data_ptr() + offset, splits
        hd.hidden.total = n * hid if total is None else total
        hd.hidden_bias, hd.hidden_relu, hd.hid = None, 1, hid
        hd.w_head, hd.b_head = w.data_ptr(), b.data_ptr()
        return hd
    return _lib, h, head, u, (scratch, w, b)


def test_served_step_refusals_launch_nothing(twins):
    _lib, h, head, u, keep = _served_args(twins)
    smp, g, st, ro = twins[1], h.games[1], h.states[1], twins[1]._rollout
    before = _snapshot(smp)

    def refused(match, game=g, state=st, hd=None, uniforms=u, step=0, max_len=4.0):
        with pytest.raises(RuntimeError, match=match):
            _lib.env_step_served(game, state, ro, head() if hd is None else hd, None, uniforms, step, max_len, 0.99, 30)

    for hid in (0, 6, 1028):
        refused("multiple of 4", hd=head(hid=hid))
    refused("too wide", hd=head(hid=260, splits=128))            # one step past the fold's 64 KiB, either way
    refused("too wide", hd=head(hid=1024, splits=128))
    refused("n_env rows", hd=head(splits=-1))
    refused("n_env rows", hd=head(total=(h.n - 1) * 64))
    refused("n_env rows", hd=head(total=(h.n + 1) * 64))
    refused("alignment", hd=head(offset=4))
    g5 = _lib.ArlGame.from_buffer_copy(g)
    g5.n_stack = 5
    refused("deeper than 4", game=g5)
    refused("max_path_length >= 1", max_len=0.5)
    refused("horizon", step=HORIZON)
    refused("horizon", step=-1)
    s2 = _lib.ArlEnvState.from_buffer_copy(st)
    s2.next_reset = None
    refused("next_reset", state=s2)
    rc = _lib.load().arl_env_step_served(C.byref(g), C.byref(st), C.byref(ro), C.byref(head()), None, None, 0, 4.0, 0.99, 30,
                                         _lib.stream_ptr())
    assert rc != 0 and b"null pointer" in _lib.load().arl_last_error()
    _assert_same(_snapshot(smp), before)


def test_env_step_refusals_launch_nothing(twins):
    _lib, h, _, u, keep = _served_args(twins)
    smp, g, st, ro = twins[0], h.games[0], h.states[0], twins[0]._rollout
    n, A = h.n, h.A
    prob = torch.full((n, A), 1. / A, device=DEV)
    value = torch.zeros(n, device=DEV)
    active = torch.ones(n, dtype=torch.uint8, device=DEV)
    before = _snapshot(smp)

    def refused(match, game=g, state=st, mbr=True, active=None, single_write=True):
        with pytest.raises(RuntimeError, match=match):
            _lib.env_step(game, state, ro, prob, value, u, 0, mbr, 4.0, 0.99, 30, active=active, single_write=single_write)

    refused("single_write needs", mbr=False)
    refused("single_write needs", active=active)
    for bad in (0, 19):
        gb = _lib.ArlGame.from_buffer_copy(g)
        gb.n_actions = bad
        refused("bad game description", game=gb)
    s0 = _lib.ArlEnvState.from_buffer_copy(st)
    s0.envs_per_stream = 0
    refused("bad state description", state=s0)
    _assert_same(_snapshot(smp), before)
