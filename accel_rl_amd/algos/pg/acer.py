"""ACER (Wang et al. 2017, "Sample Efficient Actor-Critic with Experience Replay"; the reference has none; PAPERS.md
restates it with what is recalled and what is chosen): an actor-critic with a Q head that learns a stochastic policy from
whole trajectories, on-policy AND from a memory of old rollouts.  Single GPU, feed-forward AtariAcerPolicy, discrete
actions.

One update, on-policy or replayed, is the same device work:
  AtariAcerPolicy.pi_q_rows on the batch's observations and on the extra ones (the CURRENT network, in passes of
  rows_per_pass rows) -> arl_acer_retrace_scan: Retrace(lambda) targets of Q against the recorded behaviour policy ->
  acer_loss_and_grads: live forward, average-network forward, ONE arl_acer_loss (truncated importance weight with bias
  correction, entropy bonus, trust-region projection against the average network, Q regression), backward ->
  the optimizer's step (global-norm clip, RMSprop) -> arl_acer_avg_step (AcerOptimizer).

The on-policy update is AdvActorCriticBase's loop: host / device split, two eager calls, then one captured hipGraph,
diagnostics ring.  After it the rollout -- observations, extra observations, actions, rewards, dones, behaviour prob --
goes into slot (call number % slots) of a device-resident memory by stream-ordered arl_copy_bytes outside the graph (PPG's
discipline).  Then r ~ Poisson(replay_ratio) replay updates run, r capped at r_max and zero until replay_start rollouts are
stored; r and every index are drawn with np.random BEFORE anything is enqueued.  A replay update stages n_env trajectories,
drawn independently and uniformly as (slot, env) pairs, with one arl_gather_segments per stored field, and runs the update
above on them with the SAME optimizer state (the paper's shared RMSprop).  All index rows of an iteration go up in one
pinned-to-device copy; before replay update k a stream-ordered 4 n_env-byte arl_copy_bytes puts row k where the staging
launches read it (outside the graph, as the memory stores are: no device-side counter is needed, and nothing synchronises
between replay updates).  The replay update is its own captured graph: two eager, the third captured.

Defaults as recalled from the paper and the public implementation: discount 0.99, lambda 1, c 10, delta 1,
alpha 0.99, q_coeff 0.5, ent_coeff 0.01, RMSprop as A2C configures it here at 7e-4, global-norm clip 10, replay_ratio 4,
a memory of 50 000 steps, replay from 10 000 stored steps on -- both converted to rollouts at initialize; chosen here:
r_max 16, one epoch of one whole-batch update, unshuffled."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.algos.pg.aac_base import AdvActorCriticBase
from accel_rl_amd.optimizers import update_methods
from accel_rl_amd.optimizers.single import AcerOptimizer
from accel_rl_amd.util.misc import capture_graph

STORED_FIELDS = ("observations", "extra_observations", "actions", "rewards", "dones", "prob")


def _finite(x):
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool) and bool(np.isfinite(x))


def _count(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool) and x >= 1


def rollouts_of(steps, sample_size):
    """Rollouts that hold at least `steps` steps (at least one)."""
    return max(1, -(-int(steps) // int(sample_size)))


def replay_count(replay_ratio, stored, replay_start, r_max):
    """Replay updates of one iteration: 0 while fewer than replay_start rollouts are stored (nothing is drawn) or
    replay_ratio is 0, else min(np.random.poisson(replay_ratio), r_max)."""
    if stored < replay_start or replay_ratio <= 0:
        return 0
    return int(min(np.random.poisson(replay_ratio), r_max))


def draw_trajectories(r, n_env, stored):
    """i32 [r][n_env]: per replay update n_env segment numbers slot * n_env + env, independent and uniform over the
    `stored` filled slots."""
    return np.random.randint(0, stored * n_env, size=(r, n_env)).astype(np.int32)


class ACER(AdvActorCriticBase):
    """Single GPU, AtariAcerPolicy"""

    def __init__(self, discount=0.99, retrace_lambda=1.0, c=10.0, delta=1.0, alpha=0.99, q_coeff=0.5, ent_coeff=0.01,
                 replay_ratio=4, replay_steps=50000, replay_start_steps=10000, r_max=16, OptimizerCls=AcerOptimizer,
                 optimizer_args=None, lr_schedule=None, rows_per_pass=1024, use_graph=True):
        if not (_finite(discount) and 0 <= discount <= 1 and _finite(retrace_lambda) and 0 <= retrace_lambda <= 1):
            raise ValueError("discount and retrace_lambda must lie in [0, 1] (arl_acer_retrace_scan)")
        if not (isinstance(c, (int, float)) and c > 0 and isinstance(delta, (int, float)) and delta >= 0):
            raise ValueError("c must be > 0 and delta >= 0 (+inf switches the term off; arl_acer_loss)")
        if not (_finite(alpha) and 0 <= alpha <= 1):
            raise ValueError("alpha must lie in [0, 1] (arl_acer_avg_step)")
        if not (_finite(q_coeff) and _finite(ent_coeff)):
            raise ValueError("q_coeff and ent_coeff must be finite")
        if not (_finite(replay_ratio) and replay_ratio >= 0):
            raise ValueError("replay_ratio must be finite and >= 0")
        for name, n in (("replay_steps", replay_steps), ("replay_start_steps", replay_start_steps), ("r_max", r_max)):
            if not _count(n):
                raise ValueError("%s must be an integer >= 1, got %r" % (name, n))
        if rows_per_pass is not None and not _count(rows_per_pass):
            raise ValueError("rows_per_pass must be None (one pass) or an integer >= 1")
        args = dict(learning_rate=7e-4, update_method=update_methods.rmsprop, update_method_args=dict(), epochs=1,
                    minibatch_size=None, grad_norm_clip=10, shuffle=False)
        args.update(optimizer_args or dict())
        if args["grad_norm_clip"] is None:
            raise ValueError("ACER: optimizer_args' grad_norm_clip must be a number -- the replay updates step the shared "
                             "optimizer state one update at a time, which the clip-free update (its step count and norm "
                             "log are closed once per call) does not offer (INTEGRATION.md, section E)")
        self.optimizer = OptimizerCls(avg_alpha=alpha, **args) if issubclass(OptimizerCls, AcerOptimizer) \
            else OptimizerCls(**args)
        self.retrace_lambda, self.c, self.delta, self.alpha = float(retrace_lambda), float(c), float(delta), float(alpha)
        self.q_coeff = float(q_coeff)
        self.replay_ratio, self.replay_steps, self.replay_start_steps = float(replay_ratio), replay_steps, replay_start_steps
        self.r_max, self.rows_per_pass = int(r_max), rows_per_pass
        super().__init__(discount=discount, gae_lambda=retrace_lambda, v_loss_coeff=q_coeff, ent_loss_coeff=ent_coeff,
                         lr_schedule=lr_schedule, use_graph=use_graph)

    def initialize(self, policy, env_spec, sample_size, horizon, mid_batch_reset):
        from accel_rl_amd.policies.dqn.atari_acer_policy import AtariAcerPolicy
        if not isinstance(policy, AtariAcerPolicy):
            raise NotImplementedError("ACER trains an AtariAcerPolicy (one output row of logits and action values); got "
                                      "%s (INTEGRATION.md, section E)" % type(policy).__name__)
        if policy.recurrent:
            raise NotImplementedError("ACER: recurrent policies are not built (INTEGRATION.md, section E)")
        if not mid_batch_reset:
            raise NotImplementedError("ACER: mid_batch_reset=False is not built -- the scan cuts at `done` and there are "
                                      "no `valids` (INTEGRATION.md, section E)")
        opt = self.optimizer
        if opt.parallelism_tag != "single":
            raise NotImplementedError("ACER: single GPU only, got a %r optimizer (%s) (INTEGRATION.md, section E)" %
                                      (opt.parallelism_tag, type(opt).__name__))
        if not isinstance(opt, AcerOptimizer):
            raise TypeError("ACER needs an optimizer that steps the average network and offers whole_batch_update "
                            "(AcerOptimizer); got %s" % type(opt).__name__)
        super().initialize(policy, env_spec, sample_size, horizon, mid_batch_reset)
        dev, n_env = policy.device, self._n_env
        policy.update_target()                               # the average network starts as the network
        self.replay_rollouts = rollouts_of(self.replay_steps, sample_size)
        self.replay_start = min(rollouts_of(self.replay_start_steps, sample_size), self.replay_rollouts)
        obs_shape = tuple(env_spec.observation_space.shape)
        segs = self.replay_rollouts * n_env

        def field_tensors(n):               # one trajectory (segment) per leading index
            return dict(observations=torch.zeros((n, horizon) + obs_shape, dtype=torch.uint8, device=dev),
                        extra_observations=torch.zeros((n,) + obs_shape, dtype=torch.uint8, device=dev),
                        actions=torch.zeros((n, horizon), dtype=torch.uint8, device=dev),
                        rewards=torch.zeros((n, horizon), dtype=torch.float32, device=dev),
                        dones=torch.zeros((n, horizon), dtype=torch.uint8, device=dev),
                        prob=torch.zeros((n, horizon, policy.n_act), dtype=torch.float32, device=dev))
        self._mem = field_tensors(segs) if self.replay_ratio > 0 else None
        self._staged = field_tensors(n_env) if self.replay_ratio > 0 else None
        self._idx_host = torch.zeros((self.r_max, n_env), dtype=torch.int32).pin_memory()
        self._idx_table = torch.zeros((self.r_max, n_env), dtype=torch.int32, device=dev)
        self._idx_now = torch.zeros(n_env, dtype=torch.int32, device=dev)
        self._rp_qret = torch.zeros(sample_size, dtype=torch.float32, device=dev)
        self._dummy = torch.zeros(sample_size, dtype=torch.float32, device=dev)
        # (sum of rho, steps with rho > 1) per env of the last scan, on-policy / replayed; allocated here, so the captured
        # graphs keep writing the same blocks
        self._scan_stats = torch.zeros((n_env, 2), dtype=torch.float32, device=dev)
        self._rp_scan_stats = torch.zeros((n_env, 2), dtype=torch.float32, device=dev)
        self._r_host = torch.zeros(1, dtype=torch.float32).pin_memory()
        self._r_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self._last_stats = None
        self._calls = 0
        self._replays = 0
        self._replay_graph = None

    # ---- host side ----
    def optimize_policy(self, itr, samples_data):
        if self._done_event is not None:            # (the pinned index table may still be read by the previous call)
            self._done_event.synchronize()
        n_env = self._n_env
        stored = min(self._calls + 1, self.replay_rollouts)              # this call's rollout included
        r = replay_count(self.replay_ratio, stored, self.replay_start, self.r_max) if self._mem is not None else 0
        if r:
            self._idx_host[:r].copy_(torch.from_numpy(draw_trajectories(r, n_env, stored)))
        self._r_host.fill_(float(r))
        out = super().optimize_policy(itr, samples_data)
        if self._mem is not None:
            slot = self._calls % self.replay_rollouts
            for name, src in self._fields_of(samples_data).items():
                _lib.copy_bytes(self._mem[name][slot * n_env:(slot + 1) * n_env], src)
        self._calls += 1
        if r:
            _lib.copy_bytes(self._idx_table, self._idx_host)
            for k in range(r):
                _lib.copy_bytes(self._idx_now, self._idx_table[k])
                self._enqueue_replay()
        self._done_event.record(torch.cuda.current_stream(self.policy.device))
        return out

    @staticmethod
    def _fields_of(samples_data):
        s = samples_data
        return dict(observations=s["observations"], extra_observations=s["extra_observations"], actions=s["actions"],
                    rewards=s["rewards"], dones=s["dones"], prob=s["agent_infos"]["prob"])

    # ---- device work (captured) ----
    def _retrace(self, fields, qret, stats, tag):
        """Retrace targets of one batch from the parameters as they stand, into qret."""
        pol, half = self.policy, self.policy.half_stride
        obs = fields["observations"].reshape((-1,) + tuple(fields["observations"].shape[-3:]))
        prob, out = pol.pi_q_rows(obs, self.rows_per_pass, tag=tag + "_rows")
        prob_last, out_last = pol.pi_q_rows(fields["extra_observations"], self.rows_per_pass, tag=tag + "_last")
        _lib.acer_retrace_scan(prob, prob_last, out[:, half:], out_last[:, half:], fields["prob"].reshape(prob.shape),
                               fields["actions"].reshape(-1), fields["rewards"].reshape(-1), fields["dones"].reshape(-1),
                               self.discount, self.retrace_lambda, self._n_env, self._horizon, qret, stats=stats)

    def process_samples(self, itr, samples_data):
        """Retrace targets of the rollout into opt["returns"], once per call (IMPALA's _retarget, done once)."""
        self._retrace(self._fields_of(samples_data), self._opt_buf["returns"], self._scan_stats, "acer_on")
        return self._opt_buf

    def _losses(self, mb):
        stats = self.policy.acer_loss_and_grads(mb, self.c, self.delta, self.q_coeff, self.ent_loss_coeff)
        self._last_stats = stats
        pi_loss, q_loss = stats[0].sum(), stats[1].sum()
        return torch.stack([pi_loss, q_loss, stats[2].mean(), pi_loss + q_loss])

    def _device_optimize(self, itr, samples_data):
        _lib.copy_bytes(self._r_dev, self._r_host)
        opt_data, infos = super()._device_optimize(itr, samples_data)
        stats = self._last_stats
        return opt_data, dict(GradNorm=infos["GradNorm"], QLoss=stats[1].sum().reshape(1),
                              Entropy=stats[2].mean().reshape(1), RhoMean=stats[4].mean().reshape(1),
                              TrustScaleMean=stats[3].mean().reshape(1), ReplayUpdates=self._r_dev.clone())

    # ---- replay updates ----
    def _enqueue_replay(self):
        self._replays += 1
        if not self.use_graph or self._replays <= 2:
            self._device_replay()
        else:
            if self._replay_graph is None:
                torch.cuda.synchronize(self.policy.device)
                graph = torch.cuda.CUDAGraph()
                with capture_graph(graph):
                    self._device_replay()
                self._replay_graph = graph
            self._replay_graph.replay()
        self._params_written()

    def _device_replay(self):
        """One replay update: stage the n_env trajectories _idx_now names, Retrace from the parameters as they stand, one
        whole-batch update on the shared optimizer state."""
        for name in STORED_FIELDS:
            _lib.gather_segments(self._mem[name], self._idx_now, self._staged[name])
        st = self._staged
        self._retrace(st, self._rp_qret, self._rp_scan_stats, "acer_rp")
        rows = self._batch_size
        obs = st["observations"].reshape((rows,) + tuple(st["observations"].shape[2:]))
        by_name = dict(observations=obs, actions=st["actions"].reshape(-1), advantages=self._dummy,
                       returns=self._rp_qret, old_value=self._dummy, old_prob=st["prob"].reshape(rows, -1))
        self.optimizer.whole_batch_update(tuple(by_name[n] for n in self.optimizer._input_names))

    def pi_loss(self, policy, act, adv, old_dist_info, new_dist_info, valids):
        raise NotImplementedError("ACER's policy gradient is stated on the probabilities (include/accel_rl_hip.h, "
                                  "arl_acer_loss); tests/acer_ref.py restates it")

    @property
    def opt_info_keys(self):
        return ["GradNorm", "QLoss", "Entropy", "RhoMean", "TrustScaleMean", "ReplayUpdates"]
