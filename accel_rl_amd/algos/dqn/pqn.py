"""PQN, the "parallelised Q-network" (Gallici et al. 2024, "Simplifying Deep Temporal Difference Learning"; the
reference has none): Q-learning on the on-policy half of this tree.  No replay memory and no target network: epsilon-
greedy actions in many environments at once (GpuVecSampler serving an AtariPqnPolicy), Q(lambda) returns computed ONCE
per batch, backwards over the rollout from the current network (csrc/qlambda_scan.hip:arl_qlambda_scan), then a few epochs of
large index-gathered minibatches regressing Q(obs)[action] on those returns (csrc/dqn.hip:arl_q_regress_loss), as PPO
walks its batch.  What keeps this stable is the LayerNorm after every layer of the network (AtariPqnPolicy).

The loop -- host / device split, warm-up, hipGraph capture, diagnostics ring -- is AdvActorCriticBase's, the minibatches
PpoOptimizer's; this class gives process_samples (forward over the rollout + the scan), _losses and the epsilon
schedule (DQN's linear one: update_epsilon, prep_eval / post_eval; the sampler's host_draws table reads the policy's
epsilon per rollout).  prep_opt_inputs is the parent's: `advantages`, `old_value` and `old_prob` ride along unread.

Defaults are the paper's Atari settings as recalled: discount 0.99, lambda 0.65, 2 epochs of 32 minibatches
(minibatch_size = sample_size // 32), learning rate 2.5e-4 annealed linearly to 0, global-norm clip 10, squared loss,
epsilon 1 -> 0.001 over the first 10 % of the run, greedy evaluation.  The paper's RAdam is not among update_methods:
adam (epsilon 1e-5) stands in."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.algos.dqn.dqn import DQN
from accel_rl_amd.algos.pg.aac_base import AdvActorCriticBase
from accel_rl_amd.optimizers import update_methods
from accel_rl_amd.optimizers.single import PpoOptimizer
from accel_rl_amd.policies.dqn.atari_pqn_policy import AtariPqnPolicy

MINIBATCHES_PER_EPOCH = 32


class PQN(AdvActorCriticBase):

    def __init__(self, discount=0.99, q_lambda=0.65, delta_clip=None, OptimizerCls=PpoOptimizer, optimizer_args=None,
                 eps_greedy_args=None, lr_schedule="linear", rows_per_pass=1024, use_graph=True):
        if not (np.isfinite(discount) and 0 <= discount <= 1 and np.isfinite(q_lambda) and 0 <= q_lambda <= 1):
            raise ValueError("discount and q_lambda must lie in [0, 1] (arl_qlambda_scan)")
        if delta_clip is not None and not (np.isfinite(delta_clip) and delta_clip > 0):
            raise ValueError("delta_clip must be None (squared loss) or finite and > 0")
        opt_args, eps_args = self._get_default_sub_args()
        opt_args.update(optimizer_args or dict())
        self.optimizer = OptimizerCls(**opt_args)
        unknown = set(eps_greedy_args or ()) - set(eps_args)
        if unknown:
            raise TypeError("unexpected eps_greedy_args: %s" % sorted(unknown))
        eps_args.update(eps_greedy_args or dict())
        self._eps_initial, self._eps_final = eps_args["initial"], eps_args["final"]
        self._eps_eval, self._eps_anneal_steps = eps_args["eval"], eps_args["anneal_steps"]
        self._eps_anneal_fraction = eps_args["anneal_fraction"]
        self.q_lambda, self.delta_clip, self.rows_per_pass = q_lambda, delta_clip, rows_per_pass
        super().__init__(discount=discount, gae_lambda=q_lambda, lr_schedule=lr_schedule, use_graph=use_graph)

    @staticmethod
    def _get_default_sub_args():
        # minibatch_size None: sample_size // MINIBATCHES_PER_EPOCH, known at initialize
        # anneal_steps None: anneal_fraction of the run, known at set_n_itr
        opt_args = dict(learning_rate=2.5e-4, update_method=update_methods.adam, update_method_args=dict(epsilon=1e-5),
                        epochs=2, minibatch_size=None, grad_norm_clip=10, shuffle=True)
        eps_greedy_args = dict(initial=1., final=0.001, eval=0., anneal_steps=None, anneal_fraction=0.1)
        return opt_args, eps_greedy_args

    def initialize(self, policy, env_spec, sample_size, horizon, mid_batch_reset):
        if type(policy) is not AtariPqnPolicy:
            raise TypeError("PQN trains an AtariPqnPolicy itself, not another policy (got %s)" % type(policy).__name__)
        if not mid_batch_reset:
            raise NotImplementedError("PQN: mid_batch_reset=False is not built -- the return cuts at `done` and there are "
                                      "no `valids` (INTEGRATION.md, section E)")
        if self.optimizer._minibatch_size is None:
            self.optimizer._minibatch_size = max(1, sample_size // MINIBATCHES_PER_EPOCH)
        super().initialize(policy, env_spec, sample_size, horizon, mid_batch_reset)
        self._sample_size = sample_size
        self._eps_anneal_itr = max(1, (self._eps_anneal_steps or 0) // sample_size)
        self._mb_stats = None
        policy.set_epsilon(self._eps_initial)

    def set_n_itr(self, n_itr):
        super().set_n_itr(n_itr)
        if self._eps_anneal_steps is None:
            self._eps_anneal_itr = max(1, int(self._eps_anneal_fraction * n_itr))

    # ---- epsilon: DQN's linear schedule and evaluation switch, on this algorithm's fields ----
    def update_epsilon(self, itr):
        DQN.update_epsilon(self, itr)

    def prep_eval(self, itr):
        DQN.prep_eval(self, itr)

    def post_eval(self, itr):
        DQN.post_eval(self, itr)

    def optimize_policy(self, itr, samples_data):
        out = super().optimize_policy(itr, samples_data)
        self.update_epsilon(itr)            # (the next rollout's host_draws reads it)
        return out

    # ---- device work (captured) ----
    def _device_optimize(self, itr, samples_data):
        n_mb, b = self.optimizer._n_minibatches, self.optimizer._minibatch_size
        if self._mb_stats is None or tuple(self._mb_stats.shape) != (n_mb, 2, b):
            # (loss_rows, td_abs) of every minibatch of a call, written by the loss kernel itself; allocated in the
            # eager warm-up calls, so the captured graph keeps writing the same block
            self._mb_stats = torch.zeros((n_mb, 2, b), dtype=torch.float32, device=self.policy.device)
        self._mb_next = 0
        opt_data, infos = super()._device_optimize(itr, samples_data)
        sums = self._mb_stats.sum(dim=2).t().contiguous()           # [2, n_mb]
        return opt_data, dict(Loss=sums[0], TdAbs=sums[1] * (1. / b), GradNorm=infos["GradNorm"])

    def process_samples(self, itr, samples_data):
        """Q(lambda) returns of the whole batch from the current network: one no-grad forward over the n_env * horizon
        observations and the n_env extra ones (in passes of rows_per_pass rows), then one arl_qlambda_scan."""
        n, t = self._n_env, self._horizon
        opt = self._opt_buf
        q = self.policy.q_rows(samples_data["observations"], self.rows_per_pass, tag="rows")
        q_last = self.policy.q_rows(samples_data["extra_observations"], self.rows_per_pass, tag="last")
        _lib.qlambda_scan(q, q_last, samples_data["rewards"], samples_data["dones"], self.discount, self.q_lambda, n, t,
                          self.policy.n_act, opt["returns"])
        return opt

    def _losses(self, mb):
        """One minibatch: the regression loss on the precomputed returns and its gradient into flat_grads.  Returns a
        4-tuple as the parent's (the optimizer reads [3]): here the per-row losses, whose sum is the loss."""
        out = self._mb_stats[self._mb_next]
        self._mb_next += 1
        loss_rows, td_abs = self.policy.pqn_loss_and_grads(mb["observations"], mb["idx"], mb["actions"], mb["returns"],
                                                           self.delta_clip, out=out)
        return None, None, None, loss_rows

    @property
    def opt_info_keys(self):
        return ["Loss", "TdAbs", "GradNorm"]
