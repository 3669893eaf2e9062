"""IMPALA's learner (Espeholt et al. 2018, "IMPALA: Scalable Distributed Deep-RL with Importance Weighted Actor-Learner
Architectures"; the reference has none): an advantage actor-critic whose value targets and policy-gradient advantages
are V-trace's -- recomputed from the CURRENT network on the rollout, under truncated importance weights against the
behaviour policy the sampler recorded (csrc/vtrace_scan.hip:arl_vtrace_scan).  That makes walking a rollout more than
once principled: from the second epoch on the data are off-policy, and every epoch trains on targets computed from the
parameters as they stand at its start.  (PPO keeps the targets of before the first update and bounds the damage with its
clip.)  Single GPU, feed-forward policies; no replay of old rollouts.

The loop -- host / device split, warm-up, hipGraph capture, diagnostics ring -- is AdvActorCriticBase's, the minibatches
PpoOptimizer's (VtraceOptimizer adds the call at the start of each epoch).  The loss is the fused head kernel's kind 0
(A2C): -mean(log pi(a) adv) + c_v mean((V - vs)^2) - c_e entropy, the importance weight being folded into `adv` by the
scan.  process_samples does nothing; the epoch hook does the retargeting: AtariCnnPolicy.prob_value_rows on the
rollout's observations and on the extra ones, then one arl_vtrace_scan into the tensors the minibatches gather from.

Defaults: V-trace's as recalled from the paper -- discount 0.99, lambda 1, rho_bar = c_bar = 1 (and the
same bar on the policy gradient's weight), value-loss coefficient 0.5, entropy coefficient 0.01, global-norm clip 40 --
and RMSprop as A2C configures it here (learning rate 7e-4), one epoch of one whole-batch update."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.algos.pg.aac_base import AdvActorCriticBase, valids_mean
from accel_rl_amd.optimizers import update_methods
from accel_rl_amd.optimizers.single import VtraceOptimizer


def _finite(x):
    return isinstance(x, (int, float, np.floating, np.integer)) and bool(np.isfinite(x))


class IMPALA(AdvActorCriticBase):
    """Single GPU"""

    def __init__(self, discount=0.99, vtrace_lambda=1.0, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, v_loss_coeff=0.5,
                 ent_loss_coeff=0.01, OptimizerCls=VtraceOptimizer, optimizer_args=None, lr_schedule=None,
                 rows_per_pass=1024, use_graph=True):
        if not (_finite(discount) and 0 <= discount <= 1 and _finite(vtrace_lambda) and 0 <= vtrace_lambda <= 1):
            raise ValueError("discount and vtrace_lambda must lie in [0, 1] (arl_vtrace_scan)")
        for name, bar in (("rho_bar", rho_bar), ("c_bar", c_bar), ("pg_rho_bar", pg_rho_bar)):
            if not (_finite(bar) and bar > 0):
                raise ValueError("%s must be finite and > 0 (arl_vtrace_scan), got %r" % (name, bar))
        if not (_finite(v_loss_coeff) and _finite(ent_loss_coeff)):
            raise ValueError("v_loss_coeff and ent_loss_coeff must be finite")
        if rows_per_pass is not None and not (isinstance(rows_per_pass, (int, np.integer)) and rows_per_pass >= 1):
            raise ValueError("rows_per_pass must be None (one pass) or an integer >= 1")
        args = dict(learning_rate=7e-4, update_method=update_methods.rmsprop, update_method_args=dict(),
                    epochs=1, minibatch_size=None, grad_norm_clip=40, shuffle=True)
        args.update(optimizer_args or dict())
        if not (isinstance(args["epochs"], (int, np.integer)) and args["epochs"] >= 1):
            raise ValueError("optimizer_args: epochs must be an integer >= 1")
        self.optimizer = OptimizerCls(**args)
        self.vtrace_lambda, self.rho_bar, self.c_bar, self.pg_rho_bar = vtrace_lambda, rho_bar, c_bar, pg_rho_bar
        self.rows_per_pass = rows_per_pass
        super().__init__(discount=discount, gae_lambda=vtrace_lambda, v_loss_coeff=v_loss_coeff,
                         ent_loss_coeff=ent_loss_coeff, lr_schedule=lr_schedule, use_graph=use_graph)

    loss_kind = 0

    def pi_loss(self, policy, act, adv, old_dist_info, new_dist_info, valids):
        """A2C's expression; `adv` is the scan's (importance weight included, no gradient through it)."""
        logli = policy.distribution.log_likelihood_sym(act, new_dist_info)
        return - valids_mean(logli * adv, valids)

    def initialize(self, policy, env_spec, sample_size, horizon, mid_batch_reset):
        if policy.recurrent:
            raise NotImplementedError("IMPALA: recurrent policies are not built -- the retargeting forward walks rows, not "
                                      "trajectories (INTEGRATION.md, section E)")
        if not mid_batch_reset:
            raise NotImplementedError("IMPALA: mid_batch_reset=False is not built -- the scan cuts at `done` and there are "
                                      "no `valids` (INTEGRATION.md, section E)")
        if self.optimizer.parallelism_tag != "single":
            raise NotImplementedError("IMPALA: single GPU only, got a %r optimizer (%s) (INTEGRATION.md, section E)" %
                                      (self.optimizer.parallelism_tag, type(self.optimizer).__name__))
        if not hasattr(type(self.optimizer), "_epoch_hook"):
            raise TypeError("IMPALA needs an optimizer that calls _epoch_hook(epoch) at the start of every epoch "
                            "(VtraceOptimizer); got %s" % type(self.optimizer).__name__)
        if not hasattr(policy, "prob_value_rows"):
            raise TypeError("the policy must provide prob_value_rows (the no-grad forward over the rollout); got %s" %
                            type(policy).__name__)
        super().initialize(policy, env_spec, sample_size, horizon, mid_batch_reset)
        self.optimizer._epoch_hook = self._retarget
        self._samples = None
        # (sum of the ratios, steps above rho_bar) per env, of the last scan; allocated here, so the captured graph
        # keeps writing the same block
        self._vt_stats = torch.zeros((self._n_env, 2), dtype=torch.float32, device=policy.device)

    # ---- device work (captured) ----
    def _device_optimize(self, itr, samples_data):
        self._samples = samples_data
        opt_data, infos = super()._device_optimize(itr, samples_data)
        mean = self._vt_stats.sum(dim=0) * (1. / self._batch_size)           # of the LAST epoch's scan
        return opt_data, dict(GradNorm=infos["GradNorm"], RhoMean=mean[0:1], RhoClipFrac=mean[1:2])

    def process_samples(self, itr, samples_data):
        """Nothing to do before the first epoch that the epochs do not do themselves (_retarget)."""
        return self._opt_buf

    def _retarget(self, epoch):
        """Start of an epoch: V-trace targets and advantages of the whole batch from the parameters as they stand -- one
        no-grad forward over the n_env * horizon observations and the n_env extra ones (in passes of rows_per_pass rows),
        then one arl_vtrace_scan into opt["returns"] / opt["advantages"], which the minibatches gather from by idx."""
        s, opt = self._samples, self._opt_buf
        prob, value = self.policy.prob_value_rows(s["observations"], self.rows_per_pass, tag="vt_rows")
        _, last_value = self.policy.prob_value_rows(s["extra_observations"], self.rows_per_pass, tag="vt_last")
        value, last_value = self._scan_values(value, last_value)
        _lib.vtrace_scan(prob, s["agent_infos"]["prob"], s["actions"], value, last_value, s["rewards"], s["dones"],
                         self.discount, self.vtrace_lambda, self.rho_bar, self.c_bar, self.pg_rho_bar, self._n_env,
                         self._horizon, opt["returns"], opt["advantages"], stats=self._vt_stats)

    @property
    def opt_info_keys(self):
        return ["GradNorm", "RhoMean", "RhoClipFrac"]
