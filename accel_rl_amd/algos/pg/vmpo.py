"""V-MPO (Song et al. 2019, "V-MPO: On-Policy Maximum a Posteriori Policy Optimization for Discrete and Continuous
Control"; the reference has none; PAPERS.md restates it from memory, with what is recalled and what is chosen): an
on-policy actor-critic without a ratio and without a clip.  Per minibatch the policy is regressed onto the better half of
the rows with weights psi = softmax(A / eta) over that half; a trust region KL(pi_old || pi) <= eps_alpha is held by a
learned multiplier alpha; the temperature eta is learned from the dual loss eta eps_eta + eta log mean exp(A / eta).

Single GPU, feed-forward, synchronous.  pi_old and V_old are the behaviour policy's prob / value as the sampler recorded
them: the network at the start of optimize_policy plays the part of the paper's target network for the epochs x
minibatches updates of one call.  The loop -- host / device split, warm-up, hipGraph capture, diagnostics ring -- is
AdvActorCriticBase's, the minibatches PpoOptimizer's; VmpoOptimizer adds the duals and their step.  Per minibatch:
arl_vmpo_weights on the advantages (A = R - V_rollout, n-step returns by default, no standardisation) of the minibatch's
rows -> psi and the temperature's gradient; the policy's loss kind 4 (arl_vmpo_head_loss_parts: -sum psi log pi(a) +
c_v mean (V - R)^2 + alpha mean KL, and the backward pass); the network's optimiser step; arl_vmpo_dual_step on (eta,
alpha) with the projection x = max(x, 1e-8).  No entropy bonus, no valids.

Defaults as recalled from the paper's Atari table (they want checking against the paper): eta_init 1,
alpha_init 5, eps_eta 0.01, eps_alpha 0.005, Adam 1e-4, discount 0.99, value-loss coefficient 0.5; chosen here: 4 epochs
of 2 minibatches (half the batch each; optimizer_args' minibatch_size None = the whole batch), so that the KL term acts
from the second update of a call on."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.algos.pg.aac_base import AdvActorCriticBase
from accel_rl_amd.optimizers import update_methods
from accel_rl_amd.optimizers.base import NORM_LOG_LEN
from accel_rl_amd.optimizers.single import VmpoOptimizer

DUAL_FLOOR = 1e-8           # the projection of arl_vmpo_dual_step


def _finite(x):
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool) and bool(np.isfinite(x))


class VMPO(AdvActorCriticBase):
    """Single GPU, feed-forward policies"""

    def __init__(self, eps_eta=0.01, eps_alpha=0.005, eta_init=1.0, alpha_init=5.0, v_loss_coeff=0.5, discount=0.99,
                 gae_lambda=1, OptimizerCls=VmpoOptimizer, optimizer_args=None, lr_schedule=None, use_graph=True):
        if not (_finite(discount) and 0 <= discount <= 1 and _finite(gae_lambda) and 0 <= gae_lambda <= 1):
            raise ValueError("discount and gae_lambda must lie in [0, 1]")
        for name, eps in (("eps_eta", eps_eta), ("eps_alpha", eps_alpha)):
            if not (_finite(eps) and eps >= 0):
                raise ValueError("%s must be finite and >= 0, got %r" % (name, eps))
        for name, x in (("eta_init", eta_init), ("alpha_init", alpha_init)):
            if not (_finite(x) and x >= DUAL_FLOOR):
                raise ValueError("%s must be finite and >= 1e-8 (the duals' projection), got %r" % (name, x))
        if not _finite(v_loss_coeff):
            raise ValueError("v_loss_coeff must be finite")
        args = dict(learning_rate=1e-4, update_method=update_methods.adam, update_method_args=dict(), epochs=4,
                    minibatch_size="half", grad_norm_clip=None, shuffle=True)
        args.update(optimizer_args or dict())
        if not (isinstance(args["epochs"], (int, np.integer)) and not isinstance(args["epochs"], bool) and
                args["epochs"] >= 1):
            raise ValueError("optimizer_args: epochs must be an integer >= 1")
        bs = args["minibatch_size"]
        self._half_batch = isinstance(bs, str)
        if self._half_batch:
            if bs != "half":
                raise ValueError("optimizer_args: minibatch_size must be an integer >= 1, None (the whole batch) or 'half'")
            args["minibatch_size"] = None           # (set at initialize, where the batch size is known)
        elif bs is not None and not (isinstance(bs, (int, np.integer)) and not isinstance(bs, bool) and bs >= 1):
            raise ValueError("optimizer_args: minibatch_size must be an integer >= 1, None (the whole batch) or 'half'")
        self.optimizer = OptimizerCls(dual_init=(eta_init, alpha_init), eps_alpha=eps_alpha, **args)
        self.eps_eta, self.eps_alpha = float(eps_eta), float(eps_alpha)
        self.eta_init, self.alpha_init = float(eta_init), float(alpha_init)
        super().__init__(discount=discount, gae_lambda=gae_lambda, v_loss_coeff=v_loss_coeff, ent_loss_coeff=0.,
                         lr_schedule=lr_schedule, use_graph=use_graph)

    loss_kind = 4

    def pi_loss(self, policy, act, adv, old_dist_info, new_dist_info, valids):
        """-sum(psi log pi(a)): `adv` carries the minibatch's weights psi (arl_vmpo_weights; normalised, no gradient
        through them), so there is no mean."""
        if valids is not None:
            raise NotImplementedError("V-MPO takes no valids")
        return - torch.sum(adv * policy.distribution.log_likelihood_sym(act, new_dist_info))

    def initialize(self, policy, env_spec, sample_size, horizon, mid_batch_reset):
        if policy.recurrent:
            raise NotImplementedError("VMPO: recurrent policies are not built -- the top half is taken over rows, not "
                                      "trajectories (INTEGRATION.md, section E)")
        if not mid_batch_reset:
            raise NotImplementedError("VMPO: mid_batch_reset=False is not built -- the V-MPO kernels take no `valids` "
                                      "(INTEGRATION.md, section E)")
        opt = self.optimizer
        if opt.parallelism_tag != "single":
            raise NotImplementedError("VMPO: single GPU only, got a %r optimizer (%s): a per-rank top half is another "
                                      "algorithm (INTEGRATION.md, section E)" % (opt.parallelism_tag, type(opt).__name__))
        if not isinstance(opt, VmpoOptimizer):
            raise TypeError("VMPO needs an optimizer that owns the duals and steps them (VmpoOptimizer); got %s" %
                            type(opt).__name__)
        rows = int(sample_size)
        bs = max(rows // 2, 1) if self._half_batch else (rows if opt._minibatch_size is None else int(opt._minibatch_size))
        if bs > _lib.VMPO_MAX_ROWS:
            raise ValueError("VMPO: minibatches of %d rows; arl_vmpo_weights selects among at most %d (INTEGRATION.md, "
                             "section E)" % (bs, _lib.VMPO_MAX_ROWS))
        updates = opt._epochs * (rows // bs)
        if updates < 1 or updates > NORM_LOG_LEN:
            raise ValueError("VMPO: epochs * (sample_size // minibatch_size) = %d * (%d // %d) = %d updates; one "
                             "optimizer call takes 1 to %d (INTEGRATION.md, section E)" %
                             (opt._epochs, rows, bs, updates, NORM_LOG_LEN))
        opt._minibatch_size = bs
        super().initialize(policy, env_spec, sample_size, horizon, mid_batch_reset)
        dev = policy.device
        self._psi = torch.zeros(rows, dtype=torch.float32, device=dev)
        # (eta, alpha, mean KL) after the call's last update; allocated here, so the captured graph keeps writing the
        # same block
        self._vm_stats = torch.zeros(3, dtype=torch.float32, device=dev)

    # ---- device work (captured) ----
    def _device_optimize(self, itr, samples_data):
        opt_data, infos = super()._device_optimize(itr, samples_data)
        opt = self.optimizer
        self._vm_stats[0:2].copy_(opt.duals)
        self._vm_stats[2:3].copy_(opt._loss4[2:3])
        stats = self._vm_stats.clone()
        return opt_data, dict(GradNorm=infos["GradNorm"], Eta=stats[0:1], Alpha=stats[1:2], MeanKL=stats[2:3])

    def _losses(self, mb):
        """One minibatch: psi and the temperature's dual terms from the advantages of its rows (into the optimizer's
        temp4), then the policy's forward, V-MPO's head kernel and the backward pass into flat_grads.  Returns loss4 =
        (pi_loss, v_loss, mean KL, their plain sum)."""
        opt = self.optimizer
        _lib.vmpo_weights(mb["advantages"], mb.get("idx"), opt.duals, self.eps_eta, self._psi, opt.temp4)
        return self.policy.loss_and_grads(dict(mb, psi=self._psi), self.loss_kind, 0., self.v_loss_coeff, 0.,
                                          self._lr_mult, None, duals=opt.duals)

    @property
    def opt_info_keys(self):
        return ["GradNorm", "Eta", "Alpha", "MeanKL"]
