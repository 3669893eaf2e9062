"""Fully parameterized quantile functions (FQF, Yang et al. 2019; the reference has none): ImplicitQuantileDQN whose
fractions are proposed per state by the policy's fraction layer (AtariFqfPolicy) and trained to minimise the
1-Wasserstein distance to the network's quantile function, minus ent_coef times the proposal's entropy
(csrc/fqf.hip:arl_fqf_fractions / arl_fqf_loss).  Replay, n-step returns, prioritized replay, double DQN, schedules and
the main optimizer defaults are QuantileDQN's; the fraction layer has its own update (FqfOptimizer), by default the
paper's: RMSprop, learning rate 2.5e-9, rho 0.95, epsilon 1e-5.  The number of fractions N belongs to the policy."""
import numpy as np

from accel_rl_amd.algos.dqn.iqn import ImplicitQuantileDQN
from accel_rl_amd.optimizers import update_methods
from accel_rl_amd.optimizers.dqn import FqfOptimizer
from accel_rl_amd.policies.dqn.atari_fqf_policy import AtariFqfPolicy


class FQF(ImplicitQuantileDQN):

    def __init__(self, kappa=1.0, ent_coef=0.0, fraction_optimizer_args=None, **kwargs):
        if not (np.isfinite(ent_coef) and ent_coef >= 0):
            raise ValueError("ent_coef must be finite and >= 0")
        self.ent_coef = ent_coef
        cls = kwargs.setdefault("OptimizerCls", FqfOptimizer) or FqfOptimizer
        if not (isinstance(cls, type) and issubclass(cls, FqfOptimizer)):
            raise TypeError("FQF updates the fraction layer through an FqfOptimizer (got %r)" % (cls,))
        kwargs["OptimizerCls"] = cls
        frac = dict(learning_rate=2.5e-9, update_method=update_methods.rmsprop,
                    update_method_args=dict(rho=0.95, epsilon=1e-5))
        frac.update(fraction_optimizer_args or dict())
        self.fraction_optimizer_args = frac
        opt_args = dict(kwargs.pop("optimizer_args", None) or dict())
        opt_args["fraction_args"] = frac
        super().__init__(kappa=kappa, optimizer_args=opt_args, **kwargs)

    def build_loss(self, env_spec, policy):
        if not isinstance(policy, AtariFqfPolicy):
            raise TypeError("FQF trains an AtariFqfPolicy (got %s)" % type(policy).__name__)
        gamma_n = float(np.float32(self.discount ** self.reward_horizon))

        def loss(minibatch):
            loss_rows, priorities = policy.fqf_loss_and_grads(*self._unpack(minibatch, policy), gamma_n, self.kappa,
                                                              self.ent_coef, double_dqn=self.double_dqn)
            return priorities, loss_rows            # (the loss is their sum: DqnOptimizer)

        return self._loss_inputs(), loss
