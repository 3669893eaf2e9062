"""Implicit quantile networks (IQN, Dabney et al. 2018; the reference has none): DQN's replay, n-step returns,
prioritized replay and schedules with the pairwise quantile-Huber loss taken at fractions drawn afresh for every
sample (csrc/iqn.hip:arl_iqn_loss).  Defaults and the kappa check are QuantileDQN's; priorities are the clipped
per-sample loss.  The numbers of fractions (N, N', K) belong to the policy: AtariIqnPolicy."""
import numpy as np

from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy


class ImplicitQuantileDQN(QuantileDQN):

    def __init__(self, kappa=1.0, **kwargs):
        if kwargs.get("dueling_dqn"):
            raise NotImplementedError("dueling implicit quantile networks are not built (INTEGRATION.md, section E)")
        super().__init__(kappa=kappa, **kwargs)

    def build_loss(self, env_spec, policy):
        if not isinstance(policy, AtariIqnPolicy):
            raise TypeError("ImplicitQuantileDQN trains an AtariIqnPolicy (got %s)" % type(policy).__name__)
        gamma_n = float(np.float32(self.discount ** self.reward_horizon))

        def loss(minibatch):
            loss_rows, priorities = policy.iqn_loss_and_grads(*self._unpack(minibatch, policy), gamma_n, self.kappa,
                                                              double_dqn=self.double_dqn)
            return priorities, loss_rows            # (the loss is their sum: DqnOptimizer)

        return self._loss_inputs(), loss
