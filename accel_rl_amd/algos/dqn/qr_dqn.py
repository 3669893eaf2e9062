"""Quantile-regression DQN (QR-DQN, Dabney et al. 2018; the reference has none): DQN's replay, n-step returns,
prioritized replay and schedules with the pairwise quantile-Huber loss of csrc/dqn.hip:arl_qrdqn_loss.  Defaults
are the paper's: adam, learning rate 5e-5, epsilon = 0.01 / batch_size, epsilon-greedy 1 -> 0.01 (eval 0.001),
kappa = 1 (kappa = 0: plain quantile regression).  Priorities are the clipped per-sample loss."""
import numpy as np

from accel_rl_amd.algos.dqn.dqn import DQN
from accel_rl_amd.optimizers import update_methods


class QuantileDQN(DQN):

    def __init__(self, kappa=1.0, **kwargs):
        if not (np.isfinite(kappa) and kappa >= 0):
            raise ValueError("kappa must be finite and >= 0")
        self.kappa = kappa
        super().__init__(**kwargs)

    def _get_default_sub_args(self):
        opt_args = dict(learning_rate=5e-5, update_method=update_methods.adam,
                        grad_norm_clip=10 if self.dueling_dqn else None,
                        update_method_args=dict(epsilon=0.01 / self.batch_size),
                        scale_conv_grads=self.dueling_dqn)
        eps_greedy_args = dict(initial=1., final=0.01, eval=0.001, anneal_steps=int(1e6))
        priority_args = dict(alpha=0.6, beta_initial=0.4, beta_final=1., beta_anneal_steps=50e6,
                             default_priority=1.)
        return opt_args, eps_greedy_args, priority_args

    def build_loss(self, env_spec, policy):
        self._check_dueling(policy)
        gamma_n = float(np.float32(self.discount ** self.reward_horizon))

        def loss(minibatch):
            loss_rows, priorities = policy.qr_loss_and_grads(*self._unpack(minibatch, policy), gamma_n, self.kappa,
                                                             double_dqn=self.double_dqn)
            return priorities, loss_rows            # (the loss is their sum: DqnOptimizer)

        return self._loss_inputs(), loss
