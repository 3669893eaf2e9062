"""Munchausen RL (Vieillard, Pietquin, Geist 2020, "Munchausen Reinforcement Learning"; the reference has none): DQN
and IQN with a soft-max bootstrap over the target net's action values and the scaled, clipped log-policy bonus
alpha * clip(tau_e log pi(action | obs), l0, 0) added to the reward (csrc/dqn.hip:arl_mdqn_loss,
csrc/iqn.hip:arl_miqn_loss).  The whole change lives in the target: replay, serving, schedules, priorities and
update_target are the parents'.  Defaults are the paper's, which are QuantileDQN's: adam, learning rate 5e-5,
epsilon = 0.01 / batch_size, epsilon-greedy 1 -> 0.01 (eval 0.001); entropy_tau = 0.03, munchausen_alpha = 0.9,
munchausen_clip = -1.  Nothing is selected by an argmax, so there is no double-DQN form; the bonus of the intermediate
steps of an n-step return is not in the replay's disc_n_return, so reward_horizon must be 1."""
import numpy as np

from accel_rl_amd.algos.dqn.dqn import DQN
from accel_rl_amd.algos.dqn.iqn import ImplicitQuantileDQN
from accel_rl_amd.algos.dqn.qr_dqn import QuantileDQN
from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy


def _check_munchausen_args(entropy_tau, munchausen_alpha, munchausen_clip, kwargs):
    """The entry points' rules (a violation there is ARL_E_ARG), and the two refusals."""
    if not (np.isfinite(entropy_tau) and entropy_tau > 0):
        raise ValueError("entropy_tau must be finite and > 0")
    if not (np.isfinite(munchausen_alpha) and munchausen_alpha >= 0):
        raise ValueError("munchausen_alpha must be finite and >= 0")
    if not (np.isfinite(munchausen_clip) and munchausen_clip <= 0):
        raise ValueError("munchausen_clip must be finite and <= 0")
    if kwargs.get("double_dqn"):
        raise NotImplementedError("Munchausen targets select no action: there is no double-DQN form "
                                  "(INTEGRATION.md, section E)")
    if kwargs.get("reward_horizon", 1) != 1:
        raise NotImplementedError("n-step Munchausen returns are not built: the bonus of the intermediate steps is not "
                                  "in the replay's disc_n_return (INTEGRATION.md, section E)")


class MunchausenDQN(DQN):

    def __init__(self, entropy_tau=0.03, munchausen_alpha=0.9, munchausen_clip=-1.0, **kwargs):
        _check_munchausen_args(entropy_tau, munchausen_alpha, munchausen_clip, kwargs)
        self.entropy_tau, self.munchausen_alpha, self.munchausen_clip = entropy_tau, munchausen_alpha, munchausen_clip
        super().__init__(**kwargs)

    _get_default_sub_args = QuantileDQN._get_default_sub_args

    def build_loss(self, env_spec, policy):
        if type(policy) is not AtariDqnPolicy:
            raise TypeError("MunchausenDQN trains an AtariDqnPolicy itself, not a subclass (got %s)" %
                            type(policy).__name__)
        self._check_dueling(policy)
        gamma_n = float(np.float32(self.discount))

        def loss(minibatch):
            loss_rows, td_abs = policy.munchausen_loss_and_grads(
                *self._unpack(minibatch, policy), gamma_n, self.delta_clip, self.entropy_tau,
                self.munchausen_alpha, self.munchausen_clip)
            return td_abs, loss_rows                # (the loss is their sum: DqnOptimizer)

        return self._loss_inputs(), loss


class MunchausenIQN(ImplicitQuantileDQN):

    def __init__(self, entropy_tau=0.03, munchausen_alpha=0.9, munchausen_clip=-1.0, **kwargs):
        _check_munchausen_args(entropy_tau, munchausen_alpha, munchausen_clip, kwargs)
        self.entropy_tau, self.munchausen_alpha, self.munchausen_clip = entropy_tau, munchausen_alpha, munchausen_clip
        super().__init__(**kwargs)

    def build_loss(self, env_spec, policy):
        if not isinstance(policy, AtariIqnPolicy):
            raise TypeError("MunchausenIQN trains an AtariIqnPolicy (got %s)" % type(policy).__name__)
        gamma_n = float(np.float32(self.discount))

        def loss(minibatch):
            loss_rows, priorities = policy.munchausen_loss_and_grads(
                *self._unpack(minibatch, policy), gamma_n, self.kappa, self.entropy_tau,
                self.munchausen_alpha, self.munchausen_clip)
            return priorities, loss_rows            # (the loss is their sum: DqnOptimizer)

        return self._loss_inputs(), loss
