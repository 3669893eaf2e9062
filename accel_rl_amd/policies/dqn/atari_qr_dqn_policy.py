"""Quantile-regression DQN policy for Atari (QR-DQN, Dabney et al. 2018; the reference has none): conv stack ->
dense -> n_actions x n_quantiles quantile locations theta; Q_a is the mean of action a's quantiles; a target
network; epsilon-greedy action serving.  No support [V_min, V_max], no projection.

The stored output is the categorical head's -- one more dense MFMA call whose rows (one per action, + one value
row when dueling) are padded to `_atom_stride` columns, zero weights and zero gradients in the padding -- so the
layout hooks, the parameter names and the flat order are AtariCatDqnPolicy's with n_quantiles in place of n_atoms
(`self.n_atoms` is that alias for the inherited hooks).  What differs is what follows the layer: csrc/dqn.hip's
arl_qrdqn_act (mean over quantiles, first maximum) and arl_qrdqn_loss (pairwise quantile-Huber loss).
"""
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.dqn.atari_cat_dqn_policy import AtariCatDqnPolicy


class AtariQrDqnPolicy(AtariCatDqnPolicy):

    loss_folds_heads = False        # the quantile loss reads finished theta (no split-partial-sum entry point)

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(),
                 pixel_scale=255., epsilon=1, n_quantiles=64, dueling=False, initial_param_values=None):
        if not 2 <= n_quantiles <= 64:
            raise NotImplementedError("n_quantiles must be in [2, 64]")
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, epsilon=epsilon, n_atoms=n_quantiles, dueling=dueling,
                         initial_param_values=initial_param_values)
        self.n_quantiles = n_quantiles

    def incorporate_z(self, z):
        raise NotImplementedError("a quantile policy has no support: train it with QuantileDQN")

    def cat_loss_and_grads(self, *args, **kwargs):
        raise NotImplementedError("a quantile policy has no categorical loss: train it with QuantileDQN")

    def _serve(self, out, override, onehot, greedy=None):
        _lib.qrdqn_act(out, override, self.n_act, self.n_quantiles, onehot, greedy, dueling=self._dueling)

    # ---- training ------------------------------------------------------------
    def qr_loss_and_grads(self, obs, next_obs, actions, returns, terminals, is_weights, gamma_n, kappa,
                          double_dqn=False):
        """One minibatch of QuantileDQN.build_loss: forward of the policy net on obs, of the target net (and, for
        double DQN, the policy net) on next_obs, the quantile-Huber loss (kappa 0: plain quantile regression), and the
        full backward pass into flat_grads.  Returns (loss_rows f32[B] whose sum is the loss, priorities f32[B]).
        No host synchronisation and no allocation outside _buffer: it runs inside the captured update graph."""
        with torch.no_grad():
            b = obs.shape[0]
            x, theta, acts, hids, tgt_theta, pol_next = self._forward_for_loss(obs, next_obs, double_dqn,
                                                                               head_parts=False)
            dtheta = self._buffer(("dtheta", b), (b, self._head_width))
            pack = self._buffer(("loss_pri", b), (2, b))        # one buffer: DqnOptimizer's statistics ring takes both rows at once
            loss_rows, priorities = pack[0], pack[1]
            _lib.qrdqn_loss(theta, tgt_theta, pol_next, actions, returns, terminals, is_weights, self.n_act,
                            self.n_quantiles, gamma_n, kappa, dtheta, loss_rows, priorities, dueling=self._dueling)
            self._head_backward(dtheta, x, acts, hids)
            return loss_rows, priorities
