"""Soft actor-critic for discrete actions (SAC-Discrete, Christodoulou 2019, "Soft Actor-Critic for Discrete Action
Settings"; the reference has none): an off-policy actor-critic that learns a stochastic policy from the replay memory.
The actor, the two critics with their target copies and the temperature live in AtariSacDiscretePolicy; the loss is
csrc/sac.hip (arl_sacd_loss, arl_sacd_alpha_grad); the four updates are SacOptimizer's.  Replay, prioritized replay
(priority = the mean clipped |TD error| of the two critics), the beta schedule, the target period, min_steps_learn,
training_intensity and augment_args with one view are DQN's.  There is no epsilon: exploration is the policy's own
entropy, held near target_entropy = target_entropy_scale * log(n_actions) by the learned temperature; evaluation serves
the first maximum of the logits (eval_deterministic).

Defaults as recalled from the paper and its common Atari implementation (restated from memory): batch 64,
adam at 3e-4 with epsilon 1e-4 for the networks and the temperature, one update per 4 environment steps, target copy
every 8 000 steps, 20 000 steps before learning, target_entropy_scale 0.89, squared loss.  No action is selected by an
argmax, so there is no double-DQN form; the entropy bonus of the intermediate steps of an n-step return is not in the
replay's disc_n_return, so reward_horizon must be 1."""
import numpy as np
import torch

from accel_rl_amd.algos.dqn.dqn import DQN
from accel_rl_amd.optimizers import update_methods
from accel_rl_amd.optimizers.dqn import SacOptimizer
from accel_rl_amd.policies.dqn.atari_sac_discrete_policy import AtariSacDiscretePolicy


class SacDiscrete(DQN):

    def __init__(self, target_entropy_scale=0.89, eval_deterministic=True, batch_size=64, min_steps_learn=int(2e4),
                 delta_clip=None, training_intensity=16, target_update_steps=int(8e3), **kwargs):
        """training_intensity counts minibatch samples per environment step: 16 = one update of 64 per 4 steps."""
        if not (np.isfinite(target_entropy_scale) and target_entropy_scale >= 0):
            raise ValueError("target_entropy_scale must be finite and >= 0")
        if kwargs.get("double_dqn"):
            raise NotImplementedError("the soft target selects no action: there is no double-DQN form "
                                      "(INTEGRATION.md, section E)")
        if kwargs.get("dueling_dqn"):
            raise NotImplementedError("dueling critics are not built for SAC-Discrete (INTEGRATION.md, section E)")
        if kwargs.get("reward_horizon", 1) != 1:
            raise NotImplementedError("n-step SAC returns are not built: the entropy bonus of the intermediate steps is "
                                      "not in the replay's disc_n_return (INTEGRATION.md, section E)")
        cls = kwargs.setdefault("OptimizerCls", SacOptimizer) or SacOptimizer
        if not (isinstance(cls, type) and issubclass(cls, SacOptimizer)):
            raise TypeError("SacDiscrete updates its four parameter ranges through a SacOptimizer (got %r)" % (cls,))
        kwargs["OptimizerCls"] = cls
        self.target_entropy_scale, self.eval_deterministic = target_entropy_scale, bool(eval_deterministic)
        super().__init__(batch_size=batch_size, min_steps_learn=min_steps_learn, delta_clip=delta_clip,
                         training_intensity=training_intensity, target_update_steps=target_update_steps, **kwargs)
        self._last_stats = None

    def _get_default_sub_args(self):
        opt_args, eps_greedy_args, priority_args = super()._get_default_sub_args()
        opt_args = dict(learning_rate=3e-4, update_method=update_methods.adam, update_method_args=dict(epsilon=1e-4),
                        grad_norm_clip=None)
        return opt_args, eps_greedy_args, priority_args          # (the epsilon-greedy schedule is never used)

    def build_loss(self, env_spec, policy):
        if type(policy) is not AtariSacDiscretePolicy:
            raise TypeError("SacDiscrete trains an AtariSacDiscretePolicy itself, not a subclass or another policy "
                            "(got %s)" % type(policy).__name__)
        gamma_n = float(np.float32(self.discount))
        self.target_entropy = float(np.float32(self.target_entropy_scale * np.log(policy.n_act)))

        def loss(minibatch):
            stats = policy.sac_loss_and_grads(*self._unpack(minibatch, policy), gamma_n, self.delta_clip,
                                              self.target_entropy)
            self._last_stats = stats                # (inside the captured graph: rewritten by every replay)
            return stats[1], stats[0]               # td_abs, q_loss_rows (the loss is their sum: DqnOptimizer)

        return self._loss_inputs(), loss

    def optimize_policy(self, itr, samples_data):
        """DQN's loop; the actor's loss, the entropy and the temperature are those of the call's last update."""
        opt_minibatch, info = super().optimize_policy(itr, samples_data)
        if info and self._last_stats is not None:
            stats = self._last_stats
            info.update(PiLoss=[stats[2].sum()], Entropy=[stats[3].mean()],
                        Alpha=[torch.exp(self.policy.log_alpha[0])])
        return opt_minibatch, info

    def update_epsilon(self, itr):
        pass

    def prep_eval(self, itr):
        self._prev_deterministic = self.policy.get_deterministic()
        self.policy.set_deterministic(self.eval_deterministic)

    def post_eval(self, itr):
        self.policy.set_deterministic(self._prev_deterministic)

    @property
    def opt_info_keys(self):
        return ["Priority", "Loss", "PiLoss", "Entropy", "Alpha"]
