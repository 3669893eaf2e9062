"""DrQ (Kostrikov, Yarats, Fergus 2020, "Image Augmentation Is All You Need"; the reference has none): double + dueling
+ n-step DQN for the data-efficient regime (Atari-100k) whose every replayed observation is padded by `pad` pixels with
its own border and cropped back at a random offset -- inside the replay memory's extraction gather
(csrc/replay.hip:arl_replay_extract_shift) -- and whose target is averaged over `k_targets` shifted copies of next_obs
and whose loss over `m_online` shifted copies of obs, inside the loss launch (csrc/dqn.hip:arl_drq_loss).  Replay,
serving, schedules, priorities (td_abs, averaged over the m views) and update_target are DQN's; prioritized replay is
allowed.

Defaults: the paper's Atari-100k settings AS RESTATED FROM MEMORY (the paper was not at hand): double +
dueling, reward_horizon 10, batch_size 32, replay_size 1e5, min_steps_learn 1600, training_intensity 32 (one update per
environment step), target_update_steps 1, adam with learning rate 1e-4, grad_norm_clip 10, epsilon-greedy 1 -> 0.1 over
5 000 steps (eval 0.05), pad 4, K = M = 1.  The paper's intensity jitter is not built.

target_update_steps = 1 means "after every update" in the paper.  DQN.optimize_policy copies the target net once per
call -- _target_update_itr = max(1, target_update_steps // sample_size) = 1 -- that is once per sampler batch, after its
_updates_per_optimize updates, not once per update: with a sampler batch of one step per environment the two agree."""
import numpy as np

from accel_rl_amd.algos.dqn.dqn import DQN
from accel_rl_amd.optimizers import update_methods
from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy


class DrQ(DQN):

    _multi_view = True

    def __init__(self, k_targets=1, m_online=1, pad=4, aug_seed=0, **kwargs):
        for name, v in (("k_targets", k_targets), ("m_online", m_online)):
            if not (isinstance(v, (int, np.integer)) and 1 <= v <= 8):
                raise ValueError("%s must be an integer in 1 .. 8 (arl_drq_loss)" % name)
        if not (isinstance(pad, (int, np.integer)) and 0 <= pad <= 64):
            raise ValueError("pad must be an integer in 0 .. 64 (arl_replay_extract_shift)")
        if kwargs.get("augment_args") is not None:
            raise TypeError("DrQ builds augment_args itself from pad, aug_seed, k_targets and m_online")
        self.k_targets, self.m_online, self.pad, self.aug_seed = int(k_targets), int(m_online), int(pad), int(aug_seed)
        for key, value in dict(double_dqn=True, dueling_dqn=True, reward_horizon=10, batch_size=32,
                               replay_size=int(1e5), min_steps_learn=1600, training_intensity=32,
                               target_update_steps=1).items():
            kwargs.setdefault(key, value)
        kwargs["augment_args"] = dict(pad=self.pad, seed=self.aug_seed, k_targets=self.k_targets, m_online=self.m_online)
        super().__init__(**kwargs)

    def _get_default_sub_args(self):
        opt_args = dict(learning_rate=1e-4, update_method=update_methods.adam, grad_norm_clip=10,
                        update_method_args=dict(), scale_conv_grads=self.dueling_dqn)
        eps_greedy_args = dict(initial=1., final=0.1, eval=0.05, anneal_steps=5000)
        d_clip = self.delta_clip
        priority_args = dict(alpha=0.6, beta_initial=0.4, beta_final=1., beta_anneal_steps=50e6,
                             default_priority=d_clip if d_clip is not None else 1.)
        return opt_args, eps_greedy_args, priority_args

    def build_loss(self, env_spec, policy):
        if type(policy) is not AtariDqnPolicy:
            raise TypeError("DrQ trains an AtariDqnPolicy itself, not a subclass (got %s)" % type(policy).__name__)
        self._check_dueling(policy)
        gamma_n = float(np.float32(self.discount ** self.reward_horizon))

        def loss(minibatch):
            loss_rows, td_abs = policy.drq_loss_and_grads(*self._unpack(minibatch, policy), gamma_n, self.delta_clip,
                                                          self.double_dqn, self.m_online, self.k_targets)
            return td_abs, loss_rows                # (the loss is their sum: DqnOptimizer)

        return self._loss_inputs(), loss
