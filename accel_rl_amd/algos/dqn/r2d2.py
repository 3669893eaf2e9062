"""R2D2 (Kapturowski, Ostrovski, Quan, Munos, Dabney 2019: "Recurrent Experience Replay in Distributed Reinforcement
Learning"; the reference has none): DQN's host-side logic -- training intensity, epsilon / beta schedules, target-network
period, evaluation hooks -- over replayed SEQUENCES from a stored recurrent state (replay_buffers/sequence.py), for a
recurrent Q policy (policies/dqn/atari_r2d2_policy.py).  Per sequence: `burn_in` steps that only warm the state up,
`train_len` steps of n-step double-Q learning under the invertible value rescaling h(x) = sign(x)(sqrt(|x| + 1) - 1) +
eps x, and the priority eta max_t |d| + (1 - eta) mean_t |d| (csrc/r2d2.hip: arl_r2d2_loss).  Arguments and defaults follow
the paper as recalled; its distributed actors are not built (one sampler, one learner)."""
import numpy as np

from accel_rl_amd.algos.dqn.dqn import DQN
from accel_rl_amd.algos.dqn.replay_buffers.sequence import SequenceReplayBuffer
from accel_rl_amd.optimizers import update_methods


class R2D2(DQN):

    def __init__(self, discount=0.997, batch_size=64, min_steps_learn=int(5e4), replay_size=int(1e6),
                 training_intensity=8, target_update_steps=int(1e4), reward_horizon=5, burn_in=40, train_len=80,
                 seq_stride=40, value_rescale=True, rescale_eps=1e-3, priority_eta=0.9, OptimizerCls=None,
                 optimizer_args=None, eps_greedy_args=None, dueling_dqn=True, prioritized_replay=True, priority_args=None):
        for name, value, low in (("burn_in", burn_in, 0), ("train_len", train_len, 1), ("seq_stride", seq_stride, 1),
                                 ("reward_horizon", reward_horizon, 1), ("batch_size", batch_size, 1)):
            if not (isinstance(value, (int, np.integer)) and value >= low):
                raise ValueError("%s must be an integer >= %d, got %r" % (name, low, value))
        if not (np.isfinite(priority_eta) and 0. <= priority_eta <= 1.):
            raise ValueError("priority_eta must lie in [0, 1], got %r" % (priority_eta,))
        if value_rescale and not (np.isfinite(rescale_eps) and rescale_eps > 0.):
            raise ValueError("rescale_eps must be finite and > 0 under value_rescale, got %r" % (rescale_eps,))
        self.burn_in, self.train_len, self.seq_stride = int(burn_in), int(train_len), int(seq_stride)
        self.value_rescale, self.rescale_eps, self.priority_eta = bool(value_rescale), rescale_eps, priority_eta
        super().__init__(discount=discount, batch_size=batch_size, min_steps_learn=min_steps_learn, delta_clip=None,
                         replay_size=replay_size, training_intensity=training_intensity,
                         target_update_steps=target_update_steps, reward_horizon=reward_horizon,
                         OptimizerCls=OptimizerCls, optimizer_args=optimizer_args, eps_greedy_args=eps_greedy_args,
                         double_dqn=True, dueling_dqn=dueling_dqn, prioritized_replay=prioritized_replay,
                         priority_args=priority_args)

    def _get_default_sub_args(self):
        opt_args = dict(learning_rate=1e-4, update_method=update_methods.adam, grad_norm_clip=None,
                        update_method_args=dict(epsilon=1e-3))
        eps_greedy_args = dict(initial=1., final=0.1, eval=0.05, anneal_steps=int(1e6))
        priority_args = dict(alpha=0.9, beta_initial=0.6, beta_final=0.6, beta_anneal_steps=50e6, default_priority=1.)
        return opt_args, eps_greedy_args, priority_args

    def initialize(self, policy, env_spec, sample_size, horizon, mid_batch_reset):
        if not (int(policy.recurrent) and hasattr(policy, "r2d2_loss_and_grads")):
            raise NotImplementedError("R2D2 trains a recurrent Q policy that provides r2d2_loss_and_grads "
                                      "(policies/dqn/atari_r2d2_policy.py: AtariR2d2Policy), got %s; feed-forward Q policies "
                                      "train with DQN and its kin (INTEGRATION.md, section E)" % type(policy).__name__)
        if not mid_batch_reset:
            raise NotImplementedError("R2D2 needs mid_batch_reset=True: the replay memory stores every step")
        per_update = self.batch_size * self.train_len
        if self.training_intensity * sample_size % per_update:
            raise ValueError("training_intensity * sample_size (%d * %d) must be a multiple of batch_size * train_len "
                             "(%d * %d)" % (self.training_intensity, sample_size, self.batch_size, self.train_len))
        self._updates_per_optimize = int(self.training_intensity * sample_size // per_update)
        self._eps_anneal_itr = max(1, self._eps_anneal_steps // sample_size)
        self._target_update_itr = max(1, self.target_update_steps // sample_size)
        self._min_itr_learn = self.min_steps_learn // sample_size
        if self.prioritized_replay:
            self._priority_beta_anneal_itr = max(1, self._priority_beta_anneal_steps // sample_size)
        self.policy = policy
        replay_args = dict(env_spec=env_spec, size=self.replay_size, reward_horizon=self.reward_horizon,
                           sampling_horizon=horizon, n_environments=sample_size // horizon, discount=self.discount,
                           reward_dtype="float32", device=getattr(policy, "device", "cuda:0"), burn_in=self.burn_in,
                           train_len=self.train_len, seq_stride=self.seq_stride, n_step=self.reward_horizon,
                           state_keys=policy.state_info_keys, hidden=policy._H, prioritized=self.prioritized_replay)
        if self.prioritized_replay:
            replay_args.update(self._priority_args)
        self.replay_buffer = SequenceReplayBuffer(**replay_args)        # (its refusals come before any device work)
        self.replay_buffer.reuse_outputs = True       # minibatches are consumed before the next one is drawn
        input_list, loss = self.build_loss(env_spec, policy)
        self.optimizer.initialize(inputs=input_list, loss=loss, target=policy)

    def build_loss(self, env_spec, policy):
        self._check_dueling(policy)
        gamma_n = float(self.discount) ** self.reward_horizon
        n_state = len(policy.state_info_keys)
        eps = self.rescale_eps if self.value_rescale else 0.0

        def loss(minibatch):
            obs, act, ret, term, resets = minibatch[:5]
            init_states, isw = minibatch[5:5 + n_state], minibatch[5 + n_state]
            loss_rows, priorities = policy.r2d2_loss_and_grads(obs, act, ret, term, resets, init_states, isw, gamma_n,
                                                               self.burn_in, self.train_len, self.reward_horizon,
                                                               rescale_eps=eps, eta=self.priority_eta)
            return priorities, loss_rows                # (the loss is their sum: DqnOptimizer)

        # (DQN.optimize_policy runs as it is: the sequence replay hands its importance weights over on the device in both
        # modes -- ones under uniform replay -- and priorities are written back only under prioritized replay)
        inputs = ["obs", "act", "disc_n_return", "terminal", "resets"] + list(policy.state_info_keys)
        return inputs + ["importance_sample_weights"], loss
