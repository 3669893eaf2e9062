"""Sequence replay for R2D2 (Kapturowski et al. 2019; the reference has none): a FrameReplayBuffer -- frames, actions,
n-step returns and terminals exactly as the other replay memories store them -- plus, per environment, the recurrent
state recorded before every `seq_stride`-th step and a ring of reset flags (csrc/r2d2.hip: arl_seq_store), sampled as
whole sequences of U = burn_in + train_len + reward_horizon steps that start on those strides (arl_seq_prepare, then
arl_replay_extract on the expanded index lists).  The sum tree's leaves are sequence slots, not steps.

Which slots can be sampled is a pure host function of the write cursor (`sampleable_slots`); the tree's
zeros_forward / zeros_backward are derived from the same two distances, so its non-zero leaves are that set."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.algos.dqn.replay_buffers.frame import FrameReplayBuffer
from accel_rl_amd.algos.dqn.replay_buffers.sum_tree import PartedSumTree


def slot_zeros(seq_stride, seq_len, n_stack):
    """(zeros_forward, zeros_backward) in slot units.  Forward of the cursor: the slots whose first step has lost one of
    its n_stack - 1 history frames to the writes at the cursor (first step < n_stack - 1 steps ahead of it).  Backward:
    the slots that started fewer than seq_len steps ago -- their last states are not written yet (and with them the
    n-step returns of their train rows, which are final once the n trailing rows are in)."""
    return -(-(n_stack - 1) // seq_stride), (seq_len - 1) // seq_stride


def sampleable_slots(cursor, full, size, seq_stride, seq_len, n_stack):
    """bool[size / seq_stride]: slot k (first step at ring index k * seq_stride) can be sampled when the next step is
    written at `cursor` (a multiple of seq_stride) and the ring has (`full`) or has not wrapped yet.  The n-step
    returns need no term of their own: the return of a train row is final once the row n steps later is written, and
    that row belongs to the sequence."""
    if cursor % seq_stride or size % seq_stride:
        raise ValueError("cursor and size must be multiples of seq_stride")
    first = np.arange(size // seq_stride) * seq_stride
    if not full:                            # steps 0 .. cursor - 1 exist; before step 0 the history is blank, not lost
        return first + seq_len <= cursor
    ahead = (first - cursor) % size         # distance from the cursor (the oldest step) to the slot's first step
    return (ahead >= n_stack - 1) & (ahead + seq_len <= size)


class SequenceReplayBuffer(FrameReplayBuffer):

    def __init__(self, burn_in, train_len, seq_stride, state_keys, hidden, n_step=None, prioritized=True, alpha=0.9,
                 beta_initial=0.6, default_priority=1., **kwargs):
        n, horizon = kwargs["reward_horizon"], kwargs["sampling_horizon"]
        n_env = kwargs["n_environments"]
        n_stack = tuple(kwargs["env_spec"].observation_space.shape)[0]
        self.burn_in, self.train_len, self.seq_stride = int(burn_in), int(train_len), int(seq_stride)
        self.seq_len = U = self.burn_in + self.train_len + n
        S = self.seq_stride
        # every refusal before anything touches the device
        if n_step is not None and n_step != n:
            raise ValueError("reward_horizon (%d) must equal the n of the n-step targets (%d): the stored returns are "
                             "the targets' returns" % (n, n_step))
        if S < 1 or self.train_len < 1 or self.burn_in < 0:
            raise ValueError("need seq_stride >= 1, train_len >= 1, burn_in >= 0")
        if horizon % S:
            raise ValueError("sampling_horizon (%d) must be a multiple of seq_stride (%d)" % (horizon, S))
        sampling_size = horizon * n_env
        env_size = -(-kwargs["size"] // sampling_size) * sampling_size // n_env      # as FrameReplayBuffer rounds it
        if env_size % S:                    # (a ring rounded up to whole sampler batches as above always passes)
            raise ValueError("env_replay_size (%d) must be a multiple of seq_stride (%d)" % (env_size, S))
        if U > env_size - (n_stack - 1):
            raise ValueError("a sequence of %d steps and its %d history frames do not fit a ring of %d steps"
                             % (U, n_stack - 1, env_size))
        if not 1 <= len(state_keys) <= 2 or hidden % 4 or not 4 <= hidden <= 1024:
            raise ValueError("need one or two state tensors of width % 4 == 0 in 4 .. 1024")
        zf, zb = slot_zeros(S, U, n_stack)
        if prioritized and zf + zb + horizon // S > env_size // S:
            raise ValueError("ring too small for the sum tree: %d slots per environment, %d switched off around the "
                             "cursor and %d appended per batch" % (env_size // S, zf + zb, horizon // S))
        super().__init__(**kwargs)
        assert self.env_replay_size == env_size
        self.state_keys, self.hidden = tuple(state_keys), int(hidden)
        self.n_slots = env_size // S
        dev = self.device
        self.state_store = [torch.zeros((n_env, self.n_slots, hidden), dtype=torch.float32, device=dev)
                            for _ in self.state_keys]
        self.reset_ring = torch.zeros((n_env, env_size), dtype=torch.uint8, device=dev)
        self._buffer_full = False
        self.prioritized = bool(prioritized)
        self.alpha, self.beta = alpha, beta_initial
        if self.prioritized:
            self.priority_tree = PartedSumTree(part_size=self.n_slots, num_parts=n_env, zeros_forward=zf, zeros_backward=zb,
                                               default_value=default_priority ** alpha, n_advance=horizon // S, device=dev)
        self.default_probability = default_priority ** alpha

    def set_beta(self, value):
        self.beta = value

    def sampleable(self):
        return sampleable_slots(self.idx, self._buffer_full, self.env_replay_size, self.seq_stride, self.seq_len,
                                self.num_img_obs)

    def append_data(self, samples_data):
        idx = self.idx
        super().append_data(samples_data)
        infos = samples_data["agent_infos"]
        # after which rows the sampler zeroed the state (`dones` alone is wrong with episodic lives: algos/pg/aac_base.py)
        resets = samples_data.get("env_infos", dict()).get("need_reset", samples_data["dones"])
        _lib.seq_store([infos[k].view(-1, self.hidden) for k in self.state_keys], resets.view(-1), self.n_environments,
                       self.sampling_horizon, self.env_replay_size, self.seq_stride, idx, self.state_store,
                       self.reset_ring)
        if self.idx == 0:
            self._buffer_full = True
        if self.prioritized:
            self.priority_tree.advance()

    # ---- sampling ------------------------------------------------------------------------------------------------------
    def _seq_outputs(self, b):
        cache = self.__dict__.setdefault("_seq_cache", dict())
        if self.reuse_outputs and b in cache:
            return cache[b]
        dev, rows = self.device, b * self.seq_len
        out = dict(env_rows=torch.empty(rows, dtype=torch.int32, device=dev),
                   step_rows=torch.empty(rows, dtype=torch.int32, device=dev),
                   resets=torch.empty(rows, dtype=torch.uint8, device=dev),
                   states=[torch.empty((b, self.hidden), dtype=torch.float32, device=dev) for _ in self.state_keys],
                   is_weights=torch.empty(b, dtype=torch.float32, device=dev))
        if self.reuse_outputs:
            for t in [out["resets"], out["is_weights"]] + out["states"]:
                t._arl_static = True
            cache[b] = out
        return out

    def extract_sequences(self, env_idxs, slot_idxs, out=None):
        """(env, slot) i32 device tensors (or host lists) -> (obs, act, ret, term, resets, *initial states): B * U rows,
        [sequence][time]."""
        if not isinstance(env_idxs, torch.Tensor):
            env_idxs, slot_idxs = self._upload_idxs(env_idxs, slot_idxs)
        out = out or self._seq_outputs(env_idxs.numel())
        _lib.seq_prepare(env_idxs, slot_idxs, self.seq_len, self.env_replay_size, self.seq_stride, self.state_store,
                         self.reset_ring, out["env_rows"], out["step_rows"], out["states"], out["resets"])
        obs, _, act, ret, term = self.extract_batch(out["env_rows"], out["step_rows"])
        return (obs, act, ret, term, out["resets"]) + tuple(out["states"])

    def sample_batch(self, batch_size, device_weights=True):
        """-> (obs u8[B * U, ...], act, ret, term, resets, *initial states, is_weights f32[B]) on the device."""
        if not device_weights:
            raise NotImplementedError("sequence replay hands its importance weights over on the device")
        out = self._seq_outputs(batch_size)
        isw = out["is_weights"]
        if not self.prioritized:
            env_idxs, slot_idxs = self.sample_idxs(batch_size)
            isw.fill_(1.)
            return self.extract_sequences(env_idxs, slot_idxs, out) + (isw,)
        tree = self.priority_tree
        dev = tree.sample_n_device(batch_size, self.beta, isw)
        if dev is not None:
            env_idxs, slot_idxs, probs = dev
            data = self.extract_sequences(env_idxs, slot_idxs, out)
            if tree.confirm_unique():
                return data + (isw,)
            env_idxs, slot_idxs, probs = tree.top_up()                 # the reference's sum tree would have drawn more
        else:
            env_idxs, slot_idxs, probs = tree.sample_n(batch_size)
        data = self.extract_sequences(env_idxs, slot_idxs, out)
        w = (1. / probs) ** self.beta
        w /= max(w)
        isw.copy_(torch.from_numpy(w.astype(np.float32)))
        return data + (isw,)

    def sample_idxs(self, batch_size):
        """uniform mode: host RNG, with replacement, over the sampleable slots."""
        slots = np.flatnonzero(self.sampleable())
        if not len(slots):
            raise RuntimeError("no sequence can be sampled yet")
        env_idxs = np.random.randint(low=0, high=self.n_environments, size=batch_size)
        return env_idxs, slots[np.random.randint(low=0, high=len(slots), size=batch_size)]

    def update_batch_priorities(self, priorities):
        if not self.prioritized:
            return
        if isinstance(priorities, torch.Tensor) and priorities.is_cuda and priorities.dtype == torch.float32:
            self.priority_tree.update_last_samples_pow(priorities, self.alpha)
            return
        priorities = np.asarray(priorities.cpu() if hasattr(priorities, "cpu") else priorities)
        self.priority_tree.update_last_samples(priorities ** self.alpha)
