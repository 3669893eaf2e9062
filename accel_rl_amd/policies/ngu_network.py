"""The controllable-state embedding of NGU's episodic bonus ("Never Give Up", Badia et al. 2020; PAPERS.md has what is
recalled and what is chosen): an `_RndTrunk` -- AtariCnnPolicy's conv stack and one LINEAR dense layer of width E -- on
the same whitened one-plane input as RND's two networks.  The observation statistics are RndNetwork's: shared, not
duplicated.

`embed` is a no-grad pass over all rows like RndNetwork.errors.  The embedding is trained by the paper's
inverse-dynamics head: a two-layer MLP on the pair of embeddings of the frames before and after an action predicts that
action.  Its parameters W1 [2E, H], b1, W2 [H, A], b2 are this trunk's "head" tensors, so they live in its flat bucket
and one optimiser step moves trunk and head.  `loss_and_grads` is arl_rnd_obs_prepare on the interleaved rows (idx - 1,
idx) -> the trunk on 2B rows -> arl_invdyn_loss_parts (csrc/episodic.hip) -> `_backward_trunk`.  Initial values from a
private np.random.RandomState(seed)."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.rnd_network import _RndTrunk
from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox

STATE_KEYS = ("embedding", "mem", "n_ins", "dist_mean", "err_moments")


def _int_in(x, lo, hi):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool) and lo <= x <= hi


class NguEmbedding(_RndTrunk):

    def __init__(self, rnd, embedding_size=32, head_hidden=128, seed=0, conv_filters=(32, 64, 64), conv_filter_sizes=(8, 4, 3),
                 conv_strides=(4, 2, 1), conv_pads=((0, 0), (0, 0), (0, 0))):
        """rnd: the RndNetwork whose observation statistics and input stage this embedding shares."""
        if not (_int_in(embedding_size, 4, _lib.EPI_MAX_WIDTH) and embedding_size % 4 == 0):
            raise ValueError("embedding_size must be a multiple of 4 in 4 .. %d, got %r" % (_lib.EPI_MAX_WIDTH,
                                                                                           embedding_size))
        if not _int_in(seed, 0, 2 ** 32 - 1):
            raise ValueError("seed must be an integer in 0 .. 2^32 - 1, got %r" % (seed,))
        if not (_int_in(head_hidden, 4, 256) and head_hidden % 4 == 0 and
                ((2 * embedding_size + 31) // 32) * ((head_hidden + 31) // 32) <= 16):
            raise ValueError("head_hidden must be a multiple of 4 in 4 .. 256 with ceil(2 E / 32) ceil(H / 32) <= 16 "
                             "(arl_invdyn_loss_parts), got %r for embedding_size %d" % (head_hidden, embedding_size))
        self.embedding_size, self.head_hidden, self.seed, self._rnd = int(embedding_size), int(head_hidden), int(seed), rnd
        super().__init__(np.random.RandomState(self.seed), [self.embedding_size], conv_filters=conv_filters,
                         conv_filter_sizes=conv_filter_sizes, conv_strides=conv_strides, conv_pads=conv_pads)

    def initialize(self, env_spec, n_env, memory_size, device=None):
        """After rnd.initialize.  env_spec: the policy's; mem f32[n_env, memory_size, E] and the running moments start
        as zeros."""
        c, h, w = env_spec.observation_space.shape
        n_act = env_spec.action_space.n
        if not 2 <= n_act <= 64:
            raise ValueError("the inverse-dynamics head takes 2 .. 64 actions, got %d" % n_act)
        super().initialize(EnvSpec(UintBox((1, h, w)), Discrete(n_act)), device=device)
        dev, self.n_env = self.device, int(n_env)
        self._head_ws = _lib.invdyn_workspace(self.embedding_size, self.head_hidden, n_act, dev)
        self.loss2 = torch.zeros(4, dtype=torch.float32, device=dev)        # (loss, accuracy) of the last update
        self.mem = torch.zeros((self.n_env, int(memory_size), self.embedding_size), dtype=torch.float32, device=dev)
        self.n_ins = torch.zeros(self.n_env, dtype=torch.int32, device=dev)
        self.dist_mean = torch.zeros(2, dtype=torch.float64, device=dev)
        self.err_moments = torch.zeros(3, dtype=torch.float64, device=dev)

    # ---- the head's tensors, in the trunk's bucket (reference layout = internal layout)
    def _head_reference_init(self, fan, n_act):
        out = []
        for rows, cols in ((2 * fan, self.head_hidden), (self.head_hidden, n_act)):
            w = self._rng.randn(rows, cols).astype(np.float32)              # NormCInit(1.0), as the dense layers
            w *= 1.0 / np.sqrt(np.square(w).sum(axis=0, keepdims=True))
            out += [w, np.zeros(cols, np.float32)]
        return out, ["InvW1", "Invb1", "InvW2", "Invb2"]

    def _head_internal_shapes(self, fan, n_act):
        return [(2 * fan, self.head_hidden), (self.head_hidden,), (self.head_hidden, n_act), (n_act,)]

    def _head_to_internal(self, ref_tail):
        return list(ref_tail)

    def loss_and_grads(self, observations, extra_observations, idx, actions, dones):
        """One training pass on the pairs (row idx[b] - 1, row idx[b]) with the action of row idx[b] (idx None: every
        row): the weighted cross-entropy of the head and its gradient into the flat bucket (overwritten).  A pair weighs
        0 where the row is the first of its env's rollout or either row has `done`.  Returns loss2, a device
        f32[4] = (loss, accuracy, 0, 0)."""
        with torch.no_grad():
            rnd = self._rnd
            horizon = rnd._horizon(observations)
            if idx is None:
                idx = rnd._all_rows(observations.shape[0])
            b = idx.shape[0]
            rows = idx.long()
            before = (rows - 1).clamp_(min=0)
            dones = dones.reshape(-1)
            weight = ((rows % horizon != 0) & (dones[rows] == 0) & (dones[before] == 0)).float()
            pairs = torch.stack((before, rows), dim=1).reshape(-1).int()
            h, w = rnd._frame_hw
            x = self._buffer(("ngu_x", 2 * b), (2 * b, h, w, 4))
            _lib.rnd_obs_prepare(observations, extra_observations, pairs, rnd.n_env, horizon, rnd.obs_count, rnd.obs_mean,
                                 rnd.obs_m2, x)
            acts, hids = self._trunk(x)
            de = self._buffer(("ngu_de", b), (2 * b, self.embedding_size))
            k = self._k_head
            self._folds.invdyn_loss(hids[-1], self._w[k], self._w[k + 1], self._w[k + 2], self._w[k + 3],
                                    actions.reshape(-1)[rows].to(torch.uint8), weight, de, self._g[k], self._g[k + 1],
                                    self._g[k + 2], self._g[k + 3], self.loss2, self._head_ws)
            self._backward_trunk(x, acts, hids, de, masked=True)
            return self.loss2

    def embed(self, observations, extra_observations, out, rows_per_pass=None):
        """out f32[rows, E] <- the embedding of every row's next frame, in passes of at most rows_per_pass rows (None:
        one pass).  Rows are independent: the passes compute what one pass computes."""
        rnd = self._rnd
        with torch.no_grad():
            n = observations.shape[0]
            step = n if not rows_per_pass else min(n, int(rows_per_pass))
            h, w = rnd._frame_hw
            for lo in range(0, n, step):
                hi = min(lo + step, n)
                idx = None if hi - lo == n else rnd._all_rows(n)[lo:hi]
                x = self._buffer(("ngu_x", hi - lo), (hi - lo, h, w, 4))
                _lib.rnd_obs_prepare(observations, extra_observations, idx, rnd.n_env, rnd._horizon(observations),
                                     rnd.obs_count, rnd.obs_mean, rnd.obs_m2, x)
                out[lo:hi].copy_(self._trunk(x)[1][-1])
            return out

    # ---- everything the episodic bonus carries across iterations, as NumPy arrays
    def _state_tensors(self):
        return dict(embedding=self.flat_params, mem=self.mem, n_ins=self.n_ins, dist_mean=self.dist_mean,
                    err_moments=self.err_moments)

    def ngu_state(self):
        return {k: t.detach().cpu().numpy().copy() for k, t in self._state_tensors().items()}

    def set_ngu_state(self, state):
        tensors = self._state_tensors()
        if sorted(state) != sorted(tensors):
            raise ValueError("set_ngu_state: keys %s, expected %s" % (sorted(state), sorted(tensors)))
        for k, t in tensors.items():
            a = np.asarray(state[k])
            if a.shape != tuple(t.shape) or a.dtype != np.dtype(str(t.dtype).split(".")[1]):
                raise ValueError("set_ngu_state: %s is %s %s, expected %s %s" % (k, a.dtype, a.shape, t.dtype, tuple(t.shape)))
        for k, t in tensors.items():
            t.copy_(torch.from_numpy(np.ascontiguousarray(state[k])))
        self.note_params_changed()
