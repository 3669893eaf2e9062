"""Random network distillation (Burda et al. 2018; PAPERS.md has what is recalled and what is chosen): a fixed, randomly
initialised target network and a trained predictor network embed the newest frame of every NEXT observation; the
predictor's squared error is the exploration bonus.

Two parameter buckets of the same conv stack, each an AtariCnnPolicy trunk on the one-plane float input (zero-padded to
four channels, as the policy pads short frame stacks; `_u8_conv1 = False`):

  target    convs -> one LINEAR dense layer of width E; written at initialisation, never after
  predictor convs -> dense + rectifier layers `predictor_hidden` -> a LINEAR dense layer of width E; trained

The launches are AtariCnnPolicy's (`_trunk`, `_backward_trunk`, `_layer_geoms`, FoldList, the workspaces).  The last
dense layer is the only difference: no rectifier in the forward pass, the embedding's gradient handed to the backward
pass as `masked=True`, and -- where the weight-gradient kernel does not carry the bias sums along -- an unmasked bias
sum (`_bias_grad_by_ones`) in place of the rectifier-masked streaming kernel, whose mask is wrong for an output that may
be negative.  Plain rectifiers where the paper has leaky ones (the contraction kernels carry only the rectifier); the
policies' own initialisers, drawn from a private np.random.RandomState(rnd_seed): constructing RND moves nobody else's
random numbers.

Around the trunks: arl_rnd_obs_stats (running per-pixel moments), arl_rnd_obs_prepare (the normalised, clamped input),
arl_rnd_error (the bonus, and with it the predictor's loss and gradient).  csrc/rnd.hip; include/accel_rl_hip.h states
every expression and order."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy
from accel_rl_amd.spaces import Discrete, EnvSpec, UintBox
from accel_rl_amd.util import seed as _seed

STATE_KEYS = ("target", "predictor", "obs_count", "obs_mean", "obs_m2", "rew_moments", "rho")


class _RndTrunk(AtariCnnPolicy):
    """AtariCnnPolicy's trunk with a linear last dense layer and no output layers; initial values from `rng`."""

    _u8_conv1 = False
    serves_rows = False

    def __init__(self, rng, dense_sizes, **conv_args):
        super().__init__(hidden_sizes=dense_sizes, **conv_args)
        self._rng = rng

    def initialize(self, env_spec, device=None, **kwargs):
        # the conv initialiser draws from the layer RNG (util/seed.py): ours for the length of this call
        saved, _seed._layer_rng = _seed._layer_rng, self._rng
        try:
            super().initialize(env_spec, device=device, **kwargs)
        finally:
            _seed._layer_rng = saved

    def _hidden_reference_init(self, fan):
        ref, names, self._hid_geom = [], [], []
        for i, hs in enumerate(self.hidden_sizes):
            if hs % 4:
                raise NotImplementedError("dense sizes must be multiples of 4 (got %d)" % hs)
            w = self._rng.randn(fan, hs).astype(np.float32)             # NormCInit(1.0), as the policies' dense layers
            w *= 1.0 / np.sqrt(np.square(w).sum(axis=0, keepdims=True))
            ref += [w, np.zeros(hs, np.float32)]
            names += ["FC%dW" % i, "FC%db" % i]
            self._hid_geom.append((hs, fan))
            fan = hs
        return ref, names, fan

    def _head_reference_init(self, fan, n_act):
        return [], []

    def _head_internal_shapes(self, fan, n_act):
        return []

    def _head_to_internal(self, ref_tail):
        return []

    def _trunk(self, x, w=None, tag=""):
        """AtariCnnPolicy._trunk whose last dense layer keeps its sign: hids[-1] is the embedding."""
        b = x.shape[0]
        w = self._w if w is None else w
        _, dense_g = self._layer_geoms(b)
        acts = self._convs(x, w, tag)
        hids, k, a = [], 2 * self._n_conv, acts[-1]
        for j, (hs, fan_in) in enumerate(self._hid_geom):
            hcur = self._buffer(("hid" + tag, j, b), (b, hs))
            _lib.conv2d_fwd(a, w[k], w[k + 1], hcur, dense_g[j], j + 1 < self._n_hid, self._conv_ws)
            hids.append(hcur)
            a = hcur
            k += 2
        return acts, hids

    def _bias_grad_left(self, d, y, rows, channels, k):
        if k == 2 * (self._n_conv + self._n_hid - 1):       # the linear layer: column sums of d as they are
            self._bias_grad_by_ones(d, rows, k)
        else:
            super()._bias_grad_left(d, y, rows, channels, k)


class RndNetwork(object):

    def __init__(self, conv_filters=(32, 64, 64), conv_filter_sizes=(8, 4, 3), conv_strides=(4, 2, 1),
                 conv_pads=((0, 0), (0, 0), (0, 0)), embedding_size=512, predictor_hidden=(512, 512), rnd_seed=0):
        if not (isinstance(embedding_size, (int, np.integer)) and not isinstance(embedding_size, bool) and
                4 <= embedding_size <= 1024 and embedding_size % 4 == 0):
            raise ValueError("embedding_size must be a multiple of 4 in 4 .. 1024, got %r" % (embedding_size,))
        if any((not isinstance(h, (int, np.integer))) or isinstance(h, bool) or h < 4 or h % 4 for h in predictor_hidden):
            raise ValueError("predictor_hidden: multiples of 4, got %r" % (predictor_hidden,))
        if not (isinstance(rnd_seed, (int, np.integer)) and not isinstance(rnd_seed, bool) and 0 <= rnd_seed < 2 ** 32):
            raise ValueError("rnd_seed must be an integer in 0 .. 2^32 - 1, got %r" % (rnd_seed,))
        self.embedding_size, self.predictor_hidden, self.rnd_seed = int(embedding_size), tuple(predictor_hidden), int(rnd_seed)
        self._conv_args = dict(conv_filters=conv_filters, conv_filter_sizes=conv_filter_sizes, conv_strides=conv_strides,
                               conv_pads=conv_pads)

    def initialize(self, env_spec, n_env, device=None):
        """env_spec: the policy's (the frame is one H x W plane of its observations); n_env: length of `rho`."""
        c, h, w = env_spec.observation_space.shape
        rng = np.random.RandomState(self.rnd_seed)
        frame = EnvSpec(UintBox((1, h, w)), Discrete(1))
        self.target = _RndTrunk(rng, [self.embedding_size], **self._conv_args)
        self.target.initialize(frame, device=device)
        self.predictor = _RndTrunk(rng, list(self.predictor_hidden) + [self.embedding_size], **self._conv_args)
        self.predictor.initialize(frame, device=device)
        dev = self.device = self.predictor.device
        self._frame_hw, self.n_env = (h, w), int(n_env)
        f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)     # noqa: E731
        self.obs_count, self.obs_mean, self.obs_m2 = f64(1), f64(h * w), f64(h * w)
        self.rew_moments, self.rho = f64(3), f64(self.n_env)
        self._stats_ws = _lib.rnd_obs_stats_workspace(h, w, dev)
        self._rows = dict()

    # ---- the predictor's bucket, for its optimiser
    flat_params = property(lambda self: self.predictor.flat_params)
    flat_grads = property(lambda self: self.predictor.flat_grads)

    def _horizon(self, observations):
        rows = observations.shape[0]
        if rows % self.n_env:
            raise ValueError("%d observation rows are no whole number of steps of %d envs" % (rows, self.n_env))
        return rows // self.n_env

    def update_obs_stats(self, observations, extra_observations):
        _lib.rnd_obs_stats(observations, extra_observations, self.n_env, self._horizon(observations), self.obs_count,
                           self.obs_mean, self.obs_m2, self._stats_ws)

    def _input(self, observations, extra_observations, idx, b):
        h, w = self._frame_hw
        x = self.predictor._buffer(("rnd_x", b), (b, h, w, 4))
        _lib.rnd_obs_prepare(observations, extra_observations, idx, self.n_env, self._horizon(observations),
                             self.obs_count, self.obs_mean, self.obs_m2, x)
        return x

    def _all_rows(self, n):
        rows = self._rows.get(n)
        if rows is None:
            rows = self._rows[n] = torch.arange(n, dtype=torch.int32, device=self.device)
        return rows

    def errors(self, observations, extra_observations, err, rows_per_pass=None):
        """The bonus pass: err f32[n_env * horizon] <- the predictor's mean squared error on every row's frame, in passes
        of at most rows_per_pass rows (None: one pass) so that the scratch activations are bounded.  Rows are independent:
        the passes compute what one pass computes."""
        with torch.no_grad():
            n = observations.shape[0]
            step = n if not rows_per_pass else min(n, int(rows_per_pass))
            for lo in range(0, n, step):
                hi = min(lo + step, n)
                idx = None if hi - lo == n else self._all_rows(n)[lo:hi]
                x = self._input(observations, extra_observations, idx, hi - lo)
                _, t_hids = self.target._trunk(x)
                _, p_hids = self.predictor._trunk(x)
                _lib.rnd_error(p_hids[-1], t_hids[-1], err[lo:hi])
            return err

    def loss_and_grads(self, observations, extra_observations, idx=None):
        """One training pass on rows idx (None: all): the mean squared error between the two embeddings and its gradient
        into the predictor's flat gradient bucket (overwritten).  Returns the loss, a device f32[1]."""
        with torch.no_grad():
            b = observations.shape[0] if idx is None else idx.shape[0]
            x = self._input(observations, extra_observations, idx, b)
            _, t_hids = self.target._trunk(x)
            acts, hids = self.predictor._trunk(x)
            buf = self.predictor._buffer
            err, loss = buf(("rnd_err", b), (b,)), buf(("rnd_loss", b), (1,))
            dpred = buf(("rnd_dpred", b), (b, self.embedding_size))
            _lib.rnd_error(hids[-1], t_hids[-1], err, dpred, loss)
            self.predictor._backward_trunk(x, acts, hids, dpred, masked=True)
            return loss

    # ---- everything RND carries across iterations, as NumPy arrays
    def _state_tensors(self):
        return dict(target=self.target.flat_params, predictor=self.predictor.flat_params, obs_count=self.obs_count,
                    obs_mean=self.obs_mean, obs_m2=self.obs_m2, rew_moments=self.rew_moments, rho=self.rho)

    def rnd_state(self):
        return {k: t.detach().cpu().numpy().copy() for k, t in self._state_tensors().items()}

    def set_rnd_state(self, state):
        tensors = self._state_tensors()
        if sorted(state) != sorted(tensors):
            raise ValueError("set_rnd_state: keys %s, expected %s" % (sorted(state), sorted(tensors)))
        for k, t in tensors.items():
            a = np.asarray(state[k])
            if a.shape != tuple(t.shape) or a.dtype != np.dtype(str(t.dtype).split(".")[1]):
                raise ValueError("set_rnd_state: %s is %s %s, expected %s %s" % (k, a.dtype, a.shape, t.dtype, tuple(t.shape)))
        for k, t in tensors.items():
            t.copy_(torch.from_numpy(np.ascontiguousarray(state[k])))
        self.target.note_params_changed()
        self.predictor.note_params_changed()
