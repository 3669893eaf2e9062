"""Noisy-net DQN policy for Atari: conv stack -> noisy dense layers -> one Q value per action; a target network;
exploration through learned per-weight noise scales instead of epsilon-greedy.

Mirror of the reference's AtariNoisyNetDqnPolicy / NoisyNetDqnCnn / NoisyDenseLayer
(accel_rl/policies/dqn/atari_noisy_net_dqn_policy.py:20-148, policies/dqn/networks/noisy_net_dqn_cnn.py:11-137,
policies/dqn/layers/noisy_layer.py:15-147; the reference's policy file imports a network module that does not exist,
the network built here is NoisyNetDqnCnn).  Every hidden dense layer and the output layer "output_q" is a noisy layer
with factorized Gaussian noise:

    y = x W + b + f(e_out) * ((x * f(e_in)) W_sigma + b_sigma),   f(e) = sgn(e) sqrt(|e|)

(= x (W + W_sigma * f(e_in) f(e_out)^T) + b + b_sigma * f(e_out) without a per-row weight matrix).  Every forward pass
draws fresh noise on the device: one arl_noisy_noise launch after the conv stack writes every noisy layer's f(e_in),
f(e_out) and x * f(e_in) of the first one; per layer two dense MFMA launches (x W, (x f(e_in)) W_sigma, split partial sums
left unfolded) and one arl_noisy_dense_combine launch that folds both, applies the noise, bias and rectifier and writes
the next layer's h * f(e_in); the output layer's combine advances the pass counter.  common_noise=False (the default,
Noisy-DQN): every row draws its own noise; common_noise=True: one draw per call shared by its rows -- the online
network's two loss passes (obs, next_obs) run as one 2B-row pass that counts as two calls.  The seed and the call counter
live in a device buffer (`_noise_state`), so a replayed hipGraph (rollout, update) draws fresh noise, the same sequence
as eager calls would.  Policy and target network share that one generator.

Backward per noisy layer (top down): arl_noisy_dense_bwd_prep (g2 = g f(e_out), db, db_sigma), two arl_conv2d_bwd_pair
launches (dW = g^T x with g W, dW_sigma = g2^T (x f(e_in)) with g2 W_sigma, both masked by the rectifier below, weight
folds deferred to the pass's one arl_fold_many) and arl_noisy_dense_bwd_dx (dx = g W + f(e_in) g2 W_sigma).

Parameters, in the reference's flat order (Lasagne add_param order per layer): the conv layers, then per noisy layer
W (fan_in, units), b, W_sigma (fan_in, units), b_sigma -- FC0W, FC0b, FC0Wsigma, FC0bsigma, ..., OutputW, Outputb,
OutputWsigma, Outputbsigma.  Internally W_sigma has W's layout ((units, fan_in); the output layer padded to 32 rows whose
weights and gradients stay exactly zero) and the output layer's sigma pair sits before its W, b in the bucket.

Initialisation, in the reference's draw order: the noise seed np.random.randint(1, 123456) first
(atari_noisy_net_dqn_policy.py:44), the conv layers' Glorot weights, then per noisy layer its NormCInit W (np.random)
and -- use_mu_init -- uniform(-v, v) for W and then for b, v = sqrt(1 / fan_in), from Lasagne's RNG (get_rng(); here
util.seed.layer_rng(), which also stands in for it in GlorotUniform) (noisy_layer.py:64-69); W_sigma and b_sigma the
constant sigma_0 / sqrt(fan_in) (:72).  The target network is a copy (no draws of its own), as for AtariDqnPolicy.

No epsilon: get_epsilon() is 0, set_epsilon is a no-op and no action call draws from np.random (:144-148).

Not built: factorized=False (per-row independent noise, B x fan_in x units normals per
call), dueling and categorical variants (the reference has none).
"""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import ObsRows, _norm_c
from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy
from accel_rl_amd.util.seed import layer_rng


class AtariNoisyNetDqnPolicy(AtariDqnPolicy):

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(), pixel_scale=255.,
                 epsilon=1, factorized=True, common_noise=False, sigma_0=0.4, use_mu_init=True,
                 initial_param_values=None, dueling=False, shared_last_bias=False):
        if not factorized:
            raise NotImplementedError("noisy layers with independent (non-factorized) noise are not built "
                                      "(INTEGRATION.md, section E)")
        if dueling or shared_last_bias:
            raise NotImplementedError("noisy dueling / shared-bias networks are not built (INTEGRATION.md, section E)")
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, epsilon=0, initial_param_values=initial_param_values)
        self.factorized, self.common_noise = True, bool(common_noise)
        self.sigma_0, self.use_mu_init = float(sigma_0), bool(use_mu_init)

    def initialize(self, env_spec, device=None, **kwargs):
        self.noise_seed = int(np.random.randint(1, 123456))      # atari_noisy_net_dqn_policy.py:44, before any weight
        n = 4 * len(self.hidden_sizes)
        # construction order [hidden layers' 4 each..., Output Wsigma, bsigma, Output W, b] -> the reference's flat order
        self._tail_perm = list(range(n)) + [n + 2, n + 3, n, n + 1]
        super().initialize(env_spec, device=device, **kwargs)
        self._noise_state = torch.tensor([self.noise_seed, 0], dtype=torch.int64, device=self.device)
        self._sigma_ws = _lib.conv_workspace(self.device)
        self._noise_of = dict()

    # ---- parameters ------------------------------------------------------------
    def _noisy_init(self, fan, units, norm):
        """One NoisyDenseLayer's W, b in the reference's draw order (noisy_layer.py:58-72)."""
        w = _norm_c((fan, units), norm)
        b = np.zeros(units, np.float32)
        if self.use_mu_init:
            v = np.sqrt(1 / fan)
            w = layer_rng().uniform(-v, v, w.shape).astype(np.float32)
            b = layer_rng().uniform(-v, v, b.shape).astype(np.float32)
        s = np.float32(self.sigma_0 / np.sqrt(fan))
        return [w, b, np.full((fan, units), s, np.float32), np.full(units, s, np.float32)]

    def _hidden_reference_init(self, fan):
        ref, names, self._hid_geom = [], [], []
        for i, hs in enumerate(self.hidden_sizes):
            if hs % 4:
                raise NotImplementedError("hidden sizes must be multiples of 4 (got %d)" % hs)
            ref += self._noisy_init(fan, hs, 1.0)
            names += ["FC%dW" % i, "FC%db" % i, "FC%dWsigma" % i, "FC%dbsigma" % i]
            self._hid_geom.append((hs, fan))
            fan = hs
        out = self._noisy_init(fan, self.n_act, 0.01)         # output_q (noisy_net_dqn_cnn.py:78-89)
        self._out_ref = out[:2]
        return ref + out[2:], names + ["OutputWsigma", "Outputbsigma"], fan

    def _head_reference_init(self, fan, n_act):
        self._q_stride = (n_act + 31) // 32 * 32
        return list(self._out_ref), ["OutputW", "Outputb"]

    def _hidden_internal_shapes(self):
        shapes = [s for hs, fan_in in self._hid_geom for s in ((hs, fan_in), (hs,), (hs, fan_in), (hs,))]
        return shapes + [(self._q_stride, self._hid_geom[-1][0]), (self._q_stride,)]

    def _hidden_to_reference(self, arrs):
        out = []
        for j in range(len(self._hid_geom)):
            w, b, ws, bs = arrs[4 * j:4 * j + 4]
            if j == 0:
                out += [self._conv_flat_to_reference(w), b, self._conv_flat_to_reference(ws), bs]
            else:
                out += [w.T, b, ws.T, bs]
        a, n = self.n_act, 4 * len(self._hid_geom)
        return out + [arrs[n][:a].T, arrs[n + 1][:a]]

    def _hidden_to_internal(self, refs):
        out = []
        for j in range(len(self._hid_geom)):
            w, b, ws, bs = refs[4 * j:4 * j + 4]
            if j == 0:
                out += [self._conv_flat_to_internal(w), b, self._conv_flat_to_internal(ws), bs]
            else:
                out += [w.T, b, ws.T, bs]
        a, n = self.n_act, 4 * len(self._hid_geom)
        ws = np.zeros((self._q_stride, refs[n].shape[0]), np.float32)
        bs = np.zeros(self._q_stride, np.float32)
        ws[:a], bs[:a] = refs[n].T, refs[n + 1]
        return out + [ws, bs]

    def _k_hidden(self, j):
        """Index of hidden layer j's W in params / grads (b, W_sigma, b_sigma follow)."""
        return 2 * self._n_conv + 4 * j

    @property
    def _k_out_sigma(self):
        return self._k_head - 2

    # ---- forward -----------------------------------------------------------
    def _convs(self, x, w, tag):
        b = x.shape[0]
        conv_g, _ = self._layer_geoms(b)
        acts, a = [], x
        for i, (nf, ci, sz, st, pad, ho, wo) in enumerate(self._conv_geom):
            z = self._buffer(("act" + tag, i, b), (b, ho, wo, nf))
            if isinstance(a, ObsRows):
                _lib.conv2d_u8_fwd(a.obs, a.idx, self._scale, w[0], w[1], z, conv_g[0], True)
            else:
                _lib.conv2d_fwd(a, w[2 * i], w[2 * i + 1], z, conv_g[i], True, self._conv_ws)
            acts.append(z)
            a = z
        return acts

    def _noise_layers(self, b, tag):
        """[(fan_in, units, out_stride, (fein, feout, xs))] of every noisy layer for a pass of b rows (scratch)."""
        geo = [(fan_in, hs, hs) for hs, fan_in in self._hid_geom] + [(self._hid_geom[-1][0], self.n_act, self._q_stride)]
        out = []
        for l, (fan_in, units, stride) in enumerate(geo):
            bufs = (self._buffer(("fein" + tag, l, b), (b, fan_in)), self._buffer(("feout" + tag, l, b), (b, stride)),
                    self._buffer(("xs" + tag, l, b), (b, fan_in)))
            out.append((fan_in, units, stride, bufs))
        return out

    def _rows_per_draw(self, b, tag):
        if not self.common_noise:
            return 1
        return b // 2 if tag == "2" else b        # tag "2": the online network's obs + next_obs pass = two calls

    def _logits(self, x, w=None, tag="", parts_ws=None):
        """[B, q_stride] noisy Q values (+ the trunk's activations); one fresh noise draw per call."""
        if parts_ws is not None:
            raise NotImplementedError("the noisy output layer folds its own partial sums")
        w = self._w if w is None else w
        b = x.shape[0]
        _, dense_g = self._layer_geoms(b)
        acts = self._convs(x, w, tag)
        layers = self._noise_layers(b, tag)
        _lib.noisy_noise(self._noise_state,
                         [(fein, feout, acts[-1] if l == 0 else None, xs, fan_in, units, stride, l)
                          for l, (fan_in, units, stride, (fein, feout, xs)) in enumerate(layers)],
                         b, self._rows_per_draw(b, tag))
        geoms = list(dense_g) + [self._head_geom(b)]
        ks = [self._k_hidden(j) for j in range(self._n_hid)] + [self._k_head]
        ksig = [k + 2 for k in ks[:-1]] + [self._k_out_sigma]
        hids, a = [], acts[-1]
        for l, (fan_in, units, stride, (fein, feout, xs)) in enumerate(layers):
            last = l == self._n_hid
            k, ks_ = ks[l], ksig[l]
            yw = self._buffer(("nyw" + tag, l, b), (b, stride))
            ys = self._buffer(("nys" + tag, l, b), (b, stride))
            it_w = _lib.conv2d_fwd_parts(a, w[k], w[k + 1], yw, geoms[l], False, self._conv_ws)
            it_s = _lib.conv2d_fwd_parts(xs, w[ks_], w[ks_ + 1], ys, geoms[l], False, self._sigma_ws)
            y = self._buffer(("logits" + tag, b) if last else ("hid" + tag, l, b), (b, stride))
            nxt = None if last else layers[l + 1][3]
            _lib.noisy_dense_combine(it_w, w[k + 1], it_s, w[ks_ + 1], feout, y, not last,
                                     fein_next=None if last else nxt[0], xs_next=None if last else nxt[2],
                                     state=self._noise_state if last else None)
            if not last:
                hids.append(y)
            a = y
        self._noise_of[hids[-1].data_ptr()] = [bufs for _, _, _, bufs in layers]
        return a, acts, hids

    # ---- acting: greedy on the noisy Q values, no host randomness ---------------
    def host_draws(self, horizon, n_envs, n_groups=2):
        """No epsilon (atari_noisy_net_dqn_policy.py:144-148): an all-greedy override table, and no np.random draw."""
        self._select_overrides(horizon, n_envs, lambda: (
            None, torch.full((horizon, n_envs), -1, dtype=torch.int32, device=self.device)))
        return np.full(horizon * n_envs, 0.5)

    def get_actions(self, observations, deterministic=False):
        return self.greedy_actions(observations).cpu().numpy(), dict()

    def get_action(self, observation, deterministic=False):
        return int(self.greedy_actions(observation[None])[0].item()), dict()

    def get_epsilon(self):
        return 0.

    def set_epsilon(self, value):
        pass

    def munchausen_loss_and_grads(self, *args, **kwargs):
        raise NotImplementedError("a noisy Munchausen agent is not built (INTEGRATION.md, section E)")

    # ---- training: the noisy layers' backward, then the conv stack's ----------------
    def _head_backward(self, dout, x, acts, hids):
        b = x.shape[0]
        _, dense_g = self._layer_geoms(b)
        noise = self._noise_of[hids[-1].data_ptr()]            # this pass's noise (rows 0..b-1: the obs rows)
        folds, g = self._folds, self.grads
        d = dout
        for l in range(self._n_hid, -1, -1):
            last = l == self._n_hid
            k = self._k_head if last else self._k_hidden(l)
            ks_ = self._k_out_sigma if last else k + 2
            geom = self._head_geom(b) if last else dense_g[l]
            inp = hids[l - 1] if l > 0 else acts[-1]
            fein, feout, xs = (t[:b] for t in noise[l])
            units = d.shape[1]
            g2 = self._buffer(("ng2", l, b), (b, units))
            _lib.noisy_dense_bwd_prep(d, feout, g2, g[k + 1], g[ks_ + 1])
            fan_in = fein.shape[1]
            dxw = self._buffer(("ndxw", l, b), (b, fan_in))
            dxs = self._buffer(("ndxs", l, b), (b, fan_in))
            folds.conv2d_bwd_pair(d, self._w[k], inp, dxw, inp, self._g[k], geom, self._fold_ws(("dw", k)))
            folds.conv2d_bwd_pair(g2, self._w[ks_], inp, dxs, xs, self._g[ks_], geom, self._fold_ws(("dw", ks_)))
            _lib.noisy_dense_bwd_dx(dxw, dxs, fein, dxw)
            d = dxw
        self._backward_convs(x, acts, d.view(acts[-1].shape), masked=True)
