"""The noisy dense layers that AtariNoisyNetDqnPolicy and AtariNoisyNetCatDqnPolicy share: their parameters, their
forward walk and their backward pass (host code; the kernels are csrc/noisy.hip).

The reference's NoisyDenseLayer (accel_rl/policies/dqn/layers/noisy_layer.py:15-147) with factorized Gaussian noise:

    y = x W + b + f(e_out) * ((x * f(e_in)) W_sigma + b_sigma),   f(e) = sgn(e) sqrt(|e|)

(= x (W + W_sigma * f(e_in) f(e_out)^T) + b + b_sigma * f(e_out) without a per-row weight matrix).  Every hidden dense
layer and the output layer of a noisy policy is such a layer.

Forward (`_noisy_pass`): the conv stack; one noise launch (the policy's `_draw_noise`) that writes every noisy layer's
f(e_in), f(e_out) and x * f(e_in) of the first one; per layer two dense MFMA launches (x W, (x f(e_in)) W_sigma, split
partial sums left unfolded) and one arl_noisy_dense_combine launch that folds both, applies the noise, bias and
rectifier and writes the next layer's h * f(e_in).  The output layer's combine advances the pass counter; a pass that
leaves its output layer to a loss launch (defer_output) advances it in its last hidden combine.

Generator: the seed and the call counter live in a device buffer (`_noise_state`), so a replayed hipGraph (rollout,
update) draws fresh noise, the same sequence as eager calls would.  Policy and target network share that one generator.
common_noise=False (the default, Noisy-DQN): every row draws its own noise; common_noise=True: one draw per call shared
by its rows -- the online network's two loss passes (obs, next_obs) run as one 2B-row pass that counts as two calls.

Backward per noisy layer (top down, `_head_backward`): arl_noisy_dense_bwd_prep (g2 = g f(e_out), db, db_sigma), two
arl_conv2d_bwd_pair launches (dW = g^T x with g W, dW_sigma = g2^T (x f(e_in)) with g2 W_sigma, both masked by the
rectifier below, weight folds deferred to the pass's one arl_fold_many) and arl_noisy_dense_bwd_dx
(dx = g W + f(e_in) g2 W_sigma).

Parameters, in the reference's flat order (Lasagne add_param order per layer): the conv layers, then per noisy layer
W (fan_in, units), b, W_sigma (fan_in, units), b_sigma -- FC0W, FC0b, FC0Wsigma, FC0bsigma, ..., OutputW, Outputb,
OutputWsigma, Outputbsigma.  Internally W_sigma has W's layout (the policy's `_head_*` hooks for the output layer: its
padding's weights and gradients stay exactly zero) and the output layer's sigma pair sits before its W, b in the bucket.

Initialisation, in the reference's draw order: the noise seed np.random.randint(1, 123456) first
(atari_noisy_net_dqn_policy.py:44), the conv layers' Glorot weights, then per noisy layer its NormCInit W (np.random)
and -- use_mu_init -- uniform(-v, v) for W and then for b, v = sqrt(1 / fan_in), from Lasagne's RNG (get_rng(); here
util.seed.layer_rng(), which also stands in for it in GlorotUniform) (noisy_layer.py:64-69); W_sigma and b_sigma the
constant sigma_0 / sqrt(fan_in) (:72).  The target network is a copy (no draws of its own).

No epsilon: get_epsilon() is 0, set_epsilon is a no-op and no action call draws from np.random (:144-148).
"""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import _norm_c
from accel_rl_amd.util.seed import layer_rng


class NoisyLayers(object):
    """Mixin in front of a QPolicyBase subclass.  The policy gives `_out_units()`, the `_head_*` layout hooks and
    `_draw_noise(x_c, layers, b, tag)`, its noise launch; a dueling policy overrides the hooks whose non-dueling form
    is here."""

    def _set_noisy(self, factorized, common_noise, sigma_0, use_mu_init):
        if not factorized:
            raise NotImplementedError("noisy layers with independent (non-factorized) noise are not built "
                                      "(INTEGRATION.md, section E)")
        self.factorized, self.common_noise = True, bool(common_noise)
        self.sigma_0, self.use_mu_init = float(sigma_0), bool(use_mu_init)

    def initialize(self, env_spec, device=None, **kwargs):
        self.noise_seed = int(np.random.randint(1, 123456))      # atari_noisy_net_dqn_policy.py:44, before any weight
        if not self._dueling:
            n = 4 * len(self.hidden_sizes)
            # construction order [hidden layers' 4 each..., Output Wsigma, bsigma, Output W, b] -> the reference's flat order
            self._tail_perm = list(range(n)) + [n + 2, n + 3, n, n + 1]
        super().initialize(env_spec, device=device, **kwargs)
        self._noise_state = torch.tensor([self.noise_seed, 0], dtype=torch.int64, device=self.device)
        self._sigma_ws = _lib.conv_workspace(self.device)
        self._out_ws = dict()             # pass tag -> (W, W_sigma) workspaces of a deferred output layer
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
        out = self._noisy_init(fan, self._out_units(), 0.01)      # the output layer; its W, b: _head_reference_init
        self._out_ref = out[:2]
        return ref + out[2:], names + ["OutputWsigma", "Outputbsigma"], fan

    def _hidden_internal_shapes(self):
        shapes = [s for hs, fan_in in self._hid_geom for s in ((hs, fan_in), (hs,), (hs, fan_in), (hs,))]
        return shapes + self._head_internal_shapes(self._hid_geom[-1][0], self.n_act)

    def _dense_to(self, w, j, to_ref):
        if j == 0:
            return self._conv_flat_to_reference(w) if to_ref else self._conv_flat_to_internal(w)
        return w.T

    def _hidden_to_reference(self, arrs):
        out = []
        for j in range(len(self._hid_geom)):
            w, b, ws, bs = arrs[4 * j:4 * j + 4]
            out += [self._dense_to(w, j, True), b, self._dense_to(ws, j, True), bs]
        n = 4 * len(self._hid_geom)
        return out + self._head_to_reference(arrs[n], arrs[n + 1])

    def _hidden_to_internal(self, refs):
        out = []
        for j in range(len(self._hid_geom)):
            w, b, ws, bs = refs[4 * j:4 * j + 4]
            out += [self._dense_to(w, j, False), b, self._dense_to(ws, j, False), bs]
        n = 4 * len(self._hid_geom)
        return out + self._head_to_internal(refs[n:n + 2])

    def _k_hidden(self, j):
        """Index of hidden layer j's W in params / grads (b, W_sigma, b_sigma follow)."""
        return 2 * self._n_conv + 4 * j

    @property
    def _k_out_sigma(self):
        return self._k_head - 2

    # ---- forward -----------------------------------------------------------
    def _rows_per_draw(self, b, tag):
        if not self.common_noise:
            return 1
        return b // 2 if tag == "2" else b        # tag "2": the online network's obs + next_obs pass = two calls

    def _noise_buffers(self, b, tag):
        """This pass's noise buffers (scratch): (fein, feout, xs) per noisy layer of the internal network."""
        t = "n" + tag
        geo = [(fan_in, hs) for hs, fan_in in self._hid_geom] + [(self._hid_geom[-1][0], self._head_width)]
        return [tuple(self._buffer((t, l, k, b), (b, n)) for k, n in enumerate((fan_in, units, fan_in)))
                for l, (fan_in, units) in enumerate(geo)]

    def _hidden_forward(self, a, w, layers, b, tag, defer_output):
        """The hidden noisy layers on a = the conv output [B, fan_in]; returns their activations."""
        _, dense_g = self._layer_geoms(b)
        hids = []
        for l, (hs, fan_in) in enumerate(self._hid_geom):
            fein, feout, xs = layers[l]
            k = self._k_hidden(l)
            yw = self._buffer(("nyw" + tag, l, b), (b, hs))
            ys = self._buffer(("nys" + tag, l, b), (b, hs))
            it_w = _lib.conv2d_fwd_parts(a, w[k], w[k + 1], yw, dense_g[l], False, self._conv_ws)
            it_s = _lib.conv2d_fwd_parts(xs, w[k + 2], w[k + 3], ys, dense_g[l], False, self._sigma_ws)
            y = self._buffer(("hid" + tag, l, b), (b, hs))
            last_hid = l + 1 == self._n_hid
            _lib.noisy_dense_combine(it_w, w[k + 1], it_s, w[k + 3], feout, y, True, fein_next=layers[l + 1][0],
                                     xs_next=layers[l + 1][2],
                                     state=self._noise_state if (defer_output and last_hid) else None)
            hids.append(y)
            a = y
        return hids

    def _noisy_pass(self, x, w, tag, defer_output):
        """Convs, noise, hidden layers, the output layer's two products.  Returns (output, acts, hids): output = the
        [B, head width] noisy output layer, or -- defer_output -- (W item, W_sigma item, f(e_out), b, b_sigma) for the
        loss launch to fold (the pass's counter then advances in its last hidden combine)."""
        b = x.shape[0]
        acts = self._convs(x, w, tag)
        x_c = acts[-1].view(b, -1)
        layers = self._noise_buffers(b, tag)
        self._draw_noise(x_c, layers, b, tag)
        hids = self._hidden_forward(x_c, w, layers, b, tag, defer_output)
        # the output layer: x W and (x f(e_in)) W_sigma; folded here or (defer_output) by the loss launch
        _, feout, xs = layers[-1]
        k, ks_ = self._k_head, self._k_out_sigma
        geom = self._head_geom(b)
        if defer_output:
            if tag not in self._out_ws:
                self._out_ws[tag] = (_lib.conv_workspace(self.device), _lib.conv_workspace(self.device))
            ws_w, ws_s = self._out_ws[tag]
        else:
            ws_w, ws_s = self._conv_ws, self._sigma_ws
        yw = self._buffer(("nyw" + tag, "out", b), (b, self._head_width))
        ys = self._buffer(("nys" + tag, "out", b), (b, self._head_width))
        it_w = _lib.conv2d_fwd_parts(hids[-1], w[k], w[k + 1], yw, geom, False, ws_w)
        it_s = _lib.conv2d_fwd_parts(xs, w[ks_], w[ks_ + 1], ys, geom, False, ws_s)
        self._noise_of[hids[-1].data_ptr()] = layers
        if defer_output:
            return (it_w, it_s, feout, w[k + 1], w[ks_ + 1]), acts, hids
        out = self._buffer(("logits" + tag, b), (b, self._head_width))
        _lib.noisy_dense_combine(it_w, w[k + 1], it_s, w[ks_ + 1], feout, out, False, state=self._noise_state)
        return out, acts, hids

    def _logits(self, x, w=None, tag="", parts_ws=None):
        """[B, head width] noisy output layer (+ the trunk's activations); one fresh noise draw per call."""
        if parts_ws is not None:
            raise NotImplementedError("the noisy output layer folds its own partial sums")
        return self._noisy_pass(x, self._w if w is None else w, tag, False)

    # ---- acting: greedy on the noisy output, no host randomness ---------------
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
