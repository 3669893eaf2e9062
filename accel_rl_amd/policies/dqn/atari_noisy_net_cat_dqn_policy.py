"""Noisy-net categorical ("C51") DQN policy for Atari -- the network of a full Rainbow: conv stack -> noisy dense layers ->
n_actions x n_atoms logits (dueling: + a value stream), softmax over atoms per action; a target network; exploration
through learned per-weight noise scales instead of epsilon-greedy.

The reference's CatDqnCnn (accel_rl/policies/dqn/networks/catdqn_cnn.py:40-99) with every DenseLayer replaced by its
NoisyDenseLayer (policies/dqn/layers/noisy_layer.py:15-147, factorized): the hidden layers, "action_atoms" and, dueling,
"hidden_Val_0" and "Val".  Softmax over atoms and the dueling merge are AtariCatDqnPolicy's (csrc/dqn.hip).  The noisy
layer, its forward walk, backward pass, generator, parameter order and initial draws are NoisyLayers'
(policies/dqn/noisy_layers.py); this file holds the dueling arms, the noise launch and the fused loss.  Which
(layer, which, element range) of the generator each e_in / e_out is: include/accel_rl_hip.h, above arl_noisy_draw.

Internal layout (AtariCatDqnPolicy / QPolicyBase): the output matrix has n_actions (+ 1 value) rows of atoms, each padded
to `atom_stride`; dueling stacks the two streams' hidden layers into ONE 2H layer and their output layers into ONE
block-structured matrix.  W_sigma has W's layout, padding and dueling mask (off-block and padding entries and their
gradients stay exactly zero).  Per pass: one arl_noisy_draws launch; the dueling hidden layer has one sigma product per
stream, each with its own f(e_in), folded by arl_noisy_duel_combine into its own columns; the stacked output layer needs
no such split: its block-structured W_sigma reads the advantage half of x f(e_in) for the advantage rows and the value
half for the value row.  The update's two output-layer combines and the logits round trip can be folded into the loss
launch (arl_noisy_catdqn_loss_parts, `loss_folds_heads`, off by default; a product past the launch's split limit takes
the unfused pair: the combines, then arl_catdqn_loss).

Dueling parameters in the reference's flat order (value branch first): FCVal0*, Val*, FC0*, Output*; initial draws in
construction order hidden_0, action_atoms, hidden_Val_0, Val.  Serving is arl_catdqn_act on the noisy logits.
"""
import os

import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import ObsRows
from accel_rl_amd.policies.dqn.atari_cat_dqn_policy import AtariCatDqnPolicy
from accel_rl_amd.policies.dqn.noisy_layers import NoisyLayers


class AtariNoisyNetCatDqnPolicy(NoisyLayers, AtariCatDqnPolicy):

    # True: the update's output-layer combines and the loss run as one arl_noisy_catdqn_loss_parts launch (same bits).
    # Off by default: on the MI355X the fused launch is the slower one (LABNOTES.md, "Noisy Rainbow"): it re-folds every
    # logit from the split partial sums each time a lane reads it, serially, where the combine launches fold each once
    # across the whole chip.  ARL_NOISY_LOSS_FUSED=1 (the env switch: same-box A/B) turns it on.
    loss_folds_heads = os.environ.get("ARL_NOISY_LOSS_FUSED", "0") != "0"

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(), pixel_scale=255.,
                 n_atoms=51, dueling=False, common_noise=False, sigma_0=0.4, use_mu_init=True, factorized=True,
                 initial_param_values=None):
        self._set_noisy(factorized, common_noise, sigma_0, use_mu_init)
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, epsilon=0, n_atoms=n_atoms, dueling=dueling,
                         initial_param_values=initial_param_values)
        if not len(self.hidden_sizes):
            raise NotImplementedError("the noisy categorical network is built with at least one hidden layer")

    def initialize(self, env_spec, device=None, **kwargs):
        if self._dueling:
            # construction order [FC0 x4, FCVal0 x4, Output Wsigma, bsigma, Val Wsigma, bsigma, Output W, b, Val W, b]
            # -> the reference's flat order (value branch first)
            self._tail_perm = [4, 5, 6, 7, 14, 15, 10, 11, 0, 1, 2, 3, 12, 13, 8, 9]
        super().initialize(env_spec, device=device, **kwargs)
        self._sigma_ws2 = _lib.conv_workspace(self.device) if self._dueling else None
        self.fused_max_splits = _lib.noisy_catdqn_loss_limits()[0]

    # ---- parameters: the dueling arms ------------------------------------------
    def _hidden_reference_init(self, fan):
        if not self._dueling:
            return super()._hidden_reference_init(fan)        # hidden..., action_atoms (catdqn_cnn.py:67-74)
        hs = self.hidden_sizes[0]
        if hs % 4:
            raise NotImplementedError("hidden sizes must be multiples of 4 (got %d)" % hs)
        hid = self._noisy_init(fan, hs, 1.0)                # construction order: hidden_0, action_atoms,
        out = self._noisy_init(hs, self._out_units(), 0.01)  # hidden_Val_0, Val (catdqn_cnn.py:58-93)
        hid_val = self._noisy_init(fan, hs, 1.0)
        val = self._noisy_init(hs, self.n_atoms, 0.01)
        self._duel_head_ref = out[:2] + val[:2]
        self._hid_geom = [(2 * hs, fan)]
        names = ["FC0W", "FC0b", "FC0Wsigma", "FC0bsigma", "FCVal0W", "FCVal0b", "FCVal0Wsigma", "FCVal0bsigma",
                 "OutputWsigma", "Outputbsigma", "ValWsigma", "Valbsigma"]
        return hid + hid_val + out[2:] + val[2:], names, 2 * hs

    def _head_reference_init(self, fan, n_act):
        while (self._rows * self._atom_stride) % 32 and self._atom_stride < 64:     # AtariCatDqnPolicy's padding
            self._atom_stride += 4
        if self._dueling:
            return list(self._duel_head_ref), ["OutputW", "Outputb", "ValW", "Valb"]
        return list(self._out_ref), ["OutputW", "Outputb"]

    def _hidden_to_reference(self, arrs):
        if not self._dueling:
            return super()._hidden_to_reference(arrs)
        hs = self.hidden_sizes[0]
        w, b, ws, bs = arrs[:4]
        out = []
        for rows in (slice(0, hs), slice(hs, 2 * hs)):
            out += [self._dense_to(w[rows], 0, True), b[rows], self._dense_to(ws[rows], 0, True), bs[rows]]
        return out + self._head_to_reference(arrs[4], arrs[5])

    def _hidden_to_internal(self, refs):
        if not self._dueling:
            return super()._hidden_to_internal(refs)
        out = [np.concatenate([self._dense_to(refs[i], 0, False), self._dense_to(refs[i + 4], 0, False)], axis=0)
               if i % 2 == 0 else np.concatenate([refs[i], refs[i + 4]]) for i in range(4)]
        return out + self._head_to_internal(refs[8:12])

    # ---- forward: the noise launch and the dueling arms -------------------------
    def _duel_sigma_geom(self, b):
        key = ("duel_sigma", b, _lib.default_route)
        if key not in self._geoms:
            hs2, fan = self._hid_geom[0]
            self._geoms[key] = _lib.dense_geom(b, fan, hs2 // 2)
        return self._geoms[key]

    def _noise_buffers(self, b, tag):
        """Dueling: the stacked hidden layer's (fein_adv, fein_val, feout, xs_adv, xs_val) and the stacked output
        layer's (fein, feout, xs)."""
        if not self._dueling:
            return super()._noise_buffers(b, tag)
        t = "n" + tag
        two_h, fan = self._hid_geom[0]
        hid = tuple(self._buffer((t, 0, k, b), (b, n)) for k, n in enumerate((fan, fan, two_h, fan, fan)))
        out = tuple(self._buffer((t, 1, k, b), (b, n)) for k, n in enumerate((two_h, self._head_width, two_h)))
        return [hid, out]

    def _draw_noise(self, x_c, layers, b, tag):
        """One arl_noisy_draws launch: every e_in / e_out of the pass (the statement: include/accel_rl_hip.h)."""
        if self._dueling:
            (fa, fv, fo_h, xa, xv), (fi_o, fo_o, _) = layers
            two_h, fan = self._hid_geom[0]
            h, a_s, s = two_h // 2, self.n_act * self._atom_stride, self._atom_stride
            w_o = self._head_width
            draws = [(fa, x_c, xa, fan, fan, 0, 0), (fo_h[:, :h], None, None, h, two_h, 0, 1),
                     (fi_o[:, :h], None, None, h, two_h, 1, 0), (fo_o[:, :a_s], None, None, a_s, w_o, 1, 1),
                     (fv, x_c, xv, fan, fan, 2, 0), (fo_h[:, h:], None, None, h, two_h, 2, 1),
                     (fi_o[:, h:], None, None, h, two_h, 3, 0), (fo_o[:, a_s:], None, None, s, w_o, 3, 1)]
        else:
            draws = []
            for l, (fein, feout, xs) in enumerate(layers):
                fan_in, units = fein.shape[1], feout.shape[1]
                draws += [(fein, x_c if l == 0 else None, xs if l == 0 else None, fan_in, fan_in, l, 0),
                          (feout, None, None, units, units, l, 1)]
        _lib.noisy_draws(self._noise_state, draws, b, self._rows_per_draw(b, tag))

    def _hidden_forward(self, a, w, layers, b, tag, defer_output):
        """Dueling: the stacked hidden layer -- one W product, one sigma product per stream, one combine."""
        if not self._dueling:
            return super()._hidden_forward(a, w, layers, b, tag, defer_output)
        _, dense_g = self._layer_geoms(b)
        fa, fv, fo_h, xa, xv = layers[0]
        fi_o, _, xs_o = layers[1]
        two_h, fan = self._hid_geom[0]
        h = two_h // 2
        k = self._k_hidden(0)
        yw = self._buffer(("nyw" + tag, 0, b), (b, two_h))
        ys_lo, ys_hi = (self._buffer(("nys" + tag, 0, i, b), (b, h)) for i in range(2))
        it_w = _lib.conv2d_fwd_parts(a, w[k], w[k + 1], yw, dense_g[0], False, self._conv_ws)
        sg = self._duel_sigma_geom(b)
        it_lo = _lib.conv2d_fwd_parts(xa, w[k + 2][:h * fan], w[k + 3][:h], ys_lo, sg, False, self._sigma_ws)
        it_hi = _lib.conv2d_fwd_parts(xv, w[k + 2][h * fan:], w[k + 3][h:], ys_hi, sg, False, self._sigma_ws2)
        y = self._buffer(("hid" + tag, 0, b), (b, two_h))
        _lib.noisy_duel_combine(it_w, w[k + 1], it_lo, it_hi, w[k + 3], fo_h, y, h, True, fein_next=fi_o,
                                xs_next=xs_o, state=self._noise_state if defer_output else None)
        return [y]

    def _fold_output(self, deferred, rows, out):
        """The unfused path for a deferred output layer: its combine (the counter already advanced)."""
        it_w, it_s, feout, bias, b_sigma = deferred
        _lib.noisy_dense_combine(it_w, bias, it_s, b_sigma, feout[:rows], out, False)

    # ---- training ------------------------------------------------------------
    def fused_loss_takes(self, deferred):
        """Whether arl_noisy_catdqn_loss_parts takes these output-layer products (its limits; else the unfused pair)."""
        return all(it.splits <= self.fused_max_splits for d in deferred for it in d[:2])

    def cat_loss_and_grads(self, obs, next_obs, actions, returns, terminals, is_weights, v_min, v_max, gamma_n,
                           double_dqn=False):
        """CategoricalDQN.build_loss (cat_dqn.py:40-109) through the noisy network; returns (loss_rows, kl) f32[B].
        Double DQN from u8 rows (the Rainbow path): the target pass and the online obs + next_obs pass leave their output
        layers unfolded, and one arl_noisy_catdqn_loss_parts launch folds, noises and takes the loss."""
        if not (self.loss_folds_heads and double_dqn and self._u8):
            return super().cat_loss_and_grads(obs, next_obs, actions, returns, terminals, is_weights, v_min, v_max,
                                              gamma_n, double_dqn=double_dqn)
        with torch.no_grad():
            b = obs.shape[0]
            both = self._pair_rows(obs, next_obs)
            tgt, _, _ = self._noisy_pass(ObsRows(both[b:], None), self._w_target, "t", True)
            on, acts2, hids2 = self._noisy_pass(ObsRows(both, None), self._w, "2", True)
            r = self._head_width
            dlogits = self._buffer(("dlogits", b), (b, r))
            pack = self._buffer(("loss_kl", b), (2, b))
            loss_rows, kl = pack[0], pack[1]
            if self.fused_loss_takes((tgt, on)):
                srcs = [_lib.noisy_logit_src(it_w, bias, it_s, bs, fo, row0, r)
                        for (it_w, it_s, fo, bias, bs), row0 in ((on, 0), (tgt, 0), (on, b))]
                wts = self._dgrad_weight_items(b) if os.environ.get("ARL_WT_IN_LOSS", "1") != "0" else []
                _lib.noisy_catdqn_loss_parts(srcs[0], srcs[1], srcs[2], self.z, actions, returns, terminals,
                                             is_weights, self.n_act, self.n_atoms, self._atom_stride, v_min, v_max,
                                             gamma_n, dlogits, loss_rows, kl, dueling=self._dueling, dgrad_weights=wts)
                self._wt_fresh = bool(wts)
            else:
                tgt_logits = self._buffer(("logitst", b), (b, r))
                logits2 = self._buffer(("logits2", 2 * b), (2 * b, r))
                self._fold_output(tgt, b, tgt_logits)
                self._fold_output(on, 2 * b, logits2)
                _lib.catdqn_loss(logits2[:b], tgt_logits, logits2[b:], self.z, actions, returns, terminals,
                                 is_weights, self.n_act, self.n_atoms, v_min, v_max, gamma_n, dlogits, loss_rows, kl,
                                 dueling=self._dueling)
            try:
                self._head_backward(dlogits, ObsRows(both[:b], None), [a[:b] for a in acts2], [h[:b] for h in hids2])
            finally:
                self._wt_fresh = False
            return loss_rows, kl

    def _head_backward(self, dout, x, acts, hids):
        """Dueling: the stacked hidden layer's two sigma products each get their own g2 block and data gradient."""
        if not self._dueling:
            return super()._head_backward(dout, x, acts, hids)
        b = x.shape[0]
        _, dense_g = self._layer_geoms(b)
        (fa, fv, fo_h, xa, xv), (fi_o, fo_o, xs_o) = [[t[:b] for t in lay] for lay in self._noise_of[hids[-1].data_ptr()]]
        folds, g = self._folds, self.grads
        two_h, fan = self._hid_geom[0]
        h = two_h // 2
        # output layer (block-structured over the stacked 2H hidden units)
        k, ks_ = self._k_head, self._k_out_sigma
        geom = self._head_geom(b)
        g2 = self._buffer(("ng2", 1, b), tuple(dout.shape))
        _lib.noisy_dense_bwd_prep(dout, fo_o, g2, g[k + 1], g[ks_ + 1])
        dxw = self._buffer(("ndxw", 1, b), (b, two_h))
        dxs = self._buffer(("ndxs", 1, b), (b, two_h))
        folds.conv2d_bwd_pair(dout, self._w[k], hids[0], dxw, hids[0], self._g[k], geom, self._fold_ws(("dw", k)))
        folds.conv2d_bwd_pair(g2, self._w[ks_], hids[0], dxs, xs_o, self._g[ks_], geom, self._fold_ws(("dw", ks_)))
        _lib.noisy_dense_bwd_dx(dxw, dxs, fi_o, dxw)
        # stacked hidden layer: one W product, one sigma product per stream
        k = self._k_hidden(0)
        g2_lo, g2_hi = (self._buffer(("ng2", 0, i, b), (b, h)) for i in range(2))
        _lib.noisy_duel_bwd_prep(dxw, fo_h, h, g2_lo, g2_hi, g[k + 1], g[k + 3])
        inp = acts[-1]
        d0 = self._buffer(("ndxw", 0, b), (b, fan))
        ds_lo, ds_hi = (self._buffer(("ndxs", 0, i, b), (b, fan)) for i in range(2))
        sg = self._duel_sigma_geom(b)
        folds.conv2d_bwd_pair(dxw, self._w[k], inp, d0, inp, self._g[k], dense_g[0], self._fold_ws(("dw", k)))
        folds.conv2d_bwd_pair(g2_lo, self._w[k + 2][:h * fan], inp, ds_lo, xa, self._g[k + 2][:h * fan], sg,
                              self._fold_ws(("dw", k + 2, 0)))
        folds.conv2d_bwd_pair(g2_hi, self._w[k + 2][h * fan:], inp, ds_hi, xv, self._g[k + 2][h * fan:], sg,
                              self._fold_ws(("dw", k + 2, 1)))
        _lib.noisy_duel_bwd_dx(d0, ds_lo, fa, ds_hi, fv, d0)
        self._backward_convs(x, acts, d0.view(acts[-1].shape), masked=True)
        # the folds have run: keep the absent blocks' gradients (W and W_sigma) at exactly zero
        self.grads[self._k_head].mul_(self._duel_mask)
        self.grads[self._k_out_sigma].mul_(self._duel_mask)
