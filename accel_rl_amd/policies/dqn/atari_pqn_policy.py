"""Q-network of PQN (Gallici et al. 2024, "Simplifying Deep Temporal Difference Learning"; the reference has none):
AtariDqnPolicy's network with LayerNorm + rectifier after every conv layer and every hidden dense layer -- what keeps
Q-learning stable without a target network --, the output layer plain.  As the authors' implementation (as recalled:
the paper is not at hand) a conv activation is normalised over its channel axis, a dense one over its units.

  forward :  every contraction runs WITHOUT its rectifier (bias only), one arl_ln_relu_fwd per layer follows
             (csrc/layernorm.hip); the pre-normalisation output z and (mean, rstd) per row are kept for the backward pass
  backward:  the data-gradient launches hand over d loss / d y already multiplied by y > 0 (y = relu(LN(z)): still the
             right mask); one arl_ln_relu_bwd per layer (AtariCnnPolicy._through_activation) turns it, in place, into
             d loss / d z and leaves the partial sums of dgamma / dbeta to the pass's one fold launch; the layer's
             weight-gradient launch then carries its bias gradient as for every other policy.

Parameters: gamma / beta of every normalised layer live in the flat bucket -- the conv layers' right behind the conv
(W, b) tensors, so that everything before `grad_split_offset` still belongs to the conv stack, the dense layers' at its
end -- and in get / set_param_values behind the output layer: Conv<i>LNg, Conv<i>LNb, .., FC<j>LNg, FC<j>LNb
(gamma = 1, beta = 0 at initialisation).  QPolicyBase's target bucket is kept (update_target, target_q work) but PQN
reads none.  Serving, epsilon-greedy draws, evaluation and the host twins are QPolicyBase's, on `_logits`.
"""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import ObsRows
from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy

LN_MAX_WIDTH = 1024         # arl_ln_relu_fwd / _bwd: 4 <= width <= 1024, width % 4 == 0


class AtariPqnPolicy(AtariDqnPolicy):

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(), pixel_scale=255.,
                 epsilon=1, dueling=False, shared_last_bias=False, ln_eps=1e-5, initial_param_values=None):
        if dueling:
            raise NotImplementedError("AtariPqnPolicy: no dueling network (INTEGRATION.md, section E)")
        if shared_last_bias:
            raise NotImplementedError("AtariPqnPolicy: no shared output bias (INTEGRATION.md, section E)")
        if not list(hidden_sizes):
            raise NotImplementedError("AtariPqnPolicy: at least one hidden dense layer is required (INTEGRATION.md, "
                                      "section E)")
        for width in list(conv_filters) + list(hidden_sizes):
            if width < 4 or width > LN_MAX_WIDTH or width % 4:
                raise NotImplementedError("AtariPqnPolicy: normalised widths (conv filters, hidden units) must be multiples "
                                          "of 4 in 4 .. %d, got %d (INTEGRATION.md, section E)" % (LN_MAX_WIDTH, width))
        if not (np.isfinite(ln_eps) and ln_eps > 0):
            raise ValueError("ln_eps must be finite and > 0")
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, epsilon=epsilon, initial_param_values=initial_param_values)
        self._ln_eps = float(ln_eps)
        self._ln_saved = dict()             # (tag, layer) -> (z, stats) of the latest forward pass

    # ---- parameters: (gamma, beta) per normalised layer, tensors k_ln + 2 L, k_ln + 2 L + 1 (L: conv layers, then dense)
    def _ln_layers(self):
        return ([("Conv%d" % i, nf) for i, nf in enumerate(self.conv_filters)] +
                [("FC%d" % j, hs) for j, hs in enumerate(self.hidden_sizes)])

    def _head_reference_init(self, fan, n_act):
        ref, names = super()._head_reference_init(fan, n_act)
        for name, width in self._ln_layers():
            ref += [np.ones(width, np.float32), np.zeros(width, np.float32)]
            names += [name + "LNg", name + "LNb"]
        return ref, names

    def _head_internal_shapes(self, fan, n_act):
        return super()._head_internal_shapes(fan, n_act) + [(width,) for _, width in self._ln_layers() for _ in range(2)]

    def _head_to_internal(self, ref_tail):
        return super()._head_to_internal(ref_tail[:2]) + [np.asarray(a, np.float32) for a in ref_tail[2:]]

    def _bucket_order(self, n):
        n_conv2, k_ln = 2 * len(self._conv_geom), self._k_head + 2
        return (list(range(n_conv2)) + list(range(k_ln, k_ln + n_conv2)) + list(range(n_conv2, k_ln)) +
                list(range(k_ln + n_conv2, n)))

    def bucket_to_reference(self, flat):
        arr = self._internal_arrays(flat)
        return np.concatenate([super().bucket_to_reference(flat)] +
                              [a.reshape(-1) for a in arr[self._k_head + 2:]]).astype(np.float32)

    def initialize(self, env_spec, device=None, **kwargs):
        super().initialize(env_spec, device=device, **kwargs)
        self._k_ln = self._k_head + 2
        # one workspace per layer: the column-sum partials stay live until the backward pass's fold launch
        self._ln_ws = [_lib.ln_bwd_workspace(self.device) for _ in self._ln_layers()]

    # ---- forward: contraction (bias, no rectifier) -> LayerNorm + rectifier ------------------------------------------
    def _ln_relu(self, z, layer, w, tag, b):
        k = self._k_head + 2 + 2 * layer
        y = self._buffer(("act" + tag, layer, b), tuple(z.shape))
        stats = self._buffer(("ln_stats" + tag, layer, b), (z.numel() // z.shape[-1], 2))
        _lib.ln_relu_fwd(z, w[k], w[k + 1], self._ln_eps, y, stats)
        self._ln_saved[(tag, layer)] = (z, stats)
        return y

    def _convs(self, x, w=None, tag=""):
        b = x.shape[0]
        w = self._w if w is None else w
        conv_g, _ = self._layer_geoms(b)
        acts, a = [], x
        for i, (nf, ci, sz, st, pad, ho, wo) in enumerate(self._conv_geom):
            z = self._buffer(("pre" + tag, i, b), (b, ho, wo, nf))
            if isinstance(a, ObsRows):
                _lib.conv2d_u8_fwd(a.obs, a.idx, self._scale, w[0], w[1], z, conv_g[0], False)
            else:
                _lib.conv2d_fwd(a, w[2 * i], w[2 * i + 1], z, conv_g[i], False, self._conv_ws)
            a = self._ln_relu(z, i, w, tag, b)
            acts.append(a)
        return acts

    def _trunk(self, x, w=None, tag=""):
        b = x.shape[0]
        w = self._w if w is None else w
        _, dense_g = self._layer_geoms(b)
        acts = self._convs(x, w, tag)
        hids, k, a = [], 2 * self._n_conv, acts[-1]
        for j, (hs, fan_in) in enumerate(self._hid_geom):
            z = self._buffer(("prehid" + tag, j, b), (b, hs))
            _lib.conv2d_fwd(a, w[k], w[k + 1], z, dense_g[j], False, self._conv_ws)
            a = self._ln_relu(z, self._n_conv + j, w, tag, b)
            hids.append(a)
            k += 2
        return acts, hids

    def q_rows(self, observations, rows_per_pass=None, tag="rows"):
        """f32 [n, q_stride]: the current network on u8 observations [n, C, H, W], apart from the training pass's
        activations; in passes of rows_per_pass rows (None: one pass) so that a whole rollout fits the scratch buffers of
        one.  `tag` names the scratch and the result: two calls whose results must live together take two tags."""
        with torch.no_grad():
            n = observations.shape[0]
            step = n if not rows_per_pass else min(n, int(rows_per_pass))
            if step == n:
                return self._logits(self._scaled(observations, tag=tag), tag=tag)[0]
            out = self._buffer(("q_rows" + tag, n), (n, self._q_stride))
            for lo in range(0, n, step):
                rows = observations[lo:min(lo + step, n)]
                out[lo:lo + rows.shape[0]].copy_(self._logits(self._scaled(rows, tag=tag), tag=tag)[0])
            return out

    # ---- training ----------------------------------------------------------------------------------------------------
    def _through_activation(self, layer, d, masked, y):
        """d = d loss / d y (masked: already times y > 0) -> d loss / d z in place; dgamma / dbeta join the pending folds."""
        z, stats = self._ln_saved[("", layer)]
        k = self._k_ln + 2 * layer
        if self._folds._n + 6 > _lib.FOLD_MAX_ITEMS:        # (a deep network: the fold list is full before the pass ends)
            self._folds.run()
        self._folds.ln_relu_bwd(d, y, z, stats, self._w[k], masked, d, self.grads[k], self.grads[k + 1], self._ln_ws[layer])
        return d, True

    def _bias_grad_left(self, d, y, rows, channels, k):
        # d is the gradient of the layer's pre-normalisation output: the rectifier's mask does not apply to it
        self._bias_grad_by_ones(d.view(rows, channels), rows, k)

    def pqn_loss_and_grads(self, obs, idx, actions, returns, delta_clip, out=None):
        """One minibatch of PQN: forward on the rows obs[idx] (idx None: all; u8 rows are read in place by conv 1), the
        regression loss of Q(obs)[action] on returns[idx] (csrc/dqn.hip:arl_q_regress_loss; delta_clip None: squared) and
        the full backward pass into flat_grads.  actions / returns are full-batch arrays, rows selected by idx.
        Returns (loss_rows f32[B] whose sum is the loss, td_abs f32[B]), the two rows of one (2, B) buffer (`out`, when
        given).  No host synchronisation and no allocation outside _buffer: it runs inside the captured update graph."""
        with torch.no_grad():
            x = self._scaled(obs, idx)
            q, acts, hids = self._logits(x)
            b = q.shape[0]
            dq = self._buffer(("dlogits", b), tuple(q.shape))
            pack = self._buffer(("loss_td", b), (2, b)) if out is None else out
            _lib.q_regress_loss(q, idx, actions, returns, self.n_act, delta_clip, dq, pack[0], pack[1])
            self._backward_from_dq(dq, x, acts, hids)
            return pack[0], pack[1]

    def _replay_loss_refused(self, *args, **kwargs):
        raise NotImplementedError("AtariPqnPolicy trains through pqn_loss_and_grads (algos/dqn/pqn.py), not a replay loss "
                                  "(INTEGRATION.md, section E)")

    q_loss_and_grads = drq_loss_and_grads = munchausen_loss_and_grads = _replay_loss_refused
