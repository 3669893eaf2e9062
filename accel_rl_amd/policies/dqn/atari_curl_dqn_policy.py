"""DQN policy with CURL's contrastive auxiliary loss on the conv stack (Srinivas, Laskin, Abbeel 2020, "CURL: Contrastive
Unsupervised Representations for Reinforcement Learning"; the reference has none): AtariDqnPolicy plus

    z_q = conv stack(view 0) W_p + b_p                      f32[B][D]   queries: the online encoder, one dense MFMA call
    z_k = momentum conv stack(view 1) W_p' + b_p'           f32[B][D]   keys: the momentum encoder, constants
    S   = z_q W z_k^T,  L = coef mean_i (logsumexp_j S_ij - S_ii)       (csrc/curl.hip: arl_curl_loss_parts, one launch)

Three more tensors in the policy's own bucket, behind the output layer in construction order, in the flat bucket and in
get_param_values: the projection W_p (F, D), b_p (D) and the bilinear form W (D, D) in the reference layout.  They are
stored (d_stride, F), (d_stride,) and (d_stride, d_stride), d_stride = D rounded up to 32 with zeros (and zero gradients) in
the padding; W_p's fan-in axis is in the conv output's NHWC-flatten order, converted like the first dense layer's.  The
target bucket carries an unused copy of them, which keeps update_target and snapshots those of QPolicyBase.

The momentum encoder is `flat_momentum`: a copy of the conv tensors followed by a copy of (W_p, b_p), equal to the online
values after initialize / set_param_values and moved by momentum_step (arl_acer_avg_step) after every update.

The backward pass has ONE conv-stack backward: the projection's data gradient, already multiplied by the rectifier mask of
the last conv activation, joins the dense layers' (masked) data gradient at the seam in front of _backward_convs.
"""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import _norm_c
from accel_rl_amd.policies.dqn.atari_dqn_policy import AtariDqnPolicy

LATENT_MAX = 128                # arl_curl_loss_parts: ARL_CURL_MAX_WIDTH


class AtariCurlDqnPolicy(AtariDqnPolicy):

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(), pixel_scale=255.,
                 epsilon=1, dueling=False, shared_last_bias=False, latent=128, initial_param_values=None):
        if not (isinstance(latent, (int, np.integer)) and 4 <= latent <= LATENT_MAX and latent % 4 == 0):
            raise ValueError("latent must be a multiple of 4 in 4 .. %d (arl_curl_loss_parts), got %r" % (LATENT_MAX, latent))
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, epsilon=epsilon, dueling=dueling, shared_last_bias=shared_last_bias,
                         initial_param_values=initial_param_values)
        self.latent = int(latent)
        self._d_stride = (self.latent + 31) // 32 * 32
        self._seam_grad = None
        self.curl_diag = None               # (contrastive loss, accuracy) of the last curl_loss_and_grads call (device)

    # ---- the three tensors behind the output layer (construction order) ------------------------------------------
    def _head_reference_init(self, fan, n_act):
        head, names = super()._head_reference_init(fan, n_act)
        self._n_head_ref = len(head)
        co, ho, wo = self._conv_out
        d = self.latent
        extra = [_norm_c((co * ho * wo, d), 1.0), np.zeros(d, np.float32), np.random.rand(d, d).astype(np.float32)]
        return head + extra, names + ["CurlProjW", "CurlProjb", "CurlW"]

    def _head_internal_shapes(self, fan, n_act):
        co, ho, wo = self._conv_out
        s = self._d_stride
        return super()._head_internal_shapes(fan, n_act) + [(s, co * ho * wo), (s,), (s, s)]

    def _head_to_internal(self, ref_tail):
        d, s = self.latent, self._d_stride
        wp_ref, bp_ref, w_ref = ref_tail[-3:]
        wp = np.zeros((s, wp_ref.shape[0]), np.float32)
        bp = np.zeros(s, np.float32)
        w = np.zeros((s, s), np.float32)
        wp[:d] = self._conv_flat_to_internal(wp_ref)
        bp[:d] = bp_ref
        w[:d, :d] = w_ref
        return super()._head_to_internal(ref_tail[:-3]) + [wp, bp, w]

    # (the dueling permutation of the reference's flat order covers the tensors before these three: they stay behind)
    def _tail_to_flat(self, tail):
        n = len(tail) if self._tail_perm is None else len(self._tail_perm)
        return super()._tail_to_flat(tail[:n]) + list(tail[n:])

    def _tail_from_flat(self, tail):
        n = len(tail) if self._tail_perm is None else len(self._tail_perm)
        return super()._tail_from_flat(tail[:n]) + list(tail[n:])

    def bucket_to_reference(self, flat):
        arr = self._internal_arrays(flat)
        d, k = self.latent, self._k_proj
        extra = [self._conv_flat_to_reference(arr[k][:d]), arr[k + 1][:d], arr[k + 2][:d, :d]]
        return np.concatenate([super().bucket_to_reference(flat)] +
                              [np.ascontiguousarray(x).reshape(-1) for x in extra]).astype(np.float32)

    @property
    def _k_proj(self):
        return self._k_head + 2

    # ---- the momentum encoder --------------------------------------------------------------------------------------
    def initialize(self, env_spec, device=None, **kwargs):
        super().initialize(env_spec, device=device, **kwargs)
        k = self._k_proj
        n_conv = self.grad_split_offset                     # the conv tensors lead the bucket
        p0, p1 = self._offsets[k], self._offsets[k + 2]     # W_p and b_p are adjacent
        self._mom_ranges = [(0, 0, n_conv), (n_conv, p0, p1 - p0)]      # (offset in flat_momentum, in flat_params, count)
        self.flat_momentum = torch.empty(n_conv + p1 - p0, dtype=torch.float32, device=self.device)
        sizes = [int(np.prod(s)) for s in self._shapes]
        self._w_mom = [None] * len(self._shapes)            # the layers' (W, b) views _convs and the projection read
        for i in list(range(2 * self._n_conv)) + [k, k + 1]:
            o = self._offsets[i] if i < k else n_conv + self._offsets[i] - p0
            self._w_mom[i] = self.flat_momentum[o:o + sizes[i]]
        self._curl_ws = _lib.curl_workspace(self._d_stride, self.device)
        self.sync_momentum()

    def sync_momentum(self):
        """The momentum encoder <- the online encoder (what initialize and set_param_values leave)."""
        for om, op, n in self._mom_ranges:
            self.flat_momentum[om:om + n].copy_(self.flat_params[op:op + n])

    def momentum_step(self, tau):
        """momentum <- (1 - tau) momentum + tau online, as arl_acer_avg_step states it (alpha = 1 - tau)."""
        for om, op, n in self._mom_ranges:
            _lib.acer_avg_step(self.flat_momentum[om:om + n], self.flat_params[op:op + n], 1. - tau)

    def _set_from_reference_arrays(self, ref):
        super()._set_from_reference_arrays(ref)
        if getattr(self, "flat_momentum", None) is not None:
            self.sync_momentum()

    # ---- training --------------------------------------------------------------------------------------------------
    def _proj_geom(self, b):
        key = ("curl_proj", b, _lib.default_route)
        if key not in self._geoms:
            co, ho, wo = self._conv_out
            self._geoms[key] = _lib.dense_geom(b, co * ho * wo, self._d_stride)
        return self._geoms[key]

    def _backward_convs(self, x, acts, d_act, masked=False, corun=None):
        """The seam: the projection's masked data gradient on the last conv activation joins the dense layers'."""
        extra, self._seam_grad = self._seam_grad, None
        if extra is not None:
            assert masked, "the dense layers hand their data gradient on masked"
            d_act.view(-1).add_(extra.view(-1))
        super()._backward_convs(x, acts, d_act, masked, corun=corun)

    def curl_loss_and_grads(self, obs, next_obs, actions, returns, terminals, is_weights, gamma_n, delta_clip, double_dqn,
                            coef):
        """One minibatch of CURL.build_loss: obs holds two shifted views of each of the B samples, view-major, next_obs
        one (FrameReplayBuffer(augment=...), m_online = 2, k_targets = 1).  The Q loss is q_loss_and_grads' on view 0; the
        queries are view 0's last conv activation through the projection, the keys view 1 through the momentum convs and
        the momentum projection; arl_curl_loss_parts gives coef * InfoNCE with dzq and the bilinear form's gradient; the
        projection's backward (weight, bias, masked data gradient) is one launch, and the conv stack runs its backward
        once on the sum of both data gradients.  Returns (loss_rows f32[B] whose sum is the Q loss, td_abs f32[B]) as
        q_loss_and_grads; `curl_diag` f32[2 of 4] = (coef * contrastive loss, accuracy) stays on the policy.  No host
        synchronisation and no allocation outside _buffer: it runs inside the captured update graph."""
        b = actions.numel()
        if obs.shape[0] != 2 * b or next_obs.shape[0] != b:
            raise ValueError("curl_loss_and_grads: obs / next_obs must hold 2 B = %d / B = %d rows (got %d / %d)" %
                             (2 * b, b, obs.shape[0], next_obs.shape[0]))
        with torch.no_grad():
            x, q, acts, hids, tgt_q, pol_next = self._forward_for_loss(obs[:b], next_obs, double_dqn)
            k, s, geom = self._k_proj, self._d_stride, self._proj_geom(b)
            zq = self._buffer(("curl_zq", b), (b, s))
            _lib.conv2d_fwd(acts[-1], self._w[k], self._w[k + 1], zq, geom, False, self._conv_ws)
            acts_k = self._convs(self._scaled(obs[b:], tag="k"), w=self._w_mom, tag="k")
            zk = self._buffer(("curl_zk", b), (b, s))
            _lib.conv2d_fwd(acts_k[-1], self._w_mom[k], self._w_mom[k + 1], zk, geom, False, self._conv_ws)
            dzq = self._buffer(("curl_dzq", b), (b, s))
            diag = self._buffer(("curl_diag",), (4,))
            self._folds.curl_loss(zq, zk, self._w[k + 2], coef, dzq, self._g[k + 2], diag, self._curl_ws)
            self.curl_diag = diag
            # the projection: weight gradient with the bias gradient riding along, data gradient times the rectifier mask
            d_proj = self._buffer(("curl_dx", b), tuple(acts[-1].shape))
            done = self._folds.conv2d_bwd_pair(dzq, self._w[k], acts[-1], d_proj, acts[-1], self._g[k], geom,
                                               self._fold_ws(("dw", k)), dbias=self.grads[k + 1])
            if not done:        # generic kernels
                self._bias_grad_by_ones(dzq, b, k)
            self._seam_grad = d_proj

            def launch(dq, loss_rows, td_abs):
                _lib.dqn_loss(q, tgt_q, pol_next, actions, returns, terminals, is_weights, self.n_act, gamma_n,
                              delta_clip, dq, loss_rows, td_abs, dueling=self._dueling)

            try:
                return self._loss_and_backward(x, q, acts, hids, launch)
            finally:
                self._seam_grad = None
