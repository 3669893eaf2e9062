"""An LRU memory policy: conv stack -> embedding -> one linear recurrent unit over TIME -> (softmax pi, linear V).  The
layer is the LRU of Orvieto et al. 2023 -- a diagonal complex linear recurrence with the stable exponential
parametrisation and the ring initialisation --, reset inside the scan the way S5 is used in RL (Lu et al. 2023); neither
paper is at hand and the reference has no such policy: one layer, no LayerNorm, no gating.

    e_t   = relu(xf_t W_x + b_x)                      [E], xf_t = the conv stack's flattened output
    u_t   = e_t W_b                                   [N] complex: column 2 j = re, 2 j + 1 = im of channel j
    lam_j = exp(-exp(nu_j) + i theta_j) ;  gam_j = sqrt(1 - |lam_j|^2)
    h_t   = keep_t (lam (.) h_(t-1)) + gam (.) u_t    keep_t = 0 right after a reset
    y_t   = relu(e_t + hflat_t W_c + b_o)  ->  AtariCnnPolicy's policy / value head

The recurrent state is one tensor per environment, "lru_0" [n_env, 2 N]: the N complex channels as interleaved (re, im)
pairs, zeros at the start and after a reset; in training the stored state is a constant.

The recurrence is elementwise, so every dense product is one all-rows contraction outside it (AtariCnnPolicy's,
csrc/mfma_conv.hip) and the recurrence itself is one csrc/lru.hip launch per direction at any horizon up to 1 024:
arl_lru_fwd / arl_lru_bwd, then arl_lru_param_fold for nu and theta.  Serving is arl_lru_fwd at T = 1 in place on the
state.  arl_lru_params runs at the head of every forward, so a captured update sees the stepped parameters.

Parameters after the convs, in network order: LruWx (fan, E), LruBx, LruNu (N), LruTheta (N), LruWb (E, 2 N), LruWc
(2 N, E), LruBo; then the output layers.
"""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import _norm_c
from accel_rl_amd.policies.atari_lstm_policy import RecurrentCnnPolicy

_NAMES = ["LruWx", "LruBx", "LruNu", "LruTheta", "LruWb", "LruWc", "LruBo"]


def _refuse(msg):
    raise NotImplementedError("AtariLruPolicy: %s (INTEGRATION.md, section E)" % msg)


class AtariLruPolicy(RecurrentCnnPolicy):

    _state_keys = ("lru_0",)

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(256,), state_size=128,
                 r_min=0.9, r_max=0.999, max_phase=np.pi / 10, pixel_scale=255., alternating_sampler=False,
                 initial_param_values=None):
        if not isinstance(state_size, (int, np.integer)) or isinstance(state_size, bool):
            _refuse("state_size must be an integer, got %r" % (state_size,))
        if len(hidden_sizes) != 1 or hidden_sizes[0] < 4 or hidden_sizes[0] % 4:
            _refuse("exactly one hidden size, the embedding width, a multiple of 4; got %r" % (tuple(hidden_sizes),))
        if not _lib.lru_shape_ok(1, state_size):
            _refuse("state_size even in 2 .. %d, got %r" % (_lib.LRU_MAX_STATE, state_size))
        if not (0. <= r_min < r_max < 1. and 0. < max_phase <= 2 * np.pi):
            _refuse("0 <= r_min < r_max < 1 and 0 < max_phase <= 2 pi; got %r, %r, %r" % (r_min, r_max, max_phase))
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, initial_param_values=initial_param_values)
        self.state_size, self._ring = int(state_size), (float(r_min), float(r_max), float(max_phase))
        self._state_w = 2 * self.state_size

    def serve_supported(self):
        return False

    # ---- parameters ----------------------------------------------------------------------------------------------------
    def _hidden_reference_init(self, fan):
        e, n, (r_min, r_max, max_phase) = self._H, self.state_size, self._ring
        self._hid_geom, self._rec_fan = [], fan
        w_x = _norm_c((fan, e), 1.0)
        # the ring initialisation: |lam| with lam uniform on the ring r_min <= |lam| <= r_max, the phase in [0, max_phase]
        mag2 = np.random.uniform(size=n) * (r_max ** 2 - r_min ** 2) + r_min ** 2
        nu = np.log(-0.5 * np.log(np.maximum(mag2, 1e-30))).astype(np.float32)
        theta = (np.random.uniform(size=n) * max_phase).astype(np.float32)
        return ([w_x, np.zeros(e, np.float32), nu, theta, _norm_c((e, 2 * n), 1.0), _norm_c((2 * n, e), 1.0),
                 np.zeros(e, np.float32)], list(_NAMES), e)

    def _hidden_internal_shapes(self):
        e, n = self._H, self.state_size
        return [(e, self._rec_fan), (e,), (n,), (n,), (2 * n, e), (e, 2 * n), (e,)]

    def _hidden_to_reference(self, a):
        return [self._conv_flat_to_reference(a[0]), a[1], a[2], a[3], a[4].T, a[5].T, a[6]]

    def _hidden_to_internal(self, r):
        return [self._conv_flat_to_internal(r[0]), r[1], r[2], r[3], r[4].T, r[5].T, r[6]]

    def reference_layout(self, obs_shape, n_act):
        """[(name, shape)] of get_param_values' tensors for observations (c, h, w) and n_act actions; needs no device."""
        c, h, w = obs_shape
        out = []
        for i, (nf, sz, st, pad) in enumerate(zip(self.conv_filters, self.conv_filter_sizes, self.conv_strides,
                                                  self.conv_pads)):
            out += [("Conv%dW" % i, (nf, c, sz, sz)), ("Conv%db" % i, (nf,))]
            c, h, w = nf, (h + 2 * pad[0] - sz) // st + 1, (w + 2 * pad[1] - sz) // st + 1
        e, n = self._H, self.state_size
        out += zip(_NAMES, [(c * h * w, e), (e,), (n,), (n,), (e, 2 * n), (2 * n, e), (e,)])
        return out + [("OutputW", (e, n_act)), ("Outputb", (n_act,)), ("OutputW", (e, 1)), ("Outputb", (1,))]

    # ---- recurrent state -----------------------------------------------------------------------------------------------
    def reset(self, n_batch=None):
        if n_batch is not None:
            self._state = [torch.zeros((n_batch, self._state_w), dtype=torch.float32, device=self.device)]

    # ---- forward -------------------------------------------------------------------------------------------------------
    def _embed(self, xf, rows, tag):
        e = self._buffer(("emb" + tag, rows), (rows, self._H))
        _lib.conv2d_fwd(xf, self._w[self._k_x], self._w[self._k_x + 1], e, self._geom(rows, self._rec_fan, self._H), True,
                        self._conv_ws)
        return e

    def _recur(self, e, h0, n_seg, t_len, resets, idx, h_last, tag):
        """e [n_seg T, E] from the states h0 [n_seg, 2 N] -> (u, lam, gam, h_all, y): y = relu(e + h_all W_c + b_o)."""
        w, k, ee, sw = self._w, self._k_x, self._H, self._state_w
        rows = n_seg * t_len
        buf = lambda name, r, c: self._buffer((name + tag, r), (r, c))                # noqa: E731
        lam, gam = buf("lam", self.state_size, 2), self._buffer(("gam" + tag,), (self.state_size,))
        _lib.lru_params(w[k + 2], w[k + 3], lam, gam)
        u, h_all, t, y = buf("u", rows, sw), buf("h_all", rows, sw), buf("branch", rows, ee), buf("y", rows, ee)
        _lib.conv2d_fwd(e, w[k + 4], None, u, self._geom(rows, ee, sw), False, self._conv_ws)
        _lib.lru_fwd(u.view(n_seg, t_len, sw), lam, gam, h0, h_all.view(n_seg, t_len, sw), h_last, resets, idx)
        _lib.conv2d_fwd(h_all, w[k + 5], w[k + 6], t, self._geom(rows, sw, ee), False, self._conv_ws)
        _lib.add_relu(e, t, t, y)
        return u, lam, gam, h_all, y

    def _step(self, observations, state, tag="s"):
        """One served step on `state` [b, 2 N], which advances in place."""
        b = observations.shape[0]
        _, xf = self._conv_features(self._scaled(observations, tag=tag), tag=tag)
        y = self._recur(self._embed(xf, b, tag), state, b, 1, None, None, state, tag)[-1]
        prob = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
        value = torch.empty(b, dtype=torch.float32, device=self.device)
        _lib.pg_head_infer(y, self.params[self._k_head], self.params[self._k_head + 1], prob, value)
        return prob, value

    def prob_value(self, observations, state_infos=None):
        """Does not advance the internal state: the step runs on a copy."""
        with torch.no_grad():
            prev = self._state if state_infos is None else list(state_infos)
            scratch = self._buffer(("state_v", prev[0].shape[0]), tuple(prev[0].shape))
            scratch.copy_(prev[0])
            return self._step(observations, scratch, tag="v")

    def act_step(self, observations, rows=None):
        """(prob, value, previous state); the state advances.  The returned state is valid until the next act_step."""
        with torch.no_grad():
            b = observations.shape[0]
            state = self._state[0] if rows is None else self._state[0][rows[0]:rows[1]]
            if state.shape[0] != b:
                raise ValueError("act_step: %d observations for %d state rows" % (b, state.shape[0]))
            ret = self._buffer(("prev_ret0", b), (b, self._state_w))
            ret.copy_(state)
            prob, value = self._step(observations, state)
            return prob, value, ret

    # ---- training ------------------------------------------------------------------------------------------------------
    def traj_minibatch(self, mb):
        """RecurrentCnnPolicy's, with the state's row width."""
        traj, t_len = mb["traj"], int(mb["horizon"])
        n_seg = traj.numel()
        idx = self._buffer(("traj_idx", n_seg, t_len), (n_seg * t_len,), dtype=torch.int32)
        state = [self._buffer(("traj_state0", n_seg), (n_seg, self._state_w))]
        valids = mb.get("valids")
        inv = self._buffer(("traj_inv", n_seg, t_len), (1,)) if valids is not None else None
        _lib.traj_minibatch(traj, t_len, [mb["lru_0"]], valids, idx, state, inv)
        return dict(mb, traj_idx=idx, traj_state=state, inv_count=inv)

    def loss_and_grads(self, mb, kind, clip_param, v_loss_coeff, ent_loss_coeff, lr_mult, inv_count=None,
                       tie_rule=_lib.PPO_TIE_THEANO, keep_forward=False):
        """RecurrentCnnPolicy's contract (rows [trajectory][time], `horizon`, optional `traj` and `resets`) with one
        recurrence launch per direction in place of the scan.  keep_forward: self.last_forward = (prob, value) of every
        row, from one more head launch."""
        if mb.get("idx") is not None:
            raise NotImplementedError("recurrent training takes whole trajectories: no row minibatches")
        t_len = int(mb["horizon"])
        if not 1 <= t_len <= _lib.LRU_MAX_STEPS:
            _refuse("the horizon must be in 1 .. %d, got %d" % (_lib.LRU_MAX_STEPS, t_len))
        with torch.no_grad():
            idx = traj_state = None
            if mb.get("traj") is not None:
                if "traj_idx" not in mb:
                    mb = self.traj_minibatch(mb)
                idx, traj_state = mb["traj_idx"], mb["traj_state"]
                if inv_count is None and mb.get("valids") is not None:
                    inv_count = mb["inv_count"]
            x = self._scaled(mb["observations"]) if idx is None else self._scaled(mb["observations"], idx)
            rows = x.shape[0]
            nb = rows // t_len
            assert nb * t_len == rows
            w, g, k, kh = self._w, self.grads, self._k_x, self._k_head
            ee, n, sw = self._H, self.state_size, self._state_w
            buf = lambda name, r, c: self._buffer((name, r), (r, c))                  # noqa: E731
            acts, xf = self._conv_features(x)
            e = self._embed(xf, rows, "")
            if traj_state is not None:
                h0 = traj_state[0]
            else:                               # the stored state before each segment's step 0 (a constant)
                h0 = buf("h0", nb, sw)
                h0.copy_(mb["lru_0"].view(nb, t_len, sw)[:, 0])
            resets = mb.get("resets")
            u, lam, gam, h_all, y = self._recur(e, h0, nb, t_len, resets, idx, None, "")
            # ---- head + losses; dx = d loss / d (e + h W_c + b_o), masked by y > 0
            dout = buf("dout", rows, self.n_act + 1)
            dx = buf("dh_all", rows, ee)
            loss4 = self._buffer(("loss", rows), (4,))
            _lib.pg_head_loss(y, self.params[kh], self.params[kh + 1], mb["actions"], mb["advantages"], mb["returns"],
                              mb.get("old_prob"), mb.get("valids"), idx, lr_mult, inv_count, self.n_act, kind, clip_param,
                              v_loss_coeff, ent_loss_coeff, dout, dx, g[kh], g[kh + 1], loss4, self._loss_ws,
                              relu_mask_dh=True, tie_rule=tie_rule)
            if keep_forward:
                prob, value = torch.empty((rows, self.n_act), device=self.device), torch.empty(rows, device=self.device)
                _lib.pg_head_infer(y, self.params[kh], self.params[kh + 1], prob, value)
                self.last_forward = (prob, value)
            # ---- the read-out, the recurrence (du over d h's buffer), the input projection
            g_c, g_b = self._geom(rows, sw, ee), self._geom(rows, ee, sw)
            self._bias_grad_by_ones(dx, rows, k + 5)
            _lib.conv2d_bwd_weight(dx, h_all, self._g[k + 5], g_c, self._conv_ws)
            dh = buf("d_state", rows, sw)
            _lib.conv2d_bwd_data(dx, w[k + 5], None, dh, g_c)
            dlam, dgam = self._buffer(("dlam_parts", nb), (nb, n, 2)), self._buffer(("dgam_parts", nb), (nb, n))
            seg = lambda a: a.view(nb, t_len, sw)                                     # noqa: E731
            _lib.lru_bwd(seg(u), seg(h_all), h0, lam, gam, seg(dh), seg(dh), dlam, dgam, resets, idx)
            _lib.conv2d_bwd_weight(dh, e, self._g[k + 4], g_b, self._conv_ws)
            de = buf("de", rows, ee)
            _lib.conv2d_bwd_data(dh, w[k + 4], None, de, g_b)
            # ---- d e = the residual's + the recurrence's, masked by e > 0 in place with b_x's gradient; then the
            # embedding's contraction, the convs, and nu and theta from the recurrence's partials
            _lib.add_relu(dx, de, de)
            _lib.relu_bwd_bias_grad(de, e, rows, ee, g[k + 1], self._fold_ws(("db", "emb")))
            g_x = self._geom(rows, self._rec_fan, ee)
            _lib.conv2d_bwd_weight(de, xf, self._g[k], g_x, self._conv_ws)
            dxf = buf("dxf", rows, self._rec_fan)
            _lib.conv2d_bwd_data(de, w[k], None, dxf, g_x)
            self._backward_convs(x, acts, dxf.view(acts[-1].shape))
            _lib.lru_param_fold(dlam, dgam, w[k + 2], w[k + 3], self._g[k + 2], self._g[k + 3])
            return loss4
