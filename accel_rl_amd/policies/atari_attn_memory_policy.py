"""An attention-memory policy: conv stack -> embedding -> one layer of windowed causal attention over TIME -> (softmax
pi, linear V).  The memory is Transformer-XL's cached segment (Dai et al. 2019) used the way GTrXL uses it in RL
(Parisotto et al. 2020); neither paper is at hand and the reference has no such policy: one layer, no
LayerNorm, no gating, a learned bias per head and age instead of the sinusoidal relative encoding.

    e_t  = relu(xf_t W_x + b_x)                       [E], xf_t = the conv stack's flattened output
    q_t  = e_t W_q ;  (k, v)_c = c W_kv               no bias: an empty memory slot (a zero vector) has k = v = 0
    s_ta = scale q_t . k_(t-a) + rel[h][a]            a = 0 .. M: e_t itself and the M embeddings before it
    o_t  = sum_a softmax_a(s_t)_a v_(t-a)
    y_t  = relu(e_t + o_t W_o + b_o)  ->  AtariCnnPolicy's policy / value head

The recurrent state is one tensor per environment, "mem_0" [n_env, M E]: the last M embeddings as a shift register, slot
M - 1 the most recent, zeros at the start and after a reset.  There are no validity counters: an empty slot's score is
its relative bias alone and its value zero, in serving and in training alike.

Serving runs csrc/tattention.hip's arl_tattn_fwd at T = 1 on the window [state ; e_t] that arl_tattn_shift builds while
it shifts the state.  Training runs a segment's whole time dimension in one arl_tattn_fwd and one arl_tattn_bwd launch on
the context [stored memory (M rows, a constant: Transformer-XL's stop-gradient) ; e_0 .. e_(T-1)]; with mb["resets"] an
entry older than the last reset before the query counts as an empty slot, which is what the sampler's zeroed state
produced.  Every contraction is AtariCnnPolicy's (csrc/mfma_conv.hip); the sums are arl_add_relu's.

Parameters after the convs, in network order: AttnWx (fan, E), AttnBx, AttnWq (E, H d), AttnWkv (E, 2 H d), AttnWo
(H d, E), AttnBo, AttnRel (H, M + 1); then the output layers.
"""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import _norm_c
from accel_rl_amd.policies.atari_lstm_policy import RecurrentCnnPolicy

STATE_MAX_WIDTH = 1024          # arl_traj_minibatch's widest state row


def _refuse(msg):
    raise NotImplementedError("AtariAttnMemoryPolicy: %s (INTEGRATION.md, section E)" % msg)


class AtariAttnMemoryPolicy(RecurrentCnnPolicy):

    _state_keys = ("mem_0",)

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(256,), memory_len=3,
                 n_heads=2, head_dim=32, pixel_scale=255., alternating_sampler=False, initial_param_values=None):
        def whole(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not (whole(memory_len) and whole(n_heads) and whole(head_dim)):
            _refuse("memory_len, n_heads and head_dim must be integers, got %r, %r, %r" % (memory_len, n_heads, head_dim))
        if len(hidden_sizes) != 1 or hidden_sizes[0] < 4 or hidden_sizes[0] % 4:
            _refuse("exactly one hidden size, the embedding width, a multiple of 4; got %r" % (tuple(hidden_sizes),))
        if not _lib.tattn_shape_ok(1, memory_len, n_heads, head_dim):
            _refuse("memory_len in 1 .. %d, head_dim a multiple of 4 in 4 .. %d, n_heads >= 1 and n_heads * head_dim <= %d; "
                    "got %r, %r, %r" % (_lib.TATTN_MAX_MEM, _lib.ATTN_MAX_HEAD_DIM, _lib.ATTN_MAX_WIDTH, memory_len,
                                        head_dim, n_heads))
        if memory_len * hidden_sizes[0] > STATE_MAX_WIDTH:
            _refuse("memory_len * embedding width must be at most %d (the stored state's row), got %d x %d" %
                    (STATE_MAX_WIDTH, memory_len, hidden_sizes[0]))
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, initial_param_values=initial_param_values)
        self.memory_len, self.n_heads, self.head_dim = int(memory_len), int(n_heads), int(head_dim)
        self._state_w = self.memory_len * self._H

    def serve_supported(self):
        return False

    # ---- parameters ----------------------------------------------------------------------------------------------------
    def _hidden_reference_init(self, fan):
        e, hd, m = self._H, self.n_heads * self.head_dim, self.memory_len
        self._hid_geom, self._rec_fan = [], fan
        return ([_norm_c((fan, e), 1.0), np.zeros(e, np.float32), _norm_c((e, hd), 1.0), _norm_c((e, 2 * hd), 1.0),
                 _norm_c((hd, e), 1.0), np.zeros(e, np.float32), np.zeros((self.n_heads, m + 1), np.float32)],
                ["AttnWx", "AttnBx", "AttnWq", "AttnWkv", "AttnWo", "AttnBo", "AttnRel"], e)

    def _hidden_internal_shapes(self):
        e, hd = self._H, self.n_heads * self.head_dim
        return [(e, self._rec_fan), (e,), (hd, e), (2 * hd, e), (e, hd), (e,), (self.n_heads, self.memory_len + 1)]

    def _hidden_to_reference(self, a):
        return [self._conv_flat_to_reference(a[0]), a[1], a[2].T, a[3].T, a[4].T, a[5], a[6]]

    def _hidden_to_internal(self, r):
        return [self._conv_flat_to_internal(r[0]), r[1], r[2].T, r[3].T, r[4].T, r[5], r[6]]

    def reference_layout(self, obs_shape, n_act):
        """[(name, shape)] of get_param_values' tensors for observations (c, h, w) and n_act actions; needs no device."""
        c, h, w = obs_shape
        out = []
        for i, (nf, sz, st, pad) in enumerate(zip(self.conv_filters, self.conv_filter_sizes, self.conv_strides,
                                                  self.conv_pads)):
            out += [("Conv%dW" % i, (nf, c, sz, sz)), ("Conv%db" % i, (nf,))]
            c, h, w = nf, (h + 2 * pad[0] - sz) // st + 1, (w + 2 * pad[1] - sz) // st + 1
        e, hd = self._H, self.n_heads * self.head_dim
        out += [("AttnWx", (c * h * w, e)), ("AttnBx", (e,)), ("AttnWq", (e, hd)), ("AttnWkv", (e, 2 * hd)),
                ("AttnWo", (hd, e)), ("AttnBo", (e,)), ("AttnRel", (self.n_heads, self.memory_len + 1))]
        return out + [("OutputW", (e, n_act)), ("Outputb", (n_act,)), ("OutputW", (e, 1)), ("Outputb", (1,))]

    # ---- recurrent state -----------------------------------------------------------------------------------------------
    def reset(self, n_batch=None):
        if n_batch is not None:
            self._state = [torch.zeros((n_batch, self._state_w), dtype=torch.float32, device=self.device)]

    # ---- forward -------------------------------------------------------------------------------------------------------
    def _attend(self, e, ctx, n_seg, t_len, resets, idx, lse, tag):
        """e [n_seg T, E] and its context ctx [n_seg (M + T), E] -> (q, kv, a, x, y): y = relu(x), x = e + a W_o + b_o."""
        w, k, ee, h, d, m = self._w, self._k_x, self._H, self.n_heads, self.head_dim, self.memory_len
        rows, crow = n_seg * t_len, n_seg * (m + t_len)
        buf = lambda name, r, c: self._buffer((name + tag, r), (r, c))                # noqa: E731
        q, kv, a = buf("q", rows, h * d), buf("kv", crow, 2 * h * d), buf("attn", rows, h * d)
        t, x, y = buf("branch", rows, ee), buf("skip", rows, ee), buf("y", rows, ee)
        _lib.conv2d_fwd(e, w[k + 2], None, q, self._geom(rows, ee, h * d), False, self._conv_ws)
        _lib.conv2d_fwd(ctx, w[k + 3], None, kv, self._geom(crow, ee, 2 * h * d), False, self._conv_ws)
        _lib.tattn_fwd(q.view(n_seg, t_len, h, d), kv.view(n_seg, m + t_len, 2, h, d), self.params[k + 6].detach(),
                       a.view(n_seg, t_len, h * d), lse, resets, idx)
        _lib.conv2d_fwd(a, w[k + 4], w[k + 5], t, self._geom(rows, h * d, ee), False, self._conv_ws)
        _lib.add_relu(e, t, x, y)
        return q, kv, a, x, y

    def _embed(self, xf, rows, tag):
        e = self._buffer(("emb" + tag, rows), (rows, self._H))
        _lib.conv2d_fwd(xf, self._w[self._k_x], self._w[self._k_x + 1], e, self._geom(rows, self._rec_fan, self._H), True,
                        self._conv_ws)
        return e

    def _step(self, observations, state, prev_out=None, tag="s"):
        """One served step on `state` [b, M E], which shifts in place; prev_out, when given, receives it as it was."""
        b, m = observations.shape[0], self.memory_len
        _, xf = self._conv_features(self._scaled(observations, tag=tag), tag=tag)
        e = self._embed(xf, b, tag)
        window = self._buffer(("window" + tag, b), (b * (m + 1), self._H))
        _lib.tattn_shift(state, e, window, prev_out)
        y = self._attend(e, window, b, 1, None, None, None, tag)[-1]
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
        """(prob, value, previous memory); the memory advances.  The returned memory is valid until the next act_step."""
        with torch.no_grad():
            b = observations.shape[0]
            state = self._state[0] if rows is None else self._state[0][rows[0]:rows[1]]
            if state.shape[0] != b:
                raise ValueError("act_step: %d observations for %d state rows" % (b, state.shape[0]))
            ret = self._buffer(("prev_ret0", b), (b, self._state_w))
            prob, value = self._step(observations, state, ret)
            return prob, value, ret

    # ---- training ------------------------------------------------------------------------------------------------------
    def traj_minibatch(self, mb):
        """RecurrentCnnPolicy's, with the memory's row width."""
        traj, t_len = mb["traj"], int(mb["horizon"])
        n_seg = traj.numel()
        idx = self._buffer(("traj_idx", n_seg, t_len), (n_seg * t_len,), dtype=torch.int32)
        state = [self._buffer(("traj_state0", n_seg), (n_seg, self._state_w))]
        valids = mb.get("valids")
        inv = self._buffer(("traj_inv", n_seg, t_len), (1,)) if valids is not None else None
        _lib.traj_minibatch(traj, t_len, [mb["mem_0"]], valids, idx, state, inv)
        return dict(mb, traj_idx=idx, traj_state=state, inv_count=inv)

    def loss_and_grads(self, mb, kind, clip_param, v_loss_coeff, ent_loss_coeff, lr_mult, inv_count=None,
                       tie_rule=_lib.PPO_TIE_THEANO, keep_forward=False):
        """RecurrentCnnPolicy's contract (rows [trajectory][time], `horizon`, optional `traj` and `resets`) with one
        attention launch per direction in place of the scan.  keep_forward: self.last_forward = (prob, value) of every
        row, from one more head launch."""
        if mb.get("idx") is not None:
            raise NotImplementedError("recurrent training takes whole trajectories: no row minibatches")
        t_len = int(mb["horizon"])
        if not 1 <= t_len <= _lib.TATTN_MAX_STEPS:
            _refuse("the horizon must be in 1 .. %d, got %d" % (_lib.TATTN_MAX_STEPS, t_len))
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
            ee, h, d, m = self._H, self.n_heads, self.head_dim, self.memory_len
            crow = nb * (m + t_len)
            buf = lambda name, r, c: self._buffer((name, r), (r, c))                  # noqa: E731
            acts, xf = self._conv_features(x)
            e = self._embed(xf, rows, "")
            init = traj_state[0] if traj_state is not None else mb["mem_0"].view(nb, t_len, -1)[:, 0]
            ctx = buf("ctx", crow, ee)
            ctx3 = ctx.view(nb, m + t_len, ee)
            ctx3[:, :m].copy_(init.reshape(nb, m, ee))
            ctx3[:, m:].copy_(e.view(nb, t_len, ee))
            resets = mb.get("resets")
            lse = self._buffer(("lse", rows), (nb, h, t_len))
            q, kv, a, _, y = self._attend(e, ctx, nb, t_len, resets, idx, lse, "")
            # ---- head + losses; dx = d loss / d (e + o W_o + b_o), masked by y > 0
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
            # ---- the out-projection, the attention, the q and kv projections
            g_o, g_q, g_kv = self._geom(rows, h * d, ee), self._geom(rows, ee, h * d), self._geom(crow, ee, 2 * h * d)
            self._bias_grad_by_ones(dx, rows, k + 4)
            _lib.conv2d_bwd_weight(dx, a, self._g[k + 4], g_o, self._conv_ws)
            da = buf("da", rows, h * d)
            _lib.conv2d_bwd_data(dx, w[k + 4], None, da, g_o)
            dq, dkv = buf("dq", rows, h * d), buf("dkv", crow, 2 * h * d)
            parts = self._buffer(("drel_parts", nb), (nb, h, m + 1))
            _lib.tattn_bwd(q.view(nb, t_len, h, d), kv.view(nb, m + t_len, 2, h, d), self.params[k + 6].detach(),
                           a.view(nb, t_len, h * d), lse, da, dq, dkv, parts, resets, idx)
            _lib.tattn_rel_fold(parts, g[k + 6])
            _lib.conv2d_bwd_weight(dq, e, self._g[k + 2], g_q, self._conv_ws)
            _lib.conv2d_bwd_weight(dkv, ctx, self._g[k + 3], g_kv, self._conv_ws)
            # ---- d e = the residual's + the q path's + the kv path's in-segment rows (the stored memory is a constant)
            de_q, de_ctx, de_kv = buf("de_q", rows, ee), buf("de_ctx", crow, ee), buf("de_kv", rows, ee)
            _lib.conv2d_bwd_data(dq, w[k + 2], None, de_q, g_q)
            _lib.conv2d_bwd_data(dkv, w[k + 3], None, de_ctx, g_kv)
            de_kv.view(nb, t_len, ee).copy_(de_ctx.view(nb, m + t_len, ee)[:, m:])
            de = buf("de", rows, ee)
            _lib.add_relu(dx, de_q, de)
            _lib.add_relu(de, de_kv, de)
            # masked by e > 0 in place, and b_x's gradient with it; then the embedding's contraction and the convs
            _lib.relu_bwd_bias_grad(de, e, rows, ee, g[k + 1], self._fold_ws(("db", "emb")))
            g_x = self._geom(rows, self._rec_fan, ee)
            _lib.conv2d_bwd_weight(de, xf, self._g[k], g_x, self._conv_ws)
            dxf = buf("dxf", rows, self._rec_fan)
            _lib.conv2d_bwd_data(de, w[k], None, dxf, g_x)
            self._backward_convs(x, acts, dxf.view(acts[-1].shape))
            return loss4
