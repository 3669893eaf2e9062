"""A relational policy for the single-GPU learners (A2C, PPO, IMPALA and their mixins): multi-head self-attention over the
positions of the conv stack's last feature map, after Zambaldi et al. 2018 ("Relational Deep Reinforcement Learning" /
"Deep reinforcement learning with relational inductive biases"; the reference has none).  The paper is not at hand
(PAPERS.md): the block is restated from memory, with deliberate differences -- no LayerNorm, no per-entity MLP, blocks
not weight-shared, flatten instead of the feature-wise max-pool.  With r the rectified output [B, ho, wo, C] of the last
trunk convolution, x = r and N = ho * wo positions, each of n_blocks blocks computes

    rc  = coords(r)                 [B, ho, wo, C + 4]: r, the column and row coordinate in -1 .. 1, two zero channels
    qkv = conv1x1(rc, 3 * H * d)    bias, no rectifier; channel (which * H + h) * d + e, which = 0 / 1 / 2 for Q / K / V
    a   = attention(qkv)            softmax_j(Q K^T / sqrt(d)) V per sample and head, [B, ho, wo, H * d]
    t   = conv1x1(a, C)             bias, no rectifier
    x   = x + t ;  r = relu(x)

then r flattened (h, w, c) -> hidden_sizes dense + rectifier layers -> AtariCnnPolicy's policy / value head.

The default trunk is spec 1's filters, sizes and strides (atari_cnn_specs) with the padding of conv 2 and conv 3 cut to
(0, 1) and (0, 0): 104 x 80 -> 25 x 19 -> 11 x 9 -> 9 x 7 = 63 positions of 64 channels.  Spec 1 as it stands leaves
12 x 9 = 108 positions, more than the one-tile attention kernel's 64 (csrc/attention.hip), and is refused like every such
trunk unless max_positions (64 .. 256) admits it: a trunk of more than 64 positions runs on the key-tiled pair
arl_attn_tiled_fwd / _bwd, every other one on arl_attn_fwd / _bwd whatever max_positions says.

Every contraction is AtariCnnPolicy's (csrc/mfma_conv.hip; the block's two are 1 x 1 convolutions); between them run
csrc/attention.hip (arl_entity_coords_fwd / _bwd, arl_attn_fwd / _bwd) and arl_add_relu:

  forward :  the trunk as a chain; per block coords -> conv -> attention (with lse in a training pass) -> conv ->
             arl_add_relu, which writes the new x and r.  Kept for the backward pass: every rc, qkv, a, lse, and r.
  backward:  g = d loss / d x of the last block's output (the dense layer's data gradient, masked by r > 0).  Per block,
             last to first: the out-projection: dW from (g, a), db = column sums of g, da = dgrad(g, W) unmasked;
             arl_attn_bwd: dqkv; the qkv conv: dW from (dqkv, rc), db from dqkv, d_rc = dgrad(dqkv, W) masked by rc > 0
             (on the first C channels: r > 0); g <- g + d_rc[..., :C] (arl_entity_coords_bwd), for the first block masked
             by the trunk's r > 0: there x is itself a rectified conv output.  The trunk then runs the base's chain on g.
             Every gradient lives in a buffer of its own until the pass ends.

Parameters, in network order: Conv<i>W/b, R<k>QkvW/b, R<k>OutW/b, FC<j>W/b, the output layers.
"""
import os

import numpy as np

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy

MAX_BLOCKS = 4
# spec 1's filters, sizes and strides; the padding of conv 2 and conv 3 cut so that a 104 x 80 frame leaves 9 x 7 positions
DEFAULT_TRUNK = dict(conv_filters=(32, 64, 64), conv_filter_sizes=(8, 4, 3), conv_strides=(4, 2, 1),
                     conv_pads=((0, 0), (0, 1), (0, 0)))


class AtariRelationalPolicy(AtariCnnPolicy):

    def __init__(self, conv_filters=DEFAULT_TRUNK["conv_filters"], conv_filter_sizes=DEFAULT_TRUNK["conv_filter_sizes"],
                 conv_strides=DEFAULT_TRUNK["conv_strides"], conv_pads=DEFAULT_TRUNK["conv_pads"], n_blocks=1, n_heads=2,
                 head_dim=32, hidden_sizes=(256,), pixel_scale=255., initial_param_values=None, max_positions=64):
        def whole(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        if not (whole(n_blocks) and 1 <= n_blocks <= MAX_BLOCKS):
            raise NotImplementedError("AtariRelationalPolicy: n_blocks must be in 1 .. %d, got %r (INTEGRATION.md, section "
                                      "E)" % (MAX_BLOCKS, n_blocks))
        if not (whole(head_dim) and 4 <= head_dim <= _lib.ATTN_MAX_HEAD_DIM and head_dim % 4 == 0):
            raise NotImplementedError("AtariRelationalPolicy: head_dim must be a multiple of 4 in 4 .. %d, got %r "
                                      "(INTEGRATION.md, section E)" % (_lib.ATTN_MAX_HEAD_DIM, head_dim))
        if not (whole(n_heads) and n_heads >= 1 and n_heads * head_dim <= _lib.ATTN_MAX_WIDTH):
            raise NotImplementedError("AtariRelationalPolicy: n_heads >= 1 and n_heads * head_dim <= %d, got %r x %d "
                                      "(INTEGRATION.md, section E)" % (_lib.ATTN_MAX_WIDTH, n_heads, head_dim))
        if not list(hidden_sizes):
            raise NotImplementedError("AtariRelationalPolicy: at least one hidden dense layer is required (INTEGRATION.md, "
                                      "section E)")
        if not list(conv_filters):
            raise NotImplementedError("AtariRelationalPolicy: at least one trunk convolution is required (INTEGRATION.md, "
                                      "section E)")
        if not (whole(max_positions) and _lib.ATTN_MAX_POS <= max_positions <= _lib.ATTN_TILED_MAX_POS):
            raise NotImplementedError("AtariRelationalPolicy: max_positions must be in %d .. %d, got %r (INTEGRATION.md, "
                                      "section E)" % (_lib.ATTN_MAX_POS, _lib.ATTN_TILED_MAX_POS, max_positions))
        self.n_blocks, self.n_heads, self.head_dim = int(n_blocks), int(n_heads), int(head_dim)
        self.max_positions = int(max_positions)
        self._n_trunk, self._trunk_c = len(conv_filters), int(conv_filters[-1])
        block = [3 * self.n_heads * self.head_dim, self._trunk_c]
        # the base's flat conv list: the trunk, then two 1 x 1 convolutions per block
        super().__init__(list(conv_filters) + block * self.n_blocks, list(conv_filter_sizes) + [1, 1] * self.n_blocks,
                         list(conv_strides) + [1, 1] * self.n_blocks,
                         [tuple(p) for p in conv_pads] + [(0, 0), (0, 0)] * self.n_blocks,
                         hidden_sizes=hidden_sizes, pixel_scale=pixel_scale, initial_param_values=initial_param_values)

    def conv_names(self):
        return ["Conv%d" % i for i in range(self._n_trunk)] + ["R%d%s" % (k, s) for k in range(self.n_blocks)
                                                               for s in ("Qkv", "Out")]

    def _next_conv_input_channels(self, i, nf):
        if i < self._n_trunk - 1:
            return nf
        # after the trunk and after a block: r with its coordinate channels; after a qkv conv: the attention's output
        return self.n_heads * self.head_dim if (i - self._n_trunk) % 2 == 0 else self._trunk_c + 4

    def positions(self, obs_shape):
        """(ho, wo) of the trunk's last feature map for observations (c, h, w); needs no device."""
        _, h, w = obs_shape
        for sz, st, pad in list(zip(self.conv_filter_sizes, self.conv_strides, self.conv_pads))[:self._n_trunk]:
            h, w = (h + 2 * pad[0] - sz) // st + 1, (w + 2 * pad[1] - sz) // st + 1
        return h, w

    def reference_layout(self, obs_shape, n_act):
        """[(name, shape)] of get_param_values' tensors for observations (c, h, w) and n_act actions; needs no device."""
        c = obs_shape[0]
        out = []
        for i, name in enumerate(self.conv_names()):
            sz = self.conv_filter_sizes[i]
            out += [(name + "W", (self.conv_filters[i], c, sz, sz)), (name + "b", (self.conv_filters[i],))]
            c = self._next_conv_input_channels(i, self.conv_filters[i])
        ho, wo = self.positions(obs_shape)
        fan = self._trunk_c * ho * wo
        for j, hs in enumerate(self.hidden_sizes):
            out += [("FC%dW" % j, (fan, hs)), ("FC%db" % j, (hs,))]
            fan = hs
        return out + [("OutputW", (fan, n_act)), ("Outputb", (n_act,)), ("OutputW", (fan, 1)), ("Outputb", (1,))]

    def initialize(self, env_spec, device=None, **kwargs):
        shape = tuple(env_spec.observation_space.shape)
        ho, wo = self.positions(shape)
        if ho < 1 or wo < 1 or ho * wo > self.max_positions:
            raise NotImplementedError("AtariRelationalPolicy: the trunk leaves %d x %d positions of a %d x %d image; the "
                                      "attention kernel takes 1 .. %d (INTEGRATION.md, section E)" %
                                      (ho, wo, shape[1], shape[2], self.max_positions))
        if self._trunk_c % 4:
            raise NotImplementedError("conv filter counts must be multiples of 4 (got %d)" % self._trunk_c)
        self.rows_per_pass()
        super().initialize(env_spec, device=device, **kwargs)
        self.param_short_names[:2 * self._n_conv] = [n + s for n in self.conv_names() for s in "Wb"]
        layout = self.reference_layout(shape, self.n_act)
        assert [n for n, _ in layout] == self.param_short_names and [s for _, s in layout] == list(self._ref_shapes)
        # k-contiguous weight copies for the trunk's data gradients only; the blocks' read W itself, with the same bits
        self._wt = {i: t for i, t in self._wt.items() if i < self._n_trunk}

    def serve_supported(self):
        return False

    def rows_per_pass(self):
        if isinstance(self.max_rows_per_pass, str):
            raise NotImplementedError("AtariRelationalPolicy: max_rows_per_pass = %r is not supported, give a number or "
                                      "None (INTEGRATION.md, section E)" % (self.max_rows_per_pass,))
        return self.max_rows_per_pass

    # -------------------------------------------------------------- forward
    def _scaled_f32(self, obs_u8, idx=None, tag=""):
        c, h, w = self._obs_shape
        if c == 4 and (h * w) % 16 == 0:            # every Atari frame stack: the vectorised gather
            return super()._scaled_f32(obs_u8, idx, tag)
        b = obs_u8.shape[0] if idx is None else idx.shape[0]
        out = self._buffer(("x" + tag, b), (b, self._c_pad, h, w), channels_last=True)
        _lib.gather_scale_obs_nhwc_any(obs_u8, idx, out, self._scale)
        return out

    def _convs(self, x, w=None, tag=""):
        """-> [trunk activations, blocks, r]: r = relu of the last block's output [B, ho, wo, C] (what the first dense
        layer reads and is masked by); blocks = per block dict(rc, qkv, a, lse); lse only in a training pass."""
        b = x.shape[0]
        w = self._w if w is None else w
        conv_g, _ = self._layer_geoms(b)
        trunk = super()._convs(x, w, tag, upto=self._n_trunk)
        r = xs = trunk[-1]
        _, ho, wo, c = r.shape
        heads, d = self.n_heads, self.head_dim
        attn_fwd = _lib.attn_tiled_fwd if ho * wo > _lib.ATTN_MAX_POS else _lib.attn_fwd
        blocks = []
        for k in range(self.n_blocks):
            kq, ko = self._n_trunk + 2 * k, self._n_trunk + 2 * k + 1
            rc = self._buffer(("rc" + tag, k, b), (b, ho, wo, c + 4))
            qkv = self._buffer(("qkv" + tag, k, b), (b, ho * wo, 3, heads, d))
            a = self._buffer(("attn" + tag, k, b), (b, ho, wo, heads * d))
            lse = self._buffer(("lse" + tag, k, b), (b, heads, ho * wo)) if self._bits_pass else None
            t = self._buffer(("branch" + tag, k, b), (b, ho, wo, c))
            x_new = self._buffer(("skip" + tag, k, b), (b, ho, wo, c))
            r_new = self._buffer(("act" + tag, ko, b), (b, ho, wo, c))
            _lib.entity_coords_fwd(r, rc)
            _lib.conv2d_fwd(rc, w[2 * kq], w[2 * kq + 1], qkv, conv_g[kq], False, self._conv_ws)
            attn_fwd(qkv, a, lse)
            _lib.conv2d_fwd(a, w[2 * ko], w[2 * ko + 1], t, conv_g[ko], False, self._conv_ws)
            _lib.add_relu(xs, t, x_new, r_new)
            blocks.append(dict(rc=rc, qkv=qkv, a=a, lse=lse))
            xs, r = x_new, r_new
        return [trunk, blocks, r]

    # ------------------------------------------------------------- training
    def _block_conv_backward(self, k, d, inp, d_in, b, conv_g, corun, group, inp_rectified):
        """Conv layer k's gradients through _layer_grads (d: the gradient of its unrectified output); -> the co-run job if
        no launch has taken it yet."""
        nf, ci, sz, st, pad, ho, wo = self._conv_geom[k]
        if self._folds._n + 2 > _lib.FOLD_MAX_ITEMS:        # (the fold list is full before the pass ends)
            self._folds.run()
        self._layer_grads(d, True, d, b * ho * wo, nf, 2 * k, conv_g[k], inp, d_in, corun=corun, defer=group,
                          inp_rectified=inp_rectified)
        return None if (corun is not None and self._folds.corun_taken) else corun

    def _backward_convs(self, x, acts, d_act, masked=False, corun=None):
        """d_act = the gradient of the last block's output x (the dense layer's data gradient comes masked by r > 0)."""
        assert masked, "the relational stack takes the gradient of its unrectified output"
        b = x.shape[0]
        conv_g, _ = self._layer_geoms(b)
        group = os.environ.get("ARL_WGRAD_GROUP", "1") != "0"
        trunk, blocks, _ = acts
        shape = tuple(trunk[-1].shape)
        g = d_act.view(shape)
        attn_bwd = _lib.attn_tiled_bwd if shape[1] * shape[2] > _lib.ATTN_MAX_POS else _lib.attn_bwd
        # every gradient in a buffer of its own, all held until the end of the pass: a deferred weight gradient reads
        # them at run_wgrads(), and under graph capture a tensor nobody holds hands its memory to the next _buffer
        live = []
        for k in range(self.n_blocks - 1, -1, -1):
            kq, ko = self._n_trunk + 2 * k, self._n_trunk + 2 * k + 1
            blk = blocks[k]
            da = self._buffer(("dx_conv", ko, b), tuple(blk["a"].shape))
            corun = self._block_conv_backward(ko, g, blk["a"], da, b, conv_g, corun, group, False)
            dqkv = self._buffer(("dqkv", k, b), tuple(blk["qkv"].shape))
            attn_bwd(blk["qkv"], blk["a"], blk["lse"], da, dqkv)
            d_rc = self._buffer(("dx_conv", kq, b), tuple(blk["rc"].shape))
            corun = self._block_conv_backward(kq, dqkv, blk["rc"], d_rc, b, conv_g, corun, group, True)
            g_in = self._buffer(("dskip", k, b), shape)
            _lib.entity_coords_bwd(g, d_rc, trunk[-1] if k == 0 else None, g_in)
            live += [g, da, dqkv, d_rc]
            g = g_in
        if self._folds._n + 2 * self._n_trunk > _lib.FOLD_MAX_ITEMS:
            self._folds.run()
        super()._backward_convs(x, trunk, g, True, corun=corun, upto=self._n_trunk)
        del live

    def _bias_grad_left(self, d, y, rows, channels, k):
        # d is the gradient of the contraction's output with every mask that applies already in it
        self._bias_grad_by_ones(d.view(rows, channels), rows, k)
