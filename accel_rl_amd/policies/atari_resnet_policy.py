"""The residual network of IMPALA (Espeholt et al. 2018, "IMPALA: Scalable Distributed Deep-RL with Importance Weighted
Actor-Learner Architectures"; the reference has none) as a policy for the single-GPU learners (A2C, PPO, IMPALA).  The
paper is not at hand: the network is restated from memory.  Per section s with channels[s] filters:

    z = conv3x3(in, channels[s])                  stride 1, pad 1, bias, no rectifier
    x = maxpool(z)                                3 x 3 window, stride 2, pad 1 on both sides (-inf)
    blocks_per_section times:
        h = relu(conv3x3(relu(x)))                bias
        x = x + conv3x3(h)                        bias, no rectifier
    in of the next section = relu(x)              (x itself is only ever read through relu(x) and the skip)

then relu(x) flattened (h, w, c) -> hidden_sizes dense + rectifier layers -> AtariCnnPolicy's policy / value head.
The pool pads by one on BOTH sides, out = (in - 1) // 2 + 1 (104 x 80 -> 52 x 40 -> 26 x 20 -> 13 x 10): the original's
TensorFlow SAME pooling pads at the end only -- a deliberate difference.

Every contraction is AtariCnnPolicy's (csrc/mfma_conv.hip, any arl_conv_geom); between them run the streaming kernels of
csrc/resnet.hip (whose arl_gather_scale_obs_nhwc_any also feeds the first conv where the observations are not four
planes of a multiple of 16 bytes, which every Atari frame stack is):

  forward :  section conv (bias) -> arl_maxpool3s2_fwd, which writes x, r = relu(x) and the position of every maximum;
             per block conv (bias + rectifier, on r) -> conv (bias) -> arl_add_relu, which writes x + t over x and the
             next r.  Kept for the backward pass: every r, every h, every arg -- never x or z.
  backward:  g = d loss / d x of the last block's output (the dense layer's data gradient, masked by r > 0).  Per block,
             last to first: conv 2: dW from (g, h), db = column sums of g, d1 = dgrad(g, W2) masked by h; conv 1: dW from
             (d1, r), db from d1, dx = dgrad(d1, W1) masked by r; g <- g + dx (arl_add_relu without its rectifier).
             arl_maxpool3s2_bwd turns g into dz; the section conv: dW from (dz, in), db from dz, and the data gradient
             masked by the section below's last r is that section's g.
             Mask and input of every data gradient are the same tensor, so each layer is one AtariCnnPolicy._layer_grads
             call; the bias gradients ride in the weight-gradient launches (all-ones contraction where the generic
             kernels ran); the fold list runs whenever it is nearly full (ARL_FOLD_MAX_ITEMS).

Parameters, in network order: S<s>ConvW/b, S<s>B<b>Conv0W/b, S<s>B<b>Conv1W/b, .., FC<j>W/b, the output layers; conv W
Glorot-uniform, dense W NormC, biases 0.  The conv tensors lead the flat bucket (grad_split_offset as for every policy).
"""
import os

import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import AtariCnnPolicy

MAX_SECTIONS, MAX_BLOCKS, MAX_CHANNELS = 4, 4, 1024         # (channels: arl_maxpool3s2_fwd's limit)


class AtariResnetPolicy(AtariCnnPolicy):

    _u8_conv1 = False           # the first conv is 3 x 3 with padding: it reads the scaled f32 observations

    def __init__(self, channels=(16, 32, 32), blocks_per_section=2, hidden_sizes=(256,), pixel_scale=255.,
                 initial_param_values=None):
        channels = [int(c) for c in channels]
        if not 1 <= len(channels) <= MAX_SECTIONS:
            raise NotImplementedError("AtariResnetPolicy: 1 .. %d sections, got %d (INTEGRATION.md, section E)" %
                                      (MAX_SECTIONS, len(channels)))
        if not (isinstance(blocks_per_section, (int, np.integer)) and 1 <= blocks_per_section <= MAX_BLOCKS):
            raise NotImplementedError("AtariResnetPolicy: blocks_per_section must be in 1 .. %d, got %r (INTEGRATION.md, "
                                      "section E)" % (MAX_BLOCKS, blocks_per_section))
        for c in channels:
            if c < 4 or c > MAX_CHANNELS or c % 4:
                raise NotImplementedError("AtariResnetPolicy: channel counts must be multiples of 4 in 4 .. %d, got %d "
                                          "(INTEGRATION.md, section E)" % (MAX_CHANNELS, c))
        if not list(hidden_sizes):
            raise NotImplementedError("AtariResnetPolicy: at least one hidden dense layer is required (INTEGRATION.md, "
                                      "section E)")
        self.channels, self.blocks_per_section = channels, int(blocks_per_section)
        per = 1 + 2 * self.blocks_per_section               # conv layers per section: its own, then two per block
        filters = [c for c in channels for _ in range(per)]
        self._section_conv = [s * per for s in range(len(channels))]       # conv index of every section's first conv
        super().__init__(filters, [3] * len(filters), [1] * len(filters), [(1, 1)] * len(filters),
                         hidden_sizes=hidden_sizes, pixel_scale=pixel_scale, initial_param_values=initial_param_values)

    def conv_names(self):
        return ["S%dConv" % s if k == 0 else "S%dB%dConv%d" % (s, (k - 1) // 2, (k - 1) % 2)
                for s in range(len(self.channels)) for k in range(1 + 2 * self.blocks_per_section)]

    def reference_layout(self, obs_shape, n_act):
        """[(name, shape)] of get_param_values' tensors for observations (c, h, w) and n_act actions; needs no device."""
        c, h, w = obs_shape
        out = []
        for i, name in enumerate(self.conv_names()):
            out += [(name + "W", (self.conv_filters[i], c, 3, 3)), (name + "b", (self.conv_filters[i],))]
            c = self.conv_filters[i]
            h, w = self._next_conv_input_hw(i, h, w)
        fan = c * h * w
        for j, hs in enumerate(self.hidden_sizes):
            out += [("FC%dW" % j, (fan, hs)), ("FC%db" % j, (hs,))]
            fan = hs
        return out + [("OutputW", (fan, n_act)), ("Outputb", (n_act,)), ("OutputW", (fan, 1)), ("Outputb", (1,))]

    def _next_conv_input_hw(self, i, ho, wo):
        return _lib.maxpool3s2_out_hw(ho, wo) if i in self._section_conv else (ho, wo)

    def initialize(self, env_spec, device=None, **kwargs):
        c, h, w = env_spec.observation_space.shape
        if h < 1 or w < 1:
            raise NotImplementedError("AtariResnetPolicy: a %d x %d image leaves a section's pooled image empty "
                                      "(INTEGRATION.md, section E)" % (h, w))
        self.rows_per_pass()
        super().initialize(env_spec, device=device, **kwargs)
        self.param_short_names[:2 * self._n_conv] = [n + s for n in self.conv_names() for s in "Wb"]
        layout = self.reference_layout((c, h, w), self.n_act)
        assert [n for n, _ in layout] == self.param_short_names and [s for _, s in layout] == list(self._ref_shapes)
        # no k-contiguous weight copies for the data gradients: more layers qualify than one arl_conv2d_dgrad_weights
        # call takes (ARL_DGRAD_WT_MAX); the data gradients read W itself, with the same bits
        self._wt = {}

    def serve_supported(self):
        return False

    def rows_per_pass(self):
        if isinstance(self.max_rows_per_pass, str):
            raise NotImplementedError("AtariResnetPolicy: max_rows_per_pass = %r is not supported, give a number or None "
                                      "(INTEGRATION.md, section E)" % (self.max_rows_per_pass,))
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
        """-> [sections, r]: r = relu of the last block's output [B, Ho, Wo, K] (what the first dense layer reads and is
        masked by); sections = per section dict(inp, arg, r = [blocks + 1 rectified block inputs], h = [blocks])."""
        b = x.shape[0]
        w = self._w if w is None else w
        conv_g, _ = self._layer_geoms(b)
        per = 1 + 2 * self.blocks_per_section
        sections, a = [], x
        for s, i in enumerate(self._section_conv):
            nf, ci, sz, st, pad, ho, wo = self._conv_geom[i]
            z = self._buffer(("pre" + tag, s, b), (b, ho, wo, nf))
            _lib.conv2d_fwd(a, w[2 * i], w[2 * i + 1], z, conv_g[i], False, self._conv_ws)
            po, pw = _lib.maxpool3s2_out_hw(ho, wo)
            shape = (b, po, pw, nf)
            xs = self._buffer(("skip" + tag, s, b), shape)
            t = self._buffer(("branch" + tag, s, b), shape)
            r = self._buffer(("act" + tag, i, b), shape)
            arg = self._buffer(("arg" + tag, s, b), shape, dtype=torch.uint8)
            _lib.maxpool3s2_fwd(z, xs, r, arg)
            sec = dict(inp=a, arg=arg, r=[r], h=[])
            for k in range(i + 1, i + per, 2):
                hcur = self._buffer(("act" + tag, k, b), shape)
                _lib.conv2d_fwd(r, w[2 * k], w[2 * k + 1], hcur, conv_g[k], True, self._conv_ws)
                _lib.conv2d_fwd(hcur, w[2 * k + 2], w[2 * k + 3], t, conv_g[k + 1], False, self._conv_ws)
                r = self._buffer(("act" + tag, k + 1, b), shape)
                _lib.add_relu(xs, t, xs, r)
                sec["h"].append(hcur)
                sec["r"].append(r)
            sections.append(sec)
            a = r
        return [sections, a]

    # ------------------------------------------------------------- training
    def _conv_backward(self, k, d, y, inp, d_in, b, conv_g, corun, group):
        """Conv layer k's gradients through _layer_grads (d: the gradient of its output, mask applied; y: that output's
        stand-in for a bias fallback that does not read it); -> the co-run job if no launch has taken it yet."""
        nf, ci, sz, st, pad, ho, wo = self._conv_geom[k]
        if self._folds._n + 2 > _lib.FOLD_MAX_ITEMS:        # (15 + layers: the fold list is full before the pass ends)
            self._folds.run()
        self._layer_grads(d, True, y, b * ho * wo, nf, 2 * k, conv_g[k], inp, d_in, corun=corun if d_in is not None else None,
                          defer=group)
        if corun is not None and d_in is not None and self._folds.corun_taken:
            return None
        return corun

    def _backward_convs(self, x, acts, d_act, masked=False, corun=None):
        """d_act = the gradient of the last block's output x (the dense layer's data gradient comes masked by r > 0)."""
        assert masked, "the residual stack takes the gradient of its unrectified output"
        b = x.shape[0]
        conv_g, _ = self._layer_geoms(b)
        group = os.environ.get("ARL_WGRAD_GROUP", "1") != "0"
        sections = acts[0]
        per = 1 + 2 * self.blocks_per_section
        g = d_act
        # every layer's gradients live in buffers of their own, all held until the end of the pass: a deferred weight
        # gradient reads them at run_wgrads(), and under graph capture a tensor nobody holds any more hands its memory to
        # the next _buffer of its size (here, unlike in a plain stack, the next layer's)
        live = []
        for s in range(len(sections) - 1, -1, -1):
            i, sec = self._section_conv[s], sections[s]
            shape = tuple(sec["r"][0].shape)
            g = g.view(shape)
            for blk in range(self.blocks_per_section - 1, -1, -1):
                k1, k2 = i + 1 + 2 * blk, i + 2 + 2 * blk
                r_in, hcur = sec["r"][blk], sec["h"][blk]
                d1 = self._buffer(("dx_conv", k2, b), shape)
                corun = self._conv_backward(k2, g, hcur, hcur, d1, b, conv_g, corun, group)
                dx = self._buffer(("dx_conv", k1, b), shape)
                corun = self._conv_backward(k1, d1, hcur, r_in, dx, b, conv_g, corun, group)
                g_in = self._buffer(("dskip", k1, b), shape)
                _lib.add_relu(g, dx, g_in)
                live += [g, d1, dx]
                g = g_in
            nf, ci, sz, st, pad, ho, wo = self._conv_geom[i]
            dz = self._buffer(("dpre", s, b), (b, ho, wo, nf))
            _lib.maxpool3s2_bwd(g, sec["arg"], dz)
            live += [g, dz]
            g = self._buffer(("dx_conv", i, b), tuple(sec["inp"].shape)) if s > 0 else None
            corun = self._conv_backward(i, dz, dz, sec["inp"], g, b, conv_g, corun, group)
        self._folds.run_wgrads()
        if corun is not None:
            _lib.corun_job_run(corun)           # no launch could carry it: on its own, ahead of the step's update
        self._folds.run()
        del live

    def _bias_grad_left(self, d, y, rows, channels, k):
        # d is the gradient of the contraction's output with every mask that applies already in it
        self._bias_grad_by_ones(d.view(rows, channels), rows, k)
