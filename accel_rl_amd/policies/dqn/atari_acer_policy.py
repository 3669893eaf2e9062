"""ACER's network (Wang et al. 2017, "Sample Efficient Actor-Critic with Experience Replay"; the reference has none): one
trunk (QPolicyBase's conv stack -> dense) and ONE output layer of width 2S, S = n_actions rounded up to a multiple of 32:
columns [0, A) are the policy's logits, columns [S, S + A) the action values Q; the padding holds zero weights and takes
zero gradients (AtariDqnPolicy's rule).  The reference-order parameter vector carries OutputW / Outputb (logits), then
QW / Qb.

Serving is SAC-Discrete's: csrc/sac.hip:arl_sacd_act at row stride 2S puts out the soft-max row, from which the sampler's
categorical kernel draws with the real uniforms of host_draws (the override table forces nothing), so the sampler records
the soft-max row as the behaviour policy; set_deterministic serves the first maximum of the logits for evaluation
(q_policy_base.SoftmaxServeMixin, shared with AtariSacDiscretePolicy).  Serving in groups (HostEnvSampler.serve_group) is
refused: that path records a one-hot row, which ACER would read as the behaviour policy.

QPolicyBase's second bucket, `flat_target`, is the AVERAGE network here (`flat_avg`): update_target() stays the hard copy,
used once at initialisation; the learner moves it with arl_acer_avg_step after every optimizer step (algos/pg/acer.py).

  pi_q_rows            no-grad forward over many rows in passes -> (soft-max rows, raw output rows), for the Retrace scan
  acer_loss_and_grads  one minibatch: live forward, average-network forward on the same rows, ONE arl_acer_loss
                       (csrc/acer.hip), the output layer's and the trunk's backward pass into flat_grads
"""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import _norm_c
from accel_rl_amd.policies.dqn.q_policy_base import QPolicyBase, SoftmaxServeMixin


class AtariAcerPolicy(SoftmaxServeMixin, QPolicyBase):

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(), pixel_scale=255.,
                 deterministic=False, dueling=False, shared_last_bias=False, recurrent=False, initial_param_values=None):
        if recurrent:
            raise NotImplementedError("AtariAcerPolicy: no recurrent network (INTEGRATION.md, section E)")
        if dueling:
            raise NotImplementedError("AtariAcerPolicy: no dueling network (INTEGRATION.md, section E)")
        if shared_last_bias:
            raise NotImplementedError("AtariAcerPolicy: no shared output bias (INTEGRATION.md, section E)")
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, initial_param_values=initial_param_values)
        self._deterministic = bool(deterministic)
        self._draws = dict()              # n_envs -> the uniforms of the last host_draws, [horizon][n_envs]

    # ---- output layer: [logits | Q], each half padded to S columns ----------------------------------------------------
    def _head_reference_init(self, fan, n_act):
        if n_act > _lib.MAX_ACTIONS:
            raise NotImplementedError("AtariAcerPolicy: at most %d actions (arl_acer_loss; INTEGRATION.md, section E)" %
                                      _lib.MAX_ACTIONS)
        self._half = (n_act + 31) // 32 * 32
        return ([_norm_c((fan, n_act), 0.01), np.zeros(n_act, np.float32),
                 _norm_c((fan, n_act), 0.01), np.zeros(n_act, np.float32)], ["OutputW", "Outputb", "QW", "Qb"])

    def _head_internal_shapes(self, fan, n_act):
        return [(2 * self._half, fan), (2 * self._half,)]

    def _head_to_reference(self, wh, bh):
        a, s = self.n_act, self._half
        return [wh[:a].T, bh[:a], wh[s:s + a].T, bh[s:s + a]]

    def _head_to_internal(self, ref_tail):
        a, s = self.n_act, self._half
        w = np.zeros((2 * s, ref_tail[0].shape[0]), np.float32)
        b = np.zeros(2 * s, np.float32)
        w[:a], b[:a] = ref_tail[0].T, ref_tail[1]
        w[s:s + a], b[s:s + a] = ref_tail[2].T, ref_tail[3]
        return [w, b]

    @property
    def _head_width(self):
        return 2 * self._half

    @property
    def half_stride(self):
        """S: the column of the output row at which the action values start."""
        return self._half

    @property
    def flat_avg(self):
        """The average network's bucket (QPolicyBase's target bucket, moved by arl_acer_avg_step)."""
        return self.flat_target

    # ---- serving: SoftmaxServeMixin (as AtariSacDiscretePolicy's actor) --------------------------------------------------
    def serve_group(self, observations, row0, n_envs):
        raise NotImplementedError("AtariAcerPolicy is not served in groups (HostEnvSampler): that path draws the action "
                                  "in the policy and records a ONE-HOT row, which ACER would read as the behaviour policy "
                                  "mu; sample with GpuVecSampler, which records the soft-max row (INTEGRATION.md, "
                                  "section E)")

    # ---- the rollout's rows for the Retrace scan -------------------------------------------------------------------------
    def pi_q_rows(self, observations, rows_per_pass=None, tag="rows"):
        """(prob f32 [n, A], out f32 [n, 2S]): the current network's soft-max rows and raw output rows on u8 observations
        [n, C, H, W], apart from the training pass's activations; in passes of rows_per_pass rows (None: one pass).  `tag`
        names the scratch and the results: two calls whose results must live together take two tags."""
        if not tag:
            raise ValueError("pi_q_rows needs a tag of its own: the empty one is the training pass's scratch")
        with torch.no_grad():
            n = observations.shape[0]
            step = n if not rows_per_pass else min(n, int(rows_per_pass))
            prob = self._buffer(("acer_prob" + tag, n), (n, self.n_act))
            out = self._buffer(("acer_out" + tag, n), (n, 2 * self._half))
            for lo in range(0, n, step):
                rows = observations[lo:min(lo + step, n)]
                m = rows.shape[0]
                part = self._logits(self._scaled(rows, tag=tag), tag=tag)[0]
                _lib.sacd_act(part, None, self.n_act, prob[lo:lo + m], None, deterministic=False)
                _lib.copy_bytes(out[lo:lo + m], part)
            return prob, out

    # ---- training -----------------------------------------------------------------------------------------------------------
    def acer_loss_and_grads(self, mb, c, delta, q_coeff, ent_coeff, out=None):
        """One minibatch of ACER: the live network and the average network (w = the average bucket) on the rows
        mb["observations"][mb["idx"]] (idx None: all), one arl_acer_loss against mb["old_prob"], mb["actions"] and
        mb["returns"] (the Retrace targets) -- full-batch arrays, rows selected by idx --, then the full backward pass
        into flat_grads.  Returns stats f32[5][B]: pi_loss_rows | q_loss_rows | ent_rows | trust scale | rho(a_t) (`out`,
        when given).  No host synchronisation and no allocation outside _buffer: it runs inside the captured graphs."""
        with torch.no_grad():
            idx = mb.get("idx")
            x = self._scaled(mb["observations"], idx)
            avg = self._logits(x, w=self._w_target, tag="avg")[0]
            live, acts, hids = self._logits(x)
            b = live.shape[0]
            dout = self._buffer(("dlogits", b), tuple(live.shape))
            stats = self._buffer(("acer_stats", b), (5, b)) if out is None else out
            _lib.acer_loss(live, avg, mb["old_prob"], mb["actions"], mb["returns"], idx, self.n_act, c, delta, q_coeff,
                           ent_coeff, dout, stats)
            self._head_backward(dout, x, acts, hids)
            return stats

    def _pg_loss_refused(self, *args, **kwargs):
        raise NotImplementedError("AtariAcerPolicy trains through acer_loss_and_grads (algos/pg/acer.py), not the "
                                  "actor-critic head loss (INTEGRATION.md, section E)")

    loss_and_grads = _pg_loss_refused
