"""Fully parameterized quantile function policy for Atari (FQF, Yang et al. 2019, "Fully Parameterized Quantile Function
for Distributional RL"; the reference has none): AtariIqnPolicy whose fractions are neither fixed nor drawn but proposed
per state by one dense layer on the conv features, ONE set per sample for every pass of that sample (Algorithm 1):

    psi     = conv stack(obs)                           f32[B][F]           (as AtariIqnPolicy)
    logits  = psi W_frac + b_frac                       f32[B][n_stride]    (one dense MFMA call at B rows, no rectifier)
    tau, tau_hat, tau_mid, q, log q, H                                      (arl_fqf_fractions: soft-max, cumulative sum)
    theta   = the implicit quantile network at tau_hat  f32[B N][a_stride]  (_quantile_pass in its given mode)
    Q_a     = sum_k (tau_{k+1} - tau_k) theta(k, a)                         (arl_fqf_act / arl_fqf_loss)

N = n_quantiles fractions serve every pass: online and target net, training and action serving.  The fraction layer
(W_frac (F, N), b_frac (N) in the reference layout) is the LAST layer in construction order, in the flat bucket and in
get_param_values; it is stored (n_stride, F), n_stride = N rounded up to 32 with zero rows (and zero gradients) in the
padding, its fan-in axis in psi's NHWC-flatten order and converted like the first dense layer's.  The target bucket
carries an unused copy of it, which keeps update_target and snapshots those of QPolicyBase.  Nothing is drawn: the
(seed, counter) state of the parent stays where it is.
"""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import ObsRows, _norm_c
from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy


class AtariFqfPolicy(AtariIqnPolicy):

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(), pixel_scale=255.,
                 epsilon=1, n_quantiles=32, dueling=False, initial_param_values=None):
        if dueling:
            raise NotImplementedError("dueling FQF networks are not built (INTEGRATION.md, section E)")
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, epsilon=epsilon, n_quantiles=n_quantiles,
                         n_target_quantiles=n_quantiles, n_policy_quantiles=n_quantiles,
                         initial_param_values=initial_param_values)
        self._n_stride = (n_quantiles + 31) // 32 * 32
        self.frac_rows = self.entropy = None        # of the last fqf_loss_and_grads call (device tensors)

    # ---- output layer, then the fraction layer (construction order) -----------------------------------------------
    def _head_reference_init(self, fan, n_act):
        head, names = super()._head_reference_init(fan, n_act)
        n = self.n_quantiles
        frac = [_norm_c((self._f, n), 0.01), np.zeros(n, np.float32)]      # near-uniform fractions at the start
        return head + frac, names + ["FracW", "Fracb"]

    def _head_internal_shapes(self, fan, n_act):
        return super()._head_internal_shapes(fan, n_act) + [(self._n_stride, self._f), (self._n_stride,)]

    def _frac_to_reference(self, w, b):
        n = self.n_quantiles
        return [self._conv_flat_to_reference(w[:n]), b[:n]]

    def _head_to_internal(self, ref_tail):
        n = self.n_quantiles
        w = np.zeros((self._n_stride, self._f), np.float32)
        b = np.zeros(self._n_stride, np.float32)
        w[:n] = self._conv_flat_to_internal(ref_tail[2])
        b[:n] = ref_tail[3]
        return super()._head_to_internal(ref_tail[:2]) + [w, b]

    def bucket_to_reference(self, flat):
        arr = self._internal_arrays(flat)
        frac = self._frac_to_reference(arr[self._k_frac], arr[self._k_frac + 1])
        return np.concatenate([super().bucket_to_reference(flat)] +
                              [np.ascontiguousarray(x).reshape(-1) for x in frac]).astype(np.float32)

    @property
    def _k_frac(self):
        return self._k_head + 2

    @property
    def frac_offset(self):
        """Offset of the fraction layer in the flat bucket: it and everything behind it is FqfOptimizer's second range."""
        return self._offsets[self._k_frac]

    # ---- the fraction layer's forward -----------------------------------------------------------------------------
    def _frac_geom(self, b):
        key = ("frac", b, _lib.default_route)
        if key not in self._geoms:
            self._geoms[key] = _lib.dense_geom(b, self._f, self._n_stride)
        return self._geoms[key]

    def _fractions(self, psi, tag="", logits=None, serving=False):
        """psi f32[b][F] -> (logits, tau f32[b][N + 1], tau_hat f32[b N], tau_mid f32[b (N - 1)] or None, q, logq,
        entropy); serving: only tau and tau_hat are written (the others come back None)."""
        b, n = psi.shape[0], self.n_quantiles
        if logits is None:
            k = self._k_frac
            logits = self._buffer(("fqf_logits" + tag, b), (b, self._n_stride))
            _lib.conv2d_fwd(psi, self._w[k], self._w[k + 1], logits, self._frac_geom(b), False, self._conv_ws)
        tau = self._buffer(("fqf_tau" + tag, b), (b, n + 1))
        tau_hat = self._buffer(("fqf_tau_hat" + tag, b), (b * n,))
        tau_mid = q = logq = entropy = None
        if not serving:
            tau_mid = self._buffer(("fqf_tau_mid" + tag, b), (b * (n - 1),)) if n > 1 else None
            q = self._buffer(("fqf_q" + tag, b), (b, n))
            logq = self._buffer(("fqf_logq" + tag, b), (b, n))
            entropy = self._buffer(("fqf_entropy" + tag, b), (b,))
        _lib.fqf_fractions(logits, n, tau, tau_hat, tau_mid, q, logq, entropy)
        return logits, tau, tau_hat, tau_mid, q, logq, entropy

    # ---- serving --------------------------------------------------------------------------------------------------
    def _serve_obs(self, observations, override, onehot, greedy=None):
        """Epsilon-greedy / greedy actions of every row at its own N proposed fractions, in passes of at most
        serve_pair_rows // N rows.  A row's fractions depend on that row alone, so the split changes no result."""
        rows, n = observations.shape[0], self.n_quantiles
        per = max(1, self.serve_pair_rows // n)
        for lo in range(0, rows, per):
            hi = min(lo + per, rows)
            psi = self._convs(self._scaled(observations[lo:hi], tag="s"), tag="s")[-1].view(hi - lo, self._f)
            _, tau, tau_hat = self._fractions(psi, tag="s", serving=True)[:3]
            theta = self._quantile_pass(psi, n, tag="s", tau_in=tau_hat)[-1]
            _lib.fqf_act(theta, tau, None if override is None else override[lo:hi], self.n_act, n, onehot[lo:hi],
                         None if greedy is None else greedy[lo:hi])
            self.served_tau = tau                   # f32[rows of the last pass][N + 1]

    # ---- training -------------------------------------------------------------------------------------------------
    def iqn_loss_and_grads(self, *args, **kwargs):
        raise NotImplementedError("AtariFqfPolicy proposes its fractions: train it with FQF (fqf_loss_and_grads)")

    def munchausen_loss_and_grads(self, *args, **kwargs):
        raise NotImplementedError("Munchausen FQF is not built: train it with FQF (fqf_loss_and_grads)")

    def fqf_loss_and_grads(self, obs, next_obs, actions, returns, terminals, is_weights, gamma_n, kappa, ent_coef,
                           double_dqn=False, fractions=None):
        """One minibatch of FQF.build_loss.  The conv passes are iqn_loss_and_grads'; the online fraction layer proposes
        N fractions per sample from the online conv features of obs; the online net runs on obs at tau_hat (N rows a
        sample, the only pass that is backpropagated) and at tau_1 .. tau_{N-1} (N - 1 rows, forward only), the target
        net -- and, for double DQN, the online net -- on next_obs at the same tau_hat; arl_fqf_loss gives the
        quantile-Huber loss with its gradient and the fraction loss's gradient w.r.t. the logits; then the backward pass
        of the tau_hat pass and the fraction layer's weight and bias gradient (no data gradient: the fraction loss does
        not reach psi) into flat_grads.  fractions f32[B][n_stride]: logits that take the proposed ones' place (tests).
        Returns (loss_rows f32[B] whose sum is the quantile loss, priorities f32[B]); frac_rows (w_b G_b: a surrogate
        whose gradient is the fraction loss's, NOT the 1-Wasserstein distance's value) and entropy stay on the policy.
        No host synchronisation and no allocation outside _buffer: it runs inside the captured update graph."""
        with torch.no_grad():
            b, f, n = obs.shape[0], self._f, self.n_quantiles
            if double_dqn and self._u8:             # the two online conv passes as ONE pass over 2B rows
                both = self._pair_rows(obs, next_obs)
                psi_t = self._convs(ObsRows(both[b:], None), w=self._w_target, tag="t")[-1]
                acts2 = self._convs(ObsRows(both, None), tag="2")
                x, acts, psi_d = ObsRows(both[:b], None), [a[:b] for a in acts2], acts2[-1][b:]
            else:
                x_next = self._scaled(next_obs, tag="n")
                psi_t = self._convs(x_next, w=self._w_target, tag="t")[-1]
                psi_d = self._convs(x_next, tag="d")[-1] if double_dqn else None
                x = self._scaled(obs)
                acts = self._convs(x)
            psi = acts[-1].view(b, f)
            _, tau, tau_hat, tau_mid, q, logq, entropy = self._fractions(psi, logits=fractions)
            _, cosf, phi, merged, hids, theta = self._quantile_pass(psi, n, tau_in=tau_hat)
            mid = self._quantile_pass(psi, n - 1, tag="m", tau_in=tau_mid)[-1] if n > 1 else None
            tgt = self._quantile_pass(psi_t.view(b, f), n, w=self._w_target, tag="t", tau_in=tau_hat)[-1]
            pol = self._quantile_pass(psi_d.view(b, f), n, tag="d", tau_in=tau_hat)[-1] if double_dqn else None
            dtheta = self._buffer(("dtheta", b), (b * n, self._a_stride))
            dlogits = self._buffer(("fqf_dlogits", b), (b, self._n_stride))
            pack = self._buffer(("loss_pri", b), (2, b))        # one buffer: the optimizer's statistics ring takes both rows
            loss_rows, priorities = pack[0], pack[1]
            frac_rows = self._buffer(("fqf_frac_rows", b), (b,))
            _lib.fqf_loss(theta, mid, tau, tau_hat, q, logq, entropy, tgt, pol, actions, returns, terminals, is_weights,
                          self.n_act, n, gamma_n, kappa, ent_coef, dtheta, loss_rows, priorities, dlogits, frac_rows)
            self.frac_rows, self.entropy = frac_rows, entropy
            # The fraction layer: weight gradient with the bias gradient riding along; its fold runs with the others at the
            # end of _pair_backward.  (Not _layer_grads: where the kernel cannot carry the bias gradient, that helper falls
            # back on a pass that applies a rectifier mask, and this layer has no rectifier.)
            k = self._k_frac
            done = self._folds.conv2d_bwd_weight(dlogits, psi, self._g[k], self._frac_geom(b), self._fold_ws(("dw", k)),
                                                 dbias=self.grads[k + 1])
            if not done:        # generic kernels
                self._bias_grad_by_ones(dlogits, b, k)
            self._pair_backward(x, acts, psi, cosf, phi, merged, hids, dtheta, b, n)
            return loss_rows, priorities
