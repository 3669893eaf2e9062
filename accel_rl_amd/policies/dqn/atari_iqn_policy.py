"""Implicit quantile network policy for Atari (IQN, Dabney et al. 2018, "Implicit Quantile Networks for Distributional
RL"; the reference has none): the quantile fractions tau ~ U(0, 1) are drawn afresh for every sample, embedded with
64 cosine features, and multiplied into the conv features:

    psi   = conv stack(obs)                           f32[B][F]           (post-rectifier, NHWC-flattened)
    c     = cos(pi i tau), i = 0 .. 63                f32[B R][64]        (arl_iqn_embed; R fractions per sample)
    phi   = relu(c W_emb + b_emb)                     f32[B R][F]         (one dense MFMA call)
    x     = psi[b] * phi[b R + r]                     f32[B R][F]         (arl_iqn_merge_fwd)
    theta = output(hidden layers(x))                  f32[B R][a_stride]  (the dense MFMA calls, at B R rows)
    Q_a   = (sum_r theta(r, a)) / R

R is n_quantiles (N: online net on obs), n_target_quantiles (N': the next observations' passes) or n_policy_quantiles
(K: action serving).  The output row is padded to `a_stride` columns (zero weights, zero gradients) as AtariDqnPolicy's.
The embedding layer (W_emb (F, 64) as stored, b_emb (F)) sits between the conv layers and the hidden layers in
construction order, in the flat bucket and in get_param_values; its unit axis is stored in psi's NHWC-flatten order
and converted like the first dense layer's fan-in axis, so the reference-layout vector describes a network whose
flatten is the reference's (c, h, w).

The fractions come from the device generator of csrc/iqn.hip, seeded by `_iqn_state` = (seed, call counter): a replayed
graph draws fresh fractions.  One update makes three passes (call offsets 0, 1, 2; the loss launch advances the
counter by 3); one serving call reads one call's stream, indexed by the observation's global row, whatever the split
into passes, and advances the counter once per pass.
"""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import ObsRows, _norm_c
from accel_rl_amd.policies.dqn.q_policy_base import QPolicyBase

N_COS = _lib.IQN_COS
# (sample, fraction) rows of one serving pass: phi and x cost rows * K * F * 4 bytes each (98 MiB each at F = 3136)
SERVE_PAIR_ROWS = 8192


class AtariIqnPolicy(QPolicyBase):

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(), pixel_scale=255.,
                 epsilon=1, n_quantiles=8, n_target_quantiles=8, n_policy_quantiles=32, dueling=False,
                 initial_param_values=None):
        if dueling:
            raise NotImplementedError("dueling implicit quantile networks are not built (INTEGRATION.md, section E)")
        for name, n in (("n_quantiles", n_quantiles), ("n_target_quantiles", n_target_quantiles),
                        ("n_policy_quantiles", n_policy_quantiles)):
            if not 1 <= n <= _lib.IQN_MAX_FRACTIONS:
                raise NotImplementedError("%s must be in [1, %d]" % (name, _lib.IQN_MAX_FRACTIONS))
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, initial_param_values=initial_param_values)
        self._epsilon = epsilon
        self.n_quantiles, self.n_target_quantiles = n_quantiles, n_target_quantiles
        self.n_policy_quantiles = n_policy_quantiles
        self.serve_pair_rows = SERVE_PAIR_ROWS

    # ---- embedding layer + hidden layers (construction order) ----------------------------------------------------
    def _hidden_reference_init(self, fan):
        if fan % 4:
            raise NotImplementedError("the flattened conv output must be a multiple of 4 wide (got %d)" % fan)
        self._f = fan
        emb = [_norm_c((N_COS, fan), 1.0), np.zeros(fan, np.float32)]          # the hidden layers' rule
        hid, names, out = super()._hidden_reference_init(fan)
        return emb + hid, ["EmbW", "Embb"] + names, out

    def _hidden_internal_shapes(self):
        return [(self._f, N_COS), (self._f,)] + super()._hidden_internal_shapes()

    def _hidden_to_reference(self, arrs):
        w, b = arrs[0], arrs[1]                 # (F in (h, w, c) order, 64), (F): the unit axis is what gets permuted
        return ([self._conv_flat_to_reference(w.T).T, self._conv_flat_to_reference(b[None, :])[:, 0]] +
                super()._hidden_to_reference(arrs[2:]))

    def _hidden_to_internal(self, refs):
        w, b = refs[0], refs[1]                 # (64, F in (c, h, w) order), (F)
        return ([self._conv_flat_to_internal(w.T).T, self._conv_flat_to_internal(b[:, None])[0]] +
                super()._hidden_to_internal(refs[2:]))

    # ---- output layer: n_actions units at every (sample, fraction) row ---------------------------------------------
    def _head_reference_init(self, fan, n_act):
        if n_act > 64:
            raise NotImplementedError("at most 64 actions (a lane of a wave per action; got %d)" % n_act)
        self._a_stride = (n_act + 31) // 32 * 32
        return [_norm_c((fan, n_act), 0.01), np.zeros(n_act, np.float32)], ["OutputW", "Outputb"]

    def _head_internal_shapes(self, fan, n_act):
        return [(self._a_stride, fan), (self._a_stride,)]

    def _head_to_reference(self, wh, bh):
        return [wh[:self.n_act].T, bh[:self.n_act]]

    def _head_to_internal(self, ref_tail):
        w = np.zeros((self._a_stride, ref_tail[0].shape[0]), np.float32)
        b = np.zeros(self._a_stride, np.float32)
        w[:self.n_act] = ref_tail[0].T
        b[:self.n_act] = ref_tail[1]
        return [w, b]

    @property
    def _head_width(self):
        return self._a_stride

    def initialize(self, env_spec, device=None, **kwargs):
        super().initialize(env_spec, device=device, **kwargs)
        self._k_emb = 2 * self._n_conv
        self.iqn_seed = int(np.random.randint(1, 123456))
        self._iqn_state = torch.tensor([self.iqn_seed, 0], dtype=torch.int64, device=self.device)

    # ---- forward --------------------------------------------------------------------------------------------------
    def _trunk(self, x, w=None, tag=""):
        raise NotImplementedError("an implicit quantile network has no fraction-free trunk: _convs + _quantile_pass")

    def _pair_geoms(self, n):
        """Geometry records of the dense layers at n = B R rows: (embedding, [hidden ...], output)."""
        key = ("iqn", n, _lib.default_route)
        gs = self._geoms.get(key)
        if gs is None:
            gs = self._geoms[key] = (_lib.dense_geom(n, N_COS, self._f),
                                     [_lib.dense_geom(n, fan_in, hs) for hs, fan_in in self._hid_geom],
                                     _lib.dense_geom(n, self._hid_geom[-1][0], self._a_stride))
        return gs

    def _quantile_pass(self, psi, r, w=None, tag="", tau_in=None, row0=0, call_offset=0):
        """Everything after the conv stack for the b rows of psi at r fractions each.  tau_in f32[b r]: given fractions
        (None: drawn from _iqn_state's stream, read only).  Returns (tau, cosf, phi, x, hids, theta)."""
        w = self._w if w is None else w
        b, f = psi.shape[0], self._f
        n = b * r
        g_emb, g_hid, g_out = self._pair_geoms(n)
        tau = self._buffer(("tau" + tag, n), (n,))
        cosf = self._buffer(("cosf" + tag, n), (n, N_COS))
        _lib.iqn_embed(tau_in, None if tau_in is not None else self._iqn_state, b, r, tau, cosf, row0=row0,
                       call_offset=call_offset)
        ke = self._k_emb
        phi = self._buffer(("phi" + tag, n), (n, f))
        _lib.conv2d_fwd(cosf, w[ke], w[ke + 1], phi, g_emb, True, self._conv_ws)
        x = self._buffer(("merged" + tag, n), (n, f))
        _lib.iqn_merge_fwd(psi, phi, b, r, f, x)
        hids, a, k = [], x, ke + 2
        for j, (hs, fan_in) in enumerate(self._hid_geom):
            hcur = self._buffer(("hid" + tag, j, n), (n, hs))
            _lib.conv2d_fwd(a, w[k], w[k + 1], hcur, g_hid[j], True, self._conv_ws)
            hids.append(hcur)
            a = hcur
            k += 2
        theta = self._buffer(("theta" + tag, n), (n, self._a_stride))
        _lib.conv2d_fwd(a, w[k], w[k + 1], theta, g_out, False, self._conv_ws)
        return tau, cosf, phi, x, hids, theta

    # ---- serving --------------------------------------------------------------------------------------------------
    def _serve_obs(self, observations, override, onehot, greedy=None):
        """Epsilon-greedy / greedy actions of every row at K fractions each, in passes of at most serve_pair_rows // K
        rows.  Every pass reads the same call's stream at its rows' global indices, so the split changes no result;
        the last pass's action launch advances the counter by the number of passes."""
        rows, k = observations.shape[0], self.n_policy_quantiles
        per = max(1, self.serve_pair_rows // k)
        starts = list(range(0, rows, per))
        for lo in starts:
            hi = min(lo + per, rows)
            obs = observations[lo:hi]
            psi = self._convs(self._scaled(obs, tag="s"), tag="s")[-1]
            theta = self._quantile_pass(psi.view(hi - lo, self._f), k, tag="s", row0=lo)[-1]
            last = hi == rows
            _lib.iqn_act(theta, None if override is None else override[lo:hi], self.n_act, k, onehot[lo:hi],
                         None if greedy is None else greedy[lo:hi], state=self._iqn_state if last else None,
                         advance=len(starts) if last else 0)

    # ---- training -------------------------------------------------------------------------------------------------
    def _loss_and_backward(self, x, acts, online, b, launch):
        """What both losses do once their forward passes are made (online: _quantile_pass of the online net on obs):
        launch(theta, tau, dtheta, loss_rows, priorities) is the loss kernel, then the full backward pass into flat_grads.
        Returns (loss_rows, priorities), the two rows of one (2, B) buffer."""
        tau, cosf, phi, merged, hids, theta = online
        n = self.n_quantiles
        dtheta = self._buffer(("dtheta", b), (b * n, self._a_stride))
        pack = self._buffer(("loss_pri", b), (2, b))        # one buffer: DqnOptimizer's statistics ring takes both rows at once
        loss_rows, priorities = pack[0], pack[1]
        launch(theta, tau, dtheta, loss_rows, priorities)
        self._pair_backward(x, acts, acts[-1].view(b, self._f), cosf, phi, merged, hids, dtheta, b, n)
        return loss_rows, priorities

    def iqn_loss_and_grads(self, obs, next_obs, actions, returns, terminals, is_weights, gamma_n, kappa,
                           double_dqn=False, taus=None):
        """One minibatch of ImplicitQuantileDQN.build_loss: the online net on obs at N fractions, the target net (and,
        for double DQN, the online net) on next_obs at N' fractions -- three passes with fractions drawn at call offsets
        0, 1, 2 --, the quantile-Huber loss at the drawn fractions (kappa 0: plain quantile regression) and the full
        backward pass into flat_grads.  taus = (tau_pred f32[B N], tau_tgt f32[B N'], tau_pol f32[B N'] or None): given
        fractions, and the call counter stays as it is.  Returns (loss_rows f32[B] whose sum is the loss, priorities
        f32[B]).  No host synchronisation and no allocation outside _buffer: it runs inside the captured update graph."""
        with torch.no_grad():
            b, f = obs.shape[0], self._f
            n, m = self.n_quantiles, self.n_target_quantiles
            t_pred, t_tgt, t_pol = taus if taus is not None else (None, None, None)
            if double_dqn and self._u8:             # the two online conv passes as ONE pass over 2B rows (_forward_for_loss)
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
            online = self._quantile_pass(psi, n, tau_in=t_pred, call_offset=0)
            tgt = self._quantile_pass(psi_t.view(b, f), m, w=self._w_target, tag="t", tau_in=t_tgt, call_offset=1)[-1]
            pol = None
            if double_dqn:
                pol = self._quantile_pass(psi_d.view(b, f), m, tag="d", tau_in=t_pol, call_offset=2)[-1]

            def launch(theta, tau, dtheta, loss_rows, priorities):
                _lib.iqn_loss(theta, tau, tgt, pol, actions, returns, terminals, is_weights, self.n_act, n, m, gamma_n,
                              kappa, dtheta, loss_rows, priorities,
                              state=None if taus is not None else self._iqn_state, advance=3)

            return self._loss_and_backward(x, acts, online, b, launch)

    def munchausen_loss_and_grads(self, obs, next_obs, actions, returns, terminals, is_weights, gamma_n, kappa, tau_e,
                                  alpha, l0, taus=None):
        """One minibatch of MunchausenIQN.build_loss: the online net on obs at N fractions (call offset 0), the target net
        on next_obs (offset 1) and on obs (offset 2) at N' fractions each -- the target conv stack runs once over the 2B
        rows of _pair_rows where the observations are u8 --, the Munchausen quantile-Huber loss of
        csrc/iqn.hip:arl_miqn_loss and the full backward pass into flat_grads.  taus = (tau_pred f32[B N], tau_next
        f32[B N'], tau_cur f32[B N']): given fractions, and the call counter stays as it is.  Returns (loss_rows, priorities)
        as iqn_loss_and_grads.  No host synchronisation and no allocation outside _buffer."""
        with torch.no_grad():
            b, f = obs.shape[0], self._f
            n, m = self.n_quantiles, self.n_target_quantiles
            t_pred, t_next, t_cur = taus if taus is not None else (None, None, None)
            if self._u8:
                both = self._pair_rows(obs, next_obs)
                psi_t2 = self._convs(ObsRows(both, None), w=self._w_target, tag="t2")[-1].view(2 * b, f)
                psi_tc, psi_tn = psi_t2[:b], psi_t2[b:]
                x = ObsRows(both[:b], None)
            else:
                psi_tn = self._convs(self._scaled(next_obs, tag="n"), w=self._w_target, tag="t")[-1].view(b, f)
                x = self._scaled(obs)
                psi_tc = self._convs(x, w=self._w_target, tag="tc")[-1].view(b, f)
            acts = self._convs(x)
            psi = acts[-1].view(b, f)
            online = self._quantile_pass(psi, n, tau_in=t_pred, call_offset=0)
            tgt_next = self._quantile_pass(psi_tn, m, w=self._w_target, tag="t", tau_in=t_next, call_offset=1)[-1]
            tgt_cur = self._quantile_pass(psi_tc, m, w=self._w_target, tag="tc", tau_in=t_cur, call_offset=2)[-1]

            def launch(theta, tau, dtheta, loss_rows, priorities):
                _lib.miqn_loss(theta, tau, tgt_next, tgt_cur, actions, returns, terminals, is_weights, self.n_act, n, m,
                               gamma_n, kappa, tau_e, alpha, l0, dtheta, loss_rows, priorities,
                               state=None if taus is not None else self._iqn_state, advance=3)

            return self._loss_and_backward(x, acts, online, b, launch)

    def _pair_backward(self, x, acts, psi, cosf, phi, merged, hids, dtheta, b, r):
        """Backward of one online pass at b r rows: output layer, hidden layers, the merge, the embedding layer's weight
        gradient, then the conv stack at b rows."""
        n, f = b * r, self._f
        g_emb, g_hid, g_out = self._pair_geoms(n)
        k = self._k_head
        dh = self._buffer(("dh", n), (n, self._hid_geom[-1][0]))
        done = self._folds.conv2d_bwd_pair(dtheta, self._w[k], hids[-1], dh, hids[-1], self._g[k], g_out,
                                           self._fold_ws(("dw", k)), dbias=self.grads[k + 1])
        if not done:        # generic kernels
            self._bias_grad_by_ones(dtheta, n, k)
        d_cur = dh
        for j in range(self._n_hid - 1, -1, -1):
            k -= 2
            hs, fan_in = self._hid_geom[j]
            inp = hids[j - 1] if j > 0 else merged
            d_prev = self._buffer(("dx_hid", j, n), (n, fan_in))
            # The data gradient is multiplied by the rectifier mask of `inp`.  For j == 0 that input is the merged
            # x = psi * phi, which no rectifier produced -- but x == 0 only where psi == 0, phi == 0 or their product
            # underflowed.  In the first two cases the mask is harmless: dphi = g psi is masked by phi > 0 and is 0
            # where psi == 0; dpsi's term g phi is 0 where phi == 0 and masked by psi > 0.  Where two positive factors
            # underflow to 0 the mask does drop a gradient that is not small (dphi = g psi with a normal psi and a phi
            # in (0, ~2^-74)); only the gradient toward the other factor is negligible there.  That case is practically
            # unreachable -- a rectified unit would have to land in that interval -- and is accepted, not corrected.
            self._layer_grads(d_cur, True, hids[j], n, hs, k, g_hid[j], inp, d_prev)
            d_cur = d_prev
        dphi = self._buffer(("dphi", n), (n, f))
        dpsi = self._buffer(("dpsi", b), (b, f))
        _lib.iqn_merge_bwd(d_cur, psi, phi, b, r, f, dphi, dpsi)
        # the embedding layer's input (the cosine features) has no gradient: weight + bias gradient only
        self._layer_grads(dphi, True, phi, n, f, self._k_emb, g_emb, cosf, None)
        self._backward_convs(x, acts, dpsi.view(acts[-1].shape), masked=True)
