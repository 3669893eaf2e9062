"""R2D2's recurrent Q policy for Atari (Kapturowski et al. 2019; the reference has none): conv stack -> one LSTM layer ->
a linear output layer on h; a target network; epsilon-greedy action serving from the kept recurrent state.

The network up to h is AtariLstmPolicy's (same cell hooks, same parameter layout, same scans: RecurrentCnnPolicy's
`_forward_scan` / `_backward_scan`); what the Q policies carry besides their network -- target bucket, epsilon, override
tables -- is q_policy_base.EpsGreedyTargetMixin.  The output layer is one dense MFMA call whose row is padded to 32
columns (zero weights, zero gradients), as AtariDqnPolicy's: n_actions values, or with `dueling` (the default) n_actions
advantages followed by the value, merged (val + (adv - mean adv)) inside arl_dqn_act and arl_r2d2_loss.  The paper's
two-stream hidden layers between the LSTM and the outputs are not built.

Training (`r2d2_loss_and_grads`) takes the sequence replay's rows [sequence][time], U = burn_in + train_len + n per
sequence: conv features and the LSTM unroll of all U steps from the stored state with the online and with the target
parameters (the reset-aware hand-over wherever the sampler zeroed the state), both output layers, csrc/r2d2.hip:
arl_r2d2_loss, then BPTT over the train window only -- the state at the end of the burn-in is a constant, and no
gradient crosses a reset."""
import numpy as np
import torch

from accel_rl_amd import _lib
from accel_rl_amd.policies.atari_cnn_policy import _norm_c
from accel_rl_amd.policies.atari_lstm_policy import AtariLstmPolicy
from accel_rl_amd.policies.dqn.q_policy_base import EpsGreedyTargetMixin


class AtariR2d2Policy(EpsGreedyTargetMixin, AtariLstmPolicy):

    def __init__(self, conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=(), pixel_scale=255.,
                 epsilon=1, dueling=True, initial_param_values=None):
        super().__init__(conv_filters, conv_filter_sizes, conv_strides, conv_pads, hidden_sizes=hidden_sizes,
                         pixel_scale=pixel_scale, initial_param_values=initial_param_values)
        self._epsilon = epsilon
        self._dueling = bool(dueling)

    # ---- output layer: n_actions units [+ "Val", 1 unit], stored as one matrix of q_stride rows
    def _head_reference_init(self, fan, n_act):
        self._q_stride = (n_act + int(self._dueling) + 31) // 32 * 32
        ref, names = [_norm_c((fan, n_act), 0.01), np.zeros(n_act, np.float32)], ["OutputW", "Outputb"]
        if self._dueling:
            ref += [_norm_c((fan, 1), 0.01), np.zeros(1, np.float32)]
            names += ["ValW", "Valb"]
        return ref, names

    def _head_internal_shapes(self, fan, n_act):
        return [(self._q_stride, fan), (self._q_stride,)]

    def _head_to_reference(self, wh, bh):
        a = self.n_act
        out = [wh[:a].T, bh[:a]]
        return out + [wh[a:a + 1].T, bh[a:a + 1]] if self._dueling else out

    def _head_to_internal(self, ref_tail):
        a = self.n_act
        w = np.zeros((self._q_stride, ref_tail[0].shape[0]), np.float32)
        b = np.zeros(self._q_stride, np.float32)
        w[:a], b[:a] = ref_tail[0].T, ref_tail[1]
        if self._dueling:
            w[a], b[a] = ref_tail[2][:, 0], ref_tail[3][0]
        return [w, b]

    def initialize(self, env_spec, device=None, **kwargs):
        super().initialize(env_spec, device=device, **kwargs)
        # (from here on `_step` is the mixin's step number of the override table, as in every Q policy; the serving step
        # of this class is `_q_step`, and RecurrentCnnPolicy._step -- the actor-critic heads -- is never called)
        self._init_target_and_tables()

    # ---- forward ---------------------------------------------------------------
    def _q_rows(self, h, w, tag):
        """[rows, q_stride] output-layer values on h [rows, H] with the (W, b) views `w`."""
        rows, kh = h.shape[0], self._k_head
        out = self._buffer(("q" + tag, rows), (rows, self._q_stride))
        _lib.conv2d_fwd(h, w[kh], w[kh + 1], out, self._geom(rows, self._H, self._q_stride), False, self._conv_ws)
        return out

    def _q_step(self, observations, prev, tag="s", w=None):
        """One step from the states `prev` -> (q [b, q_stride], new states), with the (W, b) views `w` (default: online)."""
        b, hh, gm = observations.shape[0], self._H, self._gate_mult
        w, k = self._w if w is None else w, self._k_x
        xf = self._convs(self._scaled(observations, tag=tag), w, tag)[-1].view(b, -1)
        gx = self._buffer(("gx" + tag, b), (b, gm * hh))
        gh = self._buffer(("gh" + tag, b), (b, gm * hh))
        _lib.conv2d_fwd(xf, w[k], w[k + 2], gx, self._geom(b, self._rec_fan, gm * hh), False, self._conv_ws)
        _lib.conv2d_fwd(prev[0], w[k + 1], None, gh, self._geom(b, hh, gm * hh), False, self._conv_ws)
        new = [self._buffer(("new%d" % i + tag, b), (b, hh)) for i in range(len(prev))]
        self._cell_fwd(gx, gh, prev, new, None)
        return self._q_rows(new[0], w, tag), new

    def _zeros(self, b):
        if getattr(self, "_zero_value", None) is None or self._zero_value.numel() != b:
            self._zero_value = torch.zeros(b, dtype=torch.float32, device=self.device)
        return self._zero_value

    def _state_rows(self, b, rows):
        state = self._state if rows is None else [s[rows[0]:rows[1]] for s in self._state]
        if state[0].shape[0] != b:
            raise ValueError("%d observations for %d state rows" % (b, state[0].shape[0]))
        return state

    def prob_value(self, observations, state_infos=None):
        """(one-hot row of this step's epsilon-greedy action, zero value); does NOT advance the state."""
        with torch.no_grad():
            b = observations.shape[0]
            prev = self._state if state_infos is None else list(state_infos)
            q, _ = self._q_step(observations, prev, tag="v")
            onehot = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
            _lib.dqn_act(q, self._step_overrides(b), self.n_act, onehot, None, dueling=self._dueling)
            return onehot, self._zeros(b)

    def act_step(self, observations, rows=None):
        """The sampler's serving call: (one-hot prob, zero value, *previous state), through arl_dqn_act with the step's
        row of the override table, and the state advances.  The returned previous state is only valid until the next
        act_step.  rows = (lo, hi): the observations are those of state rows lo .. hi - 1 only."""
        with torch.no_grad():
            b = observations.shape[0]
            state = self._state_rows(b, rows)
            ret = [self._buffer(("prev_ret%d" % i, b), (b, self._H)) for i in range(len(state))]
            for r, s in zip(ret, state):
                r.copy_(s)
            q, new = self._q_step(observations, state)
            override = self._step_overrides(self._state[0].shape[0])
            if override is not None and rows is not None:
                override = override[rows[0]:rows[1]]
            onehot = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
            _lib.dqn_act(q, override, self.n_act, onehot, None, dueling=self._dueling)
            for s, n in zip(state, new):
                s.copy_(n)
            return (onehot, self._zeros(b)) + tuple(ret)

    def q_values(self, observations, state_infos=None, target=False):
        """Host-interface twin: the merged action values f32 [b, n_actions] from the kept (or the given) state, with the
        online or the target parameters; does not advance the state."""
        with torch.no_grad():
            prev = self._state if state_infos is None else list(state_infos)
            out, _ = self._q_step(observations, prev, tag="qt" if target else "q", w=self._w_target if target else None)
            adv = out[:, :self.n_act]
            if not self._dueling:
                return adv.clone()
            return out[:, self.n_act:self.n_act + 1] + (adv - adv.mean(dim=1, keepdim=True))

    def greedy_actions(self, observations, state_infos=None):
        """u8 [b]: first maximum of the action values from the kept (or the given) state; does not advance the state."""
        with torch.no_grad():
            b = observations.shape[0]
            prev = self._state if state_infos is None else list(state_infos)
            q, _ = self._q_step(observations, prev, tag="g")
            onehot = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
            greedy = torch.empty(b, dtype=torch.uint8, device=self.device)
            _lib.dqn_act(q, None, self.n_act, onehot, greedy, dueling=self._dueling)
            return greedy

    def _advance_greedy(self, observations):
        """greedy actions of one served step, the state advancing (the host-interface calls below)."""
        with torch.no_grad():
            b = observations.shape[0]
            state = self._state_rows(b, None)
            prev = [s.clone() for s in state]
            q, new = self._q_step(observations, state)
            onehot = torch.empty((b, self.n_act), dtype=torch.float32, device=self.device)
            greedy = torch.empty(b, dtype=torch.uint8, device=self.device)
            _lib.dqn_act(q, None, self.n_act, onehot, greedy, dueling=self._dueling)
            for s, n in zip(state, new):
                s.copy_(n)
            return greedy, prev

    def get_actions(self, observations, deterministic=False):
        """Host-interface twin of the Q policies' get_actions (one group of one step); the state advances."""
        greedy, prev = self._advance_greedy(observations)
        acts = greedy.cpu().numpy()
        if not deterministic:
            idx = np.where(np.random.rand(len(acts)) < self._epsilon)[0]
            acts[idx] = np.random.randint(low=0, high=self.n_act, size=len(idx), dtype=np.uint8)
        return acts, dict(zip(self._state_keys, prev))

    def get_action(self, observation, deterministic=False):
        if self._state is None or self._state[0].shape[0] != 1:
            self.reset(n_batch=1)
        greedy, prev = self._advance_greedy(observation[None])
        if deterministic or (np.random.rand() > self._epsilon):
            action = int(greedy[0].item())
        else:
            action = self.action_space.sample()
        return action, {k: p[0] for k, p in zip(self._state_keys, prev)}

    def loss_and_grads(self, *args, **kwargs):
        raise NotImplementedError("AtariR2d2Policy trains by r2d2_loss_and_grads (algos/dqn/r2d2.py: R2D2), not by the "
                                  "actor-critic losses")

    # ---- training ------------------------------------------------------------
    def r2d2_loss_and_grads(self, obs, act, ret, term, resets, init_states, is_weights, gamma_n, burn_in, train_len, n,
                            rescale_eps=1e-3, eta=0.9):
        """One minibatch of R2D2's loss: obs u8 [B * U, C, H, W], act u8, ret f32, term u8 / bool, resets u8 (non-zero
        where the state was zeroed after that row's step), all [B * U] in [sequence][time] order with
        U = burn_in + train_len + n; init_states: the stored state before each sequence's first step, one [B, H] tensor
        per state key; is_weights f32 [B] or None.  Leaves the gradient in flat_grads and returns (loss_rows f32[B] whose
        sum is the loss, priorities f32[B]), the two rows of one (2, B) buffer; |TD| of the train window stays in
        `self.last_td_abs` [B, train_len].  No host synchronisation and no allocation outside _buffer: it runs inside the
        captured update graph."""
        with torch.no_grad():
            u_len = burn_in + train_len + n
            rows = obs.shape[0]
            nb = rows // u_len
            if nb * u_len != rows or act.numel() != rows or len(init_states) != len(self._state_keys):
                raise ValueError("r2d2_loss_and_grads: %d rows are not sequences of %d + %d + %d steps, or %d states for "
                                 "%d state keys" % (rows, burn_in, train_len, n, len(init_states), len(self._state_keys)))
            if term.dtype == torch.bool:
                term = term.view(torch.uint8)
            if resets.dtype == torch.bool:
                resets = resets.view(torch.uint8)
            init = list(init_states)
            kh, g = self._k_head, self.grads
            # target network: conv features, unroll, output layer (nothing kept for a backward pass)
            acts_t = self._convs(self._scaled(obs, tag="t"), self._w_target, "t")
            scan_t = self._forward_scan(acts_t[-1].view(rows, -1), nb, u_len, self._w_target, init, resets, None,
                                        tag="t", keep=False)
            q_tgt = self._q_rows(scan_t["st_all"][0], self._w_target, "t")
            # online network
            x = self._scaled(obs)
            acts, xf = self._conv_features(x)
            scan = self._forward_scan(xf, nb, u_len, self._w, init, resets, None)
            h_all = scan["st_all"][0]
            q = self._q_rows(h_all, self._w, "")
            self.last_q, self.last_q_tgt = q, q_tgt
            dq = self._buffer(("dq", rows), (rows, self._q_stride))
            pack = self._buffer(("loss_prio", nb), (2, nb))     # one buffer: DqnOptimizer's statistics ring takes both rows
            loss_rows, priorities = pack[0], pack[1]
            td_abs = self.last_td_abs = self._buffer(("td_abs", nb, train_len), (nb, train_len))
            _lib.r2d2_loss(q, q_tgt, act, ret, term, is_weights, nb, burn_in, train_len, n, self.n_act, gamma_n,
                           rescale_eps, eta, dq, td_abs, loss_rows, priorities, dueling=self._dueling)
            # output layer backward: dW = dq^T h, db = column sums of dq, dh = dq W (zero outside the train window)
            g_head = self._geom(rows, self._H, self._q_stride)
            _lib.conv2d_bwd_weight(dq, h_all, self._g[kh], g_head, self._conv_ws)
            self._bias_grad_by_ones(dq, rows, kh)
            dh_all = self._buffer(("dh_all", rows), (rows, self._H))
            _lib.conv2d_bwd_data(dq, self._w[kh], None, dh_all, g_head)
            # BPTT over the train window only; the gate gradients of every other row are zero
            self._backward_scan(scan, dh_all, burn_in, burn_in + train_len)
            for name in ("dgx", "dgh") if self._separate_dgh else ("dgx",):
                d3 = scan[name].view(nb, u_len, -1)
                if burn_in:
                    d3[:, :burn_in].zero_()
                d3[:, burn_in + train_len:].zero_()
            self._recurrent_grads(scan, x, acts, xf)
            return loss_rows, priorities
