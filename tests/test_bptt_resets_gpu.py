"""Reset-aware BPTT: arl_seq_handover (csrc/handover.hip), arl_{lstm,gru,rnn}_cell_bwd_reset
(csrc/lstm.hip, csrc/gru.hip), RecurrentCnnPolicy.loss_and_grads with mb["resets"], and A2C / RecurrentPPO with
bptt_resets=True under mid_batch_reset=True.

reset[row] != 0 at (j, t) of a [trajectory][time] batch: the recurrent state was set to zero AFTER step t of trajectory
j.  The masked recurrence is restated here in float64 (`_masked_prob_value`): the previous state of step t > 0 is
state[t-1] (1 - reset[t-1]); step 0 takes the stored state; a reset after the last step changes nothing.

1. Kernels through the C ABI against float64, every array inside a NaN-filled buffer, everything outside the addressed
   rows checked bit for bit (the construction and helpers of test_recurrent_limits_gpu.py).  The hand-over's outputs
   are copies or +0: exact.  The backward cells are held to that module's bound for the same outputs,
   max(4 E(fp32 numpy restatement), 4 * 2^-23) per case, E as defined there: leaving a gradient out adds no rounding.
   The masked formula is the plain one on inputs whose recurrent gradients are zero on the flagged rows.
   Worst figures over this module's cases (kernel = worst E observed on an MI355X, LABNOTES.md):

     kernel          output    E(fp32 numpy)   bound      kernel on gfx950
     lstm_bwd_reset  dgates    1.46e-07        5.82e-07   1.46e-07
     lstm_bwd_reset  dc_prev   1.25e-07        5.01e-07   1.25e-07
     gru_bwd_reset   dgx       1.5e-07         5.98e-07   1.5e-07
     gru_bwd_reset   dgh       1.44e-07        5.77e-07   1.44e-07
     gru_bwd_reset   dh_prev   1.7e-07         6.79e-07   1.7e-07
     rnn_bwd_reset   dpre      1.34e-07        5.37e-07   1.34e-07
     seq_handover    (all)     exact           exact      exact

   ARL_RESET_REPORT=path makes the module write every figure it measured to that file.
2. Refusals leave NaN-filled outputs untouched.
3. BPTT against float64 autograd (PPO loss, the formula of test_recurrent_ppo_gpu._ref_ppo_losses on the masked
   recurrence) at that module's bars, whole batch and trajectory minibatch; the float64 gradient that ignores the mask
   must miss the same bar by more than a factor 10, so a learner that ignored the mask could not pass.
4. Bits: an all-zero mask is today's path; a reset after every step is a batch of one-step segments.
5. Sampler and learner agree on the mask (episodic lives: `dones` alone is the wrong mask).
6. Training end to end, captured and eager, and the refusal that stays.
"""
import os

import numpy as np
import pytest
import torch

from test_recurrent_limits_gpu import (EPS, KERNELS, _Slot, _call, _contiguous, _err, _inputs, _nan_bits, _ref, _scales,
                                       _slice_layout)
from test_recurrent_ppo_gpu import (CLIP, ENT_COEFF, GRAD_ATOL, GRAD_RTOL, KINDS, TINY, V_COEFF, _data, _flat_grads, _make,
                                    _mb, _policy_cls, _ref_features, _ref_params, _ref_ppo_losses, _ref_step)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3
BWD = ["lstm_bwd", "gru_bwd", "rnn_bwd"]
REC_GRADS = dict(lstm_bwd=("dh_rec", "dc_next"), gru_bwd=("dh_rec", "dh_dir"), rnn_bwd=("dh_rec",))
BATCHES, HIDDENS = [1, 3, 65], [4, 8, 260, 1024]
PATTERNS = ["zero", "one", "mix"]


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# flags: a full-batch u8 array, optionally behind a row map, addressed as compact row row0 + b * row_step
# ---------------------------------------------------------------------------------------------------------------------

class _Flags(object):
    """want[b]: the flag launch row b must see.  Every entry of the full array the launch must NOT read holds the
    opposite value where the pattern allows, set flags are 1, 2 or 255 (non-zero is what counts), and the row map is a
    non-identity permutation into a longer array."""

    def __init__(self, rs, batch, row0, row_step, pattern, with_idx):
        n_compact = batch * row_step
        rows = row0 + np.arange(batch) * row_step
        if pattern == "mix":
            want = rs.randint(0, 2, size=batch)
            want[0] = 1
            if batch > 1:
                want[1] = 0
            full_len = n_compact + (5 if with_idx else 0)
            full = rs.randint(0, 2, size=full_len)
        else:
            want = np.full(batch, int(pattern == "one"))
            full_len = n_compact + (5 if with_idx else 0)
            full = np.full(full_len, int(pattern != "one"))
        idx = None
        if with_idx:
            idx = rs.permutation(full_len)[:n_compact]
            if (idx[rows] == rows).all():
                idx = full_len - 1 - np.arange(n_compact)
            assert not (idx[rows] == rows).all() and len(set(idx.tolist())) == n_compact
        pos = rows if idx is None else idx[rows]
        full[pos] = want
        if pattern == "mix" and batch > 1:
            assert (want == 0).any() and (want != 0).any()     # at least one row of each value
        full = (full * rs.choice([1, 2, 255], size=full_len)).astype(np.uint8)
        assert ((full[pos] != 0) == (want != 0)).all()
        self.want = want.astype(bool)
        self.reset = _dev(full)
        self.idx = None if idx is None else _dev(idx.astype(np.int32))
        self.row0, self.row_step = int(row0), int(row_step)
        self._before = (self.reset.clone(), None if idx is None else self.idx.clone())

    def args(self):
        return (self.reset.data_ptr(), None if self.idx is None else self.idx.data_ptr(), self.row0, self.row_step)

    def unchanged(self):
        return torch.equal(self.reset, self._before[0]) and (self.idx is None or torch.equal(self.idx, self._before[1]))


def _call_reset(L, kernel, A, batch, hidden, F):
    """The reset-aware C entry point; A: name -> (pointer or None, row stride); F: (reset, idx, row0, row_step)."""
    lib, st = L.load(), L.stream_ptr()
    p, s = (lambda n: A[n][0]), (lambda n: A[n][1])
    if kernel == "lstm_bwd":
        return lib.arl_lstm_cell_bwd_reset(p("dh"), s("dh"), p("dh_rec"), p("dc_next"), p("gates"), s("gates"), p("c_prev"),
                                           s("c_prev"), p("c"), s("c"), batch, hidden, p("dgates"), s("dgates"),
                                           p("dc_prev"), F[0], F[1], F[2], F[3], st)
    if kernel == "gru_bwd":
        return lib.arl_gru_cell_bwd_reset(p("dh"), s("dh"), p("dh_rec"), p("dh_dir"), p("saved"), s("saved"), p("h_prev"),
                                          s("h_prev"), batch, hidden, p("dgx"), s("dgx"), p("dgh"), s("dgh"), p("dh_prev"),
                                          F[0], F[1], F[2], F[3], st)
    if kernel == "rnn_bwd":
        return lib.arl_rnn_cell_bwd_reset(p("dh"), s("dh"), p("dh_rec"), p("h"), s("h"), batch, hidden, p("dpre"),
                                          s("dpre"), F[0], F[1], F[2], F[3], st)
    assert kernel == "handover"
    return lib.arl_seq_handover(p("h_prev"), s("h_prev"), p("c_prev"), s("c_prev"), F[0], F[1], F[2], F[3], batch, hidden,
                                p("hp"), p("hprev_out"), s("hprev_out"), p("cprev_out"), s("cprev_out"), st)


HANDOVER = dict(ins=[("h_prev", 1, True, False), ("c_prev", 1, True, True)],
                outs=[("hp", 1, False, False), ("hprev_out", 1, True, False), ("cprev_out", 1, True, True)])


def _spec(kernel):
    return HANDOVER if kernel == "handover" else KERNELS[kernel]


def _run(L, kernel, x, batch, hidden, layout, F, absent=(), plain=False):
    """One launch on host arrays x in NaN-filled buffers: the outputs as numpy arrays, after checking that nothing
    outside the addressed rows changed, inputs (and flags) included.  F = None: a NULL flag pointer; plain: the
    existing entry point without flags."""
    slots, A, outs = {}, {}, []
    for name, mult, strided, optional in _spec(kernel)["ins"] + _spec(kernel)["outs"]:
        is_out = (name, mult, strided, optional) in _spec(kernel)["outs"]
        if name in absent:
            assert optional
            A[name] = (None, 0)
            continue
        w = mult * hidden
        stride, off = layout(name, w, batch) if strided else (w, 0)
        slots[name] = _Slot(batch, w, stride, off, data=None if is_out else x[name])
        A[name] = (slots[name].ptr, stride)
        if is_out:
            outs.append(name)
    if plain:
        rc = _call(L, kernel, A, batch, hidden)
    else:
        rc = _call_reset(L, kernel, A, batch, hidden, (None, None, 0, 1) if F is None else F.args())
    L._check(rc, kernel)
    torch.cuda.synchronize()
    got = {name: slots[name].rows() for name in outs}
    for name in outs:
        assert slots[name].outside_untouched(), (kernel, name, "wrote outside its rows")
    for name in slots:
        if name not in outs:
            assert slots[name].unchanged(), (kernel, name, "input modified")
    assert F is None or F.unchanged()
    return got


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


REPORT = {}          # (kernel, output) -> [worst E(fp32 numpy), worst bound, worst E(kernel)]


def _write_report():
    path = os.environ.get("ARL_RESET_REPORT")
    if path:
        with open(path, "w") as f:
            for (k, o), (e32, b, ek) in sorted(REPORT.items()):
                f.write("%-14s %-8s fp32-numpy %.3g  bound %.3g  kernel %.3g\n" % (k + "_reset", o, e32, b, ek))


def _masked_inputs(kernel, x, want):
    """The masked formula's inputs: nothing arrives from step t + 1 on the rows whose flag is set."""
    xm = dict(x)
    for k in REC_GRADS[kernel]:
        xm[k] = np.where(want[:, None], np.float32(0), x[k])
    return xm


def _compare(kernel, xm, got, what):
    want64, want32, s = _ref(kernel, xm, np.float64), _ref(kernel, xm, np.float32), _scales(kernel, xm)
    for name, g in got.items():
        assert g.dtype == np.float32 and g.shape == want64[name].shape
        e32, valid = _err(want32[name], want64[name], s[name])
        ek, _ = _err(g, want64[name], s[name])
        bound = max(4. * e32, 4. * EPS)
        print("%s %s_reset.%s: E(fp32 numpy) %.3g  bound %.3g  E(kernel) %.3g" % (what, kernel, name, e32, bound, ek))
        assert valid.all() and e32 < 1e-5, (kernel, name, e32)
        r = REPORT.setdefault((kernel, name), [0., 0., 0.])
        r[:] = [max(r[0], e32), max(r[1], bound), max(r[2], ek)]
        _write_report()
        assert ek <= bound, (what, kernel, name, ek, bound)


def _layouts():
    """(name, layout, flag row0, flag row_step): contiguous rows; time slice 1 of T = 3 in place."""
    return [("rows", _contiguous, 0, 1), ("T3t1", _slice_layout(3, 1), 1, 3)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels against float64
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden", HIDDENS)
@pytest.mark.parametrize("kernel", BWD)
def test_reset_backward_cells_vs_float64(L, kernel, hidden):
    for batch in BATCHES:
        for lname, layout, row0, row_step in _layouts():
            rs = np.random.RandomState(1000 * BWD.index(kernel) + 7 * hidden + batch + row0)
            x = _inputs(kernel, rs, batch, hidden)
            plain = _run(L, kernel, x, batch, hidden, layout, None, plain=True)
            null = _run(L, kernel, x, batch, hidden, layout, None)
            for name in plain:                                  # NULL flags: the existing entry point, bit for bit
                assert _bits_equal(null[name], plain[name]), (kernel, name, "null flags", batch, hidden, lname)
            for with_idx in (False, True):
                for pattern in PATTERNS:
                    F = _Flags(rs, batch, row0, row_step, pattern, with_idx)
                    got = _run(L, kernel, x, batch, hidden, layout, F)
                    what = "B%d H%d %s %s%s" % (batch, hidden, lname, pattern, " idx" if with_idx else "")
                    _compare(kernel, _masked_inputs(kernel, x, F.want), got, what)
                    if pattern == "zero":                       # an all-zero mask: the existing kernel's bits
                        for name in plain:
                            assert _bits_equal(got[name], plain[name]), (what, name)
                    if pattern == "one":                        # ... and all ones: the call without the recurrent gradients
                        absent = REC_GRADS[kernel]
                        bare = _run(L, kernel, {k: (None if k in absent else v) for k, v in x.items()}, batch, hidden,
                                    layout, None, absent=absent, plain=True)
                        for name in bare:
                            assert _bits_equal(got[name], bare[name]), (what, name)


@pytest.mark.parametrize("hidden", HIDDENS)
def test_handover_is_exact(L, hidden):
    for batch in BATCHES:
        for lname, layout, row0, row_step in _layouts():
            rs = np.random.RandomState(31 * hidden + batch + row0)
            x = dict(h_prev=rs.randn(batch, hidden).astype(np.float32), c_prev=rs.randn(batch, hidden).astype(np.float32))
            x["h_prev"][0, 0] = -0.0                            # a stored -0 is copied as it is
            for with_idx in (False, True):
                for pattern in PATTERNS:
                    for with_c in (True, False):
                        F = _Flags(rs, batch, row0, row_step, pattern, with_idx)
                        absent = () if with_c else ("c_prev", "cprev_out")
                        got = _run(L, "handover", x, batch, hidden, layout, F, absent=absent)
                        want_h = np.where(F.want[:, None], np.float32(0), x["h_prev"])      # +0 where reset
                        want_c = np.where(F.want[:, None], np.float32(0), x["c_prev"])
                        what = (batch, hidden, lname, pattern, with_idx, with_c)
                        assert set(got) == ({"hp", "hprev_out", "cprev_out"} if with_c else {"hp", "hprev_out"})
                        assert _bits_equal(got["hp"], want_h) and _bits_equal(got["hprev_out"], want_h), what
                        if with_c:
                            assert _bits_equal(got["cprev_out"], want_c), what


# ---------------------------------------------------------------------------------------------------------------------
# 2. refusals
# ---------------------------------------------------------------------------------------------------------------------

def _small(kernel, batch=2, hidden=8):
    keep, A, outs = {}, {}, []
    for name, mult, strided, optional in _spec(kernel)["ins"] + _spec(kernel)["outs"]:
        is_out = (name, mult, strided, optional) in _spec(kernel)["outs"]
        t = torch.full((batch, mult * hidden), NAN, device=DEV) if is_out else torch.rand(batch, mult * hidden, device=DEV)
        keep[name] = t
        A[name] = (t.data_ptr(), mult * hidden)
        if is_out:
            outs.append(t)
    return A, keep, outs


@pytest.mark.parametrize("kernel", BWD + ["handover"])
def test_refusals_leave_the_outputs_untouched(L, kernel):
    lib = L.load()
    A, keep, outs = _small(kernel)
    flags = torch.zeros(16, dtype=torch.uint8, device=DEV)
    F = (flags.data_ptr(), None, 0, 1)
    fn = "arl_seq_handover" if kernel == "handover" else "arl_%s_cell_bwd_reset" % kernel.split("_")[0]

    def refused(code, A_=A, batch=2, hidden=8, F_=F):
        rc = _call_reset(L, kernel, A_, batch, hidden, F_)
        msg = lib.arl_last_error().decode()
        assert rc == code and fn in msg, (rc, code, msg)
    for name, mult, strided, optional in _spec(kernel)["ins"] + _spec(kernel)["outs"]:
        if not optional or kernel == "handover":                 # (the hand-over's c_prev / cprev_out go together)
            refused(E_ARG, dict(A, **{name: (None, A[name][1])}))
        if strided:
            for stride in (mult * 8 - 4, 0, -mult * 8, (1 << 28) + 4, 1 << 62):
                refused(E_RANGE, dict(A, **{name: (A[name][0], stride)}))
    for batch in (0, -1, (1 << 24) + 1):
        refused(E_RANGE, batch=batch)
    for bad in ((F[0], None, -1, 1), (F[0], None, 0, 0), (F[0], None, 2 ** 31 - 1, 1), (F[0], None, 0, 2 ** 31)):
        refused(E_RANGE, F_=bad)
    if kernel == "handover":
        refused(E_ARG, F_=(None, None, 0, 1))                    # the flags are what the launch is for
        for hidden in (6, 9, 1028, 2048, 0, -4):
            refused(E_RANGE, hidden=hidden)
        for name in ("h_prev", "hp", "hprev_out", "cprev_out"):
            refused(E_ALIGN, dict(A, **{name: (A[name][0] + 4, A[name][1])}))
        refused(E_ALIGN, dict(A, hprev_out=(A["hprev_out"][0], 10)))
    else:
        for hidden in (0, -1, (1 << 20) + 1):
            refused(E_RANGE, hidden=hidden)
    torch.cuda.synchronize()
    for t in outs:
        assert bool(_nan_bits(t).all())
    assert _call_reset(L, kernel, A, 2, 8, F) == 0              # ... and the same small call inside the limits runs
    torch.cuda.synchronize()
    for t in outs:
        assert bool(torch.isfinite(t).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. BPTT against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------

def _masked_prob_value(kind, rp, spec, data, segs, t_len, resets):
    """prob, value (float64) of the rows of segments `segs` in time order: step 0 from the stored state, step t > 0 from
    state[t-1] (1 - resets[t-1]).  resets None: the recurrence that ignores the mask."""
    rows = (torch.as_tensor(np.asarray(segs), device=DEV).long()[:, None] * t_len + torch.arange(t_len, device=DEV)[None]).reshape(-1)
    xf, k = _ref_features(rp, spec, data["observations"][rows].double() * np.float64(np.float32(1. / 255)))
    nb = len(segs)
    xf = xf.view(nb, t_len, -1)
    state = [data[key][rows].double().view(nb, t_len, -1)[:, 0] for key in data["state_keys"]]
    keep = None if resets is None else (resets[rows] == 0).double().view(nb, t_len, 1)
    hs = []
    for t in range(t_len):
        if t > 0 and keep is not None:
            state = [s * keep[:, t - 1] for s in state]
        state, kp = _ref_step(kind, rp, k, xf[:, t], state)
        hs.append(state[0])
    h_all = torch.stack(hs, dim=1).reshape(nb * t_len, -1)
    prob = torch.softmax(h_all @ rp[kp] + rp[kp + 1], 1)
    value = (h_all @ rp[kp + 2] + rp[kp + 3]).reshape(-1)
    return prob, value, rows


def _masked_ppo_losses(kind, rp, spec, data, segs, t_len, resets, clip=CLIP):
    """The (pi, v, ent) formula of test_recurrent_ppo_gpu._ref_ppo_losses (no valids: every row counts) on the masked
    recurrence."""
    prob, value, rows = _masked_prob_value(kind, rp, spec, data, segs, t_len, resets)
    n = len(rows)
    act = data["actions"][rows].long()
    adv, ret = data["advantages"][rows].double(), data["returns"][rows].double()
    pa = prob[torch.arange(n), act]
    ratio = (pa + TINY) / (data["old_prob"][rows].double()[torch.arange(n), act] + TINY)
    surr = torch.minimum(ratio * adv, torch.clamp(ratio, 1. - clip, 1. + clip) * adv)
    pi = -torch.mean(surr)
    vl = V_COEFF * torch.mean((value - ret) ** 2)
    el = -ENT_COEFF * torch.mean(-torch.sum(prob * torch.log(prob + TINY), dim=1))
    return pi, vl, el


def _learner(policy, data, t_len, segs, resets):
    from accel_rl_amd import _lib
    policy.flat_grads.zero_()
    mb = _mb(data, t_len, None if segs is None else _dev(np.asarray(segs, np.int32)))
    if resets is not None:
        mb["resets"] = resets
    loss4 = policy.loss_and_grads(mb, 1, CLIP, V_COEFF, ENT_COEFF, torch.ones(1, device=DEV), None,
                                  tie_rule=_lib.PPO_TIE_MATH).clone()
    return loss4, policy.flat_grads.clone()


def _check_learner(kind, policy, spec, data, nb, t_len, segs, resets, what, want=None):
    """loss_and_grads with `resets` against float64 autograd through the masked recurrence (or `want`, a (losses,
    gradient) pair made otherwise), at the bars of test_recurrent_ppo_gpu; returns the float64 gradient."""
    loss4, grads = _learner(policy, data, t_len, segs, resets)
    got = policy.bucket_to_reference(grads)
    if want is None:
        rp = _ref_params(policy)
        pi, vl, el = _masked_ppo_losses(kind, rp, spec, data, np.arange(nb) if segs is None else segs, t_len, resets)
        want = (torch.stack([pi, vl, el]).detach().float(), _flat_grads(pi + vl + el, rp))
    want_l, want_g = want
    scale = np.abs(want_g).max()
    assert np.isfinite(got).all() and np.isfinite(want_g).all() and scale > 0
    print("%s %s: loss4 %s want %s; max |d grad| %.3g of %.3g" % (kind, what, loss4[:3].tolist(), want_l.tolist(),
                                                                   np.abs(got - want_g).max(), scale))
    assert torch.allclose(loss4[:3], want_l, rtol=1e-4, atol=1e-6), (what, loss4.tolist(), want_l.tolist())
    assert np.allclose(got, want_g, rtol=GRAD_RTOL, atol=GRAD_ATOL * max(scale, 1e-3)), (what, np.abs(got - want_g).max(), scale)
    return want_g


def _item3_mask(nb=3, t_len=5):
    m = np.zeros((nb, t_len), np.uint8)
    m[0, 1] = 1                                                 # trajectory 0: after step 1
    m[1, 0] = m[1, 3] = 1                                       # trajectory 1: after steps 0 and 3
    m[2, 4] = 1                                                 # trajectory 2: after the last step only (changes nothing)
    return _dev(m.reshape(-1))


@pytest.mark.parametrize("hidden", [4, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_bptt_with_resets_matches_float64_autograd(kind, hidden):
    nb, t_len = 3, 5
    policy, spec = _make(kind, hidden)
    rs = np.random.RandomState(20 + hidden)
    data = _data(kind, policy, spec, rs, nb, t_len, False, hh=hidden)
    resets = _item3_mask()
    for segs in (None, [2, 0]):
        what = "H%d %s" % (hidden, "whole batch" if segs is None else "trajectories [2, 0]")
        want = _check_learner(kind, policy, spec, data, nb, t_len, segs, resets, what)
        # discrimination: the float64 gradient of the recurrence that ignores the mask misses the bar by > 10 x
        rp = _ref_params(policy)
        pi, vl, el = _masked_ppo_losses(kind, rp, spec, data, np.arange(nb) if segs is None else segs, t_len, None)
        ignoring = _flat_grads(pi + vl + el, rp)
        tol = GRAD_RTOL * np.abs(want) + GRAD_ATOL * max(np.abs(want).max(), 1e-3)
        margin = float((np.abs(ignoring - want) / tol).max())
        print("%s %s: the mask-ignoring gradient misses the bar by a factor %.3g" % (kind, what, margin))
        assert margin > 10., (kind, what, margin)
    # trajectory 2 alone: its only reset follows the last step -> the bits of the path without `resets`
    with_mask = _learner(policy, data, t_len, [2], resets)
    without = _learner(policy, data, t_len, [2], None)
    assert torch.equal(with_mask[0], without[0]) and torch.equal(with_mask[1], without[1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. bits
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_an_all_zero_mask_gives_the_bits_of_the_path_without_resets(kind, monkeypatch):
    """... and takes the reset path to get there: per pass one hand-over launch for every forward step after the first
    (in place of that step's two copies) and the reset-aware cell for every backward step; without `resets` neither."""
    from accel_rl_amd import _lib
    nb, t_len = 4, 5
    policy, spec = _make(kind)
    data = _data(kind, policy, spec, np.random.RandomState(7), nb, t_len, False)
    zeros = torch.zeros(nb * t_len, dtype=torch.uint8, device=DEV)
    calls = dict(handover=0, cell=0, plain=0)

    def counted(name, key):
        fn = getattr(_lib, name)

        def wrapper(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        monkeypatch.setattr(_lib, name, wrapper)
    counted("seq_handover", "handover")
    counted("%s_cell_bwd_reset" % kind, "cell")
    counted("%s_cell_bwd" % kind, "plain")
    for segs in (None, [3, 1]):
        calls.update(handover=0, cell=0, plain=0)
        without = _learner(policy, data, t_len, segs, None)
        assert calls == dict(handover=0, cell=0, plain=t_len), calls
        for resets in (zeros, zeros.bool()):                    # (the sampler's `dones` is a bool tensor)
            calls.update(handover=0, cell=0, plain=0)
            with_mask = _learner(policy, data, t_len, segs, resets)
            assert calls == dict(handover=t_len - 1, cell=t_len, plain=0), calls
            assert torch.equal(with_mask[0], without[0]), (kind, segs)
            assert torch.equal(with_mask[1], without[1]), (kind, segs)
        assert without[1].abs().sum() > 0


@pytest.mark.parametrize("kind", KINDS)
def test_a_reset_after_every_step_is_a_batch_of_one_step_segments(kind):
    nb, t_len = 4, 5
    policy, spec = _make(kind)
    data = _data(kind, policy, spec, np.random.RandomState(9), nb, t_len, False)
    # float64: 20 segments of one step; step 0 of each real segment keeps its stored state, every other row starts at 0
    single = dict(data)
    first = (torch.arange(nb * t_len, device=DEV) % t_len == 0).float()[:, None]
    for key in data["state_keys"]:
        single[key] = data[key] * first
    rp = _ref_params(policy)
    (pi, vl, el), _ = _ref_ppo_losses(kind, rp, spec, single, np.arange(nb * t_len), 1)
    want = (torch.stack([pi, vl, el]).detach().float(), _flat_grads(pi + vl + el, rp))
    ones = torch.ones(nb * t_len, dtype=torch.uint8, device=DEV)
    _check_learner(kind, policy, spec, data, nb, t_len, None, ones, "reset after every step", want=want)


# ---------------------------------------------------------------------------------------------------------------------
# 5. sampler and learner agree on the mask
# ---------------------------------------------------------------------------------------------------------------------

def _collect(mid_batch_reset, n_batches):
    """Batches of a game with episodic lives (breakout; frame_skip 12 so that a life is lost inside 23 steps), LSTM 256,
    horizon 5, max_path_length 23, no decorrelation, seed 3: a list of host / device copies of every batch."""
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    from accel_rl_amd.util.seed import set_seed
    logger.set_quiet(True)
    set_seed(3)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="breakout", frame_skip=12), horizon=5, n_parallel=2,
                            envs_per=4, max_path_length=23, mid_batch_reset=mid_batch_reset, max_decorrelation_steps=0,
                            device=DEV)
    env_spec, sample_size, horizon, _ = sampler.initialize(seed=4, discount=0.99, need_extra_obs=True)
    spec = dict(cnn_specs[0], hidden_sizes=[256])
    policy = _policy_cls("lstm")(**spec)
    policy.initialize(env_spec, device=DEV)
    sampler.policy_init(policy)
    out = []
    for itr in range(n_batches):
        buf, _ = sampler.obtain_samples(itr)
        torch.cuda.synchronize()
        out.append(dict(observations=buf.observations.clone(), actions=buf.actions.clone(), dones=buf.dones.clone(),
                        need_reset=buf.env_infos["need_reset"].clone(),
                        agent_infos={k: v.clone() for k, v in buf.agent_infos.items()}))
    sampler.shutdown()
    return policy, spec, out, sample_size // horizon, horizon


def test_sampler_and_learner_agree_on_the_mask():
    policy, spec, batches, nb, t_len = _collect(True, 6)
    pick = None
    for b in batches:
        dones, need = b["dones"].view(nb, t_len).cpu().numpy() != 0, b["need_reset"].view(nb, t_len).cpu().numpy() != 0
        if (dones & ~need)[:, :t_len - 1].any() and need[:, :t_len - 1].any():
            pick = b
            break
    assert pick is not None, "no batch with a lost life (done, no reset) and a reset before the last step"
    dones, need = pick["dones"].view(torch.uint8), pick["need_reset"].view(torch.uint8)
    assert bool(((dones != 0) & (need == 0)).any())             # a lost life: done = 1 without a reset
    assert bool((need.view(nb, t_len)[:, :t_len - 1] != 0).any())   # a reset at a step t < 4
    infos = pick["agent_infos"]
    data = dict(observations=pick["observations"], actions=pick["actions"], state_keys=list(policy.state_info_keys),
                hprev_0=infos["hprev_0"], cprev_0=infos["cprev_0"], old_prob=infos["prob"], old_value=infos["value"],
                valids=None)
    rp = _ref_params(policy)

    def misses(mask):
        with torch.no_grad():
            prob, value, _ = _masked_prob_value("lstm", rp, spec, data, np.arange(nb), t_len, mask)
        # the forward tests' bars (test_lstm_gpu.py: prob rtol 1e-4 atol 1e-6, value rtol 1e-4 atol 1e-5), the value's
        # atol scaled by the largest value where that is tighter
        sp, sv = infos["prob"].double(), infos["value"].double()
        atol_v = 1e-5 * min(1., float(sv.abs().max()))
        bad_p = ((prob - sp).abs() > 1e-6 + 1e-4 * prob.abs()).any(dim=1)
        bad_v = (value - sv).abs() > atol_v + 1e-4 * value.abs()
        print("max |d prob| %.3g, max |d value| %.3g (largest value %.3g)" % ((prob - sp).abs().max().item(),
                                                                              (value - sv).abs().max().item(), sv.abs().max().item()))
        return int((bad_p | bad_v).sum())
    assert misses(need) == 0                                    # env_infos.get("need_reset", dones): the sampler's resets
    assert misses(dones) > 0                                    # `dones` alone: a lost life is no reset
    # the learner on the same batch
    rs = np.random.RandomState(12)
    data["advantages"], data["returns"] = _dev(rs.randn(nb * t_len).astype(np.float32)), _dev(rs.randn(nb * t_len).astype(np.float32))
    noise = _dev(rs.randn(nb * t_len, infos["prob"].shape[1]) * 0.15)
    data["old_prob"] = torch.softmax(torch.log(infos["prob"].double()) + noise, 1).float()
    _check_learner("lstm", policy, spec, data, nb, t_len, None, pick["need_reset"], "sampled batch, whole")
    _check_learner("lstm", policy, spec, data, nb, t_len, [5, 0, 2, 7], pick["need_reset"], "sampled batch, trajectories")


# ---------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------------------------

def _algo(name, **kw):
    from accel_rl_amd.algos.pg.a2c import A2C
    from accel_rl_amd.algos.pg.ppo import RecurrentPPO
    if name == "a2c":
        return A2C(**kw)
    return RecurrentPPO(optimizer_args=dict(minibatch_size=40), **kw)


def _train(kind, algo):
    """test_recurrent_ppo_gpu._train's sizes with mid_batch_reset=True."""
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.runners.accel_rl import AccelRL
    from accel_rl_amd.sampler.gpu_sampler import GpuVecSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecSampler(EnvCls=SynthAtariEnv, env_args=dict(game="pong"), horizon=5, n_parallel=4, envs_per=4,
                            max_path_length=23, mid_batch_reset=True, max_decorrelation_steps=0, device=DEV)
    policy = _policy_cls(kind)(**dict(cnn_specs[0], hidden_sizes=[256]))
    runner = AccelRL(algo=algo, policy=policy, sampler=sampler, n_steps=160 * 8, seed=2, log_interval_steps=640)
    runner.train()
    return runner, policy, sampler


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["a2c", "ppo"])
def test_training_with_mid_batch_resets_end_to_end(name, kind):
    finals = []
    for use_graph in (True, True, False):
        algo = _algo(name, bptt_resets=True, use_graph=use_graph)
        runner, policy, sampler = _train(kind, algo)
        tab = runner.last_tabular
        assert np.isfinite(tab["GradNormAverage"]) and tab["CumCompletedTrajs"] > 0
        assert (algo._graph is not None) == use_graph           # past the two warm-up calls: replayed from one hipGraph
        names = algo.optimizer._input_names
        assert "valids" not in names and names[-1] == "resets" and not algo._use_valids
        flat = policy.get_param_values()
        assert np.isfinite(flat).all()
        finals.append(flat)
    np.testing.assert_array_equal(finals[0], finals[1])        # seeded runs agree bit for bit
    np.testing.assert_array_equal(finals[0], finals[2])        # eager = captured
    with pytest.raises(NotImplementedError, match="bptt_resets"):
        _train(kind, _algo(name))
