"""The recurrent cells (csrc/lstm.hip, csrc/gru.hip: arl_{lstm,gru,rnn}_cell_{fwd,bwd}) and BPTT through the recurrent
policies at the edges of what they accept, against float64.

1. Cell kernels.  The six formulas are written once below in numpy (`_ref`), from the comments at the head of
   lstm.hip / gru.hip and FastLstmLayer.step / GruLayer.step / RecurrentLayer.step (policies/layers.py:331-346,
   163-168, 80-82), and evaluated twice: in float64 (the reference) and in float32 in the kernel's operation order
   (the yardstick for the tolerance).  Inputs are made on the host with a seeded RandomState; float64 sees exactly the
   fp32 values the kernel saw (the backward kernels read gates / cell states made by the fp32 restatement on the
   host, not by the forward kernels).  Every call goes through the C ABI.  Every array lives inside a NaN-filled
   buffer and everything outside the addressed rows is checked bit for bit afterwards, inputs included.

   Error measure of an output array x against float64 x64:  E(x) = max |x - x64| / max(|x64|, s), s elementwise:
     1 for the activated gates and the GRU / RNN h;  max(1, |c_prev|) for the LSTM's c and h;
     backward, with D = |dh| + |dh_rec| (+ |dh_dir|) and Dc = D + |dc_next|:  LSTM dgates f: Dc max(1, |c_prev|),
     i, c~: Dc, o: D, dc_prev: Dc;  GRU dgx / dgh r: D max(1, |gh_c|), u: D (1 + |h_prev|), c: D, dh_prev: D;
     RNN dpre: D.  Where s == 0 (every gradient input absent or zero) the output must be exactly 0.
   The kernel is allowed  max(4 E(fp32 numpy), 4 * 2^-23): the factor covers the device expf / tanhf (a couple of
   ulp against the host's sub-ulp) and nothing else, -ffp-contract=off keeps the arithmetic unfused and in the
   written order.  The fp32 restatement itself must stay below 1e-5 on every non-saturated case.

   Worst figures over all non-saturated cases of this module (E(fp32 numpy) measured on the CPU; bound = 4 x that,
   not less than 4.8e-7; kernel = worst E observed on an MI355X, see LABNOTES.md):

     kernel    output    E(fp32 numpy)   bound      kernel on gfx950
     lstm_fwd  h         1.97e-07        7.88e-07   1.83e-07
     lstm_fwd  c         2.33e-07        9.32e-07   2.1e-07
     lstm_fwd  gates     1.03e-07        4.77e-07   1e-07
     lstm_bwd  dgates    2.09e-07        8.38e-07   2.09e-07
     lstm_bwd  dc_prev   1.7e-07         6.8e-07    1.7e-07
     gru_fwd   h         2.84e-07        1.13e-06   2.68e-07
     gru_fwd   saved     3.23e-07        1.29e-06   3.25e-07
     gru_bwd   dgx       1.9e-07         7.6e-07    1.9e-07
     gru_bwd   dgh       1.69e-07        6.75e-07   1.69e-07
     gru_bwd   dh_prev   1.75e-07        6.99e-07   1.75e-07
     rnn_fwd   h         7.7e-08         4.77e-07   1.04e-07
     rnn_bwd   dpre      1.47e-07        5.89e-07   1.47e-07

   (the bound is computed per case from that case's own inputs; the table lists the largest.)  ARL_CELL_REPORT=path
   makes the module write every figure it measured to that file.

   Saturation: pre-activations from {0, +-1e-8, +-1, +-8, +-17, +-20, +-50, +-88, +-89, +-104, +-1e4, +-3e38} crossed
   over the gates, c_prev up to +-1e4, gradients up to +-1e3; the whole pre-activation sits in gx (a pre-activation
   split over gx + gh would only measure the cancellation of the fp32 sum).  The GRU's gh_c, a factor and not a
   pre-activation, takes {0, +-1, +-8} against every candidate input and +-3e38 against small ones (and an r that is exactly
   0 or at least 3e-4: see _sat_inputs): with r saturated
   to exactly 0 the old order dpc * gh_c * r * (1 - r) gave inf * 0 = NaN where float64 gives 0 (fixed in gru.hip:
   gh_c (r (1 - r)) first; this case is its regression test).

2. Limits of the six entry points (include/accel_rl_hip.h): the last accepted and the first refused value of batch,
   hidden and every stride, null pointers, and that a refusal leaves NaN-filled outputs untouched.

3. BPTT: RecurrentCnnPolicy.loss_and_grads (PPO loss: the float64 restatement of test_recurrent_ppo_gpu.py, which has
   no A2C form) at hidden 4 and 1024, horizons 1 and 32, one segment, a segment invalid after step 0, and stored
   states of magnitude 10, over the whole batch and over a trajectory minibatch.  Bars: those of the hidden-256 tests
   (loss terms rtol 1e-4 atol 1e-6; gradients rtol 2e-3, atol 2e-5 of the largest entry).
"""
import itertools
import os

import numpy as np
import pytest
import torch

from test_recurrent_ppo_gpu import (CLIP, ENT_COEFF, GRAD_ATOL, GRAD_RTOL, KINDS, V_COEFF, _data, _flat_grads, _make, _mb,
                                    _policy_cls, _ref_params, _ref_ppo_losses, _ref_prob_value)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
EPS = 2. ** -23
FLT_MAX = float(np.finfo(np.float32).max)
E_ARG, E_RANGE = -1, -2
MAX_BATCH, MAX_HIDDEN, MAX_STRIDE = 1 << 24, 1 << 20, 1 << 28          # ARL_CELL_MAX_* of accel_rl_hip.h
GRID_ELEMS = 2048 * 256                                                   # arl::stream_grid's cap x 256 threads


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


# ---------------------------------------------------------------------------------------------------------------------
# the six kernels: arguments (name, width in units of hidden, strided?, optional?) and the formulas
# ---------------------------------------------------------------------------------------------------------------------

KERNELS = {
    "lstm_fwd": dict(ins=[("gx", 4, True, False), ("gh", 4, False, True), ("c_prev", 1, True, False)],
                     outs=[("h", 1, True, False), ("c", 1, True, False), ("gates", 4, True, True)]),
    "lstm_bwd": dict(ins=[("dh", 1, True, True), ("dh_rec", 1, False, True), ("dc_next", 1, False, True),
                          ("gates", 4, True, False), ("c_prev", 1, True, False), ("c", 1, True, False)],
                     outs=[("dgates", 4, True, False), ("dc_prev", 1, False, False)]),
    "gru_fwd": dict(ins=[("gx", 3, True, False), ("gh", 3, False, False), ("h_prev", 1, True, False)],
                    outs=[("h", 1, True, False), ("saved", 4, True, True)]),
    "gru_bwd": dict(ins=[("dh", 1, True, True), ("dh_rec", 1, False, True), ("dh_dir", 1, False, True),
                         ("saved", 4, True, False), ("h_prev", 1, True, False)],
                    outs=[("dgx", 3, True, False), ("dgh", 3, True, False), ("dh_prev", 1, False, False)]),
    "rnn_fwd": dict(ins=[("gx", 1, True, False), ("gh", 1, False, False)], outs=[("h", 1, True, False)]),
    "rnn_bwd": dict(ins=[("dh", 1, True, True), ("dh_rec", 1, False, True), ("h", 1, True, False)],
                    outs=[("dpre", 1, True, False)]),
}
NAMES = list(KERNELS)


def _args(kernel):
    return KERNELS[kernel]["ins"] + KERNELS[kernel]["outs"]


def _call(L, kernel, A, batch, hidden):
    """The C entry point; A: name -> (pointer or None, row stride)."""
    lib, st = L.load(), L.stream_ptr()
    p, s = (lambda n: A[n][0]), (lambda n: A[n][1])
    if kernel == "lstm_fwd":
        return lib.arl_lstm_cell_fwd(p("gx"), s("gx"), p("gh"), p("c_prev"), s("c_prev"), batch, hidden, p("h"), s("h"),
                                     p("c"), s("c"), p("gates"), s("gates"), st)
    if kernel == "lstm_bwd":
        return lib.arl_lstm_cell_bwd(p("dh"), s("dh"), p("dh_rec"), p("dc_next"), p("gates"), s("gates"), p("c_prev"),
                                     s("c_prev"), p("c"), s("c"), batch, hidden, p("dgates"), s("dgates"), p("dc_prev"),
                                     st)
    if kernel == "gru_fwd":
        return lib.arl_gru_cell_fwd(p("gx"), s("gx"), p("gh"), p("h_prev"), s("h_prev"), batch, hidden, p("h"), s("h"),
                                    p("saved"), s("saved"), st)
    if kernel == "gru_bwd":
        return lib.arl_gru_cell_bwd(p("dh"), s("dh"), p("dh_rec"), p("dh_dir"), p("saved"), s("saved"), p("h_prev"),
                                    s("h_prev"), batch, hidden, p("dgx"), s("dgx"), p("dgh"), s("dgh"), p("dh_prev"), st)
    if kernel == "rnn_fwd":
        return lib.arl_rnn_cell_fwd(p("gx"), s("gx"), p("gh"), batch, hidden, p("h"), s("h"), st)
    return lib.arl_rnn_cell_bwd(p("dh"), s("dh"), p("dh_rec"), p("h"), s("h"), batch, hidden, p("dpre"), s("dpre"), st)


def _sig(x):
    return 1. / (1. + np.exp(-x))


def _cols(a, n):
    h = a.shape[1] // n
    return [a[:, k * h:(k + 1) * h] for k in range(n)]


def _ref(kernel, x, dt):
    """The kernel's formula on the arrays x (name -> [batch][width] or None) in dtype dt, in the kernel's operation
    order (which only matters for dt = float32)."""
    x = {k: (None if v is None else v.astype(dt)) for k, v in x.items()}
    with np.errstate(over="ignore", under="ignore"):
        if kernel == "lstm_fwd":
            pre = x["gx"] if x["gh"] is None else x["gx"] + x["gh"]
            pf, pi, pg, po = _cols(pre, 4)
            f, i, g, o = _sig(pf), _sig(pi), np.tanh(pg), _sig(po)
            c = f * x["c_prev"] + i * g
            return dict(h=o * np.tanh(c), c=c, gates=np.concatenate([f, i, g, o], 1))
        if kernel == "lstm_bwd":
            f, i, g, o = _cols(x["gates"], 4)
            dh = np.zeros_like(x["c"])
            for k in ("dh", "dh_rec"):
                if x[k] is not None:
                    dh = dh + x[k]
            tc = np.tanh(x["c"])
            dc = dh * o * (1. - tc * tc)
            if x["dc_next"] is not None:
                dc = dc + x["dc_next"]
            dg = [dc * x["c_prev"] * f * (1. - f), dc * g * i * (1. - i), dc * i * (1. - g * g), dh * tc * o * (1. - o)]
            return dict(dgates=np.concatenate(dg, 1), dc_prev=dc * f)
        if kernel == "gru_fwd":
            xr, xu, xc = _cols(x["gx"], 3)
            hr, hu, hc = _cols(x["gh"], 3)
            r, u = _sig(xr + hr), _sig(xu + hu)
            c = np.tanh(xc + r * hc)
            return dict(h=(1. - u) * x["h_prev"] + u * c, saved=np.concatenate([r, u, c, hc], 1))
        if kernel == "gru_bwd":
            r, u, c, hc = _cols(x["saved"], 4)
            dh = np.zeros_like(x["h_prev"])
            for k in ("dh", "dh_rec", "dh_dir"):
                if x[k] is not None:
                    dh = dh + x[k]
            dpc = dh * u * (1. - c * c)
            dpu = dh * (c - x["h_prev"]) * u * (1. - u)
            dpr = dpc * (hc * (r * (1. - r)))
            return dict(dgx=np.concatenate([dpr, dpu, dpc], 1), dgh=np.concatenate([dpr, dpu, dpc * r], 1),
                        dh_prev=dh * (1. - u))
        if kernel == "rnn_fwd":
            return dict(h=np.tanh(x["gx"] + x["gh"]))
        dh = np.zeros_like(x["h"])
        for k in ("dh", "dh_rec"):
            if x[k] is not None:
                dh = dh + x[k]
        return dict(dpre=dh * (1. - x["h"] * x["h"]))


def _scales(kernel, x):
    """The elementwise scale s of every output (module docstring), float64."""
    a = lambda k: 0. if x.get(k) is None else np.abs(x[k].astype(np.float64))          # noqa: E731
    one = lambda k: np.maximum(1., a(k))                                                # noqa: E731
    if kernel == "lstm_fwd":
        return dict(h=one("c_prev"), c=one("c_prev"), gates=1.)
    if kernel == "lstm_bwd":
        d = a("dh") + a("dh_rec") + np.zeros(x["c"].shape)
        dc = d + a("dc_next")
        return dict(dgates=np.concatenate([dc * one("c_prev"), dc, dc, d], 1), dc_prev=dc)
    if kernel == "gru_fwd":
        return dict(h=1., saved=np.concatenate([np.ones(x["h_prev"].shape)] * 3 + [one("gh")[:, -x["h_prev"].shape[1]:]], 1))
    if kernel == "gru_bwd":
        d = a("dh") + a("dh_rec") + a("dh_dir") + np.zeros(x["h_prev"].shape)
        hc = np.maximum(1., np.abs(_cols(x["saved"], 4)[3].astype(np.float64)))
        cols = [d * hc, d * (1. + a("h_prev")), d]
        return dict(dgx=np.concatenate(cols, 1), dgh=np.concatenate(cols, 1), dh_prev=d)
    if kernel == "rnn_fwd":
        return dict(h=1.)
    return dict(dpre=a("dh") + a("dh_rec") + np.zeros(x["h"].shape))


def _err(got, want, s):
    """E = max |got - want| / max(|want|, s) over the elements where float64 has a finite value an fp32 can hold (all of
    them outside the saturation test); inf for a NaN / inf there, and for a non-zero where want == s == 0."""
    want = np.asarray(want, np.float64)
    valid = np.isfinite(want) & (np.abs(want) <= FLT_MAX)
    g = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.abs(g - want)
        den = np.maximum(np.abs(want), s) + np.zeros(want.shape)
        e = np.where(d == 0, 0., d / den)
        e = np.where(np.isfinite(g), e, np.inf)
    return (float(e[valid].max()) if valid.any() else 0.), valid


# ---- host inputs ----------------------------------------------------------------------------------------------------

def _inputs(kernel, rs, batch, hidden):
    """Standard-normal pre-activations and gradients, states of size ~1: the non-saturated regime."""
    f32 = lambda *shape: rs.randn(*shape).astype(np.float32)                             # noqa: E731
    if kernel == "lstm_fwd":
        return dict(gx=f32(batch, 4 * hidden), gh=f32(batch, 4 * hidden), c_prev=f32(batch, hidden))
    if kernel == "lstm_bwd":
        fwd = _inputs("lstm_fwd", rs, batch, hidden)
        out = _ref("lstm_fwd", fwd, np.float32)
        return dict(dh=f32(batch, hidden), dh_rec=f32(batch, hidden), dc_next=f32(batch, hidden), gates=out["gates"],
                    c_prev=fwd["c_prev"], c=out["c"])
    if kernel == "gru_fwd":
        return dict(gx=f32(batch, 3 * hidden), gh=f32(batch, 3 * hidden), h_prev=np.tanh(f32(batch, hidden)))
    if kernel == "gru_bwd":
        fwd = _inputs("gru_fwd", rs, batch, hidden)
        return dict(dh=f32(batch, hidden), dh_rec=f32(batch, hidden), dh_dir=f32(batch, hidden),
                    saved=_ref("gru_fwd", fwd, np.float32)["saved"], h_prev=fwd["h_prev"])
    if kernel == "rnn_fwd":
        return dict(gx=f32(batch, hidden), gh=f32(batch, hidden))
    fwd = _inputs("rnn_fwd", rs, batch, hidden)
    return dict(dh=f32(batch, hidden), dh_rec=f32(batch, hidden), h=_ref("rnn_fwd", fwd, np.float32)["h"])


# ---- device side ----------------------------------------------------------------------------------------------------

def _nan_bits(t):
    return t.view(torch.int32) == torch.full((1,), NAN).view(torch.int32).item()


class _Slot(object):
    """[batch][width] rows with a row stride, `off` elements into a NaN-filled buffer with 8 spare elements behind."""

    def __init__(self, batch, width, stride, off, data=None, buf=None):
        self.shape, self.strides, self.off = (batch, width), (stride if batch > 1 else width, 1), off   # one row: no stride
        need = off + (batch - 1) * stride + width + 8
        self.buf = torch.full((need,), NAN, device=DEV) if buf is None else buf
        assert self.buf.numel() >= need                                  # the kernel's rows lie inside the buffer
        if data is not None:
            self.view().copy_(torch.from_numpy(np.ascontiguousarray(data)))
        self.ptr = self.buf.data_ptr() + 4 * off
        self.before = self.buf.clone() if data is not None else None

    def view(self, buf=None):
        return (self.buf if buf is None else buf).as_strided(self.shape, self.strides, self.off)

    def rows(self):
        return self.view().cpu().numpy()

    def outside_untouched(self):
        a = self.buf.clone()
        self.view(a).fill_(NAN)
        return bool(_nan_bits(a).all())

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))


def _contiguous(name, width, batch):
    return width, 0


def _run(L, kernel, x, batch, hidden, layout=_contiguous, absent=(), alias=None, twice=True):
    """Run one kernel on host arrays x; layout(name, width, batch) -> (row stride, offset) for the strided arguments.
    absent: optional arguments passed as NULL.  alias: {output: input} sharing one buffer.  Returns the outputs as
    numpy arrays after checking that nothing outside the addressed rows changed, inputs included."""
    alias = alias or {}
    slots, A = {}, {}
    for name, mult, strided, optional in KERNELS[kernel]["ins"]:
        if name in absent:
            assert optional and x.get(name) is None
            A[name] = (None, 0)
            continue
        w = mult * hidden
        stride, off = layout(name, w, batch) if strided else (w, 0)
        slots[name] = _Slot(batch, w, stride, off, data=x[name])
        A[name] = (slots[name].ptr, stride)
    outs = []
    for name, mult, strided, optional in KERNELS[kernel]["outs"]:
        if name in absent:
            assert optional
            A[name] = (None, 0)
            continue
        w = mult * hidden
        if name in alias:
            src = slots[alias[name]]
            slots[name] = _Slot(batch, w, A[alias[name]][1], src.off, buf=src.buf)
            stride = A[alias[name]][1]
        else:
            stride, off = layout(name, w, batch) if strided else (w, 0)
            slots[name] = _Slot(batch, w, stride, off)
        A[name] = (slots[name].ptr, stride)
        outs.append(name)
    L._check(_call(L, kernel, A, batch, hidden), kernel)
    torch.cuda.synchronize()
    got = {name: slots[name].rows() for name in outs}
    for name in outs:
        assert slots[name].outside_untouched(), (kernel, name, "wrote outside its rows")
    for name, *_ in KERNELS[kernel]["ins"]:
        if name in slots and name not in alias.values():
            assert slots[name].unchanged(), (kernel, name, "input modified")
    if twice and not alias:                                      # the same call again: the same bits
        for name in outs:
            slots[name].view().fill_(NAN)
        L._check(_call(L, kernel, A, batch, hidden), kernel)
        torch.cuda.synchronize()
        for name in outs:
            assert np.array_equal(slots[name].rows().view(np.uint32), got[name].view(np.uint32)), (kernel, name, "run 2")
    return got


REPORT = {}          # (kernel, output) -> [worst E(fp32 numpy), worst bound, worst E(kernel)] over the non-saturated cases


def _write_report():
    path = os.environ.get("ARL_CELL_REPORT")
    if path:
        with open(path, "w") as f:
            for (k, o), (e32, b, ek) in sorted(REPORT.items()):
                f.write("%-9s %-8s fp32-numpy %.3g  bound %.3g  kernel %.3g\n" % (k, o, e32, b, ek))


def _compare(kernel, x, got, saturated=False, what=""):
    """Every element of every output against float64, within 4 x the fp32 restatement's own error (>= 4 ulp of s)."""
    want64, want32, s = _ref(kernel, x, np.float64), _ref(kernel, x, np.float32), _scales(kernel, x)
    for name, g in got.items():
        assert g.dtype == np.float32 and g.shape == want64[name].shape
        e32, valid = _err(want32[name], want64[name], s[name])
        ek, _ = _err(g, want64[name], s[name])
        bound = max(4. * e32, 4. * EPS)
        print("%s %s.%s: E(fp32 numpy) %.3g  bound %.3g  E(kernel) %.3g" % (what, kernel, name, e32, bound, ek))
        if not saturated:
            assert valid.all() and e32 < 1e-5, (kernel, name, e32)
            r = REPORT.setdefault((kernel, name), [0., 0., 0.])
            r[:] = [max(r[0], e32), max(r[1], bound), max(r[2], ek)]
            _write_report()
        assert ek <= bound, (what, kernel, name, ek, bound)
    return want64, s


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels against float64
# ---------------------------------------------------------------------------------------------------------------------

HIDDENS = [1, 2, 3, 4, 5, 63, 64, 65, 256, 1023, 1024]
BATCHES = [1, 2, 33, 257]


@pytest.mark.parametrize("hidden", HIDDENS)
@pytest.mark.parametrize("kernel", NAMES)
def test_cell_widths_and_odd_batches_vs_float64(L, kernel, hidden):
    for batch in BATCHES:
        rs = np.random.RandomState(1000 * NAMES.index(kernel) + 7 * hidden + batch)
        x = _inputs(kernel, rs, batch, hidden)
        _compare(kernel, x, _run(L, kernel, x, batch, hidden), what="B%d H%d" % (batch, hidden))


@pytest.mark.parametrize("shape", [(2049, 512), (4099, 260)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kernel", NAMES)
def test_cell_grid_stride_second_and_third_pass(L, kernel, shape):
    """batch * hidden > 2 x (2048 workgroups x 256 threads): every thread loops twice, some a third time."""
    batch, hidden = shape
    assert batch * hidden > 2 * GRID_ELEMS and batch * hidden % GRID_ELEMS != 0
    rs = np.random.RandomState(batch + NAMES.index(kernel))
    x = _inputs(kernel, rs, batch, hidden)
    _compare(kernel, x, _run(L, kernel, x, batch, hidden), what="B%d H%d" % shape)


def _slice_layout(t_len, t, pads=None):
    """Time slice t of a [batch][t_len][width (+ pad)] array; pads: name -> extra elements per step (a row stride wider
    than t_len x width and different for every argument)."""
    def layout(name, width, batch):
        w = width + (pads or {}).get(name, 0)
        return t_len * w, t * w
    return layout


@pytest.mark.parametrize("t_len", [1, 2, 32])
@pytest.mark.parametrize("kernel", NAMES)
def test_cell_time_slices_in_place(L, kernel, t_len):
    """Rows as the learner makes them, first, middle and last slice, every other slice NaN and untouched; then every
    strided argument with a padding (so a stride) of its own: a kernel using another array's stride reads NaN or
    writes where the check sees it."""
    batch, hidden = 33, 20
    strided = [a[0] for a in _args(kernel) if a[2]]
    for t in sorted({0, t_len // 2, t_len - 1}):
        for pads in (None, {n: p for n, p in zip(strided, (1, 2, 3, 5, 7))}):
            rs = np.random.RandomState(97 * t_len + t + NAMES.index(kernel))
            x = _inputs(kernel, rs, batch, hidden)
            got = _run(L, kernel, x, batch, hidden, layout=_slice_layout(t_len, t, pads))
            _compare(kernel, x, got, what="T%d t%d %s" % (t_len, t, "padded" if pads else "dense"))


def _bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("kernel", NAMES)
def test_cell_optional_arguments_every_combination(L, kernel):
    """Every null / non-null combination of the optional arguments, on time slices.  With every gradient input absent
    the outputs are exactly zero (s = 0); an output that an absent argument cannot influence has the same bits as in
    the call with everything present."""
    batch, hidden, t_len, t = 33, 20, 3, 1
    rs = np.random.RandomState(5 + NAMES.index(kernel))
    full = _inputs(kernel, rs, batch, hidden)
    optional = [a[0] for a in _args(kernel) if a[3]]
    optional_out = [a[0] for a in KERNELS[kernel]["outs"] if a[3]]
    base = _run(L, kernel, full, batch, hidden, layout=_slice_layout(t_len, t))
    for n_absent in range(1, len(optional) + 1):
        for absent in itertools.combinations(optional, n_absent):
            x = {k: (None if k in absent else v) for k, v in full.items()}
            got = _run(L, kernel, x, batch, hidden, layout=_slice_layout(t_len, t), absent=absent)
            assert set(got) == set(base) - set(absent)
            _compare(kernel, x, got, what="without " + "+".join(absent))
            if set(absent) <= set(optional_out):                 # only a saved-values output left out: same h, c
                for name in got:
                    assert _bits_equal(got[name], base[name]), (kernel, absent, name)
            grads_in = [n for n in optional if n not in optional_out]
            if kernel.endswith("bwd") and set(grads_in) <= set(absent):
                for name in got:
                    assert not got[name].any(), (kernel, name, "must be all zero")
    if kernel == "lstm_fwd":                                     # gh = NULL is gh = 0
        zero = _run(L, kernel, dict(full, gh=np.zeros_like(full["gh"])), batch, hidden, layout=_slice_layout(t_len, t))
        null = _run(L, kernel, dict(full, gh=None), batch, hidden, layout=_slice_layout(t_len, t), absent=("gh",))
        for name in null:
            assert _bits_equal(null[name], zero[name]), name
    if kernel == "lstm_bwd":                                     # dgates' o column does not see dc_next
        no_dc = _run(L, kernel, dict(full, dc_next=None), batch, hidden, layout=_slice_layout(t_len, t),
                     absent=("dc_next",))
        assert _bits_equal(no_dc["dgates"][:, 3 * hidden:], base["dgates"][:, 3 * hidden:])


@pytest.mark.parametrize("kernel,out,inp", [("lstm_bwd", "dc_prev", "dc_next"), ("gru_bwd", "dh_prev", "dh_dir")])
def test_cell_backward_in_place_as_the_policies_call_it(L, kernel, out, inp):
    """atari_lstm_policy.py passes `carry` as dc_next and dc_prev, atari_gru_policy.py as dh_dir and dh_prev: the same
    bits as with two buffers, also past the first grid-stride pass."""
    for batch, hidden in ((33, 20), (8, 256), (2049, 512)):
        rs = np.random.RandomState(batch)
        x = _inputs(kernel, rs, batch, hidden)
        lay = _slice_layout(5, 3) if batch < 2049 else _contiguous
        apart = _run(L, kernel, x, batch, hidden, layout=lay)
        same = _run(L, kernel, x, batch, hidden, layout=lay, alias={out: inp})
        for name in apart:
            assert _bits_equal(apart[name], same[name]), (kernel, name, batch, hidden)
        _compare(kernel, x, same, what="in place B%d H%d" % (batch, hidden))


# ---- saturation -----------------------------------------------------------------------------------------------------

SAT = np.array([0.] + [sgn * v for v in (1e-8, 1., 8., 17., 20., 50., 88., 89., 104., 1e4, 3e38) for sgn in (1., -1.)],
               np.float32)
C_PREV = np.array([0., 1e-8, -1e-8, 1., -1., 50., -50., 1e4, -1e4, 0.3, -7.], np.float32)          # 11: coprime to 23
GRADS = np.array([0., 1., -1., 1e3, -1e3, 1e-3, -0.37], np.float32)                              # 7
GRADS2 = np.array([0., 1e3, -1., 0.5, -1e3], np.float32)                                         # 5
HID_SAT = 23


def _cycle(values, n, shift=0):
    return values[(np.arange(n) + shift) % len(values)]


def _sat_inputs(kernel):
    """[batch][23]-shaped inputs: every combination of SAT over the gates' pre-activations, states and gradients cycling
    through their own lists with coprime periods."""
    hh = HID_SAT
    if kernel.startswith("lstm"):
        g = np.array(np.meshgrid(SAT, SAT, SAT, SAT, indexing="ij")).reshape(4, -1)               # 23^4 elements
        n = g.shape[1]
        batch = n // hh
        gx = np.concatenate([g[k].reshape(batch, hh) for k in range(4)], 1)
        fwd = dict(gx=gx, gh=None, c_prev=_cycle(C_PREV, n).reshape(batch, hh))
        if kernel == "lstm_fwd":
            return fwd, batch
        out = _ref("lstm_fwd", fwd, np.float32)
        return dict(dh=_cycle(GRADS, n).reshape(batch, hh), dh_rec=_cycle(GRADS2, n, 1).reshape(batch, hh),
                    dc_next=_cycle(GRADS, n, 3).reshape(batch, hh), gates=out["gates"], c_prev=fwd["c_prev"],
                    c=out["c"]), batch
    if kernel.startswith("gru"):
        small = np.array([0., 1., -1., 8., -8.], np.float32)
        a = np.array(np.meshgrid(SAT, SAT, SAT, small, indexing="ij")).reshape(4, -1)
        tiny_c = np.array([0., 1e-8, -1e-8, 1., -1.], np.float32)
        huge = np.array([3e38, -3e38], np.float32)
        # Against gh_c = +-3e38 the reset gate's pre-activation skips -17 .. -89: there r is 4e-8 .. 2e-39, far below
        # the 4 ulp of 1 to which any fp32 sigmoid is held (1 + expf(89) already overflows to r = 0, and the equivalent
        # 0.5 tanh(x / 2) + 0.5 gives 0 from -17 on), and gh_c would turn that into a candidate of +-1 against
        # tanh(gx_c): a demand the formula does not support.  r = 0 in every evaluation (<= -104) and r >= 3e-4 stay.
        r_pre = SAT[(SAT >= -8.) | (SAT <= -104.)]
        b = np.array(np.meshgrid(r_pre, SAT, tiny_c, huge, indexing="ij")).reshape(4, -1)
        g = np.concatenate([a, b], 1)
        n = g.shape[1] // hh * hh
        g = g[:, -n:]                                             # whole rows; the gh_c = +-3e38 block is kept
        batch = n // hh
        rows = lambda v: v.reshape(batch, hh)                                            # noqa: E731
        gx = np.concatenate([rows(g[0]), rows(g[1]), rows(g[2])], 1)
        gh = np.concatenate([np.zeros((batch, 2 * hh), np.float32), rows(g[3])], 1)
        hp = rows(_cycle(np.array([0., 1., -1., 0.5, -0.5, 1e-8, -1e-8], np.float32), n))
        fwd = dict(gx=gx, gh=gh, h_prev=hp)
        if kernel == "gru_fwd":
            return fwd, batch
        return dict(dh=rows(_cycle(GRADS, n, 2)), dh_rec=rows(_cycle(GRADS2, n)), dh_dir=rows(_cycle(C_PREV[:3], n)),
                    saved=_ref("gru_fwd", fwd, np.float32)["saved"], h_prev=hp), batch
    g = np.array(np.meshgrid(SAT, SAT, indexing="ij")).reshape(2, -1)                              # gx + gh: 23 x 23
    batch = g.shape[1] // hh
    fwd = dict(gx=g[0].reshape(batch, hh), gh=g[1].reshape(batch, hh))
    if kernel == "rnn_fwd":
        return fwd, batch
    n = batch * hh
    return dict(dh=_cycle(GRADS, n).reshape(batch, hh), dh_rec=_cycle(GRADS2, n).reshape(batch, hh),
                h=_ref("rnn_fwd", fwd, np.float32)["h"]), batch


@pytest.mark.parametrize("kernel", NAMES)
def test_cell_saturated_gates(L, kernel):
    x, batch = _sat_inputs(kernel)
    absent = tuple(k for k, v in x.items() if v is None)
    got = _run(L, kernel, x, batch, HID_SAT, absent=absent)
    want64, s = _compare(kernel, x, got, saturated=True, what="saturated")
    want32 = _ref(kernel, x, np.float32)
    for name, g in got.items():
        w = want64[name]
        sc = s[name] + np.zeros(w.shape)
        valid = np.isfinite(w) & (np.abs(w) <= FLT_MAX)
        assert valid.mean() > 0.9                                 # only products past FLT_MAX are left out
        assert np.isfinite(g[valid]).all(), (kernel, name, "NaN / inf where float64 has none",
                                             int((~np.isfinite(g[valid])).sum()))
        tol = max(4. * _err(want32[name], w, sc)[0], 4. * EPS) * sc
        with np.errstate(over="ignore"):
            w32 = w.astype(np.float32)
        exact = valid & ((w32 == 0.) | (np.abs(w32) == 1.))      # float64 rounds to exactly 0 / +-1 in fp32
        assert exact.any()
        assert (np.abs(g[exact].astype(np.float64) - w32[exact]) <= tol[exact]).all(), (kernel, name, "0 / +-1")
        big = valid & (np.abs(w) > tol)
        assert (np.sign(g[big]) == np.sign(w[big])).all(), (kernel, name, "sign")
    if kernel == "gru_bwd":                                       # the regression: r == 0 exactly, gh_c = +-3e38, c unsaturated
        r, u, c, hc = _cols(x["saved"], 4)
        hit = (r == 0.) & (np.abs(hc) > 1e38) & (np.abs(c) < 1.) & (u > 0.) & (np.abs(x["dh"] + x["dh_rec"] + x["dh_dir"]) > 1.)
        assert hit.any()
        assert not got["dgx"][:, :HID_SAT][hit].any() and not got["dgh"][:, :HID_SAT][hit].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. limits of the six entry points
# ---------------------------------------------------------------------------------------------------------------------

def _small_call(kernel, batch=2, hidden=4):
    """A valid small call: A (name -> (ptr, stride)), the tensors kept alive, the outputs NaN-filled."""
    keep, A, outs = {}, {}, []
    for name, mult, strided, optional in _args(kernel):
        is_out = (name, mult, strided, optional) in KERNELS[kernel]["outs"]
        t = torch.full((batch, mult * hidden), NAN, device=DEV) if is_out else torch.rand(batch, mult * hidden, device=DEV)
        keep[name] = t
        A[name] = (t.data_ptr(), mult * hidden)
        if is_out:
            outs.append(t)
    return A, keep, outs


@pytest.mark.parametrize("kernel", NAMES)
def test_cell_entry_point_refuses_past_its_limits(L, kernel):
    """Small buffers, large numbers: nothing a refused call could have touched is needed.  ARL_E_RANGE for sizes and
    strides, ARL_E_ARG for a mandatory null pointer; the message names the entry point and the limit; no output
    written."""
    lib = L.load()
    A, keep, outs = _small_call(kernel)
    fn = "arl_%s_cell_%s" % tuple(kernel.split("_"))

    def refused(code, text, A_=A, batch=2, hidden=4):
        rc = _call(L, kernel, A_, batch, hidden)
        msg = lib.arl_last_error().decode()
        assert rc == code and fn in msg and text in msg, (rc, msg, text)
    for batch in (0, -1, -(1 << 40), MAX_BATCH + 1, 1 << 40, (1 << 63) - 1):
        refused(E_RANGE, "1 <= batch <= 2^24", batch=batch)
    for hidden in (0, -1, -(1 << 31), MAX_HIDDEN + 1, 1 << 29, (1 << 30) + 3, (1 << 31) - 1):
        refused(E_RANGE, "1 <= hidden <= 2^20", hidden=hidden)
    for name, mult, strided, optional in _args(kernel):
        if not optional:
            refused(E_ARG, "null pointer", dict(A, **{name: (None, A[name][1])}))
        if strided:                                              # rows that would overlap; a row distance past 2^28
            for stride in (mult * 4 - 1, 0, -mult * 4, MAX_STRIDE + 1, 1 << 62):
                refused(E_RANGE, "row width <= stride <= 2^28", dict(A, **{name: (A[name][0], stride)}))
    torch.cuda.synchronize()
    for t in outs:
        assert bool(_nan_bits(t).all())
    assert _call(L, kernel, A, 2, 4) == 0                        # ... and the same small call inside the limits runs
    torch.cuda.synchronize()
    for t in outs:
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("shape", [(1, MAX_HIDDEN), (MAX_BATCH, 1)], ids=["hidden2^20", "batch2^24"])
@pytest.mark.parametrize("kernel", NAMES)
def test_cell_largest_accepted_sizes_vs_float64(L, kernel, shape):
    batch, hidden = shape
    rs = np.random.RandomState(hidden % 1000 + NAMES.index(kernel))
    x = _inputs(kernel, rs, batch, hidden)
    _compare(kernel, x, _run(L, kernel, x, batch, hidden, twice=False), what="B%d H%d" % shape)


@pytest.mark.parametrize("kernel", NAMES)
def test_cell_stride_limits_accepted(L, kernel):
    """The largest accepted row stride (2^28 elements, two rows 1 GiB apart) for every strided argument in turn, and
    with one row any stride at all (0, negative: it is never used)."""
    batch, hidden = 2, 4
    for name in [a[0] for a in _args(kernel) if a[2]]:
        rs = np.random.RandomState(3)
        x = _inputs(kernel, rs, batch, hidden)
        lay = lambda n, w, b: (MAX_STRIDE, 5) if n == name else (w, 0)                   # noqa: E731
        _compare(kernel, x, _run(L, kernel, x, batch, hidden, layout=lay, twice=False), what="stride 2^28 " + name)
    for stride in (0, -3, 1, 1 << 40):
        x = _inputs(kernel, np.random.RandomState(4), 1, hidden)
        got = _run(L, kernel, x, 1, hidden, layout=lambda n, w, b: (stride, 2))
        _compare(kernel, x, got, what="one row, stride %d" % stride)


# ---------------------------------------------------------------------------------------------------------------------
# 3. BPTT through the policies at the edges of what they accept
# ---------------------------------------------------------------------------------------------------------------------

def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _bptt_data(kind, policy, spec, rs, nb, t_len, hidden, masked, state_scale=None, dead_segment=None):
    data = _data(kind, policy, spec, rs, nb, t_len, masked, hh=hidden)
    if state_scale is not None:                                 # stored states of that magnitude; the behaviour policy
        for key in data["state_keys"]:                          # is rebuilt from them as _data does
            data[key] = _dev((rs.randn(nb * t_len, hidden) * state_scale).astype(np.float32))
        with torch.no_grad():
            prob, value, _ = _ref_prob_value(kind, _ref_params(policy), spec, data, np.arange(nb), t_len)
            noise = _dev(rs.randn(nb * t_len, prob.shape[1]) * 0.15)
            data["old_prob"] = torch.softmax(torch.log(prob) + noise, 1).float()
            data["old_value"] = value.float()
    if dead_segment is not None:                                # an environment that ended at step 0 of the batch
        data["valids"].view(nb, t_len)[dead_segment, 1:] = 0
        assert int(data["valids"].view(nb, t_len)[dead_segment].sum()) == 1
    return data


def _bptt_check(kind, policy, spec, data, nb, t_len, segs, what):
    """loss_and_grads on the whole batch (segs None) or on the trajectory minibatch segs, against float64 autograd."""
    from accel_rl_amd import _lib
    lr_mult = torch.ones(1, device=DEV)
    masked = data["valids"] is not None
    policy.flat_grads.zero_()
    if segs is None:
        segs = np.arange(nb)
        inv = (1. / data["valids"].sum(dtype=torch.float32)).reshape(1) if masked else None
        mb = _mb(data, t_len, None)
    else:
        inv = None
        mb = _mb(data, t_len, _dev(np.asarray(segs, np.int32)))
    loss4 = policy.loss_and_grads(mb, 1, CLIP, V_COEFF, ENT_COEFF, lr_mult, inv, tie_rule=_lib.PPO_TIE_MATH).clone()
    got = policy.bucket_to_reference(policy.flat_grads)
    rp = _ref_params(policy)
    (pi, vl, el), _ = _ref_ppo_losses(kind, rp, spec, data, segs, t_len)
    want = _flat_grads(pi + vl + el, rp)
    want_l = torch.stack([pi, vl, el]).detach().float()
    scale = np.abs(want).max()
    assert np.isfinite(got).all() and np.isfinite(want).all() and scale > 0
    print("%s %s: loss4 %s want %s; max |d grad| %.3g of %.3g" % (kind, what, loss4[:3].tolist(), want_l.tolist(),
                                                                   np.abs(got - want).max(), scale))
    assert torch.allclose(loss4[:3], want_l, rtol=1e-4, atol=1e-6), (what, loss4.tolist(), want_l.tolist())
    assert np.allclose(got, want, rtol=GRAD_RTOL, atol=GRAD_ATOL * max(scale, 1e-3)), (what, np.abs(got - want).max(), scale)


BPTT_SIZES = [(4, 5), (1024, 5), (256, 1), (256, 32)]


@pytest.mark.parametrize("size", BPTT_SIZES, ids=lambda s: "H%d-T%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_bptt_narrowest_widest_shortest_longest(kind, size):
    hidden, t_len = size
    nb = 8
    policy, spec = _make(kind, hidden)
    rs = np.random.RandomState(hidden + t_len)
    for masked in (False, True):
        data = _bptt_data(kind, policy, spec, rs, nb, t_len, hidden, masked)
        _bptt_check(kind, policy, spec, data, nb, t_len, None, "whole batch, masked %s" % masked)
        _bptt_check(kind, policy, spec, data, nb, t_len, [5, 2, 7, 0], "4 of 8 segments, masked %s" % masked)


@pytest.mark.parametrize("hidden", [4, 256, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_bptt_one_segment(kind, hidden):
    """nb = 1: every per-step dense product has one row; and a trajectory minibatch of one segment out of eight."""
    t_len = 5
    policy, spec = _make(kind, hidden)
    rs = np.random.RandomState(hidden + 1)
    for masked in (False, True):
        one = _bptt_data(kind, policy, spec, rs, 1, t_len, hidden, masked)
        _bptt_check(kind, policy, spec, one, 1, t_len, None, "one segment, whole, masked %s" % masked)
        _bptt_check(kind, policy, spec, one, 1, t_len, [0], "one segment, traj, masked %s" % masked)
        eight = _bptt_data(kind, policy, spec, rs, 8, t_len, hidden, masked)
        _bptt_check(kind, policy, spec, eight, 8, t_len, [6], "1 of 8 segments, masked %s" % masked)


@pytest.mark.parametrize("kind", KINDS)
def test_bptt_segment_invalid_after_step_0_and_large_states(kind):
    hidden, nb, t_len = 256, 8, 5
    policy, spec = _make(kind, hidden)
    rs = np.random.RandomState(11)
    dead = _bptt_data(kind, policy, spec, rs, nb, t_len, hidden, True, dead_segment=3)
    _bptt_check(kind, policy, spec, dead, nb, t_len, None, "segment 3 invalid after step 0, whole")
    _bptt_check(kind, policy, spec, dead, nb, t_len, [3, 1, 4], "segment 3 invalid after step 0, traj")
    _bptt_check(kind, policy, spec, dead, nb, t_len, [3], "only the invalid segment")
    for masked in (False, True):
        big = _bptt_data(kind, policy, spec, rs, nb, t_len, hidden, masked, state_scale=10.)
        _bptt_check(kind, policy, spec, big, nb, t_len, None, "states ~10, whole, masked %s" % masked)
        _bptt_check(kind, policy, spec, big, nb, t_len, [7, 0, 3, 4], "states ~10, traj, masked %s" % masked)


@pytest.mark.parametrize("kind", KINDS)
def test_recurrent_widths_refused_at_construction(kind):
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    cls = _policy_cls(kind)
    for hidden in (0, 2, 6, 1028):
        with pytest.raises(NotImplementedError, match="recurrent width must be a multiple of 4 and <= 1024"):
            cls(**dict(cnn_specs[0], hidden_sizes=[hidden]))
    with pytest.raises(NotImplementedError, match="exactly one recurrent layer"):
        cls(**dict(cnn_specs[0], hidden_sizes=[256, 256]))
    for hidden in (4, 1024):
        assert cls(**dict(cnn_specs[0], hidden_sizes=[hidden]))._H == hidden
