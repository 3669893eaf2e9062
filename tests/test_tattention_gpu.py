"""Windowed causal attention over time on the GPU (arl_tattn_fwd / _bwd / _rel_fold / _shift, csrc/tattention.hip) against
a float64 restatement of accel_rl_hip.h's arithmetic: dense masked matrices on the CPU, differentiated by autograd, sharing
nothing with the bindings.  The bar is the attention tests' `close`: rtol 2e-3, atol 2e-5 of max |want|."""
import numpy as np
import pytest
import torch

from test_attention_gpu import DEV, E_ALIGN, E_ARG, E_RANGE, NAN, TAIL, L, _dev, _host, _padded, close      # noqa: F401

pytestmark = pytest.mark.gpu

PATTERNS = ("null", "zeros", "step0", "last", "every", "two")


def flags_of(pattern, s, t):
    f = np.zeros((s, t), np.uint8)
    if pattern == "step0":
        f[:, 0] = 1
    elif pattern == "last":
        f[:, t - 1] = 1
    elif pattern == "every":
        f[:] = 1
    elif pattern == "two":                      # two in the middle, at other steps in every segment
        for i in range(s):
            f[i, (t // 3 + i) % t] = f[i, (2 * t // 3 + i) % t] = 1
    return f


def masks(flags, m):
    """(age [T, L], in the window [S, T, L], live [S, T, L]) from the flags [S, T]."""
    s, t = flags.shape
    age = m + np.arange(t)[:, None] - np.arange(m + t)[None, :]
    r = np.zeros((s, t), np.int64)
    for i in range(s):
        for j in range(1, t):
            r[i, j] = j if flags[i, j - 1] else r[i, j - 1]
    live = (r[:, :, None] == 0) | (np.arange(m + t)[None, None, :] >= m + r[:, :, None])
    return age, np.broadcast_to((age >= 0) & (age <= m), live.shape), live


def tattn64(q, kv, rel, flags, dout, scale):
    """float64: out [S, T, H d], lse [S, H, T], dq, dkv, drel."""
    m = kv.shape[1] - q.shape[1]
    age, win, live = masks(flags, m)
    qt, kvt, relt = (torch.from_numpy(x.astype(np.float64)).requires_grad_() for x in (q, kv, rel))
    live_t = torch.from_numpy(live.astype(np.float64))[:, None]                                # [S, 1, T, L]
    k, v = kvt[:, :, 0].transpose(1, 2), kvt[:, :, 1].transpose(1, 2)                          # [S, H, L, d]
    bias = relt[:, torch.from_numpy(np.clip(age, 0, m))]                                       # [H, T, L]
    sc = live_t * (scale * qt.transpose(1, 2) @ k.transpose(2, 3)) + bias[None]
    sc = sc.masked_fill(torch.from_numpy(~win)[:, None], -np.inf)
    out = ((torch.softmax(sc, dim=3) * live_t) @ v).transpose(1, 2).flatten(2)
    grads = torch.autograd.grad(out, (qt, kvt, relt), torch.from_numpy(dout.astype(np.float64)))
    seen = (win & live).any(axis=1)                                                            # [S, L]
    return [out.detach().numpy(), torch.logsumexp(sc, dim=3).detach().numpy()] + [g.numpy() for g in grads], seen


def run_tattn(L, q, kv, rel, reset, idx, dout, scale):
    s, t, h, d = q.shape
    m = kv.shape[1] - t
    bufs = [_padded(n) for n in (q.size, s * h * t, q.size, kv.size, s * h * (m + 1), h * (m + 1))]
    out, lse, dq, dkv, parts, drel = (b[1].view(shape) for b, shape in zip(
        bufs, ((s, t, h * d), (s, h, t), q.shape, kv.shape, (s, h, m + 1), (h, m + 1))))
    qd, kd, rd = _dev(q), _dev(kv), _dev(rel)
    L.tattn_fwd(qd, kd, rd, out, lse, reset, idx, scale)
    L.tattn_bwd(qd, kd, rd, out, lse, _dev(dout), dq, dkv, parts, reset, idx, scale)
    L.tattn_rel_fold(parts, drel)
    torch.cuda.synchronize()
    assert all(torch.isnan(b[0][-TAIL:]).all() for b in bufs)
    return out, lse, dq, dkv, drel


TM = ((1, 1), (1, 16), (5, 16), (33, 31), (64, 64), (64, 1), (2, 64))
# every (T, M) at every d; heads, segments, the reset pattern and the row map take turns; then the grid-stride walk
# (1030 items on at most 1024 workgroups) and two ramps
CASES = [(t, m, d, (1, 3)[(i + j) % 2], (1, 5)[(i + j // 2) % 2], PATTERNS[(4 * i + j) % 6], (i + j) % 3 == 0, False)
         for i, (t, m) in enumerate(TM) for j, d in enumerate((4, 32, 36, 64))]
CASES += [(2, 3, 4, 1, 1030, "two", False, False), (5, 16, 4, 3, 400, "last", True, False),
          (64, 64, 32, 3, 5, "two", True, True), (33, 31, 64, 1, 5, "null", False, True)]


@pytest.mark.parametrize("t,m,d,h,s,pattern,mapped,ramp", CASES)
def test_tattention_matches_float64_inside_its_buffers_twice(L, t, m, d, h, s, pattern, mapped, ramp):
    rs = np.random.RandomState(1000 * t + 10 * m + d + h + s)
    q, kv = rs.randn(s, t, h, d).astype(np.float32), rs.randn(s, m + t, 2, h, d).astype(np.float32)
    rel, dout = rs.randn(h, m + 1).astype(np.float32), rs.randn(s, t, h * d).astype(np.float32)
    if ramp:                    # scores over +-30: the running maximum moves between the context tiles
        kv[:, :, 0] *= (1 + 4 * (np.arange(m + t) // 16)).astype(np.float32)[None, :, None, None]
        rel *= 5
    flags = flags_of(pattern, s, t)
    reset, idx = (None if pattern == "null" else _dev(flags.reshape(-1))), None
    if mapped:                  # the segments' rows scattered over a larger batch whose other flags are all set
        rows = rs.permutation(s * t + 11)[:s * t].astype(np.int32)
        full = np.ones(s * t + 11, np.uint8)
        full[rows] = flags.reshape(-1)
        reset, idx = _dev(full), _dev(rows)
    scale = d ** -0.5
    want, seen = tattn64(q, kv, rel, flags, dout, scale)
    got = run_tattn(L, q, kv, rel, reset, idx, dout, scale)
    what = "T %d M %d d %d H %d S %d %s map %d ramp %d " % (t, m, d, h, s, pattern, mapped, ramp)
    for g, w, name in zip(got, want, ("out", "lse", "dq", "dkv", "drel")):
        assert close(_host(g), w, what + name), name
    assert not _host(got[3])[~seen].any()                       # a context row nobody sees: exact zeros
    assert all(torch.equal(x, y) for x, y in zip(run_tattn(L, q, kv, rel, reset, idx, dout, scale), got))   # the same bits
    if pattern in ("null", "zeros") and not mapped:             # an all-zero mask is no mask
        other = None if reset is not None else _dev(flags.reshape(-1))
        assert all(torch.equal(x, y) for x, y in zip(run_tattn(L, q, kv, rel, other, None, dout, scale), got))
    inference = torch.full_like(got[0], NAN)
    L.tattn_fwd(_dev(q), _dev(kv), _dev(rel), inference, None, reset, idx, scale)
    assert torch.equal(inference, got[0])                       # without lse: the same output


@pytest.mark.parametrize("with_prev", [True, False])
def test_shift_builds_the_window_and_moves_the_state(L, with_prev):
    rs = np.random.RandomState(3)
    b, m, e = 5, 3, 20
    state, new = rs.randn(b, m * e).astype(np.float32), rs.randn(b, e).astype(np.float32)
    sd, window = _dev(state), torch.full((b, m + 1, e), NAN, device=DEV)
    prev = torch.full((b, m * e), NAN, device=DEV) if with_prev else None
    L.tattn_shift(sd, _dev(new), window, prev)
    want = np.concatenate([state, new], axis=1)
    assert np.array_equal(_host(window).reshape(b, -1), want) and np.array_equal(_host(sd), want[:, e:])
    assert prev is None or np.array_equal(_host(prev), state)


def test_fold_and_shift_refusals_write_nothing(L):
    lib = L.load()
    parts, e = torch.zeros(2 * 2 * 4 + 4, device=DEV), torch.zeros(2 * 8 + 4, device=DEV)
    drel, state, window = (torch.full((n + 4,), NAN, device=DEV) for n in (8, 2 * 3 * 8, 2 * 4 * 8))
    p = lambda t: t.data_ptr()                                  # noqa: E731
    fold = lambda parts_=p(parts), s=2, h=2, m=3, d_=p(drel): lib.arl_tattn_rel_fold(parts_, s, h, m, d_, None)   # noqa: E731
    shift = lambda st=p(state), e_=p(e), m=3, w=8, win=p(window): lib.arl_tattn_shift(st, e_, 2, m, w, win, None, None)  # noqa: E731
    assert [fold(s=0), fold(h=0), fold(h=65), fold(m=0), fold(m=65)] == [E_RANGE] * 5
    assert fold(d_=None) == E_ARG and fold(d_=p(parts)) == E_ARG and fold(d_=p(drel) + 2) == E_ALIGN
    assert [shift(m=0), shift(m=65), shift(w=0), shift(w=6), shift(w=1028)] == [E_RANGE] * 5
    assert shift(e_=None) == E_ARG and shift(win=p(state)) == E_ARG and shift(win=p(window) + 4) == E_ALIGN
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (drel, state, window))


REFUSALS = [(dict(t=0), E_RANGE), (dict(t=65), E_RANGE), (dict(m=0), E_RANGE), (dict(m=65), E_RANGE), (dict(d=0), E_RANGE),
            (dict(d=6), E_RANGE), (dict(d=68), E_RANGE), (dict(h=0), E_RANGE), (dict(h=65, d=4), E_RANGE),
            (dict(s=0), E_RANGE), (dict(s=2 ** 24 + 1), E_RANGE), (dict(scale=float("inf")), E_ARG), (dict(null="q"), E_ARG),
            (dict(null="rel"), E_ARG), (dict(null="out"), E_ARG), (dict(over="out"), E_ARG), (dict(off="q"), E_ALIGN),
            (dict(off="out"), E_ALIGN)]


@pytest.mark.parametrize("change,code", REFUSALS)
def test_refusals_write_nothing(L, change, code):
    lib = L.load()
    c = dict(s=2, t=4, m=3, h=2, d=8, scale=1.0)
    n_q, n_kv = c["s"] * c["t"] * c["h"] * c["d"], c["s"] * (c["t"] + c["m"]) * 2 * c["h"] * c["d"]
    ins = {k: torch.zeros(n + 4, device=DEV) for k, n in (("q", n_q), ("kv", n_kv), ("rel", 8), ("dout", n_q))}
    outs = {k: torch.full((n + 4,), NAN, device=DEV) for k, n in (("out", n_q), ("lse", 16), ("dq", n_q), ("dkv", n_kv),
                                                                   ("parts", 16))}
    p = {k: v.data_ptr() for k, v in list(ins.items()) + list(outs.items())}
    if "null" in change:
        p[change["null"]] = None
    if "over" in change:
        p[change["over"]] = p["q"]
    if "off" in change:
        p[change["off"]] += 4
    c.update({k: v for k, v in change.items() if k in c})
    dims = (c["s"], c["t"], c["m"], c["h"], c["d"], c["scale"])
    assert lib.arl_tattn_fwd(p["q"], p["kv"], p["rel"], None, None, *dims, p["out"], p["lse"], None) == code
    dq = p["kv"] if "over" in change else p["dq"]              # (the backward's `out` is an input: its output over one)
    assert lib.arl_tattn_bwd(p["q"], p["kv"], p["rel"], None, None, p["out"], p["lse"], p["dout"], dq, p["dkv"], p["parts"],
                             *dims, None) == code
    torch.cuda.synchronize()
    assert all(torch.isnan(v).all() for v in outs.values())
