"""The linear recurrent unit over time (arl_lru_params / _fwd / _bwd / _param_fold, csrc/lru.hip) against a float64
restatement of accel_rl_hip.h's formulas: a NumPy loop over t in complex arithmetic, sharing nothing with the bindings.
The bar is the attention tests' `close`: rtol 2e-3, atol 2e-5 of max |want|.  The last test needs no device."""
import ctypes

import numpy as np
import pytest
import torch

from accel_rl_amd._lib import LRU_CHUNK_MIN as CM
from test_attention_gpu import DEV, E_ALIGN, E_ARG, E_RANGE, NAN, TAIL, L, _dev, _host, _padded, close      # noqa: F401

NAMES = ("lam", "gam", "h_all", "h_last", "du", "dnu", "dtheta")


def flags_of(pattern, s, t):
    # chunk_last / chunk_first: the last step of chunk 0 / the first of chunk 1 (a flag cuts the carry into the NEXT step)
    f, c = np.zeros((s, t), np.uint8), (t + 3) // 4
    if pattern == "every":
        f[:] = 1
    elif pattern == "last":
        f[:, t - 1] = 1
    elif pattern == "chunk_last":
        f[:, min(c, t) - 1] = 1
        f[s - 1, min(3 * c, t) - 1] = 1
    elif pattern == "chunk_first":
        f[:, min(c, t - 1)] = 1
        f[s - 1, min(2 * c, t - 1)] = 1
    return f


def lru64(nu, theta, u, h0, flags, dh):
    s, t, n = u.shape[0], u.shape[1], nu.size
    cplx = lambda a: a.astype(np.float64).reshape(a.shape[:-1] + (n, 2)) @ np.array([1, 1j])    # noqa: E731
    pairs = lambda c: np.stack([c.real, c.imag], -1).reshape(c.shape[:-1] + (2 * n,))           # noqa: E731
    e = np.exp(nu.astype(np.float64))
    mag = np.exp(-e)
    lam, gam = mag * np.exp(1j * theta.astype(np.float64)), np.sqrt(1 - mag ** 2)
    uc, hc, dc = cplx(u), cplx(h0), cplx(dh)
    keep = np.ones((s, t + 1, 1))
    keep[:, 1:t, 0] = flags[:, :t - 1] == 0
    keep[:, t] = 0
    h, du, prev = np.empty((s, t, n), complex), np.empty((s, t, n), complex), hc
    for i in range(t):
        prev = h[:, i] = keep[:, i] * lam * prev + gam * uc[:, i]
    g, dlam, dgam = np.zeros((s, n), complex), 0, 0
    for i in reversed(range(t)):
        g = dc[:, i] + keep[:, i + 1] * np.conj(lam) * g
        du[:, i] = gam * g
        dlam = dlam + (keep[:, i] * np.conj(hc if i == 0 else h[:, i - 1]) * g).sum(0)
        dgam = dgam + (uc[:, i].real * g.real + uc[:, i].imag * g.imag).sum(0)
    dtheta = -lam.imag * dlam.real + lam.real * dlam.imag
    dnu = -e * (lam.real * dlam.real + lam.imag * dlam.imag) + dgam * e * mag ** 2 / gam
    return [pairs(lam).reshape(n, 2), gam, pairs(h), pairs(h[:, -1]), pairs(du), dnu, dtheta]


def run_lru(L, nu, theta, u, h0, reset, idx, dh, in_place=False):
    (s, t, n2), n = u.shape, nu.size
    bufs = [_padded(m) for m in (2 * n, n, u.size, s * n2, u.size, s * n2, s * n, n, n)]
    lam, gam, h_all, h_last, du, dlam, dgam, dnu, dtheta = (b[1].view(shape) for b, shape in zip(
        bufs, ((n, 2), (n,), u.shape, (s, n2), u.shape, (s, n, 2), (s, n), (n,), (n,))))
    ud, h0d, dhd, nud, thd = _dev(u), _dev(h0), _dev(dh), _dev(nu), _dev(theta)
    if in_place:
        h_last, du = h0d, dhd
    L.lru_params(nud, thd, lam, gam)
    L.lru_fwd(ud, lam, gam, h0d, h_all, h_last, reset, idx)
    L.lru_bwd(ud, h_all, _dev(h0), lam, gam, dhd, du, dlam, dgam, reset, idx)
    L.lru_param_fold(dlam, dgam, nud, thd, dnu, dtheta)
    torch.cuda.synchronize()
    assert all(torch.isnan(b[0][-TAIL:]).all() for b in bufs)
    return lam, gam, h_all, h_last, du, dnu, dtheta


PATTERNS = ("null", "zeros", "chunk_last", "chunk_first", "every", "last")
# every T at every N, the rest taking turns; T = 1024 and |lam| at both ends; the grid-stride walks (4100 and 1030 items)
CASES = [(t, n, (1, 3)[(i + j) % 2], PATTERNS[(4 * i + j) % 6], (i + j) % 3 == 0, None)
         for i, t in enumerate((1, CM - 1, CM, CM + 1, 130)) for j, n in enumerate((2, 64, 66, 512))]
CASES += [(1024, 2, 1, "chunk_first", False, None), (1024, 66, 3, "null", False, 0.9999), (1024, 4, 1, "chunk_last", True, 0.9999),
          (130, 64, 3, "null", False, 0.1), (CM - 1, 66, 3, "zeros", False, 0.9999), (1024, 2, 3, "every", False, 0.1),
          (2, 2, 4100, "chunk_first", False, None), (CM + 1, 2, 1030, "chunk_last", True, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("t,n,s,pattern,mapped,mag", CASES)
def test_lru_matches_float64_inside_its_buffers_twice(L, t, n, s, pattern, mapped, mag):
    rs = np.random.RandomState(1000 * t + 10 * n + s)
    mags = rs.uniform(0.5, 0.99, size=n) if mag is None else np.full(n, mag)
    nu, theta = np.log(-np.log(mags)).astype(np.float32), rs.uniform(0, 2 * np.pi, size=n).astype(np.float32)
    u, h0, dh = (rs.randn(*shape).astype(np.float32) for shape in ((s, t, 2 * n), (s, 2 * n), (s, t, 2 * n)))
    flags = flags_of(pattern, s, t)
    reset, idx = (None if pattern == "null" else _dev(flags.reshape(-1))), None
    if mapped:                  # the segments' rows scattered over a larger batch whose other flags are all set
        rows = rs.permutation(s * t + 11)[:s * t].astype(np.int32)
        full = np.ones(s * t + 11, np.uint8)
        full[rows] = flags.reshape(-1)
        reset, idx = _dev(full), _dev(rows)
    want = lru64(nu, theta, u, h0, flags, dh)
    got = run_lru(L, nu, theta, u, h0, reset, idx, dh)
    what = "T %d N %d S %d %s map %d |lam| %s " % (t, n, s, pattern, mapped, mag)
    for g, w, name in zip(got, want, NAMES):
        assert close(_host(g), w, what + name), name
    assert torch.equal(got[3], got[2][:, -1])                   # h_last is the last step's state, bit for bit
    same = lambda other: all(torch.equal(x, y) for x, y in zip(other, got))     # noqa: E731
    assert same(run_lru(L, nu, theta, u, h0, reset, idx, dh))                   # two launches: the same bits
    assert same(run_lru(L, nu, theta, u, h0, reset, idx, dh, in_place=True))    # h_last over h0, du over dh
    if pattern in ("null", "zeros", "last") and not mapped:     # an all-zero mask is no mask; nothing reads the last flag
        assert same(run_lru(L, nu, theta, u, h0, None if reset is not None else _dev(flags.reshape(-1)), None, dh))


@pytest.mark.gpu
@pytest.mark.parametrize("t", [CM - 2, CM + 8])
def test_served_steps_in_place_reproduce_the_training_forward(L, t):
    rs, s, n = np.random.RandomState(t), 3, 66
    nu, theta = np.log(-np.log(rs.uniform(0.5, 0.99, size=n))).astype(np.float32), rs.uniform(0, 6, size=n).astype(np.float32)
    u, h0 = rs.randn(s, t, 2 * n).astype(np.float32), rs.randn(s, 2 * n).astype(np.float32)
    flags = (rs.uniform(size=(s, t)) < 0.1).astype(np.uint8)
    lam, gam, whole = torch.empty((n, 2), device=DEV), torch.empty(n, device=DEV), torch.empty((s, t, 2 * n), device=DEV)
    L.lru_params(_dev(nu), _dev(theta), lam, gam)
    L.lru_fwd(_dev(u), lam, gam, _dev(h0), whole, None, _dev(flags.reshape(-1)))
    state, step = _dev(h0), torch.empty((s, 1, 2 * n), device=DEV)
    for i in range(t):
        L.lru_fwd(_dev(u[:, i:i + 1]), lam, gam, state, step, state)
        assert torch.equal(step[:, 0], state)
        assert close(_host(state), _host(whole[:, i]).astype(np.float64), "T %d step %d" % (t, i))
        state.mul_(_dev(1 - flags[:, i:i + 1].astype(np.float32)))              # the sampler's reset_rows


def test_refusals_come_back_before_any_launch():
    """No device: s = 2, t = 4, n = 4 on host addresses that are never dereferenced; then AtariLruPolicy's constructor."""
    from accel_rl_amd import _build, _lib
    from accel_rl_amd.policies import AtariLruPolicy
    _build.build_extension()
    lib = _lib.load()
    assert all("arl_lru_" + k in _lib.EXPORTED_SYMBOLS for k in ("params", "fwd", "bwd", "param_fold")) and lib.arl_abi_version() == 5
    assert (_lib.LRU_MAX_STEPS, _lib.LRU_MAX_STATE, CM) == (1024, 512, 32)
    ok = _lib.lru_shape_ok
    assert ok(1, 2) and ok(1024, 512) and not any((ok(0, 2), ok(1025, 2), ok(1, 0), ok(1, 3), ok(1, 514)))
    raw = ctypes.create_string_buffer(16 * 512 + 64)
    p = (ctypes.addressof(raw) + 15) // 16 * 16
    a = {k: p + 512 * i for i, k in enumerate(("u", "h_all", "dh", "du", "h0", "h_last", "lam", "gam", "nu", "theta", "dlam",
                                               "dgam", "dnu", "dtheta", "idx"))}
    dims = dict(s=2, t=4, n=4)
    calls = dict(
        fwd=lambda v: lib.arl_lru_fwd(v["u"], v["lam"], v["gam"], v["h0"], None, v["idx"], v["s"], v["t"], v["n"], v["h_all"],
                                      v["h_last"], None),
        bwd=lambda v: lib.arl_lru_bwd(v["u"], v["h_all"], v["h0"], v["lam"], v["gam"], v["dh"], None, v["idx"], v["s"], v["t"],
                                      v["n"], v["du"], v["dlam"], v["dgam"], None),
        params=lambda v: lib.arl_lru_params(v["nu"], v["theta"], v["n"], v["lam"], v["gam"], None),
        fold=lambda v: lib.arl_lru_param_fold(v["dlam"], v["dgam"], v["nu"], v["theta"], v["s"], v["n"], v["dnu"], v["dtheta"], None))
    null = dict(fwd=("u", "lam", "gam", "h0", "h_all"), bwd=("u", "h_all", "h0", "lam", "gam", "dh", "du", "dlam", "dgam"),
                params=("nu", "theta", "lam", "gam"), fold=("dlam", "dgam", "nu", "theta", "dnu", "dtheta"))
    over = dict(fwd=(("h_all", "u", 0), ("h_all", "h0", 0), ("h_last", "u", 0), ("h_last", "h0", 16), ("h_last", "h_all", 240)),
                bwd=(("du", "u", 0), ("du", "dh", 16), ("du", "h_all", 0), ("dlam", "dh", 0), ("dgam", "lam", 0), ("dgam", "dlam", 0)),
                params=(("lam", "nu", 0), ("gam", "lam", 16)), fold=(("dnu", "nu", 0), ("dtheta", "dnu", 0), ("dnu", "dgam", 16)))
    size = dict(fwd=(("s", 0), ("s", 2 ** 24 + 1), ("t", 0), ("t", 1025), ("n", 0), ("n", 3), ("n", 514)),
                params=(("n", 0), ("n", 3), ("n", 514)), fold=(("s", 0), ("s", 2 ** 24 + 1), ("n", 5), ("n", 514)))
    size["bwd"] = size["fwd"]
    off = dict(fwd=(("u", 4), ("h0", 8), ("h_all", 4), ("h_last", 8), ("lam", 2), ("gam", 2), ("idx", 2)),
               bwd=(("u", 8), ("h_all", 4), ("h0", 4), ("dh", 8), ("du", 4), ("lam", 2), ("gam", 2), ("dlam", 2), ("dgam", 2)),
               params=(("nu", 2), ("theta", 1), ("lam", 2), ("gam", 3)), fold=(("dlam", 2), ("dgam", 2), ("nu", 2), ("dtheta", 2)))
    for name, call in calls.items():
        base = dict(a, **dims)
        for k in null[name]:
            assert call(dict(base, **{k: None})) == E_ARG, (name, k)
        for k, other, shift in over[name]:
            assert call(dict(base, **{k: base[other] + shift})) == E_ARG, (name, k, other)
        for k, v in size[name]:
            assert call(dict(base, **{k: v})) == E_RANGE, (name, k, v)
        for k, shift in off[name]:
            assert call(dict(base, **{k: base[k] + shift})) == E_ALIGN, (name, k)
        assert ("arl_lru_" + dict(fold="param_fold").get(name, name)).encode() in lib.arl_last_error()
    trunk = dict(conv_filters=(8, 8), conv_filter_sizes=(4, 3), conv_strides=(2, 1), conv_pads=((0, 0), (0, 0)))
    good = dict(trunk, hidden_sizes=(16,), state_size=8)
    p = AtariLruPolicy(**good)
    assert p.recurrent and p.state_info_keys == ["lru_0"] and p.supports_bptt_resets and not p.serve_supported()
    assert [x for x, _ in p.reference_layout((4, 20, 16), 5)][4:11] == ["LruWx", "LruBx", "LruNu", "LruTheta", "LruWb", "LruWc", "LruBo"]
    for change in (dict(hidden_sizes=()), dict(hidden_sizes=(16, 16)), dict(hidden_sizes=(18,)), dict(state_size=0),
                   dict(state_size=3), dict(state_size=514), dict(state_size=8.0), dict(r_min=0.95, r_max=0.9),
                   dict(r_max=1.0), dict(max_phase=0.)):
        with pytest.raises(NotImplementedError, match="section E"):
            AtariLruPolicy(**dict(good, **change))
