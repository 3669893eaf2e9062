"""The kernels every policy-gradient run passes through between rollout and learner -- csrc/scan.hip (GAE, n-step
returns, valids), csrc/batch_ops.hip (standardise, categorical sampling, NCHW gather) and the element-wise kernels of
csrc/learner.hip (NHWC gather, bias + ReLU, ReLU backward with bias gradient) -- at the edges of what their entry
points accept, driven through the raw C entry points and compared with the references of tests/batch_ref.py.

The rules of every comparison:
- scans: bit for bit with oracle.ref_port, both exact promotions, on every route of dispatch() (batch_ref.scan_route);
  the tolerance mode (promo = 2) within the bar test_wave_suffix_scan_within_tolerance takes from BASELINE.json;
- valids, sampling, gathers: equal; bias + ReLU, its backward and the bias gradient: bit for bit with NumPy float32,
  the gradient in the kernels' own order of additions (batch_ref.dbias_restatement);
- standardise: inside batch_ref.standardize_bound of a float64 two-pass reference;
- every buffer a kernel writes sits 16-byte aligned (or deliberately shifted) inside a filled allocation with 64 guard
  elements on either side, unchanged after every launch; every input sits between NaN pads of its own;
- a refused call returns its ARL_E_* code and leaves the guarded outputs untouched.

tests/test_batch_limits_host.py shows on the CPU that these very inputs tell each nearest wrong kernel apart.

Measured on an MI355X (printed at the end of the module, run with -s): the largest deviation of
arl_standardize from the float64 reference is 0.850 of the bound (n = 255 and 257, eps = 0.5, mu = 100 sigma).  The
kernel's float32 denominator could be recovered from its outputs in 92 of 93 calls (the float32 d that reproduces every
output bit); sqrt(var) = d - eps then differs from float64 by at most 8.5e-8, 9.2e-8 and 1.3e-7 relative at mu / sigma =
0, 1e2, 1e4 (the float32 roundings of d) and by 1.4e-4 at 1e6, where var = ss / c - mean^2 cancels 12 digits of a
float64: inside the bound's e64 term (4e-3 there) and far below the float32 mean's (6e-2).  The 129 tests take 6.4 s.
No kernel fault was found; none was changed."""
import numpy as np
import pytest
import torch

import batch_ref as R
from batch_ref import F32, F64
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3
FILL = {torch.float32: float("nan"), torch.float64: float("nan"), torch.int8: 91, torch.uint8: 91, torch.int32: 0}
STD = {"frac": 0.0, "sqrt": {}, "recovered": 0, "tried": 0}      # what the standardise tests measured


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    yield _lib
    print("\nbatch limits: standardise: largest deviation %.3f of the bound; sqrt(var) recovered from the outputs in %d of "
          "%d calls, largest relative error against float64 by mu / sigma: %s"
          % (STD["frac"], STD["recovered"], STD["tried"], ", ".join("%g: %.3g" % kv for kv in sorted(STD["sqrt"].items()))))


def _host(t):
    return t.detach().cpu().numpy().copy()


class Guarded(object):
    """n elements inside a filled buffer (NaN, or the byte 91), at least 64 fill elements on either side; the first
    element sits `shift` elements past a 16-byte boundary."""

    def __init__(self, n, dtype=torch.float32, shift=0, init=None):
        self.n, self.lo = n, GUARD + shift
        self.buf = torch.full((GUARD + shift + (n + 15) // 16 * 16 + GUARD,), FILL[dtype], dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + n]
        assert (self.t.data_ptr() - shift * self.buf.element_size()) % 16 == 0
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def read(self):
        return _host(self.t)

    def check(self, what=""):
        out = np.concatenate([_host(self.buf[:self.lo]), _host(self.buf[self.lo + self.n:])])
        ok = np.isnan(out).all() if out.dtype.kind == "f" else (out == 91).all()
        assert ok, "a launch wrote outside its buffer: %s" % (what,)

    def untouched(self, what=""):
        """Nothing written at all: a refused call, or a no-op."""
        self.check(what)
        raw = self.read()
        assert np.isnan(raw).all() if raw.dtype.kind == "f" else (raw == 91).all(), "a refused call wrote: %s" % (what,)


def _input(a, shift=0):
    """A read-only input between pads (NaN, or the byte 91): a read past either end is harmless and shows."""
    a = np.ascontiguousarray(a)
    return Guarded(a.size, torch.from_numpy(a[:0].reshape(-1)).dtype, shift, init=a)


def _sync():
    torch.cuda.synchronize()


def _stream(L):
    return L.stream_ptr()


# ====================================================================================================== scans

class ScanRig(object):
    """One case's inputs on the device; shifts: {name: elements} off the 16-byte boundary."""

    def __init__(self, x, shifts=None):
        s = shifts or {}
        self.n, self.T = x["n"], x["T"]
        self.r, self.v = _input(x["r"], s.get("r", 0)), _input(x["v"], s.get("v", 0))
        self.d, self.lv = _input(x["d"], s.get("d", 0)), _input(x["lv"], s.get("lv", 0))
        self.o0 = Guarded(self.n * self.T, shift=s.get("o0", 0))
        self.o1 = Guarded(self.n * self.T, shift=s.get("o1", 0))

    def run(self, L, scan, promo, gamma, lam, what=""):
        """-> (out0, out1) [n, T]: GAE (advantages, returns); n-step (returns, advantages)."""
        lib = L.load()
        for o in (self.o0, self.o1):
            o.t.fill_(float("nan"))
        if scan == "gae":
            rc = lib.arl_gae_scan(self.r.ptr, self.v.ptr, self.d.ptr, self.lv.ptr, gamma, lam, self.n, self.T, promo,
                                  self.o0.ptr, self.o1.ptr, _stream(L))
        else:
            rc = lib.arl_nstep_return(self.r.ptr, self.d.ptr, self.v.ptr, self.lv.ptr, gamma, self.n, self.T, promo,
                                      self.o0.ptr, self.o1.ptr, _stream(L))
        assert rc == 0, (what, rc, lib.arl_last_error())
        _sync()
        for o in (self.o0, self.o1):
            o.check((what, scan, promo))
        return self.o0.read().reshape(self.n, self.T), self.o1.read().reshape(self.n, self.T)


def _bit_equal(got, want, what):
    for k in range(2):
        assert R.same_bits(got[k], want[k]), (what, "output %d" % k, int((R.bits(got[k]) != R.bits(want[k])).sum()),
                                              np.argwhere(R.bits(got[k]) != R.bits(want[k]))[:4].tolist())


@pytest.mark.parametrize("i", range(len(R.SCAN_CASES)), ids=["%s-%d-%d" % c for c in R.SCAN_CASES])
def test_scan_every_route_bit_for_bit(L, i):
    """Every route of dispatch() at the smallest shapes that reach it (batch_ref.SCAN_CASES), both scans and both exact
    promotions, the done pattern cycling through none / all / t = 0 / t = T - 1 / alternating / random with set bytes
    1, 2 and 255."""
    x = R.scan_case_inputs(i)
    rig = ScanRig(x)
    for scan in ("gae", "nstep"):
        for promo, pname in R.PROMOS:
            got = rig.run(L, scan, promo, 0.99, 0.95, R.SCAN_CASES[i])
            _bit_equal(got, R.scan_oracle(x, scan, pname, 0.99, 0.95), (R.SCAN_CASES[i], scan, pname))


@pytest.mark.parametrize("gamma,lam", R.SCAN_PARAMS[1:])
def test_scan_parameters_on_every_route(L, gamma, lam):
    """(gamma, lambda) = (1, 1), (0, 0.5), (0.99, 0), (0.5, 1) on one case per route with random dones."""
    for i in R.SCAN_SUB:
        route, n, T = R.SCAN_CASES[i]
        x = R.scan_inputs(n, T, "random", 2000 + i)
        rig = ScanRig(x)
        for scan in ("gae", "nstep"):
            for promo, pname in R.PROMOS:
                got = rig.run(L, scan, promo, gamma, lam, (route, n, T))
                _bit_equal(got, R.scan_oracle(x, scan, pname, gamma, lam), (route, n, T, scan, pname, gamma, lam))


@pytest.mark.parametrize("i", R.SCAN_SUB, ids=[R.SCAN_CASES[i][0] for i in R.SCAN_SUB])
def test_scan_nonfinite_inputs_stay_in_their_env(L, i):
    """A NaN reward at t = T - 1 and a +inf value at t = 0 in an env in the middle of a tile and one at a tile's edge:
    every other env keeps the bits of the clean run, the two envs equal the oracle with NaN in the same places."""
    route, n, T = R.SCAN_CASES[i]
    x = R.scan_inputs(n, T, "random", 3000 + i)
    envs = R.poisoned_envs(route, n)
    y = R.poison(x, envs)
    sub = dict(y, r=y["r"][envs], v=y["v"][envs], d=y["d"][envs], lv=y["lv"][envs])
    keep = np.ones(n, bool)
    keep[envs] = False
    clean_rig, rig = ScanRig(x), ScanRig(y)
    for scan in ("gae", "nstep"):
        for promo, pname in R.PROMOS:
            clean = clean_rig.run(L, scan, promo, 0.99, 0.95, route)
            got = rig.run(L, scan, promo, 0.99, 0.95, route)
            want = R.scan_oracle(sub, scan, pname, 0.99, 0.95)
            for k in range(2):
                assert R.same_bits(got[k][keep], clean[k][keep]), (route, scan, pname, "a neighbour changed")
                assert R.same_bits_nan(got[k][envs], want[k]), (route, scan, pname, "the poisoned envs")
                assert np.isnan(got[k][envs]).any()


def _dev_switches(L, force, groups):
    L.load().arl_dev_scan_force_wave(force)
    L.load().arl_dev_scan_wave_groups(groups)


ALIGN_N = 70
SHIFTS = [("r", 1), ("v", 1), ("lv", 1), ("o0", 1), ("o1", 1), ("d", 1)]


@pytest.mark.parametrize("T", [5, 36, 128])
def test_scan_alignment(L, T):
    """Each of rewards, values, last_values (must not matter), either output shifted by one float, and dones shifted by
    one byte with every float aligned -- the unaligned fallback from a horizon that would take the LDS tile, the chunked
    and (promo = 2) the wave kernel.  Exact promotions: the oracle's bits.  promo = 2 below T = 96 is the exact LEGACY
    walk; at T = 128 it stays within the bar and gives the bits of the aligned promo = 2 run of the same data (the
    unaligned launch takes 2 steps per lane with scalar accesses where the aligned one takes 4 with vector accesses:
    the float64 maps are composed in another grouping, and on these inputs every float32 result still rounds alike)."""
    _dev_switches(L, 0, 0)
    x = R.scan_inputs(ALIGN_N, T, "random", 4000 + T)
    aligned = {}
    for scan in ("gae", "nstep"):
        aligned[scan] = ScanRig(x).run(L, scan, 2, 0.99, 0.95, "aligned")
    for name, shift in SHIFTS:
        rig = ScanRig(x, {name: shift})
        for scan in ("gae", "nstep"):
            for promo, pname in R.PROMOS:
                got = rig.run(L, scan, promo, 0.99, 0.95, (name, T))
                _bit_equal(got, R.scan_oracle(x, scan, pname, 0.99, 0.95), (name, T, scan, pname))
            got = rig.run(L, scan, 2, 0.99, 0.95, (name, T))
            legacy = R.scan_oracle(x, scan, "legacy", 0.99, 0.95)
            if T < 96:
                _bit_equal(got, legacy, (name, T, scan, "promo 2 = legacy"))
            else:
                for k in range(2):
                    assert R.within_wave_bar(got[k], legacy[k]), (name, T, scan, np.abs(got[k] - legacy[k]).max())
                _bit_equal(got, aligned[scan], (name, T, scan, "promo 2: shifted against aligned"))


def test_scan_tolerance_mode_default_rules(L):
    """promo = 2 without the test overrides: below T = 96 and above 512 it is the exact LEGACY walk (bit for bit); at
    T = 96 it is the wave scan, within the bar."""
    _dev_switches(L, 0, 0)
    try:
        for T in (5, 95, 513, 1000, 96):
            x = R.scan_inputs(ALIGN_N, T, "random", 5000 + T)
            rig = ScanRig(x)
            for scan in ("gae", "nstep"):
                got = rig.run(L, scan, 2, 0.99, 0.95, T)
                legacy = R.scan_oracle(x, scan, "legacy", 0.99, 0.95)
                if T != 96:
                    _bit_equal(got, legacy, (T, scan, "promo 2 = legacy"))
                else:
                    for k in range(2):
                        assert R.within_wave_bar(got[k], legacy[k]), (T, scan, np.abs(got[k] - legacy[k]).max())
    finally:
        _dev_switches(L, 0, 0)


@pytest.mark.parametrize("n,T", [(16400, 128), (8200, 512)])
def test_scan_wave_groups_chosen_by_size(L, n, T):
    """8200 segment groups: the size rule picks two groups per wave at T = 128 and, for eight steps per lane (T = 512),
    one.  Same bits as the same data with one group per wave forced; within the bar of the LEGACY oracle."""
    x = R.scan_inputs(n, T, "random", 6000 + T)
    rig = ScanRig(x)
    _dev_switches(L, 0, 0)
    try:
        for scan in ("gae", "nstep"):
            got = rig.run(L, scan, 2, 0.99, 0.95, (n, T))
            L.load().arl_dev_scan_wave_groups(1)
            one = rig.run(L, scan, 2, 0.99, 0.95, (n, T, "one group"))
            L.load().arl_dev_scan_wave_groups(0)
            _bit_equal(got, one, (n, T, scan))
            legacy = R.scan_oracle(x, scan, "legacy", 0.99, 0.95)
            for k in range(2):
                assert R.within_wave_bar(got[k], legacy[k]), (n, T, scan, np.abs(got[k] - legacy[k]).max())
    finally:
        _dev_switches(L, 0, 0)


def test_scan_refusals(L):
    """Each null pointer, n_env < 0, T = 0, promo = 3: ARL_E_ARG; n_env * T > 2^40: ARL_E_RANGE; n_env = 0: 0.  Nothing
    is written in any of them."""
    lib = L.load()
    x = R.scan_inputs(70, 5, "random", 7)
    rig = ScanRig(x)
    s = _stream(L)

    def gae(r=rig.r.ptr, v=rig.v.ptr, d=rig.d.ptr, lv=rig.lv.ptr, n=70, T=5, promo=0, o0=rig.o0.ptr, o1=rig.o1.ptr):
        return lib.arl_gae_scan(r, v, d, lv, 0.99, 0.95, n, T, promo, o0, o1, s)

    def nstep(r=rig.r.ptr, v=rig.v.ptr, d=rig.d.ptr, lv=rig.lv.ptr, n=70, T=5, promo=0, o0=rig.o0.ptr, o1=rig.o1.ptr):
        return lib.arl_nstep_return(r, d, v, lv, 0.99, n, T, promo, o0, o1, s)

    for fn in (gae, nstep):
        for name in ("r", "v", "d", "lv", "o0", "o1"):
            assert fn(**{name: None}) == E_ARG, name
        assert fn(n=-1) == E_ARG and fn(T=0) == E_ARG and fn(T=-5) == E_ARG and fn(promo=3) == E_ARG and fn(promo=-1) == E_ARG
        assert fn(n=(1 << 40) + 1, T=1) == E_RANGE and fn(n=(1 << 38) + 1, T=4) == E_RANGE
        assert fn(n=0) == 0
        _sync()
        rig.o0.untouched(fn.__name__)
        rig.o1.untouched(fn.__name__)


# ====================================================================================================== valids

def _valids_call(L, flags, n, T, valids, a, r, v):
    return L.load().arl_valids_mask(flags, n, T, valids, a, r, v, _stream(L))


@pytest.mark.parametrize("n", R.VALIDS_N)
@pytest.mark.parametrize("T", R.VALIDS_T)
def test_valids_mask(L, n, T):
    """Flag patterns none / every t = 0 / only t = T - 1 / random with flag bytes 1 and 255; each of advantages, returns
    and values null on its own, and all three; what lies past the reset holds NaN and +-inf and comes out as +0."""
    base = R.valids_base(n, T, n + T)
    for pi, pattern in enumerate(R.FLAG_PATTERNS):
        f = R.reset_flags(n, T, pattern, 11 * n + T + pi)
        valids = P.valid_mask(f)
        payload = R.valids_payload(base, valids)
        want = P.zero_invalid(valids, *payload)
        for w, p in zip(want, payload):
            assert R.same_bits(w[valids == 0], np.zeros(int((valids == 0).sum()), F32)) and R.same_bits(w[valids != 0], p[valids != 0])
        fl = _input(f)
        for nulls in ((), (0,), (1,), (2,), (0, 1, 2)):
            out = Guarded(n * T, torch.int8)
            arrs = [Guarded(n * T, init=p) for p in payload]
            ptrs = [None if k in nulls else arrs[k].ptr for k in range(3)]
            assert _valids_call(L, fl.ptr, n, T, out.ptr, *ptrs) == 0
            _sync()
            out.check((pattern, nulls))
            assert (out.read().reshape(n, T) == valids).all(), (pattern, nulls)
            for k in range(3):
                arrs[k].check((pattern, nulls, k))
                assert R.same_bits(arrs[k].read().reshape(n, T), payload[k] if k in nulls else want[k]), (pattern, nulls, k)


def test_valids_refusals(L):
    f = _input(R.reset_flags(9, 5, "random", 1))
    out, a = Guarded(45, torch.int8), Guarded(45)
    assert _valids_call(L, None, 9, 5, out.ptr, a.ptr, None, None) == E_ARG
    assert _valids_call(L, f.ptr, 9, 5, None, a.ptr, None, None) == E_ARG
    assert _valids_call(L, f.ptr, 9, 0, out.ptr, a.ptr, None, None) == E_ARG
    assert _valids_call(L, f.ptr, -1, 5, out.ptr, a.ptr, None, None) == E_ARG
    assert _valids_call(L, f.ptr, 0, 5, out.ptr, a.ptr, None, None) == 0
    _sync()
    out.untouched()
    a.untouched()


# ================================================================================================== standardise

def _standardize(L, x, valids, eps, what):
    """Two calls from the same input with a NaN-filled workspace -> the result (equal bits both times)."""
    lib = L.load()
    ws = Guarded(R.STD_BLOCKS * 3, torch.float64)
    v = _input(valids) if valids is not None else None
    outs = []
    for _ in range(2):
        ws.t.fill_(float("nan"))
        xt = Guarded(x.size, init=x)
        rc = lib.arl_standardize(xt.ptr, v.ptr if v else None, x.size, eps, ws.ptr, _stream(L))
        assert rc == 0, (what, rc)
        _sync()
        xt.check(what)
        ws.check(what)
        outs.append(xt.read())
    assert R.same_bits_nan(outs[0], outs[1]), (what, "second run differs")
    slots = min((x.size + 255) // 256, R.STD_BLOCKS)
    assert np.isnan(ws.read()[3 * slots:]).all(), (what, "a partial slot beyond the grid was written")
    return outs[0]


@pytest.mark.parametrize("n", R.STD_N)
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_standardize_within_the_derived_bound(L, n, masked):
    """N(mu, sigma) with mu / sigma = 0, 1e2, 1e4, 1e6, eps = 1e-6 and 0.5, valids bytes 0, 1, 2, 127, -1: inside
    batch_ref.standardize_bound of the float64 two-pass reference; invalid elements keep their bits."""
    for eps, ratio, x, valids in R.std_cases(n, masked):
        what = (n, masked, eps, ratio)
        got = _standardize(L, x, valids, eps, what)
        sel, y, m, var, d = R.std_reference(x, valids, eps)
        assert R.same_bits(got[~sel], x[~sel]), what
        if var == 0:
            assert R.same_bits(got[sel], np.zeros(int(sel.sum()), F32)), what
            continue
        frac = float((np.abs(got[sel].astype(F64) - y) / R.standardize_bound(y, m, var, d, n)).max())
        print("standardise n=%d masked=%d eps=%g mu/sigma=%g: %.3f of the bound" % (n, masked, eps, ratio, frac))
        STD["frac"] = max(STD["frac"], frac)
        assert frac <= 1.0, (what, frac)
        STD["tried"] += 1
        den = R.std_recover_denominator(x[sel], got[sel], m)
        if den is not None:
            rel = abs((float(den) - float(F32(eps))) - np.sqrt(var)) / np.sqrt(var)
            print("    sqrt(var) from the outputs: relative error %.3g" % rel)
            STD["recovered"] += 1
            STD["sqrt"][ratio] = max(STD["sqrt"].get(ratio, 0.0), rel)


@pytest.mark.parametrize("n", [257, 131073])
def test_standardize_edge_cases(L, n):
    rs = np.random.RandomState(n)
    x = (rs.randn(n) * 3 + 1.5).astype(F32)
    some = np.where(rs.rand(n) < 0.6, R.VALID_BYTES[rs.randint(0, 4, n)], 0).astype(np.int8)
    some[:2] = (1, 0)
    # all invalid: nothing changes
    assert R.same_bits(_standardize(L, x, np.zeros(n, np.int8), 1e-6, "all invalid"), x)
    # exactly one valid (the last element; then one in the middle): that element becomes +0
    for at in (n - 1, n // 2):
        one = np.zeros(n, np.int8)
        one[at] = -1
        want = x.copy()
        want[at] = 0
        assert R.same_bits(_standardize(L, x, one, 1e-6, "one valid"), want)
    # a constant array: all +0, masked too
    c = np.full(n, F32(3.7), F32)
    assert R.same_bits(_standardize(L, c, None, 1e-6, "constant"), np.zeros(n, F32))
    assert R.same_bits(_standardize(L, c, some, 0.5, "constant"), np.where(some != 0, F32(0), c).astype(F32))
    # a NaN in an invalid slot changes nothing
    clean = _standardize(L, x, some, 1e-6, "clean")
    bad = x.copy()
    bad[1] = np.nan
    got = _standardize(L, bad, some, 1e-6, "NaN outside the mask")
    assert np.isnan(got[1]) and R.same_bits(np.delete(got, 1), np.delete(clean, 1))
    # a NaN in a valid slot: every valid output NaN, no invalid one
    bad = x.copy()
    bad[0] = np.nan
    got = _standardize(L, bad, some, 1e-6, "NaN inside the mask")
    assert np.isnan(got[some != 0]).all() and R.same_bits(got[some == 0], x[some == 0])


def test_standardize_refusals(L):
    lib = L.load()
    x, ws = Guarded(64), Guarded(R.STD_BLOCKS * 3, torch.float64)
    assert lib.arl_standardize_workspace_bytes() == R.STD_BLOCKS * 24
    assert lib.arl_standardize(None, None, 64, 1e-6, ws.ptr, _stream(L)) == E_ARG
    assert lib.arl_standardize(x.ptr, None, 64, 1e-6, None, _stream(L)) == E_ARG
    assert lib.arl_standardize(x.ptr, None, -1, 1e-6, ws.ptr, _stream(L)) == E_ARG
    assert lib.arl_standardize(x.ptr, None, 0, 1e-6, ws.ptr, _stream(L)) == 0
    _sync()
    x.untouched()
    ws.untouched()


# ===================================================================================================== sampling

def _sample(L, p, u, what):
    B, A = p.shape
    act, pd, ud = Guarded(B, torch.uint8), _input(p), _input(u)
    rc = L.load().arl_sample_categorical(pd.ptr, ud.ptr, B, A, act.ptr, _stream(L))
    assert rc == 0, (what, rc)
    _sync()
    act.check(what)
    return act.read()


@pytest.mark.parametrize("A", R.SAMPLE_A)
@pytest.mark.parametrize("B", R.SAMPLE_B)
def test_sampling_on_exact_ties(L, A, B):
    """Probabilities that are multiples of 2^-10 (the float32 running sum is exact); u exactly a cumulative sum, one
    ulp below and one above, at the first, a middle and the last action; u = 0 and u = 1."""
    for shift in range(R.N_U_KINDS if B == 1 else 1):
        p, u = R.sample_inputs(A, B, shift)
        got = _sample(L, p, u, (A, B, shift))
        want = P.sample_actions(p, u)
        assert got.dtype == want.dtype and (got == want).all(), (A, B, shift, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("A", R.SAMPLE_A)
def test_sampling_rows_that_do_not_sum_to_one(L, A):
    p, u = R.sample_edge_rows(A)
    got = _sample(L, p, u, A)
    assert (got == P.sample_actions(p, u)).all(), (A, got)


def test_sampling_refusals(L):
    lib = L.load()
    p, u = R.sample_inputs(4, 8)
    pd, ud, act = _input(p), _input(u), Guarded(8, torch.uint8)
    s = _stream(L)
    assert lib.arl_sample_categorical(pd.ptr, ud.ptr, 8, 0, act.ptr, s) == E_ARG
    assert lib.arl_sample_categorical(pd.ptr, ud.ptr, 8, 257, act.ptr, s) == E_RANGE
    assert lib.arl_sample_categorical(pd.ptr, ud.ptr, -1, 4, act.ptr, s) == E_ARG
    assert lib.arl_sample_categorical(None, ud.ptr, 8, 4, act.ptr, s) == E_ARG
    assert lib.arl_sample_categorical(pd.ptr, None, 8, 4, act.ptr, s) == E_ARG
    assert lib.arl_sample_categorical(pd.ptr, ud.ptr, 8, 4, None, s) == E_ARG
    assert lib.arl_sample_categorical(pd.ptr, ud.ptr, 0, 4, act.ptr, s) == 0
    _sync()
    act.untouched()


# ====================================================================================================== gathers

@pytest.mark.parametrize("row_bytes", R.GATHER_ROW_BYTES)
@pytest.mark.parametrize("batch", R.GATHER_BATCH)
def test_gather_scale_obs(L, row_bytes, batch):
    lib = L.load()
    n_rows = max(batch + 2, 256 // row_bytes + 1)            # every byte value 0 .. 255 is in there
    obs = R.gather_obs(n_rows, row_bytes, row_bytes + batch)
    od = _input(obs)
    for form in R.IDX_FORMS:
        idx = R.gather_idx(form, batch, n_rows, batch)
        idd = _input(idx) if idx is not None else None
        for scale in R.GATHER_SCALES:
            out = Guarded(batch * row_bytes)
            rc = lib.arl_gather_scale_obs(od.ptr, idd.ptr if idd else None, batch, row_bytes, scale, out.ptr, _stream(L))
            assert rc == 0
            _sync()
            out.check((form, scale))
            assert R.same_bits(out.read().reshape(batch, row_bytes), R.gather_ref(obs, idx, batch, scale)), (form, scale)


def test_gather_scale_obs_refusals(L):
    lib = L.load()
    obs = R.gather_obs(4, 64, 1)
    s = _stream(L)
    od, out = _input(obs), Guarded(4 * 64)
    od4, out1 = _input(obs, shift=4), Guarded(4 * 64, shift=1)
    assert lib.arl_gather_scale_obs(od.ptr, None, 4, 24, 1.0, out.ptr, s) == E_RANGE
    assert lib.arl_gather_scale_obs(od4.ptr, None, 4, 64, 1.0, out.ptr, s) == E_ALIGN
    assert lib.arl_gather_scale_obs(od.ptr, None, 4, 64, 1.0, out1.ptr, s) == E_ALIGN
    assert lib.arl_gather_scale_obs(None, None, 4, 64, 1.0, out.ptr, s) == E_ARG
    assert lib.arl_gather_scale_obs(od.ptr, None, 4, 64, 1.0, None, s) == E_ARG
    assert lib.arl_gather_scale_obs(od.ptr, None, -1, 64, 1.0, out.ptr, s) == E_ARG
    assert lib.arl_gather_scale_obs(od.ptr, None, 4, 0, 1.0, out.ptr, s) == E_ARG
    assert lib.arl_gather_scale_obs(od.ptr, None, 0, 64, 1.0, out.ptr, s) == 0
    _sync()
    out.untouched()
    out1.untouched()


@pytest.mark.parametrize("plane", R.NHWC_PLANE_BYTES)
@pytest.mark.parametrize("batch", R.NHWC_BATCH)
def test_gather_scale_obs_nhwc(L, plane, batch):
    """4, 12, 20, 60, 2080 and 10400 live lanes: one quad, a partly filled wave, a partly filled block.  obs aligned and
    4 bytes past a 16-byte boundary (accepted: the kernel reads 4-byte words)."""
    lib = L.load()
    n_rows = batch + 2
    obs = R.gather_obs(n_rows, 4 * plane, plane + batch)
    obs4 = obs.reshape(n_rows, 4, plane)
    for obs_shift in (0, 4):
        od = _input(obs, shift=obs_shift)
        for form in R.IDX_FORMS:
            idx = R.gather_idx(form, batch, n_rows, batch)
            idd = _input(idx) if idx is not None else None
            for scale in R.GATHER_SCALES:
                out = Guarded(batch * 4 * plane)
                rc = lib.arl_gather_scale_obs_nhwc(od.ptr, idd.ptr if idd else None, batch, 4, plane, scale, out.ptr, _stream(L))
                assert rc == 0, (obs_shift, form, scale, rc)
                _sync()
                out.check((form, scale))
                want = R.gather_nhwc_ref(obs4, idx, batch, scale)
                assert R.same_bits(out.read().reshape(batch, plane, 4), want), (obs_shift, form, scale)


def test_gather_scale_obs_nhwc_refusals(L):
    lib = L.load()
    obs = R.gather_obs(3, 4 * 48, 1)
    s = _stream(L)
    od, od1, out, out1 = _input(obs), _input(obs, shift=1), Guarded(3 * 4 * 48), Guarded(3 * 4 * 48, shift=1)
    for ch in (1, 3, 5, 8):
        assert lib.arl_gather_scale_obs_nhwc(od.ptr, None, 3, ch, 48, 1.0, out.ptr, s) == E_RANGE
    assert lib.arl_gather_scale_obs_nhwc(od.ptr, None, 3, 4, 24, 1.0, out.ptr, s) == E_RANGE
    assert lib.arl_gather_scale_obs_nhwc(od1.ptr, None, 3, 4, 48, 1.0, out.ptr, s) == E_ALIGN
    assert lib.arl_gather_scale_obs_nhwc(od.ptr, None, 3, 4, 48, 1.0, out1.ptr, s) == E_ALIGN
    assert lib.arl_gather_scale_obs_nhwc(None, None, 3, 4, 48, 1.0, out.ptr, s) == E_ARG
    assert lib.arl_gather_scale_obs_nhwc(od.ptr, None, 3, 4, 48, 1.0, None, s) == E_ARG
    assert lib.arl_gather_scale_obs_nhwc(od.ptr, None, 0, 4, 48, 1.0, out.ptr, s) == 0
    _sync()
    out.untouched()
    out1.untouched()


# ============================================================================================ bias + ReLU, backward

@pytest.mark.parametrize("channels", R.RELU_CHANNELS)
@pytest.mark.parametrize("rows", R.RELU_ROWS)
def test_bias_relu_and_backward_bit_for_bit(L, rows, channels):
    """channels 12 and 1020 leave thread 255 without a row lane; 21761 rows at 12 channels and 300 at 1024 pass the
    256-workgroup cap.  y and the masked dy equal NumPy's bits (x + b == 0, -0.0, y == 0 under a non-zero dy, a NaN dy
    under the mask: selected away, not multiplied); dbias equals the restated order of additions; twice, same bits."""
    lib = L.load()
    x, b, dy = R.relu_inputs(rows, channels, 100 + rows)
    y_want = R.relu_fwd_ref(x, b)
    g_want = R.relu_bwd_ref(dy, y_want)
    db_want = R.dbias_restatement(g_want)
    bd, s = _input(b), _stream(L)
    ws = Guarded(R.RELU_BLOCK_CAP * 1024)
    assert lib.arl_relu_bwd_workspace_bytes() == 4 * R.RELU_BLOCK_CAP * 1024
    for run in range(2):
        xd = Guarded(rows * channels, init=x)
        assert lib.arl_bias_relu(xd.ptr, bd.ptr, rows, channels, s) == 0
        _sync()
        xd.check("bias_relu")
        y = xd.read().reshape(rows, channels)
        assert R.same_bits(y, y_want), (run, int((R.bits(y) != R.bits(y_want)).sum()))
        dyd, db = Guarded(rows * channels, init=dy), Guarded(channels)
        ws.t.fill_(float("nan"))
        assert lib.arl_relu_bwd_bias_grad(dyd.ptr, xd.ptr, rows, channels, db.ptr, ws.ptr, s) == 0
        _sync()
        for t in (dyd, db, ws, xd):
            t.check("relu_bwd_bias_grad")
        assert R.same_bits(xd.read().reshape(rows, channels), y_want), "y was written"
        assert R.same_bits(dyd.read().reshape(rows, channels), g_want), run
        got = db.read()
        exact = g_want.astype(F64).sum(axis=0)
        assert np.abs(got - exact).max() <= 64 * R.U32 * np.abs(g_want).astype(F64).sum(axis=0).max(), "not the column sum"
        assert R.same_bits(got, db_want), (run, int((R.bits(got) != R.bits(db_want)).sum()), np.abs(got - db_want).max())
        grid, _ = R.relu_grid(rows, channels)
        assert np.isnan(ws.read()[grid * channels:]).all(), "partials beyond the grid were written"


def test_bias_relu_refusals(L):
    lib = L.load()
    s = _stream(L)
    x, x1, b, b1 = Guarded(8 * 1032), Guarded(8 * 1032, shift=1), Guarded(1032), Guarded(1032, shift=1)
    dy, db, ws, ws1 = Guarded(8 * 1032), Guarded(1032), Guarded(256 * 1024), Guarded(256 * 1024, shift=1)
    assert lib.arl_bias_relu(x.ptr, b.ptr, 8, 6, s) == E_RANGE
    assert lib.arl_bias_relu(x.ptr, b.ptr, 8, 0, s) == E_RANGE
    assert lib.arl_bias_relu(x.ptr, b.ptr, -1, 8, s) == E_RANGE
    assert lib.arl_bias_relu(x1.ptr, b.ptr, 8, 8, s) == E_ALIGN
    assert lib.arl_bias_relu(x.ptr, b1.ptr, 8, 8, s) == E_ALIGN
    assert lib.arl_bias_relu(None, b.ptr, 8, 8, s) == E_ARG and lib.arl_bias_relu(x.ptr, None, 8, 8, s) == E_ARG
    assert lib.arl_bias_relu(x.ptr, b.ptr, 0, 8, s) == 0                      # no rows: a no-op

    def bwd(dy_=dy.ptr, y_=x.ptr, rows=8, ch=8, db_=db.ptr, ws_=ws.ptr):
        return lib.arl_relu_bwd_bias_grad(dy_, y_, rows, ch, db_, ws_, s)
    assert bwd(ch=6) == E_RANGE and bwd(ch=1028) == E_RANGE and bwd(ch=0) == E_RANGE
    assert bwd(rows=0) == E_RANGE and bwd(rows=-1) == E_RANGE
    assert bwd(dy_=x1.ptr) == E_ALIGN and bwd(y_=x1.ptr) == E_ALIGN and bwd(ws_=ws1.ptr) == E_ALIGN
    for k in ("dy_", "y_", "db_", "ws_"):
        assert bwd(**{k: None}) == E_ARG, k
    _sync()
    for t in (x, x1, b, b1, dy, db, ws, ws1):
        t.untouched()
