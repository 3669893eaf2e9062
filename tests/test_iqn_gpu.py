"""Implicit quantile networks on the device (csrc/iqn.hip: arl_iqn_embed / _merge_fwd / _merge_bwd / _act / _loss,
AtariIqnPolicy, ImplicitQuantileDQN).  The reference has no IQN, so the yardsticks are restatements of the formulas of
include/accel_rl_hip.h ("Implicit quantile networks"): a NumPy Philox4x32-10 for the generator, float64 cosines from
the exact integers, and `ref_iqn_loss` below (float64; gradient from autograd where kappa > 0, from the closed form
where kappa == 0).

Tolerances.  Cosine features: atol 2^-22 = 4 ulp at magnitude 1, the OpenCL full-profile bound of cospi / sinpi that
the device library is held to (the argument is reduced in integers, so nothing else rounds).  loss_rows and priorities:
rtol 2e-4 (the C51 / QR-DQN bar).  Gradient: rtol 2e-4 plus atol = (N' + 8) * 2^-24 * (1 + max|T| / kappa) * max_b w_b
-- the rounding of an N'-term fp32 sum of terms bounded by w_b / N' (the kernel's chains are N' / 4 + 3 additions
long) plus the rounding of T passed through the clip's slope 1 / kappa; on quantised inputs (every u exact) the second
part is absent.  Merge: bit-exact (products and sums of quantised inputs are exact in fp32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
POISON = 1e9                    # what the padding columns of every input hold: they must be ignored
STREAM = 0xC9514E31             # ARL_IQN_PHILOX_STREAM
MASK = np.uint64(0xFFFFFFFF)


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- generator ----------------------------------------------------------------------------------------------------

def philox4x32_10(ctr, k0, k1):
    """ctr uint64[n][4] holding 32-bit words -> uint64[n][4] (Salmon et al. 2011, ten rounds)."""
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    c = [ctr[:, j].astype(np.uint64) for j in range(4)]
    for i in range(10):
        if i > 0:
            k0, k1 = (k0 + w0) & 0xFFFFFFFF, (k1 + w1) & 0xFFFFFFFF
        p0, p1 = m0 * c[0], m1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return np.stack(c, axis=1)


def ref_tau(seed, call, e):
    """The drawn fraction of global pair index e (int array) in call `call`: float32, exact."""
    e = np.asarray(e, np.uint64)
    call &= 2 ** 64 - 1
    ctr = np.stack([e >> np.uint64(2), np.zeros_like(e), np.full_like(e, call & 0xFFFFFFFF), np.full_like(e, call >> 32)], axis=1)
    words = philox4x32_10(ctr, seed & 0xFFFFFFFF, STREAM)
    k = words[np.arange(e.size), (e & np.uint64(3)).astype(np.int64)] >> np.uint64(9)
    return ((2 * k.astype(np.int64) + 1) * EPS).astype(np.float32)


def _embed(rows, r, tau_in=None, state=None, row0=0, call_offset=0):
    from accel_rl_amd import _lib
    tau = torch.full((rows * r,), float("nan"), device=DEV)
    cosf = torch.full((rows * r, 64), float("nan"), device=DEV)
    _lib.iqn_embed(_dev(tau_in), state, rows, r, tau, cosf, row0=row0, call_offset=call_offset)
    torch.cuda.synchronize()
    return tau.cpu().numpy(), cosf.cpu().numpy()


def _ref_cos(tau):
    """float64 cos(pi i tau) from exact integers: i tau is exact in float64 (6 + 24 bits), so is its remainder mod 2."""
    t = np.fmod(np.arange(64, dtype=np.float64)[None, :] * tau.astype(np.float64)[:, None], 2.0)
    return np.cos(np.pi * t)


@pytest.mark.parametrize("rows,r", [(1, 1), (1, 3), (2, 2), (5, 1), (1, 64), (257, 1)])
def test_drawn_fractions_equal_the_numpy_philox_bit_for_bit(rows, r):
    seed, counter = 0x1234567 + 2 ** 33, 2 ** 32 + 5               # (the key takes the seed's low word; a 64-bit call counter)
    state = torch.tensor([seed, counter], dtype=torch.int64, device=DEV)
    tau, cosf = _embed(rows, r, state=state)
    want = ref_tau(seed, counter, np.arange(rows * r))
    np.testing.assert_array_equal(tau, want)
    k2 = tau.astype(np.float64) * 2 ** 24                           # every tau is (2k + 1) 2^-24: never 0 or 1
    assert (k2 == np.round(k2)).all() and (k2.astype(np.int64) % 2 == 1).all() and (k2 > 0).all() and (k2 < 2 ** 24).all()
    assert np.abs(cosf - _ref_cos(tau)).max() <= 2.0 ** -22
    assert state.cpu().tolist() == [seed, counter]                  # the kernel only reads the state


def test_row0_and_call_offset_address_slices_of_one_stream():
    seed, counter, rows, r = 77, 9, 40, 5
    state = torch.tensor([seed, counter], dtype=torch.int64, device=DEV)
    big, big_cos = _embed(rows, r, state=state)
    part, part_cos = _embed(7, r, state=state, row0=13)
    np.testing.assert_array_equal(part, big[13 * r:20 * r])
    np.testing.assert_array_equal(part_cos, big_cos[13 * r:20 * r])
    later = torch.tensor([seed, counter + 2], dtype=torch.int64, device=DEV)
    np.testing.assert_array_equal(_embed(rows, r, state=state, call_offset=2)[0], _embed(rows, r, state=later)[0])
    np.testing.assert_array_equal(_embed(rows, r, state=later, call_offset=-2)[0], big)
    np.testing.assert_array_equal(_embed(rows, r, state=state, call_offset=2)[0], ref_tau(seed, counter + 2, np.arange(rows * r)))
    assert not np.array_equal(_embed(rows, r, state=later)[0], big)


def test_cosine_features_against_float64():
    state = torch.tensor([5, 0], dtype=torch.int64, device=DEV)
    drawn, drawn_cos = _embed(64, 8, state=state)
    assert np.abs(drawn_cos - _ref_cos(drawn)).max() <= 2.0 ** -22
    given = np.array([2.0 ** -24, 1 - 2.0 ** -24, 0.5, 0.25, 1. / 3, 0.75], np.float32)
    tau, cosf = _embed(2, 3, tau_in=given)
    np.testing.assert_array_equal(tau, given)                       # given mode copies tau
    err = np.abs(cosf - _ref_cos(given))
    print("max cosine error: drawn %.3g, given %.3g (bound %.3g)" % (np.abs(drawn_cos - _ref_cos(drawn)).max(), err.max(),
                                                                     2.0 ** -22))
    assert err.max() <= 2.0 ** -22
    assert (cosf[:, 0] == 1.).all() and (drawn_cos[:, 0] == 1.).all()               # i = 0: exactly 1
    assert (cosf[2, 1::2] == 0.).all()                                              # tau = 0.5: exact zeros at odd i
    np.testing.assert_array_equal(cosf[2, 0::2], np.where(np.arange(32) % 2 == 0, 1., -1.).astype(np.float32))
    np.testing.assert_array_equal(cosf[3, 2::4], np.zeros(16, np.float32))          # tau = 0.25: i = 2, 6, 10, ...


# ---- merge --------------------------------------------------------------------------------------------------------

MERGE_SHAPES = [(1, 1, 4), (3, 5, 12), (2, 64, 3136)]


def _merge_case(b, r, f, seed=0):
    """Quantised inputs: psi, phi multiples of 1/8 in [0, 4) (zeros planted: both masks), g multiples of 1/8 in [-4, 4]:
    every product is a multiple of 1/64 below 16 and every sum of at most 64 of them is exact in fp32."""
    rs = np.random.RandomState(seed + b + r + f)
    psi = (rs.randint(0, 32, size=(b, f)) / 8.).astype(np.float32)
    phi = (rs.randint(0, 32, size=(b * r, f)) / 8.).astype(np.float32)
    psi[rs.rand(b, f) < 0.3] = 0.
    phi[rs.rand(b * r, f) < 0.3] = 0.
    psi.flat[0], phi.flat[-1] = 0., 0.
    g = (rs.randint(-32, 33, size=(b * r, f)) / 8.).astype(np.float32)
    return psi, phi, g


def _merge_bwd(psi, phi, g, b, r, f):
    from accel_rl_amd import _lib
    dphi = torch.full((b * r, f), float("nan"), device=DEV)
    dpsi = torch.full((b, f), float("nan"), device=DEV)
    _lib.iqn_merge_bwd(_dev(g), _dev(psi), _dev(phi), b, r, f, dphi, dpsi)
    torch.cuda.synchronize()
    return dphi.cpu().numpy(), dpsi.cpu().numpy()


@pytest.mark.parametrize("b,r,f", MERGE_SHAPES)
def test_merge_forward_and_backward_are_bit_exact(b, r, f):
    from accel_rl_amd import _lib
    rs = np.random.RandomState(b * r + f)
    psi = np.maximum(rs.randn(b, f), 0).astype(np.float32)
    phi = np.maximum(rs.randn(b * r, f), 0).astype(np.float32)
    x = torch.full((b * r, f), float("nan"), device=DEV)
    _lib.iqn_merge_fwd(_dev(psi), _dev(phi), b, r, f, x)
    np.testing.assert_array_equal(x.cpu().numpy(), np.repeat(psi, r, axis=0) * phi)
    psi, phi, g = _merge_case(b, r, f)
    dphi, dpsi = _merge_bwd(psi, phi, g, b, r, f)
    p64, h64, g64 = np.repeat(psi, r, axis=0).astype(np.float64), phi.astype(np.float64), g.astype(np.float64)
    want_dphi = np.where(h64 > 0, g64 * p64, 0.)
    want_dpsi = np.where(psi > 0, (g64 * h64).reshape(b, r, f).sum(axis=1), 0.)
    assert (want_dphi[h64 == 0] == 0).all() and (p64 == 0).any() and (h64 == 0).any()
    np.testing.assert_array_equal(dphi.astype(np.float64), want_dphi)
    np.testing.assert_array_equal(dpsi.astype(np.float64), want_dpsi)


# ---- loss ---------------------------------------------------------------------------------------------------------

def ref_iqn_loss(pred, tau, tgt, pol, act, ret, term, isw, gamma_n, kappa):
    """float64.  pred [B][N][A] at fractions tau [B][N]; tgt / pol [B][N'][A] (pol None: not double DQN); pred may be
    part of an autograd graph.  Returns a dict: rows (w_b loss_b, differentiable), loss_b, dth (closed-form
    d sum(rows) / d pred(i, action), the kernel's formula), T, u, a_next, margin, w."""
    assert pred.dtype == torch.float64 and tau.dtype == torch.float64
    b, n, n_act = pred.shape
    m = tgt.shape[1]
    ar = torch.arange(b)
    q = (pol if pol is not None else tgt).sum(dim=1) / m
    a_next = q.argmax(dim=1)
    margin = float("inf")
    if n_act > 1:
        top2 = torch.topk(q, 2, dim=1).values
        margin = (top2[:, 0] - top2[:, 1]).min().item()
    keep = 1. - term.double()
    T = ret.double()[:, None] + keep[:, None] * (gamma_n * tgt[ar, :, a_next])          # [B][j]
    th = pred[ar, :, act.long()]                                                        # [B][i]
    u = T[:, None, :] - th[:, :, None]                                                  # [B][i][j]
    ind = (u < 0).double()                                                              # u == 0: not negative
    wt = (tau[:, :, None] - ind).abs().detach()
    if kappa > 0:
        au = u.abs()
        rho = wt * torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa
        dth = -(wt * u.clamp(-kappa, kappa) / kappa).sum(dim=2)
    else:
        rho = wt * u.abs()
        dth = -(tau[:, :, None] - ind).sum(dim=2)
    loss_b = rho.sum(dim=(1, 2)) / m
    w = (isw.double() if isw is not None else torch.ones(b, dtype=torch.float64)) / b
    return dict(rows=w * loss_b, loss_b=loss_b.detach(), dth=(dth * (w / m)[:, None]).detach(), T=T.detach(),
                u=u.detach(), a_next=a_next, margin=margin, w=w)


def _block(rs, batch, r, n_act, stride, scale=2.):
    t = (rs.randn(batch, r, stride) * scale).astype(np.float32)
    t[:, :, n_act:] = POISON
    return t


def _selecting(rs, t, n_act):
    """Make the greedy action of block `t` [B][R][S] unambiguous (as tests/test_qrdqn_gpu.py:_selecting): every action
    column is centred over the fractions, given a mean in [-0.4, 0.4], and one randomly chosen action gets +1.0 at
    every fraction: the Q margin is at least 1 - 0.8 = 0.2."""
    batch = t.shape[0]
    t[:, :, :n_act] -= t[:, :, :n_act].mean(axis=1, keepdims=True)
    t[:, :, :n_act] += rs.uniform(-0.4, 0.4, size=(batch, 1, n_act)).astype(np.float32)
    chosen = rs.randint(0, n_act, size=batch)
    t[np.arange(batch), :, chosen] += np.float32(1.0)
    return chosen


def _case(seed, n_act, n, m, stride, batch, double, weighted):
    rs = np.random.RandomState(seed)
    pred, tgt = _block(rs, batch, n, n_act, stride), _block(rs, batch, m, n_act, stride)
    pol = _block(rs, batch, m, n_act, stride) if double else None
    chosen = _selecting(rs, pol if double else tgt, n_act)
    tau = ref_tau(seed, 0, np.arange(batch * n)).reshape(batch, n)
    act = rs.randint(0, n_act, size=batch).astype(np.uint8)
    ret = (rs.randn(batch) * 3).astype(np.float32)
    term = (rs.rand(batch) < 0.3).astype(np.uint8)
    if batch > 1:
        term[0], term[1] = 1, 0                     # terminal and non-terminal rows in every case
    isw = (rs.rand(batch) + 0.1).astype(np.float32) if weighted else None
    return dict(pred=pred, tau=tau, tgt=tgt, pol=pol, act=act, ret=ret, term=term, isw=isw, chosen=chosen)


def _launch(c, n_act, gamma_n, kappa, state=None, advance=0):
    from accel_rl_amd import _lib
    pred = _dev(c["pred"])
    batch, n, _ = pred.shape
    m = c["tgt"].shape[1]
    dth = torch.full_like(pred, float("nan"))
    rows = torch.full((batch,), float("nan"), device=DEV)
    pri = torch.full((batch,), float("nan"), device=DEV)
    _lib.iqn_loss(pred, _dev(c["tau"]), _dev(c["tgt"]), _dev(c["pol"]), _dev(c["act"]), _dev(c["ret"]), _dev(c["term"]),
                  _dev(c["isw"]), n_act, n, m, gamma_n, kappa, dth, rows, pri, state=state, advance=advance)
    torch.cuda.synchronize()
    return dth.cpu(), rows.cpu(), pri.cpu()


def _reference(c, n_act, gamma_n, kappa):
    f64 = lambda x: None if x is None else torch.from_numpy(x[:, :, :n_act].astype(np.float64))       # noqa: E731
    t = lambda x: None if x is None else torch.from_numpy(x)                                          # noqa: E731
    pred = f64(c["pred"]).requires_grad_()
    ref = ref_iqn_loss(pred, torch.from_numpy(c["tau"].astype(np.float64)), f64(c["tgt"]), f64(c["pol"]), t(c["act"]),
                       t(c["ret"]), t(c["term"]), t(c["isw"]), gamma_n, kappa)
    if kappa > 0:                                   # autograd; the closed form must agree with it
        ref["grad"], = torch.autograd.grad(ref["rows"].sum(), pred)
        ar = torch.arange(pred.shape[0])
        assert torch.allclose(ref["grad"][ar, :, t(c["act"]).long()], ref["dth"], rtol=1e-12, atol=1e-15)
    else:
        ref["grad"] = torch.zeros_like(pred)
        ref["grad"][torch.arange(pred.shape[0]), :, t(c["act"]).long()] = ref["dth"]
    ref["rows"] = ref["rows"].detach()
    return ref


def _check_against(ref, got, c, n_act, kappa_for_atol, exact_u=False, exact_grad=False):
    dth, rows, pri = got
    batch, n, _ = dth.shape
    m = c["tgt"].shape[1]
    assert ref["margin"] >= 0.2 - 1e-6, ref["margin"]                       # every sample: no sample is skipped
    np.testing.assert_array_equal(ref["a_next"].numpy(), c["chosen"])
    w_max = ref["w"].max().item()
    if exact_u:
        atol, rtol = (m + 8) * EPS * w_max, 0.
    else:
        atol, rtol = (m + 8) * EPS * (1 + ref["T"].abs().max().item() / kappa_for_atol) * w_max, 2e-4
    err = (dth[:, :, :n_act].double() - ref["grad"]).abs()
    print("margin %.3f  max|T| %.3f  atol %.3g  max grad err %.3g  max rel loss err %.3g" % (
        ref["margin"], ref["T"].abs().max().item(), atol, err.max().item(),
        ((rows.double() - ref["rows"]).abs() / ref["rows"].abs().clamp_min(1e-300)).max().item()))
    assert torch.isfinite(dth).all() and torch.isfinite(rows).all() and torch.isfinite(pri).all()
    np.testing.assert_allclose(rows.double().numpy(), ref["rows"].numpy(), rtol=2e-4, atol=0)
    np.testing.assert_allclose(pri.double().numpy(), ref["loss_b"].clamp(1e-6, 1e6).numpy(), rtol=2e-4, atol=0)
    if exact_grad:
        assert torch.equal(dth[:, :, :n_act].double(), ref["grad"])
    assert (err <= atol + rtol * ref["grad"].abs()).all(), err.max().item()
    other = torch.ones(dth.shape, dtype=torch.bool)                         # exact zeros outside the taken action's column
    other[torch.arange(batch), :, torch.from_numpy(c["act"]).long()] = False
    assert not dth[other].any()


LOSS_SHAPES = [(1, 1, 1, 4, 1), (2, 1, 3, 4, 3), (6, 8, 8, 8, 32), (18, 64, 64, 20, 5), (64, 5, 7, 64, 2)]   # A, N, N', stride, B


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
@pytest.mark.parametrize("kappa", [1.0, 0.25])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "A%d-N%d-M%d-S%d-B%d" % s)
def test_loss_priorities_and_gradient_vs_float64(shape, kappa, double, weighted):
    n_act, n, m, stride, batch = shape
    c = _case(100 * n_act + n + batch + 7 * int(double) + 3 * int(weighted), n_act, n, m, stride, batch, double, weighted)
    gamma_n = float(np.float32(0.99 ** 3))
    _check_against(_reference(c, n_act, gamma_n, kappa), _launch(c, n_act, gamma_n, kappa), c, n_act, kappa)


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic-tau", "drawn-tau"])
def test_plain_quantile_regression_and_the_tie_rule_on_quantised_inputs(dyadic):
    """gamma_n = 0.5, returns and target quantiles multiples of 1/4: every T_j is a multiple of 1/8; predicted quantiles
    multiples of 1/8 plus 1/16: every u is exact in fp32 and |u| >= 1/16.  Then some predicted quantiles of sample 1
    (not terminal) are set equal to some T_j: u == 0 counts as not negative.  Dyadic tau (multiples of 1/64), batch 4,
    N' = 8 and importance weights that are powers of two: every operation of the kappa == 0 gradient is exact, so it must
    equal the closed form bit for bit."""
    n_act, n, m, stride, batch = 4, 5, 8, 8, 4
    rs = np.random.RandomState(31 + int(dyadic))
    c = _case(17, n_act, n, m, stride, batch, True, True)                   # (the selecting net: pol, margin-built)
    c["tgt"][:, :, :n_act] = rs.randint(-32, 33, size=(batch, m, n_act)) / 4.
    c["ret"] = (rs.randint(-16, 17, size=batch) / 4.).astype(np.float32)
    c["pred"][:, :, :n_act] = rs.randint(-64, 64, size=(batch, n, n_act)) / 8. + 1. / 16
    if dyadic:
        c["tau"] = (rs.randint(1, 64, size=(batch, n)) / 64.).astype(np.float32)
        c["isw"] = np.array([0.5, 1., 2., 0.25], np.float32)
    gamma_n = 0.5
    ref0 = _reference(c, n_act, gamma_n, 0.)
    T, u = ref0["T"], ref0["u"]
    assert torch.equal(T.float().double(), T) and torch.equal(T * 8, (T * 8).round())
    assert torch.equal(u.float().double(), u) and u.abs().min().item() >= 1. / 16
    _check_against(ref0, _launch(c, n_act, gamma_n, 0.), c, n_act, None, exact_u=True, exact_grad=dyadic)
    sb = 1
    a0 = int(c["act"][sb])
    tied = {0: 1, 2: 0, n - 1: m - 1}
    for i, j in tied.items():
        c["pred"][sb, i, a0] = np.float32(T[sb, j].item())
    ref0, ref1 = _reference(c, n_act, gamma_n, 0.), _reference(c, n_act, gamma_n, 1.)
    assert all((ref0["u"][sb, i] == 0).any() for i in tied)
    got0, got1 = _launch(c, n_act, gamma_n, 0.), _launch(c, n_act, gamma_n, 1.)
    _check_against(ref0, got0, c, n_act, None, exact_u=True, exact_grad=dyadic)
    _check_against(ref1, got1, c, n_act, 1.)
    # what a u == 0 pair contributes at kappa == 0: -tau_i w_b / N' (not negative), and nothing at kappa = 1
    w0 = ref0["w"][sb].item()
    for i in tied:
        zero = ref0["u"][sb, i] == 0
        tau = float(c["tau"][sb, i])
        rest0 = -(w0 / m) * (tau - (ref0["u"][sb, i][~zero] < 0).double()).sum().item()
        assert abs(got0[0][sb, i, a0].item() - (rest0 - tau * w0 / m * int(zero.sum()))) <= (m + 8) * EPS * w0


# ---- action kernel ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_act,stride", [(1, 4), (6, 8), (64, 64)])
@pytest.mark.parametrize("k", [1, 32, 64])
def test_action_kernel_greedy_ties_override_onehot_and_counter(k, n_act, stride):
    from accel_rl_amd import _lib
    b = 9                                           # two workgroups of four samples and one of one
    rs = np.random.RandomState(4 + k + n_act)
    theta = _block(rs, b, k, n_act, stride)
    chosen = _selecting(rs, theta, n_act)
    if n_act > 1:                                   # two bit-identical columns, both the maximum: the lower index wins
        lo, hi = 1, n_act - 1
        theta[5, :, hi] = theta[5, :, lo]
        theta[5, :, lo] += np.float32(2.0)
        theta[5, :, hi] += np.float32(2.0)
        chosen[5] = lo if lo != hi else chosen[5]
    q = torch.from_numpy(theta[:, :, :n_act].astype(np.float64)).sum(dim=1) / k
    if n_act > 1:
        top2 = torch.topk(q, 2, dim=1).values
        assert ((top2[:, 0] - top2[:, 1])[torch.arange(b) != 5] >= 0.2 - 1e-6).all()
        if n_act > 2:
            q[5, n_act - 1] = -1e9                  # (float64 rounding must not pick between the twins)
    np.testing.assert_array_equal(q.argmax(dim=1).numpy(), chosen)
    ov = np.full(b, -1, np.int32)
    ov[::4] = rs.randint(0, n_act, size=len(ov[::4]))
    onehot = torch.full((b, n_act), float("nan"), device=DEV)
    greedy = torch.full((b,), 255, dtype=torch.uint8, device=DEV)
    state = torch.tensor([3, 10], dtype=torch.int64, device=DEV)
    _lib.iqn_act(_dev(theta), _dev(ov), n_act, k, onehot, greedy, state=state, advance=3)
    np.testing.assert_array_equal(greedy.cpu().numpy(), chosen)             # the argmax, override or not
    served = np.where(ov >= 0, ov, chosen)
    assert torch.equal(onehot.cpu(), F.one_hot(torch.from_numpy(served).long(), n_act).float())
    assert state.cpu().tolist() == [3, 13]                                  # advanced by exactly `advance`
    onehot2 = torch.full((b, n_act), float("nan"), device=DEV)
    _lib.iqn_act(_dev(theta), None, n_act, k, onehot2, None)                # no override table, no greedy output, no state
    assert torch.equal(onehot2.cpu(), F.one_hot(torch.from_numpy(chosen).long(), n_act).float())
    assert state.cpu().tolist() == [3, 13]


def test_the_loss_launch_advances_the_counter_by_exactly_advance():
    c = _case(3, 6, 8, 8, 8, 4, True, True)
    state = torch.tensor([3, 2 ** 40], dtype=torch.int64, device=DEV)
    one = _launch(c, 6, 0.97, 1.0, state=state, advance=3)
    assert state.cpu().tolist() == [3, 2 ** 40 + 3]
    two = _launch(c, 6, 0.97, 1.0)
    assert state.cpu().tolist() == [3, 2 ** 40 + 3] and all(torch.equal(x, y) for x, y in zip(one, two))


# ---- refusals -----------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    from accel_rl_amd import _lib
    lib = _lib.load()
    batch = 2
    theta = torch.zeros(batch, 66, 68, device=DEV)                          # large enough for every size named below
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    ret = torch.zeros(batch, device=DEV)
    tau = torch.zeros(batch * 66, device=DEV)
    state = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
    seven = lambda *shape: torch.full(shape, 7., device=DEV)                # noqa: E731
    dth, rowsb, pri, onehot = seven(batch, 66, 68), seven(batch), seven(batch), seven(batch, 66)
    tau_out, cosf, x, dphi, dpsi = seven(batch * 66), seven(batch * 66, 64), seven(batch * 66, 8), seven(batch * 66, 8), seven(batch, 8)
    greedy = torch.full((batch,), 7, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()                      # noqa: E731

    def loss(b=batch, a=6, n=8, m=8, s=8, kappa=1.0, pred=p(theta), out=p(dth), acts=p(act), tp=p(tau)):
        return lib.arl_iqn_loss(pred, tp, p(theta), None, acts, p(ret), p(act), None, b, a, n, m, s, 0.99, kappa, out,
                                p(rowsb), p(pri), None, 0, None)

    def serve(b=batch, a=6, n=8, s=8, th=p(theta), out=p(onehot), m=None):
        return lib.arl_iqn_act(th, None, b, a, n, s, out, p(greedy), None, 0, None)

    def embed(tin=None, st=p(state), rows=batch, r=8, out=p(tau_out), cf=p(cosf), row0=0):
        return lib.arl_iqn_embed(tin, st, row0, 0, rows, r, out, cf, None)

    def fwd(b=batch, r=8, f=8, ps=p(theta), out=p(x)):
        return lib.arl_iqn_merge_fwd(ps, p(theta), b, r, f, out, None)

    def bwd(b=batch, r=8, f=8, g=p(theta), o1=p(dphi), o2=p(dpsi)):
        return lib.arl_iqn_merge_bwd(g, p(theta), p(theta), b, r, f, o1, o2, None)

    for call in (loss, serve):
        assert call(n=0) == -1 and b"fractions" in lib.arl_last_error()
        assert call(n=65) == -1
        assert call(a=65, s=68) == -1               # n_actions > 64
        assert call(a=0) == -1
        assert call(s=10) == -1                     # not a multiple of 4
        assert call(a=6, s=4) == -1                 # a_stride < n_actions
        assert call(b=0) == -1
    assert loss(m=0) == -1 and loss(m=65) == -1
    assert loss(kappa=-1.0) == -1 and b"kappa" in lib.arl_last_error()
    assert loss(kappa=float("inf")) == -1 and loss(kappa=float("nan")) == -1
    assert loss(pred=None) == -1 and b"null" in lib.arl_last_error()
    assert loss(out=None) == -1 and loss(acts=None) == -1 and loss(tp=None) == -1
    assert serve(th=None) == -1 and serve(out=None) == -1
    assert embed(st=None) == -1 and b"exactly one" in lib.arl_last_error()  # neither tau_in nor state
    assert embed(tin=p(tau)) == -1                                          # both
    assert embed(out=None) == -1 and embed(cf=None) == -1
    assert embed(r=0) == -1 and embed(r=65) == -1 and embed(rows=0) == -1 and embed(row0=-1) == -1
    for call in (fwd, bwd):
        assert call(r=0) == -1 and call(r=65) == -1 and call(b=0) == -1
        assert call(f=6) == -1 and call(f=0) == -1
    assert fwd(ps=None) == -1 and fwd(out=None) == -1
    assert bwd(g=None) == -1 and bwd(o1=None) == -1 and bwd(o2=None) == -1
    torch.cuda.synchronize()
    for t in (dth, rowsb, pri, onehot, tau_out, cosf, x, dphi, dpsi):
        assert (t == 7.).all()
    assert (greedy == 7).all() and state.cpu().tolist() == [1, 0]
    assert loss() == 0 and serve() == 0 and embed() == 0 and fwd() == 0 and bwd() == 0      # inside the limits they run
    torch.cuda.synchronize()
    assert not (dth.view(-1)[:batch * 8 * 8] == 7.).any() and not (onehot.view(-1)[:batch * 6] == 7.).any()
    assert not (cosf.view(-1)[:batch * 8 * 64] == 7.).any() and not (x.view(-1)[:batch * 8 * 8] == 7.).any()
    assert not (dphi.view(-1)[:batch * 8 * 8] == 7.).any() and not (dpsi.view(-1) == 7.).any()


# ---- determinism --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kappa", [1.0, 0.0])
def test_two_loss_launches_are_bit_identical(kappa):
    n_act, n, m, stride, batch = 18, 51, 64, 20, 37
    c = _case(11, n_act, n, m, stride, batch, True, True)
    one, two = _launch(c, n_act, 0.97, kappa), _launch(c, n_act, 0.97, kappa)
    assert torch.isfinite(one[0]).all()
    for x, y in zip(one, two):
        assert torch.equal(x, y)


def test_two_merge_backward_launches_are_bit_identical():
    b, r, f = 2, 64, 3136
    rs = np.random.RandomState(1)
    psi = np.maximum(rs.randn(b, f), 0).astype(np.float32)
    phi = np.maximum(rs.randn(b * r, f), 0).astype(np.float32)
    g = rs.randn(b * r, f).astype(np.float32)
    one, two = _merge_bwd(psi, phi, g, b, r, f), _merge_bwd(psi, phi, g, b, r, f)
    assert np.isfinite(one[0]).all() and np.isfinite(one[1]).all()
    np.testing.assert_array_equal(one[0], two[0])
    np.testing.assert_array_equal(one[1], two[1])
    want = np.where(psi > 0, (g.astype(np.float64) * phi).reshape(b, r, f).sum(axis=1), 0.)
    assert np.abs(one[1] - want).max() <= (r + 8) * EPS * np.abs(g * phi).max() * r   # (an r-term fp32 sum)


# ---- policy and algorithm -----------------------------------------------------------------------------------------

N_ACT, BATCH, N_Q = 6, 8, 4


@pytest.fixture(scope="module")
def small():
    """AtariIqnPolicy on a small spec (2 conv layers, hidden 64, 6 actions, N = N' = 4) with perturbed parameters and a
    target net that differs, and one minibatch of 8 with given fractions."""
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    from accel_rl_amd.spaces import Discrete, UintBox, EnvSpec
    from accel_rl_amd.util.seed import set_seed
    set_seed(5)
    spec = dict(cnn_specs[0], hidden_sizes=[64])
    policy = AtariIqnPolicy(epsilon=0.3, n_quantiles=N_Q, n_target_quantiles=N_Q, n_policy_quantiles=32, **spec)
    policy.initialize(EnvSpec(UintBox((4, 104, 80)), Discrete(N_ACT)), device=DEV)
    rs = np.random.RandomState(3)
    flat = policy.get_param_values()
    assert flat.size == policy.n_params == sum(int(np.prod(s)) for s in policy._ref_shapes)
    flat = flat + (rs.randn(flat.size) * 0.01).astype(np.float32)           # non-zero biases: layout errors would show
    policy.set_param_values(flat)
    np.testing.assert_array_equal(policy.get_param_values(), flat)          # round trip through the reference layout
    policy.flat_target.copy_(policy.flat_params * 0.9)
    b = BATCH
    mb = dict(obs=_dev(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)),
              nxt=_dev(rs.randint(0, 256, size=(b, 4, 104, 80), dtype=np.uint8)),
              act=_dev(rs.randint(0, N_ACT, size=b).astype(np.uint8)), ret=_dev(rs.randn(b).astype(np.float32)),
              term=_dev((rs.rand(b) < 0.3).astype(np.uint8)), isw=_dev((rs.rand(b) + 0.2).astype(np.float32)),
              taus=tuple(_dev(rs.uniform(0.02, 0.98, size=b * N_Q).astype(np.float32)) for _ in range(3)))
    return policy, spec, mb


def _ref_theta(rp, spec, x, tau, n_act):
    """Plain float64 torch on the reference layout: conv (W, b) ..., embedding (W (64, F), b), hidden (W, b), output
    (W, b); the conv output is flattened in the reference's (c, h, w) order.  tau [B][R] -> theta [B][R][A]."""
    k = 0
    for i in range(len(spec["conv_filters"])):
        x = F.relu(F.conv2d(x, rp[k].flip(2, 3), rp[k + 1], stride=spec["conv_strides"][i],
                            padding=tuple(spec["conv_pads"][i])))
        k += 2
    psi = x.flatten(1)
    c = torch.cos(np.pi * torch.arange(64, dtype=torch.float64) * tau[:, :, None])
    phi = F.relu(c @ rp[k] + rp[k + 1])
    h = F.relu((psi[:, None, :] * phi) @ rp[k + 2] + rp[k + 3])
    return h @ rp[k + 4] + rp[k + 5]


@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
def test_training_step_matches_autograd_through_plain_torch(small, double):
    """One ImplicitQuantileDQN minibatch with given fractions: gradients of every parameter in the reference's layout,
    at the tolerances of tests/test_qrdqn_gpu.py's whole-step test (a network of the same depth)."""
    policy, spec, mb = small
    b, n = BATCH, N_Q
    assert policy.param_short_names == ["Conv0W", "Conv0b", "Conv1W", "Conv1b", "EmbW", "Embb", "FC0W", "FC0b", "OutputW",
                                        "Outputb"]
    f = policy._f
    assert [tuple(s) for s in policy._ref_shapes[4:]] == [(64, f), (f,), (f, 64), (64,), (64, N_ACT), (N_ACT,)]
    assert policy._head_width % 4 == 0 and policy._head_width >= N_ACT
    gamma_n = float(np.float32(0.99))
    counter = policy._iqn_state.cpu().tolist()
    policy.flat_grads.fill_(float("nan"))
    rows, pri = policy.iqn_loss_and_grads(mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"], gamma_n, 1.0,
                                          double_dqn=double, taus=mb["taus"] if double else mb["taus"][:2] + (None,))
    assert rows.data_ptr() + 4 * b == pri.data_ptr()            # the (2, b) buffer the optimizer's ring takes at once
    assert policy._iqn_state.cpu().tolist() == counter          # given fractions leave the counter alone
    got = policy.bucket_to_reference(policy.flat_grads)
    pad = policy.grads[policy._k_head][N_ACT:]
    assert not pad.any() and not policy.grads[policy._k_head + 1][N_ACT:].any()     # zero gradients in the padding

    def ref_params(flat_bucket):
        fl = policy.bucket_to_reference(flat_bucket)
        out, pos = [], 0
        for shape in policy._ref_shapes:
            m = int(np.prod(shape))
            out.append(torch.from_numpy(fl[pos:pos + m].reshape(shape).astype(np.float64)).requires_grad_())
            pos += m
        return out
    rp, rt = ref_params(policy.flat_params), ref_params(policy.flat_target)
    scale = float(np.float32(1. / 255))
    t_pred, t_tgt, t_pol = (t.cpu().double().view(b, n) for t in mb["taus"])
    obs, nxt = mb["obs"].cpu().double() * scale, mb["nxt"].cpu().double() * scale
    pred = _ref_theta(rp, spec, obs, t_pred, N_ACT)
    with torch.no_grad():
        tgt = _ref_theta(rt, spec, nxt, t_tgt, N_ACT)
        pol = _ref_theta(rp, spec, nxt, t_pol, N_ACT) if double else None
    ref = ref_iqn_loss(pred, t_pred, tgt, pol, mb["act"].cpu(), mb["ret"].cpu(), mb["term"].cpu(), mb["isw"].cpu(), gamma_n, 1.0)
    assert ref["margin"] > 1e-4, ref["margin"]                  # the greedy next actions are away from fp32 ties
    loss = ref["rows"].sum()
    grads = torch.autograd.grad(loss, rp)
    want = np.concatenate([g.detach().numpy().reshape(-1) for g in grads])
    print("loss %.6g vs %.6g; max grad err %.3g of max |grad| %.3g" % (rows.sum().item(), loss.item(),
                                                                       np.abs(got - want).max(), np.abs(want).max()))
    assert abs(rows.sum().item() - loss.item()) <= 1e-4 * abs(loss.item())
    assert np.allclose(rows.cpu().numpy(), ref["rows"].detach().numpy(), rtol=2e-3, atol=1e-6)
    assert np.allclose(pri.cpu().numpy(), ref["loss_b"].clamp(1e-6, 1e6).numpy(), rtol=2e-3, atol=1e-5)
    assert np.allclose(got, want, rtol=2e-3, atol=2e-5 * max(np.abs(want).max(), 1e-3)), np.abs(got - want).max()
    assert np.abs(want[sum(int(np.prod(s)) for s in policy._ref_shapes[:4]):][:64 * f]).max() > 0   # the embedding learns


def _update(policy, mb, double=True):
    rows, pri = policy.iqn_loss_and_grads(mb["obs"], mb["nxt"], mb["act"], mb["ret"], mb["term"], mb["isw"], 0.99, 1.0,
                                          double_dqn=double)
    return rows, pri


def _set_counter(policy, value):
    policy._iqn_state[1] = value


def test_counter_and_captured_graph_draw_fresh_fractions(small):
    from accel_rl_amd.util.misc import capture_graph
    policy, _, mb = small
    _set_counter(policy, 40)
    _update(policy, mb, double=True)
    assert policy._iqn_state.cpu().tolist() == [policy.iqn_seed, 43]         # one update: 3, double DQN ...
    _update(policy, mb, double=False)
    assert policy._iqn_state.cpu().tolist() == [policy.iqn_seed, 46]         # ... or not
    policy.greedy_actions(mb["obs"])
    assert policy._iqn_state.cpu().tolist()[1] == 47                         # one serving pass: 1
    try:
        policy.serve_pair_rows = 3 * policy.n_policy_quantiles               # 3 rows a pass: 8 rows = 3 passes
        policy.prob_value(mb["obs"])
        assert policy._iqn_state.cpu().tolist()[1] == 50
    finally:
        policy.serve_pair_rows = 8192
    # a captured update, replayed: fresh fractions each time, each equal to the eager call at the same counter value
    torch.cuda.synchronize()
    _set_counter(policy, 100)
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph):
        out = _update(policy, mb)
    assert policy._iqn_state.cpu().tolist()[1] == 100                        # (capturing ran nothing)
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append((out[0].clone(), out[1].clone(), policy.flat_grads.clone()))
    assert policy._iqn_state.cpu().tolist()[1] == 106
    assert not torch.equal(replays[0][0], replays[1][0])                     # two different losses
    _set_counter(policy, 100)
    for want in replays:
        rows, pri = _update(policy, mb)
        assert torch.equal(rows, want[0]) and torch.equal(pri, want[1]) and torch.equal(policy.flat_grads, want[2])
    assert torch.isfinite(replays[0][2]).all()
    del graph


def test_serving_split_does_not_change_the_actions(small):
    """11 rows at 3 rows a pass (three passes and a remainder of 2) against one pass: the fraction stream is indexed by
    the global row, so the actions agree bit for bit."""
    policy, _, mb = small
    obs = torch.cat([mb["obs"], mb["nxt"]])[:11]                             # 11 rows: passes of 3, 3, 3 and a remainder of 2
    policy.host_draws(1, 11, n_groups=1)
    policy.set_step(0)
    try:
        results = []
        for limit in (3 * policy.n_policy_quantiles, 8192):
            policy.serve_pair_rows = limit
            _set_counter(policy, 7)
            greedy = policy.greedy_actions(obs).cpu()
            passes = policy._iqn_state.cpu().tolist()[1] - 7
            _set_counter(policy, 7)
            onehot = policy.prob_value(obs)[0].cpu()
            results.append((greedy, onehot, passes))
        assert results[0][2] == 4 and results[1][2] == 1
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
        assert (results[0][1].sum(dim=1) == 1).all()
    finally:
        policy.serve_pair_rows = 8192
        policy._overrides.clear()


def test_iqn_trains_with_prioritized_replay_and_eval():
    """The QR-DQN end-to-end configuration at toy size with ImplicitQuantileDQN: GpuVecEvalSampler -> device replay
    (prioritized) -> IQN updates inside the captured graph -> target sync, epsilon / beta schedules."""
    from accel_rl_amd.algos.dqn.iqn import ImplicitQuantileDQN
    from accel_rl_amd.envs.synthetic_atari import SynthAtariEnv
    from accel_rl_amd.policies.atari_cnn_specs import cnn_specs
    from accel_rl_amd.policies.dqn.atari_iqn_policy import AtariIqnPolicy
    from accel_rl_amd.runners.accel_rl import AccelRLEval
    from accel_rl_amd.sampler.gpu_sampler_with_eval import GpuVecEvalSampler
    from accel_rl_amd.util import logger
    logger.set_quiet(True)
    sampler = GpuVecEvalSampler(eval_steps=8 * 40, eval_envs_per=1, EnvCls=SynthAtariEnv,
                                env_args=dict(game="seaquest"), horizon=4, n_parallel=4, envs_per=2,
                                max_path_length=25, max_decorrelation_steps=0, device=DEV)
    algo = ImplicitQuantileDQN(batch_size=32, min_steps_learn=64 * 4, replay_size=64 * 60, training_intensity=8,
                               target_update_steps=64 * 3, reward_horizon=3, prioritized_replay=True,
                               double_dqn=True, eps_greedy_args=dict(anneal_steps=64 * 10))
    policy = AtariIqnPolicy(**cnn_specs[0], n_quantiles=8, n_target_quantiles=8, n_policy_quantiles=16)
    first = {}
    initialize = policy.initialize

    def recording_initialize(*args, **kwargs):
        initialize(*args, **kwargs)
        first["params"] = policy.get_param_values()
    policy.initialize = recording_initialize
    runner = AccelRLEval(algo=algo, policy=policy, sampler=sampler, n_steps=64 * 24, seed=9, eval_interval_steps=64 * 8)
    runner.train()
    tab = runner.last_tabular
    for key in ("StepsInEval", "TrajsInEval", "LossAverage", "PriorityAverage", "ReturnAverage", "ParamsNorm"):
        assert key in tab, key
    assert np.isfinite(tab["LossAverage"]) and tab["LossAverage"] > 0 and tab["TrajsInEval"] > 0
    assert 1e-6 <= tab["PriorityAverage"] <= 1e6
    assert algo._updates_per_optimize == 8 * 64 // 32 and abs(policy.get_epsilon() - 0.01) < 1e-9
    assert algo.replay_buffer.beta > 0.4
    final = policy.get_param_values()
    assert np.isfinite(final).all() and not np.array_equal(final, first["params"])      # the parameters moved
    target = policy.bucket_to_reference(policy.flat_target)
    assert np.isfinite(target).all() and not np.array_equal(target, first["params"])    # the target net was synced
    assert policy._iqn_state.cpu().tolist()[1] > 3 * algo._updates_per_optimize         # updates and serving drew fractions
