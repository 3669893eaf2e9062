"""The quantile-family kernels at the limits their entry points accept (csrc/dqn.hip: arl_qrdqn_act / _loss; csrc/iqn.hip:
arl_iqn_embed / _merge_fwd / _merge_bwd / _act / _loss, arl_miqn_loss; csrc/fqf.hip: arl_fqf_fractions / _act / _loss; all
over csrc/q_loss_dev.h).  The feature tests (test_qrdqn_gpu.py, test_iqn_gpu.py, test_fqf_gpu.py, test_munchausen_gpu.py)
stay as they are; this file runs what they leave out: strides up to 2^20, block indices above 65535, merge grids above
65535 blocks, the embedding's addressing at its limits and its cosine reduction over the whole of fp32, and the corner
rows of the losses.

Yardstick: BIT FOR BIT against the fp32 restatement of tests/quantile_ref.py wherever the kernel calls no device-library
function -- the three action kernels, arl_iqn_loss, arl_qrdqn_loss, both merges, the drawn tau, the whole of
arl_fqf_loss (tau, q, logq and H are its inputs), arl_fqf_fractions' tau chain and entropy given its own q and logq, and
everything of arl_miqn_loss after T_j on inputs whose soft-max is exact (one action, or a maximum unique by far more
than 88 tau_e: every other e_a is 0, s == 1, pi is one-hot, and lp is 0 or below l0 -- the header's reduces-to-IQN
construction, with the bonus on top; or three bit-equal maxima, where pi = fl(1 / 3) and the one library value left,
logf(3), is recovered from a first launch).  The kernel's own T_j cannot be read back per j through a kappa == 0 probe
(every output sums over j), which is why T_j is made exact instead.  Orders that decide no output on well-separated
inputs get inputs of their own: action values whose greedy action depends on the order of the sum over the fractions,
and unquantised merge inputs.  Where the device library is involved the project's existing bars hold: 2^-22 for
the cosines (test_iqn_gpu.py), fqf_ref.fraction_bounds for q / logq / H, the Munchausen bounds of munchausen_ref.py for
a general soft-max; the largest error-to-bound ratio is printed.  Every output sits in a NaN-filled buffer whose guard
tail is checked untouched.

Refusals: the last accepted value is run by the test named beside it, the first refused one here.  Already pinned by
test_refusals_launch_nothing of the feature files and not repeated: 0 and 65 fractions, 0 and 65 actions, n_quantiles
1, a stride that is no multiple of 4 or below the row, batch 0, kappa / ent_coef / tau_e / alpha / l0 out of range, NULL
pointers, arl_iqn_embed's tau_in / state rule, r 0 and 65, rows 0, row0 -1, f 0 and 6, misaligned logits / dlogits.

Out of scope: batch near 2^31 and batch x r x f near 2^40 (tens of GiB); arl_mdqn_loss, arl_drq_loss, arl_q_regress_loss."""
import numpy as np
import pytest
import torch

import fqf_ref as fr
import munchausen_ref as mr
import quantile_ref as qr
from quantile_ref import F32
from test_iqn_gpu import _merge_case, ref_tau
from test_munchausen_gpu import _check_miqn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
PAD = 64                                                        # guard elements behind every output
GAMMA = float(np.float32(0.99 ** 3))
KAPPAS = (0.0, 0.25, 1.0)
BIG = 1 << 20                                                   # the largest stride every entry point accepts
E_ARG, E_RANGE, E_ALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from accel_rl_amd import _lib
    _lib.load()
    return _lib


COMPARED = [0]                                                  # elements held bit for bit so far


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nbit for bit: 0 of %d compared elements differed" % COMPARED[0])


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(t):
    return t.detach().cpu().numpy()


class Outs:
    """Outputs inside NaN-filled (integers: 0x7b-filled) buffers with a guard tail of PAD elements."""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        fill = NAN if dtype.is_floating_point else 0x7b
        big = torch.full((n + PAD,), fill, dtype=dtype, device=DEV)
        self.items.append((big, n, fill))
        return big[:n].view(shape)

    def check(self):
        torch.cuda.synchronize()
        for big, n, fill in self.items:
            tail = big[n:]
            assert bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all()), "guard tail written"

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(big).all()) if fill != fill else bool((big == fill).all()) for big, _, fill in self.items)


def _same_bits(got, want, what):
    got = _host(got) if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == F32:
        got, want = qr.bits(got), qr.bits(want.astype(F32, copy=False))
    differ = int((got != want).sum())
    assert differ == 0, "%s: %d of %d elements differ" % (what, differ, got.size)
    COMPARED[0] += got.size


def _same_bits_wide(got, want, what):
    """got [...][S] on the device against want [...][s <= S]: the leading columns bit for bit, the rest exact +0."""
    w = want.shape[-1]
    _same_bits(got[..., :w].contiguous(), want, what)
    if got.shape[-1] > w:
        rest = got[..., w:].contiguous().view(torch.int32)
        assert int(torch.count_nonzero(rest)) == 0, what + ": padding columns"
        COMPARED[0] += rest.numel()


def _wide(narrow, stride):
    """[..., s] -> a device tensor [..., stride], poison behind the s given columns."""
    t = torch.full(tuple(narrow.shape[:-1]) + (stride,), qr.POISON, device=DEV)
    t[..., :narrow.shape[-1]] = _dev(narrow)
    return t


def _serve_want(g, ov, n_act):
    served = g if ov is None else np.where(ov >= 0, ov, g)
    onehot = np.zeros((g.size, n_act), F32)
    onehot[np.arange(g.size), served] = 1
    return onehot, g.astype(np.uint8)


# ---- launchers ---------------------------------------------------------------------------------------------------------------

def _iqn(L, c, n_act, stride, kappa, state=None, advance=0, miqn=None):
    """arl_iqn_loss (miqn None) or arl_miqn_loss (miqn = (tau_e, alpha, l0), c["cur"]) at a_stride `stride`."""
    o = Outs()
    pred = _wide(c["pred"], stride)
    batch, n = pred.shape[:2]
    m = c["tgt"].shape[1]
    dth, rows, pri = o.new((batch, n, stride)), o.new((batch,)), o.new((batch,))
    tail = (_dev(c["act"]), _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), n_act, n, m, GAMMA, kappa)
    if miqn is None:
        L.iqn_loss(pred, _dev(c["tau"]), _wide(c["tgt"], stride), None if c["pol"] is None else _wide(c["pol"], stride),
                   *tail, dth, rows, pri, state=state, advance=advance)
    else:
        L.miqn_loss(pred, _dev(c["tau"]), _wide(c["tgt"], stride), _wide(c["cur"], stride), *tail, *miqn, dth, rows, pri,
                    state=state, advance=advance)
    o.check()
    return dth, rows, pri


def _check_loss(got, want, what):
    _same_bits_wide(got[0], want["dtheta"], what + " dtheta")
    _same_bits(got[1], want["rows"], what + " loss_rows")
    _same_bits(got[2], want["pri"], what + " priorities")


def _iqn_want(c, n_act, kappa):
    return qr.iqn_loss(c["pred"], c["tau"], c["tgt"], c["pol"], c["act"], c["ret"], c["term"], c["isw"], n_act, GAMMA, kappa)


def _miqn_exact_case(seed, n_act, n, m, stride, kappa, batch=qr.CORNER_BATCH):
    """corner_case with the soft-max made exact: the target net's chosen column leads by 400 (a unique maximum, also in the
    tie row), and in tgt_cur one column leads by 400 -- the taken action's (lp == 0: the bonus is clipped at 0) in the even
    rows and in the rows whose u is planted, another one's (lp == -400 < l0: clipped at l0) in the odd rows.  Returns the
    case and its T [B][N'] in fp32."""
    c = qr.corner_case(seed, n_act, n, m, stride, kappa, double=False, batch=batch)
    ar = np.arange(batch)
    c["tgt"][ar, :, c["chosen"]] += F32(400)
    if n_act > 1:
        c["tgt"][qr.ROW_TIE, :, n_act - 1] -= F32(800)
    act = qr.clamp_action(c["act"], n_act)
    taken = (ar % 2 == 0) | np.isin(ar, (qr.ROW_KAPPA_EDGES, qr.ROW_TINY_LOSS, qr.ROW_HUGE_LOSS)) | (n_act == 1)
    lead = np.where(taken, act, (act + 1) % n_act)
    c["cur"] = qr._blocks(np.random.RandomState(seed + 1), batch, m, n_act, stride)
    c["cur"][ar, :, lead] += F32(400)
    bonus = np.where(taken, F32(mr.ALPHA) * F32(0), F32(mr.ALPHA) * F32(mr.L0)).astype(F32)
    keep = np.where(c["term"] != 0, F32(0), F32(1))
    T = (c["ret"] + bonus)[:, None] + keep[:, None] * (F32(GAMMA) * c["tgt"][ar, :, c["chosen"]])
    assert T.dtype == F32
    return c, T, taken


def _fractions(L, lg, n):
    """arl_fqf_fractions on device logits [B][n_stride] -> dict of device tensors."""
    o = Outs()
    batch = lg.shape[0]
    out = dict(tau=o.new((batch, n + 1)), tau_hat=o.new((batch, n)), tau_mid=o.new((batch, max(n - 1, 1))) if n > 1 else None,
               q=o.new((batch, n)), logq=o.new((batch, n)), H=o.new((batch,)))
    L.fqf_fractions(lg, n, out["tau"], out["tau_hat"], out["tau_mid"], out["q"], out["logq"], out["H"])
    o.check()
    return out


def _check_fractions(f, lg_host, n):
    """q, logq, H against float64 at fqf_ref.fraction_bounds; tau, tau_hat, tau_mid and H bit for bit from the kernel's own
    q and logq.  Returns the largest error / bound."""
    ref = fr.ref_fractions(torch.from_numpy(lg_host[:, :n].astype(np.float64)))
    q_rel, tau_atol, logq_atol, h_atol = fr.fraction_bounds(lg_host[:, :n], n)
    q, logq, H = _host(f["q"]), _host(f["logq"]), _host(f["H"])
    q64 = ref["q"].numpy()
    # (an underflowed q_k is an exact 0 where float64 still holds ~1e-87: 2^-126 covers it, as in test_fqf_gpu.py)
    ratios = [np.max(np.abs(q - q64) / (q_rel * q64 + 2.0 ** -126)),
              np.abs(_host(f["tau"]) - ref["tau"].numpy()).max() / tau_atol,
              np.abs(logq - ref["logq"].numpy()).max() / logq_atol, np.abs(H - ref["H"].numpy()).max() / h_atol]
    assert max(ratios) <= 1, ratios
    tau, hat = qr.fqf_tau_chain(q)
    _same_bits(f["tau"], tau, "tau")
    _same_bits(f["tau_hat"], hat, "tau_hat")
    if n > 1:
        _same_bits(f["tau_mid"], tau[:, 1:n], "tau_mid")
    _same_bits(f["H"], qr.fqf_entropy(q, logq), "entropy")
    return max(ratios)


def _fqf(L, c, mid, f, n_act, stride, n_stride, kappa, ent):
    """arl_fqf_loss on the device fractions f; c: corner_case (N' = N; its tau is not used)."""
    o = Outs()
    pred = _wide(c["pred"], stride)
    batch, n = pred.shape[:2]
    dth, rows, pri = o.new((batch, n, stride)), o.new((batch,)), o.new((batch,))
    dlg, frac = o.new((batch, n_stride)), o.new((batch,))
    L.fqf_loss(pred, None if mid is None else _wide(mid, stride), f["tau"], f["tau_hat"], f["q"], f["logq"], f["H"],
               _wide(c["tgt"], stride), None if c["pol"] is None else _wide(c["pol"], stride), _dev(c["act"]),
               _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), n_act, n, GAMMA, kappa, ent, dth, rows, pri, dlg, frac)
    o.check()
    return dth, rows, pri, dlg, frac


def _fqf_want(c, mid, f, n_act, n_stride_narrow, kappa, ent):
    h = {k: None if v is None else _host(v) for k, v in f.items()}
    return qr.fqf_loss(c["pred"], mid, h["tau"], h["tau_hat"], h["q"], h["logq"], h["H"], c["tgt"], c["pol"], c["act"],
                       c["ret"], c["term"], c["isw"], n_act, n_stride_narrow, GAMMA, kappa, ent)


def _check_fqf(got, want, what):
    _check_loss(got[:3], want, what)
    _same_bits_wide(got[3], want["dlogits"], what + " dlogits")
    _same_bits(got[4], want["frac"], what + " frac_rows")


def _qr_case(seed, n_act, n, s0, batch, dueling, double):
    """theta blocks [B][A (+ 1)][s0] with poison behind the N quantiles; one action's rows lead by 20."""
    rs = np.random.RandomState(seed)
    rows = n_act + int(dueling)

    def block():
        t = (rs.randn(batch, rows, s0) * 2).astype(F32)
        t[:, :, n:] = qr.POISON
        return t
    pred, tgt, pol = block(), block(), block() if double else None
    chosen = rs.randint(0, n_act, size=batch)
    (pol if double else tgt)[np.arange(batch), chosen, :n] += F32(20)
    act = np.where(np.arange(batch) % 2 == 0, 0, n_act - 1).astype(np.uint8)
    term = (rs.rand(batch) < 0.3).astype(np.uint8)
    term[0] = 1
    if batch > 1:
        term[1] = 0
    return dict(pred=pred, tgt=tgt, pol=pol, act=act, ret=(rs.randn(batch) * 3).astype(F32), term=term,
                isw=(rs.rand(batch) + 0.1).astype(F32), chosen=chosen)


def _qr(L, c, n_act, n, stride, dueling, kappa):
    o = Outs()
    pred = _wide(c["pred"], stride)
    batch = pred.shape[0]
    dth, rows, pri = o.new(tuple(pred.shape)), o.new((batch,)), o.new((batch,))
    L.qrdqn_loss(pred, _wide(c["tgt"], stride), None if c["pol"] is None else _wide(c["pol"], stride), _dev(c["act"]),
                 _dev(c["ret"]), _dev(c["term"]), _dev(c["isw"]), n_act, n, GAMMA, kappa, dth, rows, pri, dueling=dueling)
    o.check()
    return dth, rows, pri


def _qr_want(c, n_act, n, dueling, kappa):
    return qr.qrdqn_loss(c["pred"], c["tgt"], c["pol"], c["act"], c["ret"], c["term"], c["isw"], n_act, n, dueling, GAMMA,
                         kappa)


def _qr_act(L, theta, ov, n_act, n, stride, dueling):
    o = Outs()
    batch = theta.shape[0]
    onehot, greedy = o.new((batch, n_act)), o.new((batch,), torch.uint8)
    L.qrdqn_act(_wide(theta, stride), _dev(ov), n_act, n, onehot, greedy, dueling=dueling)
    o.check()
    want = _serve_want(qr.first_max(qr.qr_q(theta, n_act, n, dueling)), ov, n_act)
    _same_bits(onehot, want[0], "qrdqn_act onehot")
    _same_bits(greedy, want[1], "qrdqn_act greedy")


# ---- strides -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride,n,m,batch", [(BIG, 3, 2, 2), (BIG, 1, 3, 2), (4100, 64, 64, qr.CORNER_BATCH)],
                         ids=["S2^20-N3-M2", "S2^20-N1-M3", "S4100-N64-M64"])
def test_the_three_strided_losses_at_wide_action_strides(L, stride, n, m, batch):
    """A = 64, the taken action in column 0 (row 0) and in column A - 1 (row 1), poison in every padding column."""
    n_act = 64
    for kappa in (1.0, 0.0):
        c = qr.corner_case(7 + n, n_act, n, m, 64, kappa)
        c = {k: None if v is None else v[:batch] for k, v in c.items()}
        assert c["act"][0] == 0 and c["act"][1] == n_act - 1
        _check_loss(_iqn(L, c, n_act, stride, kappa), _iqn_want(c, n_act, kappa), "iqn_loss S=%d kappa=%g" % (stride, kappa))
        cm, T, _ = _miqn_exact_case(11 + n, n_act, n, m, 64, kappa)
        cm = {k: None if v is None else v[:batch] for k, v in cm.items()}
        want = qr.miqn_loss_from_targets(cm["pred"], cm["tau"], T[:batch], cm["act"], cm["isw"], n_act, kappa)
        _check_loss(_iqn(L, cm, n_act, stride, kappa, miqn=(1.0, mr.ALPHA, mr.L0)), want, "miqn_loss S=%d" % stride)
        if n == m:
            _fqf_at(L, 13, n_act, n, stride, 68, kappa, batch)
    if n != m:                                                  # arl_fqf_loss has N' == N: its own shapes at 2^20
        for nn in (3, 1):
            _fqf_at(L, 17, n_act, nn, stride, 68, 1.0, batch)


def _fqf_at(L, seed, n_act, n, stride, n_stride, kappa, batch, dominant=(0,), ent=0.01):
    rs = np.random.RandomState(seed + n)
    c = qr.corner_case(seed + n, n_act, n, n, (n_act + 3) // 4 * 4, kappa)
    c = {k: None if v is None else v[:batch] for k, v in c.items()}
    mid = None if n == 1 else qr._blocks(rs, batch, n - 1, n_act, (n_act + 3) // 4 * 4)
    lg = qr.dominant_logits(rs, batch, n, (n + 3) // 4 * 4, rows=dominant)
    f = _fractions(L, _wide(lg, n_stride), n)
    ratio = _check_fractions(f, lg, n)
    got = _fqf(L, c, mid, f, n_act, stride, n_stride, kappa, ent)
    _check_fqf(got, _fqf_want(c, mid, f, n_act, (n + 3) // 4 * 4, kappa, ent), "fqf_loss N=%d S=%d NS=%d" % (n, stride, n_stride))
    return ratio, f, c, got


@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_qrdqn_loss_and_act_at_q_stride_2_to_the_20(L, dueling):
    n_act, batch = 2, 2
    for n, kappa in ((64, 1.0), (2, 0.0)):
        c = _qr_case(3 + n, n_act, n, 64, batch, dueling, True)
        _check_loss(_qr(L, c, n_act, n, BIG, dueling, kappa), _qr_want(c, n_act, n, dueling, kappa), "qrdqn_loss N=%d" % n)
        _qr_act(L, c["pol"], np.array([-1, 0], np.int32), n_act, n, BIG, dueling)


@pytest.mark.parametrize("n", [1, 2, 64])
def test_fqf_fractions_and_loss_at_n_stride_2_to_the_20(L, n):
    """dlogits' `o += 64` walk over 2^20 columns: N live ones, exact zeros behind them."""
    ratio, f, _, got = _fqf_at(L, 19, 3, n, 4, BIG, 1.0, 2)
    print("N %d, n_stride 2^20: fractions' largest error / bound %.3f" % (n, ratio))
    assert got[3].shape == (2, BIG)
    if n == 1:
        assert int(torch.count_nonzero(got[3].view(torch.int32))) == 0 and not _host(got[4]).any()
        _same_bits(f["tau"], np.array([[0, 1]] * 2, F32), "tau N=1")
        _same_bits(f["tau_hat"], np.full((2, 1), 0.5, F32), "tau_hat N=1")


def _act_want(theta, ov, n_act):
    return _serve_want(qr.first_max(qr.q_of_lane(theta, n_act)), ov, n_act)


def _iqn_act(L, theta, ov, n_act, stride, state=None, advance=0):
    o = Outs()
    batch, k = theta.shape[:2]
    onehot, greedy = o.new((batch, n_act)), o.new((batch,), torch.uint8)
    L.iqn_act(_wide(theta, stride), _dev(ov), n_act, k, onehot, greedy, state=state, advance=advance)
    o.check()
    want = _act_want(theta, ov, n_act)
    _same_bits(onehot, want[0], "iqn_act onehot")
    _same_bits(greedy, want[1], "iqn_act greedy")


def _fqf_act(L, theta, tau, ov, n_act, stride):
    """tau: device [B][K + 1] (the fractions kernel's)."""
    o = Outs()
    batch, k = theta.shape[:2]
    onehot, greedy = o.new((batch, n_act)), o.new((batch,), torch.uint8)
    L.fqf_act(_wide(theta, stride), tau, _dev(ov), n_act, k, onehot, greedy)
    o.check()
    wq = qr.wq_of_lane(theta, _host(tau), n_act)
    want = _serve_want(qr.first_max(wq), ov, n_act)
    _same_bits(onehot, want[0], "fqf_act onehot")
    _same_bits(greedy, want[1], "fqf_act greedy")
    return wq


def _act_block(rs, batch, k, n_act):
    """Random theta [B][K][A] whose action values are close (the fp32 order of the sum decides some of them); row 1: two
    bit-identical maximal columns."""
    theta = (rs.randn(batch, k, n_act) * 2).astype(F32)
    theta += (rs.randn(batch, 1, 1) * 100).astype(F32)
    if n_act > 1 and batch > 1:
        theta[1, :, n_act - 1] = theta[1, :, 0] = theta[1].max(axis=1) + F32(1)
    return theta


def test_iqn_act_and_fqf_act_at_a_stride_2_to_the_20(L):
    rs = np.random.RandomState(23)
    n_act, k, batch = 64, 2, 5
    theta = _act_block(rs, batch, k, n_act)
    ov = np.array([-1, -1, 63, 0, -1], np.int32)
    state = torch.tensor([9, 2 ** 40], dtype=torch.int64, device=DEV)
    _iqn_act(L, theta, ov, n_act, BIG, state=state, advance=5)
    assert state.cpu().tolist() == [9, 2 ** 40 + 5]
    lg = qr.dominant_logits(rs, batch, k, 4, rows=())
    f = _fractions(L, _dev(lg), k)
    _fqf_act(L, theta, f["tau"], ov, n_act, BIG)


@pytest.mark.parametrize("k", [3, 5, 63, 64])
def test_action_values_sum_the_fractions_ascending_from_zero(L, k):
    """Rows in which a descending sum over the fractions would pick another greedy action (quantile_ref.order_sensitive_theta):
    arl_iqn_act, the selection of arl_iqn_loss, and arl_fqf_act / arl_fqf_loss on the fractions kernel's own tau."""
    n_act, stride, rows = 3, 4, 8
    theta = qr.order_sensitive_theta(k, k, n_act, rows=rows)
    _iqn_act(L, theta, None, n_act, stride)
    c = qr.corner_case(k, n_act, 2, k, stride, 1.0, batch=qr.CORNER_BATCH)
    c = {key: None if v is None else v[:rows] for key, v in c.items()}
    c["pol"][:, :, :n_act] = theta
    want = _iqn_want(c, n_act, 1.0)
    assert set(want["a_next"].tolist()) <= {0, n_act - 1}
    _check_loss(_iqn(L, c, n_act, stride, 1.0), want, "iqn_loss, order-sensitive selection")
    lg = np.full((rows, (k + 3) // 4 * 4), qr.POISON, F32)
    lg[:, :k] = (np.random.RandomState(k).randn(k) * 0.5).astype(F32)
    f = _fractions(L, _dev(lg), k)
    tau = _host(f["tau"])
    assert (qr.bits(tau) == qr.bits(tau[:1])).all()
    theta = qr.order_sensitive_theta(k, k, n_act, rows=rows, tau=tau[0])
    _fqf_act(L, theta, f["tau"], None, n_act, stride)
    c = qr.corner_case(k + 1, n_act, k, k, stride, 1.0, batch=qr.CORNER_BATCH)
    c = {key: None if v is None else v[:rows] for key, v in c.items()}
    c["pol"][:, :, :n_act] = theta
    mid = qr._blocks(np.random.RandomState(k), rows, k - 1, n_act, stride)
    got = _fqf(L, c, mid, f, n_act, stride, lg.shape[1], 1.0, 0.01)
    _check_fqf(got, _fqf_want(c, mid, f, n_act, lg.shape[1], 1.0, 0.01), "fqf_loss, order-sensitive selection")


# ---- block indices above 65535 -----------------------------------------------------------------------------------------------

LOSS_GRID = 65539                                               # one workgroup per sample
ACT_GRID = 4 * 65536 + 3                                        # four samples per workgroup


def _plant_last_blocks(c, n_act):
    """Rows 65536 .. 65538: a terminal row, an out-of-range action, a tie of columns 0 and A - 1 in the selecting net."""
    c["term"][65536], c["term"][65537] = 1, 0
    c["act"][65537] = 255
    if n_act > 1:
        sel = c["tgt"] if c["pol"] is None else c["pol"]
        sel[65538, :, :n_act] = F32(-3)
        sel[65538, :, 0] = sel[65538, :, n_act - 1] = F32(7)
        c["chosen"][65538] = 0


@pytest.mark.parametrize("n_act", [1, 3])
def test_loss_kernels_past_block_65535(L, n_act):
    stride, kappa = 4, 1.0
    state = torch.tensor([1, -7], dtype=torch.int64, device=DEV)
    c = qr.corner_case(29, n_act, 1, 1, stride, kappa, batch=LOSS_GRID)
    _plant_last_blocks(c, n_act)
    want = _iqn_want(c, n_act, kappa)
    assert want["a_next"][65538] == 0 and want["dtheta"][65537, :, n_act - 1].any()
    _check_loss(_iqn(L, c, n_act, stride, kappa, state=state, advance=3), want, "iqn_loss batch 65539")
    assert state.cpu().tolist() == [1, -4]                      # advanced exactly once
    cm, T, _ = _miqn_exact_case(31, n_act, 1, 1, stride, kappa, batch=LOSS_GRID)
    assert qr.clamp_action(cm["act"], n_act)[65537] == n_act - 1
    cm["act"][65537] = 255                                      # read as A - 1, the action this odd row took anyway: same T
    cm["term"][65536] = 1
    T[65536] = cm["ret"][65536] + (F32(0) if (65536 % 2 == 0 or n_act == 1) else F32(mr.ALPHA) * F32(mr.L0))
    want = qr.miqn_loss_from_targets(cm["pred"], cm["tau"], T, cm["act"], cm["isw"], n_act, kappa)
    _check_loss(_iqn(L, cm, n_act, stride, kappa, state=state, advance=2, miqn=(0.03, mr.ALPHA, mr.L0)), want,
                "miqn_loss batch 65539")
    assert state.cpu().tolist() == [1, -2]
    # FQF: N = 1 (pred_mid NULL) on the kernel's own fractions
    rs = np.random.RandomState(37)
    lg = qr.dominant_logits(rs, LOSS_GRID, 1, 4, rows=())
    f = _fractions(L, _dev(lg), 1)
    cf = qr.corner_case(41, n_act, 1, 1, stride, kappa, batch=LOSS_GRID)
    _plant_last_blocks(cf, n_act)
    got = _fqf(L, cf, None, f, n_act, stride, 4, kappa, 0.01)
    _check_fqf(got, _fqf_want(cf, None, f, n_act, 4, kappa, 0.01), "fqf_loss batch 65539")
    # QR-DQN: N = 2
    for dueling in (False, True):
        cq = _qr_case(43, n_act, 2, 4, LOSS_GRID, dueling, False)
        cq["term"][65536], cq["act"][65537] = 1, 255
        if n_act > 1:
            cq["tgt"][65538, :n_act, :2] = F32(-3)
            cq["tgt"][65538, 0, :2] = cq["tgt"][65538, n_act - 1, :2] = F32(7)
        want = _qr_want(cq, n_act, 2, dueling, kappa)
        assert want["a_next"][65538] == 0
        _check_loss(_qr(L, cq, n_act, 2, 4, dueling, kappa), want, "qrdqn_loss batch 65539 dueling=%d" % dueling)


@pytest.mark.parametrize("n_act", [1, 3])
def test_act_kernels_and_fractions_past_block_65535(L, n_act):
    rs = np.random.RandomState(47)
    batch = ACT_GRID
    theta = _act_block(rs, batch, 1, n_act)
    ov = np.full(batch, -1, np.int32)
    ov[batch - 3] = n_act - 1                                   # an override and ...
    if n_act > 1:
        theta[batch - 2, 0, :] = F32(-1)
        theta[batch - 2, 0, 0] = theta[batch - 2, 0, n_act - 1] = F32(4)      # ... a tie in the last workgroup
    state = torch.tensor([4, 100], dtype=torch.int64, device=DEV)
    _iqn_act(L, theta, ov, n_act, 4, state=state, advance=7)
    assert state.cpu().tolist() == [4, 107]                     # advanced exactly once
    lg = qr.dominant_logits(rs, batch, 2, 4, rows=(batch - 1,))
    f = _fractions(L, _dev(lg), 2)
    print("fractions, batch %d: largest error / bound %.3f" % (batch, _check_fractions(f, lg, 2)))
    theta2 = _act_block(rs, batch, 2, n_act)
    _fqf_act(L, theta2, f["tau"], ov, n_act, 4)
    for dueling in (False, True):
        th = (rs.randn(batch, n_act + int(dueling), 4) * 2).astype(F32)
        th[:, :, 2:] = qr.POISON
        if n_act > 1:
            th[batch - 2, :n_act, :2] = F32(-1)
            th[batch - 2, 0, :2] = th[batch - 2, n_act - 1, :2] = F32(4)
        _qr_act(L, th, ov, n_act, 2, 4, dueling)


# ---- merge -------------------------------------------------------------------------------------------------------------------

def _quantised(shape, lo, hi, zero_share):
    """Multiples of 1/8 in [lo / 8, hi / 8): every product of two is exact in fp32."""
    t = torch.randint(lo, hi, shape, device=DEV, dtype=torch.int32).float() / 8
    if zero_share:
        t[torch.rand(shape, device=DEV) < zero_share] = 0.
    return t


def _equal_bits_on_device(a, b):
    COMPARED[0] += a.numel()
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def test_merge_forward_past_65536_blocks(L):
    torch.manual_seed(0)
    batch, r, f = 2049, 64, 512                                 # n4 = 2049 * 64 * 128 > 65536 * 256
    assert batch * r * (f // 4) > 65536 * 256
    psi, phi = _quantised((batch, f), 0, 32, 0.3), _quantised((batch * r, f), 0, 32, 0.3)
    o = Outs()
    x = o.new((batch * r, f))
    L.iqn_merge_fwd(psi, phi, batch, r, f, x)
    o.check()
    assert _equal_bits_on_device(x, (psi[:, None, :] * phi.view(batch, r, f)).view(batch * r, f))


def test_merge_backward_with_one_fraction_past_65536_blocks(L):
    torch.manual_seed(1)
    batch, r, f = 2049, 1, 32768                                # batch * f / 4 = 2049 * 8192 > 65536 * 256
    assert batch * (f // 4) > 65536 * 256
    psi, phi = _quantised((batch, f), 0, 32, 0.3), _quantised((batch, f), 0, 32, 0.3)
    g = _quantised((batch, f), -32, 33, 0.)
    o = Outs()
    dphi, dpsi = o.new((batch, f)), o.new((batch, f))
    L.iqn_merge_bwd(g, psi, phi, batch, r, f, dphi, dpsi)
    o.check()
    zero = torch.zeros((), device=DEV)
    assert _equal_bits_on_device(dphi, torch.where(phi > 0, g * psi, zero))
    assert _equal_bits_on_device(dpsi, torch.where(psi > 0, zero + g * phi, zero))         # (the sum starts at +0)


@pytest.mark.parametrize("b,r,f", [(1500, 3, 4), (3, 64, 12), (2, 1, 8)])
def test_merge_at_the_narrowest_row_and_with_both_masks_zero_in_the_last_row(L, b, r, f):
    psi, phi, g = _merge_case(b, r, f, seed=5)
    psi[-1, -3:], phi[-1, -2:] = 0., 0.
    psi[-1, 0], phi[-1, 0] = 0., 0.                             # both masks at one place of the last row
    o = Outs()
    x, dphi, dpsi = o.new((b * r, f)), o.new((b * r, f)), o.new((b, f))
    L.iqn_merge_fwd(_dev(psi), _dev(phi), b, r, f, x)
    L.iqn_merge_bwd(_dev(g), _dev(psi), _dev(phi), b, r, f, dphi, dpsi)
    o.check()
    want = qr.merge_bwd(g, psi, phi, r)
    _same_bits(x, qr.merge_fwd(psi, phi, r), "merge_fwd")
    _same_bits(dphi, want[0], "dphi")
    _same_bits(dpsi, want[1], "dpsi")
    p64 = (g.astype(np.float64) * phi).reshape(b, r, f).sum(axis=1)
    np.testing.assert_array_equal(_host(dpsi).astype(np.float64), np.where(psi > 0, p64, 0.))       # (_merge_case: exact sums)


@pytest.mark.parametrize("b,r,f", [(3, 64, 12), (5, 7, 4), (2, 1, 8)])
def test_merge_backward_sums_the_fractions_ascending_on_unquantised_inputs(L, b, r, f):
    """Random fp32 inputs: every product rounds and the order of the r-term sum shows in dpsi's last bits."""
    rs = np.random.RandomState(b + r + f)
    psi = np.maximum(rs.randn(b, f), 0).astype(F32)
    phi = np.maximum(rs.randn(b * r, f) * 2.0 ** rs.randint(0, 8, size=(b * r, 1)), 0).astype(F32)
    g = rs.randn(b * r, f).astype(F32)
    o = Outs()
    x, dphi, dpsi = o.new((b * r, f)), o.new((b * r, f)), o.new((b, f))
    L.iqn_merge_fwd(_dev(psi), _dev(phi), b, r, f, x)
    L.iqn_merge_bwd(_dev(g), _dev(psi), _dev(phi), b, r, f, dphi, dpsi)
    o.check()
    want = qr.merge_bwd(g, psi, phi, r)
    _same_bits(x, qr.merge_fwd(psi, phi, r), "merge_fwd")
    _same_bits(dphi, want[0], "dphi")
    _same_bits(dpsi, want[1], "dpsi")
    if r > 2:                                                   # the inputs do tell the orders apart
        rev = qr.merge_bwd(g.reshape(b, r, f)[:, ::-1].reshape(b * r, f), psi, phi.reshape(b, r, f)[:, ::-1].reshape(b * r, f), r)
        assert (qr.bits(rev[1]) != qr.bits(want[1])).any()


# ---- embed -------------------------------------------------------------------------------------------------------------------

def _embed(L, rows, r, tau_in=None, state=None, row0=0, call_offset=0):
    o = Outs()
    tau, cosf = o.new((rows * r,)), o.new((rows * r, 64))
    L.iqn_embed(_dev(tau_in), state, rows, r, tau, cosf, row0=row0, call_offset=call_offset)
    o.check()
    return _host(tau), _host(cosf)


@pytest.mark.parametrize("r,row0,rows", [(64, 2 ** 25 - 4, 3), (1, 2 ** 31 - 6, 5), (3, 2 ** 29, 3)],
                         ids=["r64-row0-2^25-4", "r1-row0-2^31-6", "r3-row0-2^29"])
def test_drawn_fractions_at_the_addressing_limits(L, r, row0, rows):
    """(row0 + rows) r = 2^31 - 64 and 2^31 - 1 (the last accepted value), and row0 r = 3 * 2^29 with r no power of two;
    e / 4 steps from one counter word to the next inside every launch."""
    seed, counter = 0x7654321 + 2 ** 35, 2 ** 33 + 11
    state = torch.tensor([seed, counter], dtype=torch.int64, device=DEV)
    e = row0 * r + np.arange(rows * r, dtype=np.int64)
    assert e[-1] < 2 ** 31 and (rows * r < 4 or len(set((e >> 2).tolist())) > 1)
    tau, cosf = _embed(L, rows, r, state=state, row0=row0)
    _same_bits(tau, ref_tau(seed, counter, e), "drawn tau")
    assert not np.array_equal(tau, ref_tau(seed, counter, np.arange(rows * r)))            # row0 is part of e
    err = np.abs(cosf - qr.cos_f64_table(tau)).max()
    print("drawn, row0 %d: largest cosine error / 2^-22 = %.3f" % (row0, err * 2 ** 22))
    assert err <= 2.0 ** -22 and (cosf[:, 0] == 1).all()
    assert state.cpu().tolist() == [seed, counter]


def test_a_negative_call_is_twos_complement(L):
    seed, rows, r = 5, 4, 5
    state = torch.tensor([seed, -3], dtype=torch.int64, device=DEV)
    tau, _ = _embed(L, rows, r, state=state, call_offset=1)
    _same_bits(tau, ref_tau(seed, -2, np.arange(rows * r)), "call -2")
    _same_bits(_embed(L, rows, r, state=state, call_offset=3)[0], ref_tau(seed, 0, np.arange(rows * r)), "call 0")
    assert not np.array_equal(tau, ref_tau(seed, 2 ** 32 - 2, np.arange(rows * r)))        # the high counter word counts


def test_given_fractions_over_the_whole_of_fp32(L):
    given = qr.tau_grid()
    tau, cosf = _embed(L, given.size, 1, tau_in=given)
    _same_bits(tau, given, "tau out == tau_in")                 # bitwise: NaN payload, sign of zero
    want = qr.cos_f64_table(given)
    err = np.abs(cosf.astype(np.float64) - want)
    worst = int(err.max(axis=1).argmax())
    print("given: %d fractions, largest cosine error / 2^-22 = %.3f (tau = %r)" % (given.size, err.max() * 2 ** 22, given[worst]))
    assert np.isfinite(cosf).all() and err.max() <= 2.0 ** -22
    assert (cosf[:, 0] == 1).all()                              # i = 0: exactly 1
    big = ~(np.abs(given) < 2.0 ** 24)                          # |tau| >= 2^24, infinities and NaN: exactly 1
    assert big.sum() >= 7 * 2 + 6 and (cosf[big] == 1).all()
    for i, x in enumerate(given):                               # an odd multiple of 1/2: exactly 0; a multiple of 1: +-1
        if np.isfinite(x) and abs(x) < 2.0 ** 24:
            ang = np.arange(64) * abs(float(x))
            half_odd = (ang * 2 == np.round(ang * 2)) & (np.round(ang * 2) % 2 == 1)
            assert (cosf[i][half_odd] == 0).all(), x
            whole = ang == np.round(ang)
            np.testing.assert_array_equal(cosf[i][whole], np.where(np.round(ang[whole]) % 2 == 0, 1., -1.).astype(F32))


# ---- loss corners, bit for bit -----------------------------------------------------------------------------------------------

N_TARGETS = (1, 2, 3, 4, 5, 63, 64)
N_PRED = (1, 63, 64)


@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("n_act,stride", [(64, 64), (1, 4)], ids=["A64", "A1"])
def test_iqn_and_miqn_loss_corners_bit_for_bit(L, n_act, stride, kappa):
    """corner_case's rows (greedy action in lane 63, a tie, actions_b = 255, is_weight 0, both priority clamps, u == 0 and
    |u| == kappa +- one ulp, tau_pred 0 and 1) at every N' x N; M-IQN at both temperatures with the bonus clipped at 0 and at l0."""
    clipped = 0
    for n in N_PRED:
        for m in N_TARGETS:
            seed = 1000 * n + 10 * m + n_act
            c = qr.corner_case(seed, n_act, n, m, stride, kappa, double=(m % 2 == 1))
            _check_loss(_iqn(L, c, n_act, stride, kappa), _iqn_want(c, n_act, kappa), "iqn_loss N=%d N'=%d" % (n, m))
            cm, T, taken = _miqn_exact_case(seed, n_act, n, m, stride, kappa)
            clipped += int((~taken).sum())
            want = qr.miqn_loss_from_targets(cm["pred"], cm["tau"], T, cm["act"], cm["isw"], n_act, kappa)
            for tau_e in mr.TAUS_E:
                _check_loss(_iqn(L, cm, n_act, stride, kappa, miqn=(tau_e, mr.ALPHA, mr.L0)), want,
                            "miqn_loss N=%d N'=%d tau_e=%g" % (n, m, tau_e))
            if n_act == 1:                                      # pi = 1, lp = 0: arl_iqn_loss's outputs
                cm["pol"] = None
                _check_loss(_iqn(L, cm, n_act, stride, kappa), want, "miqn == iqn at A = 1")
    assert (clipped > 0) == (n_act > 1)


@pytest.mark.parametrize("tau_e", mr.TAUS_E)
@pytest.mark.parametrize("kappa", [1.0, 0.0])
def test_miqn_general_soft_max_on_a_full_tile_at_a_stride_68(L, tau_e, kappa):
    """N = N' = 64 fractions x A = 64 actions, a_stride 68: the whole LDS tile, against float64 at the Munchausen bounds."""
    c = mr.miqn_case(61, 64, 64, 64, 68, 6, True)
    ratio = _check_miqn(c, mr.GAMMA, kappa, tau_e)
    print("M-IQN 64 x 64 tile, tau_e %g, kappa %g: largest gradient error / bound %.3f" % (tau_e, kappa, ratio))
    assert ratio <= 1


@pytest.mark.parametrize("tau_e", mr.TAUS_E)
def test_miqn_soft_sum_runs_over_the_actions_ascending(L, tau_e):
    """Three bit-equal maxima of Q^next: s == 3, pi = fl(1 / 3) three times, lp = -(tau_e * logf(3)).  The device's
    logf(3.f) is the one value the header does not pin; a first launch recovers it (the fp32 numbers within four ulp of
    log 3 are tried, and those under which EVERY output equals the restatement bit for bit are kept), a second launch on
    other data must then agree under it.  The soft sum has three terms of mixed magnitude: its order shows."""
    n, m, n_act, stride, kappa = 5, 64, 64, 64, 1.0
    log3 = [F32(np.log(3.))]
    for _ in range(4):
        log3 = [np.nextafter(log3[0], F32(0))] + log3 + [np.nextafter(log3[-1], F32(2))]

    def matches(c, value, descending=False):
        T = qr.three_maxima_targets(c, GAMMA, tau_e, mr.ALPHA, value, descending)
        return T, qr.miqn_loss_from_targets(c["pred"], c["tau"], T, c["act"], c["isw"], n_act, kappa)

    def agrees(got, want):
        return all(np.array_equal(qr.bits(_host(g)), qr.bits(w)) for g, w in zip(got, (want["dtheta"], want["rows"], want["pri"])))

    probe = qr.three_maxima_case(81, n, m)
    got = _iqn(L, probe, n_act, stride, kappa, miqn=(tau_e, mr.ALPHA, mr.L0))
    kept = [v for v in log3 if agrees(got, matches(probe, v)[1])]
    print("tau_e %g: logf(3) candidates that reproduce the probe launch bit for bit: %s (log 3 rounded: %r)" % (
        tau_e, [float(v) for v in kept], float(F32(np.log(3.)))))
    assert kept, "no value of logf(3) within four ulp reproduces the launch"
    for seed, mm in ((82, 64), (83, 5), (84, 2)):
        c = qr.three_maxima_case(seed, n, mm)
        got = _iqn(L, c, n_act, stride, kappa, miqn=(tau_e, mr.ALPHA, mr.L0))
        assert any(agrees(got, matches(c, v)[1]) for v in kept), "N' = %d" % mm
        up, down = matches(c, kept[0])[0], matches(c, kept[0], descending=True)[0]
        assert (qr.bits(up) != qr.bits(down)).any()             # the inputs do tell the orders apart
        for v in kept:
            if agrees(got, matches(c, v)[1]):
                _check_loss(got, matches(c, v)[1], "miqn_loss, three maxima, N' = %d" % mm)


@pytest.mark.parametrize("n_act,n,stride", [(64, 64, 64), (63, 2, 4), (64, 2, 4)])
def test_qrdqn_dueling_at_65_rows(L, n_act, n, stride):
    """A = 64 dueling: 65 rows, wave 0 takes the value row and xs[16] is full; the taken action 0 and A - 1; the value
    row's gradient and every action's share."""
    for kappa in KAPPAS:
        for double in (False, True):
            c = _qr_case(n_act + n + int(double), n_act, n, stride, 6, True, double)
            want = _qr_want(c, n_act, n, True, kappa)
            np.testing.assert_array_equal(want["a_next"], c["chosen"])
            assert want["dtheta"][:, n_act, :n].any() and want["dtheta"][0, 0, :n].any() and want["dtheta"][1, n_act - 1, :n].any()
            _check_loss(_qr(L, c, n_act, n, stride, True, kappa), want, "qrdqn_loss dueling A=%d N=%d" % (n_act, n))
        _qr_act(L, c["pred"], np.array([-1, 0, n_act - 1, -1, -1, 5 % n_act], np.int32), n_act, n, stride, True)
    plain = _qr_case(5, n_act, n, stride, 6, False, True)
    _check_loss(_qr(L, plain, n_act, n, stride, False, 1.0), _qr_want(plain, n_act, n, False, 1.0), "qrdqn_loss plain")


# ---- FQF ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_fqf_with_repeated_fractions_bit_for_bit(L, n):
    """One dominant logit: the other q_k underflow to 0, tau repeats at both ends, tau_hat is exactly 0 and 1; the same
    fractions through arl_fqf_act (a zero weight contributes an exact 0) and arl_fqf_loss (S_k, G, dlogits bit for bit)."""
    n_act, stride, n_stride, batch = 64, 64, 68, qr.CORNER_BATCH
    worst = 0.
    for kappa in KAPPAS:
        ratio, f, c, got = _fqf_at(L, 71, n_act, n, stride, n_stride, kappa, batch, dominant=(0, qr.ROW_PLAIN, qr.ROW_TIE))
        worst = max(worst, ratio)
    tau, hat, q = _host(f["tau"]), _host(f["tau_hat"]), _host(f["q"])
    if n > 2:
        for b in (0, qr.ROW_PLAIN, qr.ROW_TIE):
            assert (q[b] == 0).sum() == n - 1 and q[b, n // 2] == 1
            assert (tau[b, :n // 2 + 1] == 0).all() and (tau[b, n // 2 + 1:] == 1).all()
            assert set(hat[b].tolist()) == {0.0, 0.5, 1.0}
    theta = qr._blocks(np.random.RandomState(n), batch, n, n_act, stride, scale=1e6)
    wq = _fqf_act(L, theta, f["tau"], None, n_act, stride)
    if n > 2:
        _same_bits(wq[0], theta[0, n // 2, :n_act], "a zero weight contributes an exact 0")
    print("FQF N %d: fractions' largest error / bound %.3f" % (n, worst))
    if n == 1:
        assert not _host(got[3]).any() and not _host(got[4]).any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def test_first_refused_values_launch_nothing(L):
    """The last accepted values run elsewhere in this file: stride 2^20 (the stride tests), (row0 + rows) r = 2^31 - 1
    (the drawn-fraction test), 64 actions and 64 fractions (the corner tests), n_quantiles 2 (the QR-DQN tests); f = 2^24
    runs below.  batch x r x f = 2^40 and batch x (N + 1) = 2^31 - 1 need buffers out of this suite's reach."""
    lib = L.load()
    o = Outs()
    batch = 2
    theta = torch.zeros(batch * 66 * 68 + 8, device=DEV)
    act = torch.zeros(batch, dtype=torch.uint8, device=DEV)
    vec = torch.zeros(batch * 70, device=DEV)
    state = torch.tensor([1, 5], dtype=torch.int64, device=DEV)
    dth, rows, pri, frac = o.new((batch * 66 * 68,)), o.new((batch,)), o.new((batch,)), o.new((batch,))
    onehot, greedy = o.new((batch, 66)), o.new((batch,), torch.uint8)
    dlg, tau, hat, cosf = o.new((batch, 72)), o.new((batch * 70,)), o.new((batch * 70,)), o.new((batch * 66, 64))
    x, dphi, dpsi = o.new((batch * 66 * 8,)), o.new((batch * 66 * 8,)), o.new((batch * 8,))
    p = lambda t: t.data_ptr()                                  # noqa: E731
    th = p(theta)
    too_wide = BIG + 4

    def iqn_loss(b=batch, s=8):
        return lib.arl_iqn_loss(th, p(vec), th, None, p(act), p(vec), p(act), None, b, 6, 8, 8, s, 0.99, 1.0, p(dth), p(rows),
                                p(pri), p(state), 3, None)

    def miqn_loss(b=batch, s=8):
        return lib.arl_miqn_loss(th, p(vec), th, th, p(act), p(vec), p(act), None, b, 6, 8, 8, s, 0.99, 1.0, 0.03, 0.9, -1.0,
                                 p(dth), p(rows), p(pri), p(state), 3, None)

    def iqn_act(b=batch, s=8):
        return lib.arl_iqn_act(th, None, b, 6, 8, s, p(onehot), p(greedy), p(state), 3, None)

    def fqf_act(b=batch, s=8, k=8):
        return lib.arl_fqf_act(th, p(vec), None, b, 6, k, s, p(onehot), p(greedy), None)

    def fqf_loss(b=batch, s=8, ns=8, n=8, mid=th):
        return lib.arl_fqf_loss(th, mid, p(vec), p(vec), p(vec), p(vec), p(vec), th, None, p(act), p(vec), p(act), None, b, 6, n,
                                s, ns, 0.99, 1.0, 0.0, p(dth), p(rows), p(pri), p(dlg), p(frac), None)

    def fractions(b=batch, ns=8, n=8):
        return lib.arl_fqf_fractions(th, b, n, ns, p(tau), p(hat), None, None, None, None, None)

    def qr_loss(b=batch, s=8):
        return lib.arl_qrdqn_loss(th, th, None, p(act), p(vec), p(act), None, b, 6, 8, s, 0, 0.99, 1.0, p(dth), p(rows), p(pri),
                                  None)

    def qr_act(b=batch, s=8):
        return lib.arl_qrdqn_act(th, None, b, 6, 8, s, 0, p(onehot), p(greedy), None)

    def embed(row0=0, rows=batch, r=8, cf=p(cosf)):
        return lib.arl_iqn_embed(None, p(state), row0, 0, rows, r, p(tau), cf, None)

    def fwd(b=batch, r=8, f=8, ps=th, ph=th, out=p(x)):
        return lib.arl_iqn_merge_fwd(ps, ph, b, r, f, out, None)

    def bwd(b=batch, r=8, f=8, g=th, ps=th, ph=th, o1=p(dphi), o2=p(dpsi)):
        return lib.arl_iqn_merge_bwd(g, ps, ph, b, r, f, o1, o2, None)

    for call in (iqn_loss, miqn_loss, iqn_act, fqf_act, fqf_loss):
        assert call(s=too_wide) == E_ARG and b"a_stride" in lib.arl_last_error(), call.__name__
        assert call(b=2 ** 31) == E_ARG, call.__name__
    assert fqf_loss(ns=too_wide) == E_ARG and fractions(ns=too_wide) == E_ARG and b"n_stride" in lib.arl_last_error()
    for call in (qr_loss, qr_act):
        assert call(s=too_wide) == E_RANGE and b"q_stride" in lib.arl_last_error()
        assert call(b=2 ** 31) == E_RANGE
    # batch x (N + 1) = 2^31
    assert fractions(b=2 ** 30, n=1, ns=4) == E_ARG and fqf_act(b=2 ** 30, k=1) == E_ARG
    assert fqf_loss(b=2 ** 30, n=1, mid=None) == E_ARG and b"fractions + 1" in lib.arl_last_error()
    assert fractions(b=2 ** 31 // 65 + 1, n=64, ns=64) == E_ARG
    # (row0 + rows) x r = 2^31
    assert embed(row0=2 ** 31 - 5, rows=5, r=1) == E_ARG and b"2^31" in lib.arl_last_error()
    assert embed(row0=2 ** 25 - 3, rows=3, r=64) == E_ARG and embed(row0=2 ** 31, rows=1, r=1) == E_ARG
    # f = 2^24 + 4; batch x r x f > 2^40 with every factor inside its own limit
    for call in (fwd, bwd):
        assert call(b=1, r=1, f=2 ** 24 + 4) == E_ARG and b"2^24" in lib.arl_last_error()
        assert call(b=2 ** 10 + 1, r=64, f=2 ** 24) == E_ARG
        assert call(b=2 ** 25, r=64, f=4) == E_ARG              # batch x r = 2^31
    # misaligned vector operands
    assert embed(cf=p(cosf) + 4) == E_ALIGN and b"alignment" in lib.arl_last_error()
    assert fwd(ps=th + 4) == E_ALIGN and fwd(ph=th + 8) == E_ALIGN and fwd(out=p(x) + 4) == E_ALIGN
    assert bwd(g=th + 4) == E_ALIGN and bwd(ps=th + 4) == E_ALIGN and bwd(ph=th + 12) == E_ALIGN
    assert bwd(o1=p(dphi) + 4) == E_ALIGN and bwd(o2=p(dpsi) + 8) == E_ALIGN
    assert o.untouched() and state.cpu().tolist() == [1, 5]
    # inside the limits the same calls run
    for call in (iqn_loss, miqn_loss, iqn_act, fqf_act, fqf_loss, fractions, qr_loss, qr_act, embed, fwd, bwd):
        assert call() == 0, call.__name__
    o.check()
    assert state.cpu().tolist() == [1, 14] and not o.untouched()


def test_the_widest_accepted_merge_row(L):
    """f = 2^24, the last accepted width, with one sample and one fraction."""
    torch.manual_seed(2)
    f = 1 << 24
    psi, phi, g = _quantised((1, f), 0, 32, 0.3), _quantised((1, f), 0, 32, 0.3), _quantised((1, f), -32, 33, 0.)
    o = Outs()
    x, dphi, dpsi = o.new((1, f)), o.new((1, f)), o.new((1, f))
    L.iqn_merge_fwd(psi, phi, 1, 1, f, x)
    L.iqn_merge_bwd(g, psi, phi, 1, 1, f, dphi, dpsi)
    o.check()
    zero = torch.zeros((), device=DEV)
    assert _equal_bits_on_device(x, psi * phi)
    assert _equal_bits_on_device(dphi, torch.where(phi > 0, g * psi, zero))
    assert _equal_bits_on_device(dpsi, torch.where(psi > 0, zero + g * phi, zero))
