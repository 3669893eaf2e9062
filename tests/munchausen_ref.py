"""Shared by tests/test_munchausen_host.py and tests/test_munchausen_gpu.py: the input cases, the float64 restatements
of arl_mdqn_loss / arl_miqn_loss (include/accel_rl_hip.h), NumPy fp32 emulations of both target computations in the
kernels' stated order, and the derived error bounds.

Bounds (EPS = 2^-24; the derivation is repeated in DESIGN.md, section 16).

M-DQN, y_b (hence d_b):  atol_b = (A + 32) EPS M_b,
M_b = |returns_b| + alpha |l0| + gamma_n (max_a |q^next_a| + tau_e ln A).
soft_b = sum_a pi_a (q_a - lp_a) is an A-term fp32 sum of terms whose magnitudes sum to at most
max|q^next| + tau_e ln A (q_a - lp_a = v + tau_e log s for every a): A EPS M for the chain.  Errors of pi_a -- expf and
logf at the OpenCL full-profile 3 ulp each, the rounding of c_a / tau_e -- enter only through sum_a pi_a, which stays
1 within a few EPS per term, because the factor they multiply is the same for every a; they and the handful of
roundings in lp and y are the 32.  Dueling rows: M_b knows the merged q = val + (adv - mean adv), so the bound holds
where val and adv are of its size (the merge's own rounding is EPS (|val| + |adv|)), not where two large streams
cancel; the large-value cases are therefore plain rows.  td_abs = min(|d|, delta_clip) and the slope clip(d) are
1-Lipschitz in d: the same bound; loss_rows: the bound times w_b |slope_b| (plus the second-order term and 4 EPS of the
row itself, the fp32 operations from d to the row); dq: max_b w_b times the bound, plus rtol 1e-5.

M-IQN, T_j:  atol_bj = 2 EPS [ (A + 32) M_bj + gamma_n (N' + 1) max|tgt_next_b| D_bj / tau_e ],
M_bj = |returns_b| + alpha |l0| + gamma_n sum_a pi_a |tgt_next(j, a) - lp_a|,  D_bj = sum_a pi_a |c_ja - S_j| with
c_ja = tgt_next(j, a) - lp_a and S_j = sum_a pi_a c_ja, all from the float64 reference.  The first term is M-DQN's.
The second is new: here the factor c_ja is NOT the same for every a, so an error delta Q_a of the N'-term fp32 mean
Q^next_a (at most (N' + 1) EPS max|tgt_next_b|) moves pi_a by pi_a (delta Q_a - sum pi delta Q) / tau_e, and soft_j by
at most max|delta Q| D_bj / tau_e to first order; the factor 2 covers second order and the library functions.
Gradient: arl_iqn_loss's bound with max_j atol_bj in place of the rounding of T:
(N' + 8) EPS max_b w_b + max_j atol_bj max_b w_b / kappa, plus rtol 2e-4 (kappa == 0: the gradient depends on T only
through [u < 0], which min_ij |u_bij| > 16 max_j atol_bj, asserted for every sample, pins).  loss_rows / priorities:
rtol 2e-4 plus N max_j atol_bj (|d rho / d u| <= 1, N x N' pairs over N') times w_b."""
import numpy as np
import torch

EPS = 2.0 ** -24
POISON = 1e9                    # what the padding columns of every input hold: they must be ignored
F32 = np.float32
GAMMA = float(np.float32(0.99))
ALPHA, L0 = 0.9, -1.0

# special rows, by (row + shift) % N_KINDS: the shift makes every kind appear in the batch-1 cases too
PLAIN, CLIPPED, LP_ZERO, TWO_MAXIMA, ALL_EQUAL, CLOSE = range(6)
N_KINDS = 6


def _kinds(batch, shift):
    return (np.arange(batch) + shift) % N_KINDS


# ---- M-DQN ----------------------------------------------------------------------------------------------------------

def mdqn_case(seed, n_act, batch, dueling, weighted, scale=2.0, shift=0):
    """q, tgt_next, tgt_cur f32[B][S] (dueling: n_act advantages, then the value), poison in the padding.  Planted rows:
    CLIPPED (the taken action far below the maximum of tgt_cur: lp < l0), LP_ZERO (the taken action the maximum of
    tgt_cur by a wide gap: lp == 0), TWO_MAXIMA (two equal maxima in tgt_next and tgt_cur), ALL_EQUAL (pi uniform),
    CLOSE (values within a few tau_e: lp strictly between l0 and 0); terminal rows by rs and at rows 0 / 1."""
    rs = np.random.RandomState(seed)
    cols = n_act + int(dueling)
    stride = (cols + 3) // 4 * 4
    kinds = _kinds(batch, shift)

    def rows():
        t = (rs.randn(batch, stride) * scale).astype(F32)
        t[:, cols:] = POISON
        return t
    q, nxt, cur = rows(), rows(), rows()
    act = rs.randint(0, n_act, size=batch).astype(np.uint8)
    for b in range(batch):
        k, a0 = kinds[b], int(act[b])
        other = (a0 + 1) % n_act
        if k == CLIPPED:
            cur[b, a0] = cur[b, :n_act].min() - F32(25 * scale)
        elif k == LP_ZERO:
            cur[b, a0] = cur[b, :n_act].max() + F32(50 * scale)
            nxt[b, other] = nxt[b, :n_act].max() + F32(50 * scale)
        elif k == TWO_MAXIMA:
            top = F32(np.abs(cur[b, :n_act]).max() + scale)
            cur[b, a0] = cur[b, other] = top
            nxt[b, a0] = nxt[b, other] = F32(np.abs(nxt[b, :n_act]).max() + 0.5 * scale)
        elif k == ALL_EQUAL:
            cur[b, :n_act] = cur[b, 0]
            nxt[b, :n_act] = nxt[b, 0]
        elif k == CLOSE:
            cur[b, :n_act] = cur[b, 0] + (rs.rand(n_act) * 0.05).astype(F32)
            nxt[b, :n_act] = nxt[b, 0] + (rs.rand(n_act) * 0.05).astype(F32)
    ret = (rs.randn(batch) * 3).astype(F32)
    term = (rs.rand(batch) < 0.3).astype(np.uint8)
    if batch > 1:
        term[0], term[1] = 1, 0
    else:
        term[0] = shift & 1
    isw = (rs.rand(batch) + 0.1).astype(F32) if weighted else None
    return dict(q=q, nxt=nxt, cur=cur, act=act, ret=ret, term=term, isw=isw, kinds=kinds, n_act=n_act,
                dueling=bool(dueling))


def soft64(q, tau_e):
    """float64 [..., A] -> (lp = tau_e log pi, pi)."""
    c = q - q.max(dim=-1, keepdim=True).values
    lp = c - tau_e * torch.logsumexp(c / tau_e, dim=-1, keepdim=True)
    return lp, torch.softmax(c / tau_e, dim=-1)


def _merge64(rows, n_act, dueling):
    adv = rows[:, :n_act]
    return rows[:, n_act:n_act + 1] + (adv - adv.mean(dim=1, keepdim=True)) if dueling else adv


def huber64(d, clip):
    if clip and clip > 0:
        ad = d.abs()
        return torch.where(ad <= clip, 0.5 * d * d, clip * (ad - clip / 2.))
    return 0.5 * d * d


def ref_mdqn(c, gamma_n, delta_clip, tau_e, alpha=ALPHA, l0=L0):
    """float64.  Returns y, d, rows (w_b loss_b), td, grad (d sum(rows) / d the stored q rows, autograd), w, slope,
    lp_act, atol (the bound on y per row)."""
    n_act, dueling = c["n_act"], c["dueling"]
    cols = n_act + int(dueling)
    t64 = lambda x: torch.from_numpy(x[:, :cols].astype(np.float64))                    # noqa: E731
    qrows = t64(c["q"]).requires_grad_()
    q, qn, qc = (_merge64(r, n_act, dueling) for r in (qrows, t64(c["nxt"]), t64(c["cur"])))
    batch = q.shape[0]
    ar, act = torch.arange(batch), torch.from_numpy(c["act"]).long()
    lpn, pin = soft64(qn, tau_e)
    lp_act = soft64(qc, tau_e)[0][ar, act]
    ret, keep = torch.from_numpy(c["ret"]).double(), 1. - torch.from_numpy(c["term"]).double()
    soft = (pin * (qn - lpn)).sum(dim=1)
    y = (ret + alpha * lp_act.clamp(l0, 0.)) + keep * (gamma_n * soft)
    d = y - q[ar, act]
    w = (torch.from_numpy(c["isw"]).double() if c["isw"] is not None else torch.ones(batch, dtype=torch.float64)) / batch
    rows = w * huber64(d, delta_clip)
    grad, = torch.autograd.grad(rows.sum(), qrows)
    dd = d.detach()
    clipped = bool(delta_clip) and delta_clip > 0
    big = ret.abs() + alpha * abs(l0) + gamma_n * (qn.abs().max(dim=1).values + tau_e * np.log(n_act))
    return dict(y=y.detach(), d=dd, rows=rows.detach(), td=dd.abs().clamp(max=delta_clip) if clipped else dd.abs(),
                grad=grad, w=w, slope=dd.clamp(-delta_clip, delta_clip) if clipped else dd, lp_act=lp_act,
                atol=(n_act + 32) * EPS * big, soft=soft)


def _exp32(x):
    return np.exp(x.astype(np.float64)).astype(F32)             # correctly rounded expf of an fp32 argument


def _log32(x):
    return np.log(x.astype(np.float64)).astype(F32)


def _merge32(rows, n_act, dueling):
    """q_at of csrc/dqn.hip in fp32: row_mean sums a ascending from 0."""
    adv = rows[:, :n_act].astype(F32)
    if not dueling:
        return adv
    s = np.zeros(rows.shape[0], F32)
    for a in range(n_act):
        s = s + adv[:, a]
    mean = s / F32(n_act)
    return rows[:, n_act:n_act + 1].astype(F32) + (adv - mean[:, None])


def _soft_row32(q, tau_e):
    """v, s (a ascending, from 0), tl = tau_e logf(s) of fp32 rows [B][A], every operation rounded to fp32."""
    te = F32(tau_e)
    v = q.max(axis=1)
    s = np.zeros(q.shape[0], F32)
    for a in range(q.shape[1]):
        s = s + _exp32((q[:, a] - v) / te)
    return v, s, te * _log32(s)


def emu_mdqn_y(c, gamma_n, tau_e, alpha=ALPHA, l0=L0):
    """y_b of mdqn_loss_kernel, operation by operation in fp32 (exp / log correctly rounded)."""
    n_act, dueling = c["n_act"], c["dueling"]
    te = F32(tau_e)
    qn, qc = _merge32(c["nxt"], n_act, dueling), _merge32(c["cur"], n_act, dueling)
    v, s, tl = _soft_row32(qn, tau_e)
    soft = np.zeros(qn.shape[0], F32)
    for a in range(n_act):
        ck = qn[:, a] - v
        soft = soft + (_exp32(ck / te) / s) * (qn[:, a] - (ck - tl))
    vc, _, tlc = _soft_row32(qc, tau_e)
    lp = (qc[np.arange(qc.shape[0]), c["act"]] - vc) - tlc
    bonus = F32(alpha) * np.minimum(np.maximum(lp, F32(l0)), F32(0))
    keep = np.where(c["term"] != 0, F32(0), F32(1))
    y = (c["ret"] + bonus) + keep * (F32(gamma_n) * soft)
    assert y.dtype == F32
    return y


# ---- M-IQN ----------------------------------------------------------------------------------------------------------

def miqn_case(seed, n, m, n_act, stride, batch, weighted, scale=2.0, shift=0):
    """pred f32[B][N][S] at fractions tau f32[B][N]; tgt_next, tgt_cur f32[B][N'][S]; the special rows of mdqn_case,
    planted in whole columns so that they hold for Q = the mean over the fractions."""
    rs = np.random.RandomState(seed)
    kinds = _kinds(batch, shift)

    def block(r):
        t = (rs.randn(batch, r, stride) * scale).astype(F32)
        t[:, :, n_act:] = POISON
        return t
    pred, nxt, cur = block(n), block(m), block(m)
    act = rs.randint(0, n_act, size=batch).astype(np.uint8)
    for b in range(batch):
        k, a0 = kinds[b], int(act[b])
        other = (a0 + 1) % n_act
        if k == CLIPPED:
            cur[b, :, a0] -= F32(25 * scale)
        elif k == LP_ZERO:
            cur[b, :, a0] += F32(50 * scale)
            nxt[b, :, other] += F32(50 * scale)
        elif k == TWO_MAXIMA:
            cur[b, :, other] = cur[b, :, a0]
            nxt[b, :, other] = nxt[b, :, a0]
            for t in (cur, nxt):
                t[b, :, a0] += F32(2 * scale)
                t[b, :, other] += F32(2 * scale)
        elif k == ALL_EQUAL:
            cur[b, :, :n_act] = cur[b, :, :1]
            nxt[b, :, :n_act] = nxt[b, :, :1]
        elif k == CLOSE:
            cur[b, :, :n_act] = cur[b, :, :1] + (rs.rand(n_act) * 0.05).astype(F32)
            nxt[b, :, :n_act] = nxt[b, :, :1] + (rs.rand(m, n_act) * 0.05).astype(F32)
    tau = rs.uniform(0.02, 0.98, size=(batch, n)).astype(F32)
    ret = (rs.randn(batch) * 3).astype(F32)
    term = (rs.rand(batch) < 0.3).astype(np.uint8)
    if batch > 1:
        term[0], term[1] = 1, 0
    else:
        term[0] = shift & 1
    isw = (rs.rand(batch) + 0.1).astype(F32) if weighted else None
    return dict(pred=pred, tau=tau, nxt=nxt, cur=cur, act=act, ret=ret, term=term, isw=isw, kinds=kinds, n_act=n_act)


def ref_miqn_targets(c, gamma_n, tau_e, alpha=ALPHA, l0=L0):
    """float64: T [B][N'], its bound atol [B][N'], lp_act [B]."""
    n_act = c["n_act"]
    nxt = torch.from_numpy(c["nxt"][:, :, :n_act].astype(np.float64))
    cur = torch.from_numpy(c["cur"][:, :, :n_act].astype(np.float64))
    batch, m, _ = nxt.shape
    ar, act = torch.arange(batch), torch.from_numpy(c["act"]).long()
    lpn, pin = soft64(nxt.sum(dim=1) / m, tau_e)
    lp_act = soft64(cur.sum(dim=1) / m, tau_e)[0][ar, act]
    ret, keep = torch.from_numpy(c["ret"]).double(), 1. - torch.from_numpy(c["term"]).double()
    cja = nxt - lpn[:, None, :]                                                         # [B][j][a]
    soft = (pin[:, None, :] * cja).sum(dim=2)
    T = (ret + alpha * lp_act.clamp(l0, 0.))[:, None] + keep[:, None] * (gamma_n * soft)
    big = (ret.abs() + alpha * abs(l0))[:, None] + gamma_n * (pin[:, None, :] * cja.abs()).sum(dim=2)
    spread = (pin[:, None, :] * (cja - soft[:, :, None]).abs()).sum(dim=2)
    top = nxt.abs().amax(dim=(1, 2))
    atol = 2 * EPS * ((n_act + 32) * big + gamma_n * (m + 1) * top[:, None] * spread / tau_e)
    return dict(T=T, atol=atol, lp_act=lp_act)


def place_pred_away_from_targets(c, ref, n_slots=3):
    """For the kappa == 0 cases, whose indicator [u < 0] is discontinuous: move the taken action's predicted quantiles
    to the middles of the widest gaps between the sample's targets T_b (gaps of at least 64 max_j atol_bj only) and to
    a step of at least 1 below / above all of them, so that min |u| is at least 32 times the bound on T whatever the
    seed.  ref: ref_miqn_targets' result.  Both signs of u still occur (N > 1)."""
    n = c["pred"].shape[1]
    for b in range(ref["T"].shape[0]):
        t = np.unique(ref["T"][b].numpy())
        floor = 32 * ref["atol"][b].max().item()
        step = max(1., 2 * floor)
        slots = [t[0] - step, t[-1] + step]
        gaps = np.diff(t)
        for g in np.argsort(-gaps)[:n_slots]:
            if gaps[g] >= max(0.05, 2 * floor):
                slots.append(0.5 * (t[g] + t[g + 1]))
        c["pred"][b, :, int(c["act"][b])] = [F32(slots[i % len(slots)]) for i in range(n)]


def ref_miqn(c, gamma_n, kappa, tau_e, alpha=ALPHA, l0=L0):
    """float64: rows, loss_b, grad [B][N][A] (autograd where kappa > 0, the closed form where kappa == 0), T, atol, u, w."""
    n_act = c["n_act"]
    ref = ref_miqn_targets(c, gamma_n, tau_e, alpha, l0)
    pred = torch.from_numpy(c["pred"][:, :, :n_act].astype(np.float64)).requires_grad_()
    tau = torch.from_numpy(c["tau"].astype(np.float64))
    batch, n, _ = pred.shape
    m = ref["T"].shape[1]
    ar, act = torch.arange(batch), torch.from_numpy(c["act"]).long()
    u = ref["T"][:, None, :] - pred[ar, :, act][:, :, None]                             # [B][i][j]
    ind = (u < 0).double()
    wt = (tau[:, :, None] - ind).abs().detach()
    w = (torch.from_numpy(c["isw"]).double() if c["isw"] is not None else torch.ones(batch, dtype=torch.float64)) / batch
    if kappa > 0:
        au = u.abs()
        rho = wt * torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa
    else:
        rho = wt * u.abs()
    loss_b = rho.sum(dim=(1, 2)) / m
    rows = w * loss_b
    if kappa > 0:
        grad, = torch.autograd.grad(rows.sum(), pred)
    else:
        grad = torch.zeros_like(pred)
        grad[ar, :, act] = -(tau[:, :, None] - ind).sum(dim=2).detach() * (w / m)[:, None]
    ref.update(rows=rows.detach(), loss_b=loss_b.detach(), grad=grad, u=u.detach(), w=w)
    return ref


def _butterfly(v, op):
    """wave_sum / wave_max over the last axis of 64 lanes: lane ^ 32, ^ 16, ... ^ 1, every step rounded to fp32."""
    lanes = np.arange(64)
    for mask in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., lanes ^ mask])
    return v


def emu_miqn_targets(c, gamma_n, tau_e, alpha=ALPHA, l0=L0):
    """T_j of iqn.hip's mloss_kernel, operation by operation in fp32 (exp / log correctly rounded)."""
    n_act = c["n_act"]
    te = F32(tau_e)
    batch, m, _ = c["nxt"].shape

    def stats(theta):
        q = np.zeros((batch, 64), F32)
        for j in range(m):                                      # q_of_lane: j ascending, from 0
            q[:, :n_act] = q[:, :n_act] + theta[:, j, :n_act]
        q = q / F32(m)
        valid = np.arange(64) < n_act
        v = _butterfly(np.where(valid, q, F32(-np.inf)), np.maximum)
        cc = q - v
        e = np.where(valid, _exp32(np.where(valid, cc, F32(0)) / te), F32(0))
        s = _butterfly(e, lambda x, y: x + y)
        return cc - te * _log32(s), e / s
    lpn, pin = stats(c["nxt"])
    lpc, _ = stats(c["cur"])
    act = np.minimum(c["act"], n_act - 1)
    bonus = F32(alpha) * np.minimum(np.maximum(lpc[np.arange(batch), act], F32(l0)), F32(0))
    soft = np.zeros((batch, m), F32)
    for a in range(n_act):
        soft = soft + pin[:, a:a + 1] * (c["nxt"][:, :, a] - lpn[:, a:a + 1])
    keep = np.where(c["term"] != 0, F32(0), F32(1))
    T = (c["ret"] + bonus)[:, None] + keep[:, None] * (F32(gamma_n) * soft)
    assert T.dtype == F32
    return T


# shapes of the GPU tests, shared with the host test's emulation
MDQN_ACTIONS = (1, 2, 6, 18, 255)
MDQN_BATCHES = (1, 33, 257)
MIQN_SHAPES = ((1, 1, 1, 4), (5, 7, 3, 32), (8, 8, 6, 32), (64, 64, 18, 32), (32, 64, 64, 64))     # N, N', A, a_stride
MIQN_BATCHES = (1, 3)
TAUS_E = (0.03, 1.0)


def mdqn_seed(n_act, batch, dueling, weighted):
    return 1000 * n_act + 10 * batch + 2 * int(dueling) + int(weighted)


def miqn_seed(shape, batch, weighted):
    return 100 * shape[0] + 10 * shape[2] + 2 * batch + int(weighted)
