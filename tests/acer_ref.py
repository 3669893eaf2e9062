"""Shared by tests/test_acer_host.py and tests/test_acer_gpu.py: NumPy restatements of the four entry points of
csrc/acer.hip from the text of include/accel_rl_hip.h -- per row, in the stated order -- the input cases, and the derived
error bound of arl_acer_loss.

What is bit for bit.  arl_acer_retrace_scan is float64 from its promoted inputs on (no device-library call): retrace()
equals it bit for bit.  arl_acer_avg_step is three fp32 operations: avg_step() equals it bit for bit.  arl_acer_loss is
float64 AFTER the fp32 soft-max rows (pi, lp, pibar); where a row's expf / logf results are all exactly 0 or 1 -- one
action, or one logit ahead by more than 104 (expf(-104) == 0 in fp32, s == 1, logf(1) == 0) -- soft32() reproduces those
rows exactly and loss() equals the kernel bit for bit.

The bound elsewhere (EPS = 2^-24).  The device's fp32 soft-max differs from the exact one by at most
    u_pi_a = 2 (A + 8) EPS (1 + |c_a|) pi_a + 2^-126,     u_lp_a = 2 (A + 8) EPS (1 + |lp_a|)
(tests/sacd_ref.py derives both: 2 A + 16 roundings, expf / logf counted at 3 ulp, the rounding of c_a = z_a - m moving
e_a by |c_a| EPS, logf turning s's relative error into an absolute one).  Everything after is float64 and adds less than
2^-45 relative.  The outputs are piecewise-smooth functions F of x = (pi, lp, pibar); to first order
    |F(x + dx) - F(x)| <= sum_i |dF / dx_i| u_i
and loss_bound() evaluates exactly that sum with the Jacobian of the float64 restatement (torch autograd on the host, one
backward pass per output column), doubles it for the second-order term and the kinks of min / max (both continuous), and
adds the final rounding to fp32, 2 EPS |F| + 2^-126.  The factor 1 / (pi + 1e-6) -- up to 1e6 -- is inside the Jacobian,
not guessed."""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -126
AC_EPS = 1e-6
F32 = np.float32
POISON = 1e9                    # what padding columns of inputs hold: they must be ignored


def half_stride(n_act):
    return (n_act + 31) // 32 * 32


# ---------------------------------------------------------------- soft-max rows

def soft32(z):
    """fp32 [B][A] logits -> (pi, lp, c) in fp32 by the header's operations (numpy's exp / log stand in for expf / logf:
    equal where the results are exactly 0 or 1)."""
    z = np.asarray(z, F32)
    m = z.max(axis=1, keepdims=True)
    c = (z - m).astype(F32)
    e = np.exp(c).astype(F32)
    s = np.zeros((z.shape[0], 1), F32)
    for a in range(z.shape[1]):
        s = (s + e[:, a:a + 1]).astype(F32)
    tl = np.log(s).astype(F32)
    return (e / s).astype(F32), (c - tl).astype(F32), c


def soft64(z):
    z = np.asarray(z, np.float64)
    c = z - z.max(axis=1, keepdims=True)
    e = np.exp(c)
    s = e.sum(axis=1, keepdims=True)
    return e / s, c - np.log(s), c


def soft_exact(z):
    """True for the rows of z whose fp32 soft-max involves no expf / logf result other than exact 0 or 1."""
    z = np.asarray(z, np.float64)
    c = z - z.max(axis=1, keepdims=True)
    return ((c == 0).sum(axis=1) == 1) & ((c == 0) | (c < -104)).all(axis=1)


# ---------------------------------------------------------------- Retrace scan

def retrace(prob, prob_last, q, q_last, old_prob, actions, rewards, dones, discount, lam, n_env, horizon):
    """-> (qret f32[n_env * T], v f32[n_env * T], stats f32[n_env][2]); q, q_last: [rows][>= A], the first A columns."""
    A = prob.shape[1]
    P, PL, MU = prob.astype(np.float64), prob_last.astype(np.float64), old_prob.astype(np.float64)
    Q, QL = q[:, :A].astype(np.float64), q_last[:, :A].astype(np.float64)

    def value(p, qq):
        v = np.zeros(p.shape[0])
        for a in range(A):
            v = v + p[:, a] * qq[:, a]
        return v
    V, VL = value(P, Q), value(PL, QL)
    T = horizon
    qret_out, stats = np.zeros(n_env * T, F32), np.zeros((n_env, 2), F32)
    r64 = rewards.astype(np.float64)
    for e in range(n_env):
        qret, rho_sum, above = VL[e], 0.0, 0
        for t in range(T - 1, -1, -1):
            row = e * T + t
            a = min(int(actions[row]), A - 1)
            qret = r64[row] + (0.0 if dones[row] else discount * qret)
            qret_out[row] = F32(qret)
            rho = P[row, a] / (MU[row, a] + AC_EPS)
            cbar = lam * (rho if rho < 1.0 else 1.0)
            qret = cbar * (qret - Q[row, a]) + V[row]
            rho_sum = rho_sum + rho
            above += int(rho > 1.0)
        stats[e] = (F32(rho_sum), F32(above))
    return qret_out, V.astype(F32), stats


def scan_case(seed, n_env, horizon, n_act, q_stride, done_at=None, mu_zero=False, act255=False):
    """Inputs of one scan; q / q_last are [rows][q_stride] with poison past the actions."""
    rs = np.random.RandomState(seed)
    steps = n_env * horizon

    def probs(n):
        p = rs.rand(n, n_act).astype(np.float64) + 0.05
        return (p / p.sum(axis=1, keepdims=True)).astype(F32)

    def qrows(n):
        t = np.full((n, q_stride), POISON, F32)
        t[:, :n_act] = (rs.randn(n, n_act) * 2).astype(F32)
        return t
    c = dict(prob=probs(steps), prob_last=probs(n_env), q=qrows(steps), q_last=qrows(n_env), old_prob=probs(steps),
             actions=rs.randint(0, n_act, size=steps).astype(np.uint8), rewards=rs.randn(steps).astype(F32),
             dones=np.zeros(steps, np.uint8), n_env=n_env, horizon=horizon)
    if done_at is not None:
        c["dones"].reshape(n_env, horizon)[:, done_at] = 1
    if mu_zero:
        c["old_prob"][::2] = 0
    if act255:
        c["actions"][::3] = 255
    return c


def discounted_return(rewards, dones, last_v, discount, n_env, horizon):
    """The plain discounted bootstrapped return in float64 (what Retrace reduces to on-policy with Q flat in a)."""
    out = np.zeros(n_env * horizon)
    for e in range(n_env):
        R = float(last_v[e])
        for t in range(horizon - 1, -1, -1):
            row = e * horizon + t
            R = float(rewards[row]) + (0.0 if dones[row] else discount * R)
            out[row] = R
    return out


# ---------------------------------------------------------------- head loss

def loss_core(xp, pi, lp, pibar, Q, mu, act, qret, c, delta, q_coeff, ent_coeff, batch):
    """The header's float64 arithmetic on [B][A] arrays of module xp (numpy, or torch for the Jacobian); act int64[B].
    -> dict(dz [B][A], dq [B], stats [5][B], g, k, zs, s)."""
    A = pi.shape[1]
    rows = xp.arange(pi.shape[0])
    hot = [(act == a) for a in range(A)]
    zero = 0.0 * qret
    V = zero
    for a in range(A):
        V = V + pi[:, a] * Q[:, a]
    adv = qret - V
    P_t, L_t, Q_t = pi[rows, act], lp[rows, act], Q[rows, act]
    rho_t = P_t / (mu[rows, act] + AC_EPS)
    f = xp.where(rho_t < c, rho_t, c + zero) * adv
    g, k, w = [], [], []
    for a in range(A):
        rho = pi[:, a] / (mu[:, a] + AC_EPS)
        if c == float("inf"):                   # 1 - inf = -inf -> 0.0; said outright so that autograd sees no 0 * inf
            wa = zero
        else:
            wa = 1.0 - c / (rho + AC_EPS)
            wa = xp.where(wa > 0.0, wa, zero)
        t1 = xp.where(hot[a], f / (pi[:, a] + AC_EPS), zero)
        g.append((t1 + wa * (Q[:, a] - V)) - ent_coeff * (lp[:, a] + 1.0))
        k.append(-(pibar[:, a] / (pi[:, a] + AC_EPS)))
        w.append(wa)
    kg, kk, obj, ent = zero, zero, f * L_t, zero
    for a in range(A):
        kg = kg + k[a] * g[a]
        kk = kk + k[a] * k[a]
        obj = obj + ((w[a] * (Q[:, a] - V)) * pi[:, a]) * lp[:, a]
        ent = ent + pi[:, a] * lp[:, a]
    live = kk > 0.0
    if delta == float("inf"):                   # (kg - inf) / kk = -inf -> 0.0 (as above)
        s = zero
    else:
        s = (kg - delta) / xp.where(live, kk, 1.0 + zero)
        s = xp.where(live & (s > 0.0), s, zero)
    zs = [g[a] - s * k[a] for a in range(A)]
    pz = zero
    for a in range(A):
        pz = pz + pi[:, a] * zs[a]
    dz = xp.stack([-(pi[:, j] * (zs[j] - pz)) / batch for j in range(A)], 1)
    dqv = Q_t - qret
    stats = xp.stack([-(obj + ent_coeff * -ent) / batch, ((0.5 * q_coeff) * (dqv * dqv)) / batch, -ent, s, rho_t], 0)
    return dict(dz=dz, dq=(q_coeff * dqv) / batch, stats=stats, g=xp.stack(g, 1), k=xp.stack(k, 1),
                zs=xp.stack(zs, 1), s=s, kg=kg, kk=kk)


def loss(case, c, delta, q_coeff, ent_coeff, exact_soft):
    """arl_acer_loss on a loss_case.  exact_soft True: the fp32 soft-max restated in fp32 (bit for bit on soft_exact
    rows); False: the float64 soft-max (compare under loss_bound).  -> (dout f64[B][2S], stats f64[5][B], core)."""
    A, S, B = case["n_act"], case["half"], case["out"].shape[0]
    soft = soft32 if exact_soft else soft64
    pi, lp, _ = soft(case["out"][:, :A])
    pibar, _, _ = soft(case["out_avg"][:, :A])
    src = case["idx"].astype(np.int64) if case["idx"] is not None else np.arange(B)
    act = np.minimum(case["actions"][src].astype(np.int64), A - 1)
    f = lambda x: np.asarray(x, np.float64)              # noqa: E731
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        core = loss_core(np, f(pi), f(lp), f(pibar), f(case["out"][:, S:S + A]), f(case["old_prob"][src]), act,
                         f(case["qret"][src]), float(c), float(delta), float(q_coeff), float(ent_coeff), float(B))
    dout = np.zeros((B, 2 * S))
    dout[:, :A] = core["dz"]
    dout[np.arange(B), S + act] = core["dq"]
    return dout, core["stats"], core


def loss_bound(case, c, delta, q_coeff, ent_coeff):
    """-> (atol of dout f64[B][2S], atol of stats f64[5][B]): the module docstring's first-order bound."""
    import torch
    A, S, B = case["n_act"], case["half"], case["out"].shape[0]
    pi, lp, cz = soft64(case["out"][:, :A])
    pibar, lpb, cb = soft64(case["out_avg"][:, :A])
    chain = 2 * (A + 8) * EPS
    u = [chain * (1 + np.abs(cz)) * pi + TINY, chain * (1 + np.abs(lp)), chain * (1 + np.abs(cb)) * pibar + TINY]
    src = case["idx"].astype(np.int64) if case["idx"] is not None else np.arange(B)
    act = torch.from_numpy(np.minimum(case["actions"][src].astype(np.int64), A - 1))
    t = lambda x: torch.tensor(np.asarray(x, np.float64))              # noqa: E731
    x = [t(v).requires_grad_(True) for v in (pi, lp, pibar)]
    core = loss_core(torch, x[0], x[1], x[2], t(case["out"][:, S:S + A]), t(case["old_prob"][src]), act,
                     t(case["qret"][src]), float(c), float(delta), float(q_coeff), float(ent_coeff), float(B))

    def first_order(col):
        grads = torch.autograd.grad(col.sum(), x, retain_graph=True, allow_unused=True)
        return sum((np.abs(g.numpy()) * ui).sum(axis=1) for g, ui in zip(grads, u) if g is not None)
    dout_atol = np.full((B, 2 * S), TINY)                   # (the padding and the other Q columns are exact zeros)
    for j in range(A):
        dout_atol[:, j] = 2 * first_order(core["dz"][:, j]) + 2 * EPS * np.abs(core["dz"][:, j].detach().numpy()) + TINY
    dq = np.abs(core["dq"].detach().numpy())
    dout_atol[np.arange(B), S + act.numpy()] = 2 * EPS * dq + TINY
    stats_atol = np.zeros((5, B))
    for i in range(5):
        row = core["stats"][i]
        fo = first_order(row) if row.requires_grad else 0.
        stats_atol[i] = 2 * fo + 2 * EPS * np.abs(row.detach().numpy()) + TINY
    return dout_atol, stats_atol


PLAIN, ONE_HOT, DISJOINT, ACT_OUTSIDE = range(4)
N_KINDS = 4


def loss_case(seed, batch, n_act, with_idx, exact=False, scale=1.5):
    """Rows f32[B][2S] with poison in the padding of the inputs.  Rows by (b % N_KINDS): PLAIN; ONE_HOT (one logit of both
    networks ahead by more than 200: pi one-hot); DISJOINT (the average network's one-hot at another action than the live
    network's: pibar disjoint from pi); ACT_OUTSIDE (action byte 255).  exact: every row one-hot (bit-for-bit rows)."""
    rs = np.random.RandomState(seed)
    S = half_stride(n_act)
    n = batch + 3 if with_idx else batch                    # the full-batch arrays the index reads from

    def rows():
        t = np.full((batch, 2 * S), POISON, F32)
        t[:, :n_act] = (rs.randn(batch, n_act) * scale).astype(F32)
        t[:, S:S + n_act] = (rs.randn(batch, n_act) * 2).astype(F32)
        return t
    out, out_avg = rows(), rows()
    kinds = np.arange(batch) % N_KINDS
    for b in range(batch):
        k = ONE_HOT if (exact and kinds[b] == PLAIN) else kinds[b]
        if k in (ONE_HOT, DISJOINT) or exact:
            hot = rs.randint(n_act)
            out[b, hot] = np.abs(out[b, :n_act]).max() + F32(250)
            hot_avg = (hot + 1) % n_act if k == DISJOINT else hot
            out_avg[b, hot_avg] = np.abs(out_avg[b, :n_act]).max() + F32(250)
    mu = rs.rand(n, n_act) + 0.05
    mu = (mu / mu.sum(axis=1, keepdims=True)).astype(F32)
    mu[::5, 0] = 0                                           # a behaviour probability of exactly 0
    actions = rs.randint(0, n_act, size=n).astype(np.uint8)
    idx = rs.permutation(n)[:batch].astype(np.int32) if with_idx else None
    src = idx if with_idx else np.arange(batch)
    actions[src[kinds == ACT_OUTSIDE]] = 255
    return dict(out=out, out_avg=out_avg, old_prob=mu, actions=actions, qret=(rs.randn(n) * 2).astype(F32), idx=idx,
                n_act=n_act, half=S, kinds=kinds)


def rho_range(case):
    """(min, max) over the batch of every rho_a the case produces (float64 soft-max): to place c below, at and above."""
    A = case["n_act"]
    pi, _, _ = soft64(case["out"][:, :A])
    B = pi.shape[0]
    src = case["idx"].astype(np.int64) if case["idx"] is not None else np.arange(B)
    rho = pi / (case["old_prob"][src].astype(np.float64) + AC_EPS)
    return float(rho.min()), float(rho.max())


# ---------------------------------------------------------------- average step

def avg_step(avg, params, alpha):
    """fp32: beta = 1 - alpha; (alpha * avg) + (beta * params), three rounded operations."""
    a, beta = F32(alpha), F32(1) - F32(alpha)
    prod_a = (a * np.asarray(avg, F32)).astype(F32)
    prod_p = (beta * np.asarray(params, F32)).astype(F32)
    return (prod_a + prod_p).astype(F32)


def fma_differs(avg, params, alpha):
    """Boolean mask: where a fused alpha * avg + (beta * params) -- the product unrounded -- cannot give avg_step's
    bits: another fp32 number lies strictly closer to the exact alpha * avg + fl(beta * params) (exact rationals)."""
    a, beta = F32(alpha), F32(1) - F32(alpha)
    two = avg_step(avg, params, alpha)
    prod_p = (beta * np.asarray(params, F32)).astype(F32)
    mask = np.zeros(len(two), bool)
    for i in range(len(two)):
        exact = Fraction(float(a)) * Fraction(float(avg[i])) + Fraction(float(prod_p[i]))
        err = abs(Fraction(float(two[i])) - exact)
        for nb in (np.nextafter(two[i], F32(np.inf)), np.nextafter(two[i], F32(-np.inf))):
            if abs(Fraction(float(nb)) - exact) < err:
                mask[i] = True
    return mask


# ---------------------------------------------------------------- segment gather

def gather(src, index):
    n = src.shape[0]
    return src[np.clip(np.asarray(index, np.int64), 0, n - 1)]
