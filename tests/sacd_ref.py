"""Shared by tests/test_sacd_host.py and tests/test_sacd_gpu.py: the input cases and the float64 NumPy restatements of
arl_sacd_act, arl_sacd_loss and arl_sacd_alpha_grad (include/accel_rl_hip.h), per row and in the stated order, with the
derived error bounds.  At the end: the shapes of tests/test_r2d2_vmpo_sacd_limits_*.py and arl_sacd_alpha_grad's summation
order restated in fp32 (alpha_grad_sum32).

Bounds (EPS = 2^-24, the unit roundoff; the derivation is repeated in DESIGN.md, section 23).

The soft value  soft = sum_a pi_a x_a,  x_a = min(q1t_a, q2t_a) - alpha lp_a,  is computed in fp32 with A additions for
s, A additions for the chain, and per term a handful of single roundings (c_a = z_a - m, expf, the division, logf, the
difference lp_a, alpha lp_a, the difference x_a, the product; expf / logf counted at 3 ulp): 2 A + 16 = 2 (A + 8)
roundings.  Unlike the Munchausen soft value, x_a differs from action to action, so an error of pi_a does not cancel;
and the rounding of c_a moves e_a by |c_a| EPS relative.  The error of lp_a = c_a - logf(s) is NOT relative to |lp_a|:
s carries its A roundings as a relative error, which logf turns into an ABSOLUTE error of the same size however small
log s is (s = 1 + 3e-7 is stored as 1 + k 2^-23), so lp_a is known to (1 + |lp_a|) times the chain, and the magnitude
that stands for a term is  X_a = |min(q1t_a, q2t_a)| + alpha (1 + |lp_a|).  Every term therefore carries at most
2 (A + 8) EPS (1 + |c_a|) pi_a X_a, and pi_a |c_a| <= 1 / e keeps that finite where a logit is far behind:
    soft_atol_b = 2 (A + 8) EPS sum_a pi'_a (1 + |c'_a|) (|min(q1t_a, q2t_a)| + alpha (1 + |lp'_a|))
    y_atol_b    = 2 (A + 8) EPS |returns_b| + gamma_n soft_atol_b          (terminal rows: the first term alone)
td_abs and the slope are 1-Lipschitz in d = y - q: the same bound plus 4 EPS |d|; dq_i: w_b times it, plus rtol 2e-4;
q_loss_rows: w_b (|slope_1| + |slope_2|) y_atol + w_b y_atol^2, plus 8 EPS of the row.  The actor's side has the same
structure with g_a = alpha lp_a - min(q1_a, q2_a) in place of x_a and  G_a = alpha (1 + |lp_a|) + |min(q1_a, q2_a)|  in
place of X_a:  G_b = sum_a pi_a (1 + |c_a|) G_a,
    J_atol_b  = 2 (A + 8) EPS G_b;   pi_loss_rows: J_atol_b / B
    dl_atol_b = 2 (A + 8) EPS (max_k pi_k (1 + |c_k|) G_k + 3 G_b) / B   (pi_k (1 + |c_k|) < 2 multiplies |J| <= G_b and J's
                own error), plus rtol 2e-4;  a row of dlogits sums to 0 within A dl_atol_b
    ent_atol_b = 2 (A + 8) EPS sum_a pi_a (1 + |c_a|) (1 + |lp_a|)
arl_sacd_alpha_grad: a chain of at most B / 256 + 8 additions, expf, the division, the difference and the product:
    (B / 256 + 16) EPS alpha (sum_b |ent_b| / B + |target|).
arl_sacd_act: |pi_a - pi64_a| <= 2 (A + 8) EPS (1 + |c_a|) pi_a.
Every bound carries + 2^-126 on top: an fp32 result below the smallest normal number is a multiple of 2^-149 (or 0), so
its error is not relative to its size (a one-hot row's entropy, the probability of a logit 100 behind)."""
import numpy as np

EPS = 2.0 ** -24
POISON = 1e9                    # what the padding columns of every input hold: they must be ignored
F32 = np.float32
GAMMA = float(np.float32(0.99))
TINY = 2.0 ** -126              # the smallest normal fp32 number: below it a result may be flushed or lose its last bits

# (n_actions, stride, batch): the smallest at which the kernel can still go wrong
SHAPES = [(1, 4, 1), (2, 32, 3), (6, 32, 32), (18, 32, 65), (33, 36, 2), (64, 64, 5)]

# special rows, by (row + shift) % N_KINDS: the shift makes every kind appear over the small batches too
PLAIN, ALL_EQUAL, ONE_HOT, Q1_BELOW, Q1_ABOVE, Q_EQUAL, ACT_OUTSIDE = range(7)
N_KINDS = 7


def seed_of(shape, weighted):
    return 1000 * SHAPES.index(tuple(shape)) + 17 * int(weighted) + 3


def case(seed, n_act, stride, batch, weighted, scale=2.0, shift=0, log_alpha=-0.7):
    """Six row blocks f32[B][S] with poison in the padding.  Planted rows: ALL_EQUAL (both logit rows constant: ent ==
    log A), ONE_HOT (one logit ahead by more than 88 in both rows: pi one-hot, 0 * lp must stay 0), Q1_BELOW / Q1_ABOVE /
    Q_EQUAL (q1 <, >, == q2 in every column, the taken action's too, online and target), ACT_OUTSIDE (actions_b = 255);
    PLAIN rows mix both orders inside fminf.  Terminal rows by rs and at rows 0 / 1."""
    rs = np.random.RandomState(seed)
    kinds = (np.arange(batch) + shift) % N_KINDS

    def rows(s=scale):
        t = (rs.randn(batch, stride) * s).astype(F32)
        t[:, n_act:] = POISON
        return t
    q1, q2, t1, t2 = rows(), rows(), rows(), rows()
    lo, ln = rows(min(scale, 50.0)), rows(min(scale, 50.0))
    act = rs.randint(0, n_act, size=batch).astype(np.uint8)
    for b in range(batch):
        k = kinds[b]
        if k == ALL_EQUAL:
            lo[b, :n_act] = lo[b, 0]
            ln[b, :n_act] = ln[b, 0]
        elif k == ONE_HOT:
            lo[b, rs.randint(n_act)] = np.abs(lo[b, :n_act]).max() + F32(100)
            ln[b, rs.randint(n_act)] = np.abs(ln[b, :n_act]).max() + F32(100)
        elif k == Q1_BELOW:
            q1[b, :n_act] = q2[b, :n_act] - F32(0.5 * scale)
            t1[b, :n_act] = t2[b, :n_act] - F32(0.5 * scale)
        elif k == Q1_ABOVE:
            q1[b, :n_act] = q2[b, :n_act] + F32(0.5 * scale)
            t1[b, :n_act] = t2[b, :n_act] + F32(0.5 * scale)
        elif k == Q_EQUAL:
            q1[b] = q2[b]
            t1[b] = t2[b]
        elif k == ACT_OUTSIDE:
            act[b] = 255
    ret = (rs.randn(batch) * 3).astype(F32)
    term = (rs.rand(batch) < 0.3).astype(np.uint8)
    if batch > 1:
        term[0], term[1] = 1, 0
    else:
        term[0] = shift & 1
    isw = (rs.rand(batch) + 0.1).astype(F32) if weighted else None
    return dict(q1=q1, q2=q2, t1=t1, t2=t2, lo=lo, ln=ln, act=act, ret=ret, term=term, isw=isw, kinds=kinds,
                n_act=n_act, log_alpha=F32(log_alpha))


def soft64(z):
    """float64 [..., A] -> (c = z - max, lp, pi), a ascending."""
    z = np.asarray(z, np.float64)
    c = z - z.max(axis=-1, keepdims=True)
    e = np.exp(c)
    s = e.sum(axis=-1, keepdims=True)
    return c, c - np.log(s), e / s


def huber64(d, clip):
    """(loss, slope, clipped |d|) of arl_dqn_loss; clip None or <= 0: squared."""
    ad = np.abs(d)
    if clip and clip > 0:
        big = ad > clip
        return (np.where(big, clip * (ad - clip / 2.), 0.5 * d * d), np.where(big, np.sign(d) * clip, d),
                np.minimum(ad, clip))
    return 0.5 * d * d, d, ad


def ref_act(logits, n_act, override=None, deterministic=False):
    """-> (prob f64[B][A], greedy, atol[B][A] of the soft-max rows)."""
    z = np.asarray(logits, np.float64)[:, :n_act]
    c, _, pi = soft64(z)
    greedy = z.argmax(axis=1)                                   # (numpy: the first maximum)
    prob = pi.copy()
    for b in range(z.shape[0]):
        ov = -1 if override is None else int(override[b])
        if ov >= 0 or deterministic:
            prob[b] = 0.
            if (ov if ov >= 0 else greedy[b]) < n_act:
                prob[b, ov if ov >= 0 else greedy[b]] = 1.
    return prob, greedy, 2 * (n_act + 8) * EPS * (1 + np.abs(c)) * pi + TINY


def ref_loss(c, gamma_n, delta_clip):
    """float64, per row in the header's order.  Returns the outputs and their bounds (module docstring)."""
    A = c["n_act"]
    f = lambda x: np.asarray(x, np.float64)[:, :A]              # noqa: E731
    q1, q2, t1, t2 = f(c["q1"]), f(c["q2"]), f(c["t1"]), f(c["t2"])
    B = q1.shape[0]
    alpha = float(np.exp(np.float64(c["log_alpha"])))
    cn, lpn, pin = soft64(f(c["ln"]))
    tmin = np.minimum(t1, t2)
    soft = (pin * (tmin - alpha * lpn)).sum(axis=1)
    keep = 1. - (c["term"] != 0).astype(np.float64)
    ret = c["ret"].astype(np.float64)
    y = ret + keep * (gamma_n * soft)
    chain = 2 * (A + 8) * EPS
    soft_atol = chain * (pin * (1 + np.abs(cn)) * (np.abs(tmin) + alpha * (1 + np.abs(lpn)))).sum(axis=1)
    y_atol = chain * np.abs(ret) + keep * gamma_n * soft_atol
    act = np.minimum(c["act"].astype(np.int64), A - 1)
    ar = np.arange(B)
    w = (c["isw"].astype(np.float64) if c["isw"] is not None else np.ones(B)) / B
    out = dict(y=y, y_atol=y_atol, w=w, act=act, soft=soft, alpha=alpha)
    rows, td, slopes = 0., 0., 0.
    for i, q in ((1, q1), (2, q2)):
        d = y - q[ar, act]
        loss, slope, p = huber64(d, delta_clip)
        dq = np.zeros((B, A))
        dq[ar, act] = -w * slope
        out["dq%d" % i], out["d%d" % i] = dq, d
        rows, td, slopes = rows + w * loss, td + p, slopes + np.abs(slope)
    out.update(rows=rows, td=td / 2., slopes=slopes)
    out["td_atol"] = y_atol + 4 * EPS * (np.abs(out["d1"]) + np.abs(out["d2"])) / 2. + TINY
    out["rows_atol"] = w * (slopes * y_atol + y_atol * y_atol) + 8 * EPS * np.abs(rows) + TINY
    co, lp, pi = soft64(f(c["lo"]))
    g = alpha * lp - np.minimum(q1, q2)
    J = (pi * g).sum(axis=1)
    Ga = pi * (1 + np.abs(co)) * (alpha * (1 + np.abs(lp)) + np.abs(np.minimum(q1, q2)))
    G = Ga.sum(axis=1)
    out.update(dlogits=pi * (g - J[:, None]) / B, pi_rows=J / B, ent=-(pi * lp).sum(axis=1), pi=pi, lp=lp,
               pi_atol=chain * G / B + TINY,
               dl_atol=chain * (Ga.max(axis=1) + 3 * G) / B + TINY,
               ent_atol=chain * (pi * (1 + np.abs(co)) * (1 + np.abs(lp))).sum(axis=1) + TINY)
    return out


def ref_alpha_grad(ent_rows, log_alpha, target_entropy):
    """-> (grad, atol)."""
    ent = np.asarray(ent_rows, np.float64)
    alpha = float(np.exp(np.float64(log_alpha)))
    b = ent.size
    return (alpha * (ent.sum() / b - target_entropy),
            (b / 256. + 16) * EPS * alpha * (np.abs(ent).sum() / b + abs(target_entropy)))


# ---- the limits tests (tests/test_r2d2_vmpo_sacd_limits_gpu.py / _host.py) -------------------------------------------------

# (n_actions, stride, batch, shift): the action limit at the tight stride; 253 actions (three dead floats in the last
# float4) with one row in a second workgroup -- row 256, which the shift makes an ACT_OUTSIDE row; three and five
# workgroups with a one-row tail
LIMIT_SHAPES = [(255, 256, 3, 0), (253, 256, 257, 2), (6, 8, 513, 0), (18, 32, 1025, 3)]
ALPHA_GRAD_BATCHES = [1, 255, 256, 257, 65537]
ALPHA_GRAD_TARGET = F32(0.6)


def limit_case(shape, weighted):
    n_act, stride, batch, shift = shape
    return case(7000 + 10 * LIMIT_SHAPES.index(tuple(shape)) + int(weighted), n_act, stride, batch, weighted, shift=shift)


def alpha_grad_rows(batch):
    """entropies in [0.1, 1.6): sums of them round at nearly every addition."""
    return (np.random.RandomState(400 + batch).rand(batch) * 1.5 + 0.1).astype(F32)


def alpha_grad_sum32(ent_rows, drop_last_fold=False):
    """The header's summation order in fp32: thread t adds rows t, t + 256, ... to 0 in ascending order, then
    s[t] += s[t + h] for h = 128, 64, ... 1 -> s[0].  (Rows past the end are +0: x + 0 is x, and no partial sum is -0.)"""
    ent = np.asarray(ent_rows, F32)
    trips = -(-ent.size // 256)
    grid = np.zeros(trips * 256, F32)
    grid[:ent.size] = ent
    s = np.zeros(256, F32)
    for row in grid.reshape(trips, 256):
        s = s + row
    h = 128
    while h > (1 if drop_last_fold else 0):
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    assert s.dtype == F32
    return s[0]


def alpha_grad32(ent_rows, target_entropy):
    """arl_sacd_alpha_grad's entry 0 at log_alpha = 0 (expf(0) is exactly 1), every operation in fp32."""
    mean = alpha_grad_sum32(ent_rows) / F32(np.asarray(ent_rows).size)
    return F32(1) * (mean - F32(target_entropy))


def plain_sum32(ent_rows):
    """the rows added in ascending order in fp32: the order the kernel does NOT use."""
    s = F32(0)
    for v in np.asarray(ent_rows, F32):
        s = s + v
    return s
