"""Shared by tests/test_quantile_limits_host.py and tests/test_quantile_limits_gpu.py: an fp32 NumPy restatement of what
csrc/q_loss_dev.h, csrc/iqn.hip, csrc/fqf.hip and the quantile part of csrc/dqn.hip compute WITHOUT the device library --
every operation a np.float32 operation, in the order include/accel_rl_hip.h states ("Quantile-regression DQN output
stage", "Implicit quantile networks", "Fully parameterized quantile functions"), vectorised over the batch.  The kernels
are compiled with -ffp-contract=off, IEEE fp32 addition, multiplication and division are correctly rounded on both
sides, so wherever a kernel calls neither expf / logf nor cospif / sinpif its outputs must equal these bit for bit
(`bits` compares the words: the sign of a zero counts).

Also here: the integer argument reduction of cos_pi_i_tau (float64 supplies the final cosine), the number of
significant bits of the folded argument (the header's exactness claim), and alternative summation orders that the host
test uses to show that the chosen inputs tell the stated order from another.

The generator (ref_tau, philox4x32_10), the float64 references (ref_iqn_loss, fqf_ref, munchausen_ref) and the fp32
emulations of the soft-max targets (munchausen_ref._butterfly, emu_miqn_targets) are the feature tests' own."""
import numpy as np

from munchausen_ref import _butterfly

F32 = np.float32
LANES = 64


def bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == F32, x.dtype
    return x.view(np.uint32)


def _f32(x):
    x = np.asarray(x)
    assert x.dtype == F32, x.dtype
    return x


def pad_lanes(x):
    """[..., n <= 64] -> [..., 64], lanes >= n hold +0."""
    out = np.zeros(x.shape[:-1] + (LANES,), F32)
    out[..., :x.shape[-1]] = x
    return out


def wave_sum_64(x):
    """The 64-lane xor butterfly (lane ^ 32, ^ 16, ... ^ 1) of [..., n <= 64], lanes >= n holding +0, as it stands."""
    return _butterfly(pad_lanes(_f32(x)), lambda a, b: a + b)[..., 0]


def wave_sum(x):
    """wave_sum_64's value in lane 0 with less work: with P the power of two >= n, every step whose mask is >= P adds a
    lane that still holds +0 (x + 0: it only turns a -0 into +0), and the steps below P stay inside the first P lanes."""
    x = _f32(x)
    n = x.shape[-1]
    width = 1
    while width < n:
        width *= 2
    v = np.zeros(x.shape[:-1] + (width,), F32)
    v[..., :n] = x
    if width < LANES:
        v = v + F32(0)
    lanes = np.arange(width)
    mask = width // 2
    while mask:
        v = v + v[..., lanes ^ mask]
        mask //= 2
    return v[..., 0]


def sequential_sum(x):
    """NOT the kernels' order: lanes added one after the other, ascending."""
    s = np.zeros(x.shape[:-1], F32)
    for i in range(x.shape[-1]):
        s = s + x[..., i]
    return s


# ---- csrc/q_loss_dev.h --------------------------------------------------------------------------------------------------

def quantile_huber_term(u, tau, kappa):
    """-> (gt, rt) at u = T_j - theta_i and the fraction tau of theta_i (arrays of one shape)."""
    u, tau, kappa = _f32(u), _f32(tau), F32(kappa)
    ind = np.where(u < F32(0), F32(1), F32(0))
    wt = np.abs(tau - ind)
    if kappa > 0:
        au = np.abs(u)
        l = np.where(au <= kappa, F32(0.5) * (u * u), kappa * (au - F32(0.5) * kappa))
        return wt * np.minimum(np.maximum(u, -kappa), kappa) / kappa, wt * l / kappa
    return tau - ind, wt * np.abs(u)


def strided_partials(T, th, tau, kappa):
    """The N x N' phase: T [B][N'], th and tau [B][N] -> (g, r) [4][B][N]; partial w sums j = w, w + 4, ... ascending
    from 0 (a wave without a j leaves an exact +0)."""
    T, th, tau = _f32(T), _f32(th), _f32(tau)
    g = np.zeros((4,) + th.shape, F32)
    r = np.zeros((4,) + th.shape, F32)
    for w in range(4):
        for j in range(w, T.shape[1], 4):
            gt, rt = quantile_huber_term(T[:, j:j + 1] - th, tau, kappa)
            g[w] = g[w] + gt
            r[w] = r[w] + rt
    return g, r


def combine4(p):
    return ((p[0] + p[1]) + p[2]) + p[3]


def combine4_pairs(p):
    """NOT the kernels' order."""
    return (p[0] + p[1]) + (p[2] + p[3])


def ascending_j_sums(T, th, tau, kappa):
    """NOT the kernels' order: one chain over j = 0 .. N' - 1 per predicted fraction -> (g, r) [B][N]."""
    g, r = np.zeros(th.shape, F32), np.zeros(th.shape, F32)
    for j in range(T.shape[1]):
        gt, rt = quantile_huber_term(T[:, j:j + 1] - th, tau, kappa)
        g, r = g + gt, r + rt
    return g, r


def first_max(q):
    """[B][A] -> int[B]: a = 0, then every a whose value is > the best so far."""
    q = _f32(q)
    best = np.zeros(q.shape[0], np.int64)
    best_q = q[:, 0].copy()
    for a in range(1, q.shape[1]):
        better = q[:, a] > best_q
        best_q = np.where(better, q[:, a], best_q)
        best = np.where(better, a, best)
    return best


def clamp_action(actions, n_actions):
    return np.minimum(np.asarray(actions).astype(np.int64), n_actions - 1)


def weights(is_weights, batch):
    """w_b = (is_weight_b or 1) / batch."""
    isw = np.ones(batch, F32) if is_weights is None else _f32(is_weights)
    return isw / F32(batch)


def stage_targets(ret, term, gamma_n, tgt, a_next):
    """T [B][N'] = returns_b + keep * (gamma_n * tgt(j, a*)); tgt [B][N'][>= A]."""
    keep = np.where(np.asarray(term) != 0, F32(0), F32(1))
    picked = _f32(tgt)[np.arange(tgt.shape[0]), :, a_next]
    return _f32(ret)[:, None] + keep[:, None] * (F32(gamma_n) * picked)


def reduce_tail(T, th, tau, wgt, kappa, combine=combine4, total=wave_sum):
    """From the staged T, theta and tau to (d [B][N], loss_rows [B], priorities [B], loss_b [B])."""
    m = F32(T.shape[1])
    g, r = strided_partials(T, th, tau, kappa)
    gs, rs = combine(g), combine(r)
    d = -(wgt[:, None] / m * gs)
    loss_b = total(rs) / m
    return d, wgt * loss_b, np.minimum(np.maximum(loss_b, F32(1e-6)), F32(1e6)), loss_b


def loss_tail(T, th, tau, act, is_weights, stride, kappa):
    """loss_tail of csrc/q_loss_dev.h -> dict(dtheta [B][N][stride], rows, pri, loss_b, d): column act_b of row i holds
    d_i, everything else +0."""
    batch, n = th.shape
    d, rows, pri, loss_b = reduce_tail(T, th, tau, weights(is_weights, batch), kappa)
    dtheta = np.zeros((batch, n, stride), F32)
    dtheta[np.arange(batch), :, act] = d
    return dict(dtheta=dtheta, rows=rows, pri=pri, loss_b=loss_b, d=d)


# ---- csrc/iqn.hip -------------------------------------------------------------------------------------------------------

def q_of_lane(theta, n_actions):
    """theta [B][K][>= A] -> Q [B][A] = (sum_k theta(k, a)) / K, k ascending, the sum starts at 0."""
    theta = _f32(theta)
    s = np.zeros((theta.shape[0], n_actions), F32)
    for j in range(theta.shape[1]):
        s = s + theta[:, j, :n_actions]
    return s / F32(theta.shape[1])


def iqn_loss(pred, tau, tgt, pol, act, ret, term, isw, n_actions, gamma_n, kappa):
    """arl_iqn_loss: pred [B][N][S], tau [B][N], tgt / pol [B][N'][S] (pol None: not double DQN)."""
    act = clamp_action(act, n_actions)
    a_next = first_max(q_of_lane(tgt if pol is None else pol, n_actions))
    T = stage_targets(ret, term, gamma_n, tgt, a_next)
    out = loss_tail(T, _f32(pred)[np.arange(pred.shape[0]), :, act], tau, act, isw, pred.shape[2], kappa)
    out.update(T=T, a_next=a_next)
    return out


def miqn_loss_from_targets(pred, tau, T, act, isw, n_actions, kappa):
    """Everything of arl_miqn_loss after T_j."""
    act = clamp_action(act, n_actions)
    return loss_tail(T, _f32(pred)[np.arange(pred.shape[0]), :, act], tau, act, isw, pred.shape[2], kappa)


def merge_fwd(psi, phi, r):
    return np.repeat(_f32(psi), r, axis=0) * _f32(phi)


def merge_bwd(g, psi, phi, r):
    """-> (dphi [B R][F], dpsi [B][F]); dpsi sums r ascending from 0."""
    g, psi, phi = _f32(g), _f32(psi), _f32(phi)
    b, f = psi.shape
    dphi = np.where(phi > 0, g * np.repeat(psi, r, axis=0), F32(0))
    gp = (g * phi).reshape(b, r, f)
    s = np.zeros((b, f), F32)
    for k in range(r):
        s = s + gp[:, k]
    return dphi, np.where(psi > 0, s, F32(0))


# ---- cos_pi_i_tau's reduction, in integers ----------------------------------------------------------------------------------

def cos_reduce(i, tau_bits):
    """The branches of cos_pi_i_tau for the feature index i and the fp32 word tau_bits -> (p, sh, neg, use_sin), the
    folded angle p 2^-sh in units of pi; or None where the kernel returns 1 early (i == 0, tau == 0, |tau| >= 2^24, an
    infinity or a NaN)."""
    b = int(tau_bits) & 0x7fffffff
    ex = b >> 23
    s = (b & 0x7fffff) | 0x800000 if ex else b & 0x7fffff
    e = (ex if ex else 1) - 150
    if i == 0 or s == 0 or e >= 1:
        return None
    p, sh = i * s * 4, 2 - e
    neg = use_sin = False
    if sh < 40:
        half = 1 << sh
        p &= (half << 1) - 1
        if p > half:
            p = (half << 1) - p
        if p > (half >> 1):
            p, neg = half - p, True
        if p > (half >> 2):
            p, use_sin = (half >> 1) - p, True
    return p, sh, neg, use_sin


def cos_branch(i, tau_bits):
    """A name for the path (i, tau) takes: 'one', 'unreduced', or the folds taken, e.g. 'mod+2pi+pi+sin' / 'none'."""
    b = int(tau_bits) & 0x7fffffff
    ex = b >> 23
    s = (b & 0x7fffff) | 0x800000 if ex else b & 0x7fffff
    e = (ex if ex else 1) - 150
    if i == 0 or s == 0 or e >= 1:
        return "one"
    p, sh = i * s * 4, 2 - e
    if sh >= 40:
        return "unreduced"
    half, taken = 1 << sh, []
    p &= (half << 1) - 1
    if p > half:
        p = (half << 1) - p
        taken.append("2pi")
    if p > (half >> 1):
        p = half - p
        taken.append("pi")
    if p > (half >> 2):
        taken.append("sin")
    return "+".join(taken) if taken else "none"


def significant_bits(p):
    """Bits between the highest and the lowest set bit of the integer p, both included (0 for 0)."""
    p = int(p)
    return 0 if p == 0 else p.bit_length() - ((p & -p).bit_length() - 1)


def cos_f64(i, tau_bits):
    """float64 cos(pi i tau) through the exact integer reduction (p < 2^32: p 2^-sh is exact in float64)."""
    red = cos_reduce(i, tau_bits)
    if red is None:
        return 1.0
    p, sh, neg, use_sin = red
    t = np.ldexp(float(p), -sh) * np.pi
    v = np.sin(t) if use_sin else np.cos(t)
    if p == 0:
        v = 0.0 if use_sin else 1.0
    return -v if neg else v


def cos_f64_table(tau):
    """tau f32[P] -> float64 [P][64]."""
    w = bits(np.asarray(tau, F32))
    return np.array([[cos_f64(i, x) for i in range(64)] for x in w], np.float64)


def significant_bits_vec(i, s, sh):
    """Vectorised over the significands s (uint64 array) of one binade: the number of significant bits of the folded p
    (sh < 40).  -> int64 array."""
    one = np.uint64(1)
    half = one << np.uint64(sh)
    p = (np.uint64(i) * s.astype(np.uint64) * np.uint64(4)) & ((half << one) - one)
    p = np.where(p > half, (half << one) - p, p)
    p = np.where(p > (half >> one), half - p, p)
    p = np.where(p > (half >> np.uint64(2)), (half >> one) - p, p)
    low = p & (~p + one)                                        # the lowest set bit (0 for 0)
    with np.errstate(divide="ignore"):
        top = np.floor(np.log2(np.maximum(p, one).astype(np.float64))).astype(np.int64)
        bottom = np.floor(np.log2(np.maximum(low, one).astype(np.float64))).astype(np.int64)
    # log2 of a uint64 below 2^53 converted to float64 is exact at powers of two and floor() is safe below them: p < 2^41
    return np.where(p == 0, 0, top - bottom + 1)


# ---- csrc/dqn.hip: QR-DQN -------------------------------------------------------------------------------------------------

def qr_merged(theta, n_actions, n, dueling):
    """theta [B][A (+ 1)][S] -> theta(a, i) [B][A][N]; dueling: val_i + (adv_ai - mean_a adv_ai), the mean summed a
    ascending from 0."""
    theta = _f32(theta)
    x = theta[:, :n_actions, :n]
    if not dueling:
        return x
    s = np.zeros((theta.shape[0], n), F32)
    for a in range(n_actions):
        s = s + x[:, a]
    mean = s / F32(n_actions)
    return theta[:, n_actions, :n][:, None, :] + (x - mean[:, None, :])


def qr_q(theta, n_actions, n, dueling):
    """Q [B][A] = butterfly(theta(a, .)) / N."""
    return wave_sum(qr_merged(theta, n_actions, n, dueling)) / F32(n)


def qr_tau(n):
    return (np.arange(n).astype(F32) + F32(0.5)) / F32(n)


def qrdqn_loss(pred, tgt, pol, act, ret, term, isw, n_actions, n, dueling, gamma_n, kappa):
    """arl_qrdqn_loss: pred / tgt / pol [B][A (+ 1)][S] -> dict(dtheta (pred's shape), rows, pri, loss_b, T, a_next)."""
    batch, rows_, stride = pred.shape
    ar = np.arange(batch)
    act = clamp_action(act, n_actions)
    a_next = first_max(qr_q(tgt if pol is None else pol, n_actions, n, dueling))
    keep = np.where(np.asarray(term) != 0, F32(0), F32(1))
    T = _f32(ret)[:, None] + keep[:, None] * (F32(gamma_n) * qr_merged(tgt, n_actions, n, dueling)[ar, a_next])
    th = qr_merged(pred, n_actions, n, dueling)[ar, act]
    tau = np.broadcast_to(qr_tau(n), (batch, n))
    d, rows, pri, loss_b = reduce_tail(T, th, tau, weights(isw, batch), kappa)
    dtheta = np.zeros(pred.shape, F32)
    if dueling:
        share = d / F32(n_actions)
        dtheta[:, :n_actions, :n] = -share[:, None, :]
        dtheta[ar, act, :n] = d - share
        dtheta[:, n_actions, :n] = d
    else:
        dtheta[ar, act, :n] = d
    return dict(dtheta=dtheta, rows=rows, pri=pri, loss_b=loss_b, T=T, a_next=a_next, d=d)


# ---- csrc/fqf.hip ---------------------------------------------------------------------------------------------------------

def fqf_tau_chain(q):
    """q f32[B][N] (the kernel's own) -> (tau [B][N + 1], tau_hat [B][N]): tau_{i+1} = min(tau_i + q_i, 1) sequentially,
    tau_N = 1."""
    q = _f32(q)
    b, n = q.shape
    tau = np.zeros((b, n + 1), F32)
    for k in range(n):
        tau[:, k + 1] = F32(1) if k == n - 1 else np.minimum(tau[:, k] + q[:, k], F32(1))
    return tau, F32(0.5) * (tau[:, :-1] + tau[:, 1:])


def fqf_entropy(q, logq):
    return F32(0) - wave_sum(_f32(q) * _f32(logq))


def wq_of_lane(theta, tau, n_actions):
    """Q [B][A] = sum_j (tau_{j+1} - tau_j) * theta(j, a), j ascending, the sum starts at 0."""
    theta, tau = _f32(theta), _f32(tau)
    s = np.zeros((theta.shape[0], n_actions), F32)
    for j in range(theta.shape[1]):
        s = s + (tau[:, j + 1] - tau[:, j])[:, None] * theta[:, j, :n_actions]
    return s


def fqf_fraction_part(th, mid, tau, q, logq, H, wgt, ent_coef, n_stride):
    """th [B][N] and mid [B][N - 1] (or None) the taken action's columns -> dict(g [B][N] (g_0 = 0), G, S [B][N],
    dlogits [B][n_stride], frac [B])."""
    th, tau, q, logq, H = _f32(th), _f32(tau), _f32(q), _f32(logq), _f32(H)
    b, n = th.shape
    g = np.zeros((b, n), F32)
    if n > 1:
        g[:, 1:] = (F32(2) * _f32(mid) - th[:, 1:]) - th[:, :-1]
    G, S = np.zeros(b, F32), np.zeros((b, n), F32)
    for i in range(1, n):
        G = G + g[:, i] * tau[:, i]
        S[:, :i] = S[:, :i] + g[:, i:i + 1]                    # lanes k < i
    d = wgt[:, None] * (q * (S - G[:, None]) + F32(ent_coef) * (q * (logq + H[:, None])))
    dlogits = np.zeros((b, n_stride), F32)
    dlogits[:, :n] = d
    return dict(g=g, G=G, S=S, dlogits=dlogits, frac=wgt * G)


def fqf_suffix_including_k(g):
    """NOT the kernel's S_k: the suffix sums with i == k included."""
    b, n = g.shape
    S = np.zeros((b, n), F32)
    for i in range(1, n):
        S[:, :i + 1] = S[:, :i + 1] + g[:, i:i + 1]
    return S


def fqf_loss(pred, mid, tau, tau_hat, q, logq, H, tgt, pol, act, ret, term, isw, n_actions, n_stride, gamma_n, kappa,
             ent_coef):
    """arl_fqf_loss: pred / tgt / pol [B][N][S], mid [B][N - 1][S] or None."""
    batch, n, stride = pred.shape
    ar = np.arange(batch)
    act = clamp_action(act, n_actions)
    a_next = first_max(wq_of_lane(tgt if pol is None else pol, tau, n_actions))
    T = stage_targets(ret, term, gamma_n, tgt, a_next)
    th = _f32(pred)[ar, :, act]
    out = loss_tail(T, th, tau_hat, act, isw, stride, kappa)
    out.update(fqf_fraction_part(th, None if n == 1 else _f32(mid)[ar, :, act], tau, q, logq, H, weights(isw, batch),
                                 ent_coef, n_stride))
    out.update(T=T, a_next=a_next)
    return out


# ---- input cases ----------------------------------------------------------------------------------------------------------

POISON = 1e9                    # what the padding columns of every input hold: they must be ignored
(ROW_TERMINAL, ROW_PLAIN, ROW_ACTION_255, ROW_ZERO_WEIGHT, ROW_TIE, ROW_LAST_LANE, ROW_KAPPA_EDGES, ROW_TINY_LOSS,
 ROW_HUGE_LOSS, ROW_TAU_ENDS) = range(10)
CORNER_BATCH = 10


def kappa_edges(kappa):
    """u == 0, |u| == kappa and one ulp either side of it, both signs (kappa == 0: +-2^-100 stands for "next to 0" -- a
    normal number, so no product with it is subnormal)."""
    k = F32(kappa)
    if k == 0:
        near = [F32(2.0 ** -100)]
    else:
        near = [k, np.nextafter(k, F32(0)), np.nextafter(k, F32(np.inf))]
    return np.array([F32(0)] + near + [-x for x in near], F32)


def _blocks(rs, batch, r, n_act, stride, scale=2.):
    t = (rs.randn(batch, r, stride) * scale).astype(F32)
    t[:, :, n_act:] = POISON
    return t


def corner_case(seed, n_act, n, m, stride, kappa, double=True, batch=CORNER_BATCH, first_action=0):
    """The corner rows of the loss kernels (the ROW_* constants name them), in a batch of CORNER_BATCH or more rows; rows
    past the named ones are plain.  One action column of the selecting net gets +20 at every fraction, so the greedy
    action is `chosen` in fp32 and in float64 alike (except in ROW_TIE, where columns 0 and A - 1 are bit-identical
    maxima and the first wins).  The taken action alternates between `first_action`'s column 0 and A - 1."""
    assert batch >= CORNER_BATCH
    rs = np.random.RandomState(seed)
    pred, tgt = _blocks(rs, batch, n, n_act, stride), _blocks(rs, batch, m, n_act, stride)
    pol = _blocks(rs, batch, m, n_act, stride) if double else None
    sel = pol if double else tgt
    chosen = rs.randint(0, n_act, size=batch)
    chosen[ROW_LAST_LANE] = n_act - 1
    chosen[ROW_TIE] = 0
    sel[np.arange(batch), :, chosen] += F32(20)
    if n_act > 1:
        sel[ROW_TIE, :, n_act - 1] = sel[ROW_TIE, :, 0]
    tau = rs.uniform(0.02, 0.98, size=(batch, n)).astype(F32)
    act = np.where((np.arange(batch) + first_action) % 2 == 0, 0, n_act - 1).astype(np.uint8)
    act[ROW_ACTION_255] = 255
    ret = (rs.randn(batch) * 3).astype(F32)
    term = (rs.rand(batch) < 0.3).astype(np.uint8)
    term[ROW_TERMINAL], term[ROW_PLAIN] = 1, 0
    isw = (rs.rand(batch) + 0.1).astype(F32)
    isw[ROW_ZERO_WEIGHT] = 0
    a = clamp_action(act, n_act)
    edges = kappa_edges(kappa)
    for row, value, th in ((ROW_KAPPA_EDGES, 0., -edges[np.arange(n) % edges.size]),
                           (ROW_TINY_LOSS, 0., np.full(n, 1e-9, F32)), (ROW_HUGE_LOSS, 1e8, (rs.randn(n) * 2).astype(F32))):
        term[row], ret[row] = 1, value                          # every T_j == returns_b, u_ij = returns_b - theta_i exactly
        pred[row, :, a[row]] = th
    tau[ROW_TAU_ENDS, 0] = 0
    tau[ROW_TAU_ENDS if n > 1 else ROW_PLAIN, n - 1] = 1
    return dict(pred=pred, tau=tau, tgt=tgt, pol=pol, act=act, ret=ret, term=term, isw=isw, chosen=chosen)


def dominant_logits(rs, batch, n, n_stride, rows=(0,)):
    """Logits f32[B][n_stride] of modest spread; in `rows` one entry (the middle one) dominates by 200, so that every
    other q_k underflows to an exact 0 and tau repeats at both ends (0 .. 0, 1 .. 1)."""
    lg = np.full((batch, n_stride), POISON, F32)
    lg[:, :n] = (rs.randn(batch, n) * 1.5).astype(F32)
    for b in rows:
        lg[b, n // 2] += F32(200)
    return lg


def tau_grid():
    """Given-mode fractions over the whole of fp32: every exponent from the subnormals up to [2^24, 2^25) crossed with the
    significand fields {0, 1, 0x400000, 0x7fffff, three random ones}, both signs, and the values the header names."""
    rs = np.random.RandomState(53)
    mant = [0, 1, 0x400000, 0x7fffff] + rs.randint(2, 0x7fffff, size=3).tolist()
    words = [(ex << 23) | m for ex in range(0, 152) for m in mant]
    words += [w | 0x80000000 for w in words]
    special = np.array([0., -0., 0.25, 0.5, 0.75, 1., 2., 3., -0.5, -1., 1.5, 2.0 ** 24, -2.0 ** 24, 3e38, np.inf, -np.inf,
                        np.nan], F32)
    return np.concatenate([np.array(words, np.uint32).view(F32), special])


COS_BRANCHES = {"one", "unreduced", "none", "sin", "pi", "pi+sin", "2pi", "2pi+sin", "2pi+pi", "2pi+pi+sin"}


# ---- action values whose summation order decides the greedy action ---------------------------------------------------------------

def q_of_lane_descending(theta, n_actions):
    """NOT the kernel's order: k descending."""
    return q_of_lane(_f32(theta)[:, ::-1], n_actions)


def wq_of_lane_descending(theta, tau, n_actions):
    """NOT the kernel's order: j descending."""
    theta, tau = _f32(theta), _f32(tau)
    s = np.zeros((theta.shape[0], n_actions), F32)
    for j in range(theta.shape[1] - 1, -1, -1):
        s = s + (tau[:, j + 1] - tau[:, j])[:, None] * theta[:, j, :n_actions]
    return s


def order_sensitive_theta(seed, k, n_actions, rows=8, tau=None, candidates=4096):
    """theta [rows][k][A], k >= 3, A >= 2, in which the order of the sum over the fractions decides the greedy action:
    column A - 1 is column 0 with two entries moved by +1 / w_j1 and -1 / w_j2 (w the weights: 1 / k, or tau's steps), so
    the two action values agree to a few ulp; column 0 mixes magnitudes 1 .. 512, so that even three terms round; the other
    columns lie 1e5 below.  Of `candidates` random rows the first
    `rows` are kept in which the ascending and the descending sum pick different actions.  tau: one row f32[k + 1]."""
    assert k >= 3 and n_actions >= 2
    rs = np.random.RandomState(seed)
    theta = (rs.randn(candidates, k, n_actions) * 2).astype(F32) - F32(1e5)
    theta[:, :, 0] = (rs.randn(candidates, k) * 2.0 ** rs.randint(0, 10, size=(candidates, k))).astype(F32)
    w = np.full(k, 1. / k) if tau is None else np.diff(np.asarray(tau, np.float64))
    live = np.nonzero(w > 1e-3)[0]
    j1, j2 = live[0], live[-1]
    assert j1 != j2
    theta[:, :, n_actions - 1] = theta[:, :, 0]
    theta[:, j1, n_actions - 1] += F32(1. / w[j1])
    theta[:, j2, n_actions - 1] -= F32(1. / w[j2])
    if tau is None:
        up, down = q_of_lane(theta, n_actions), q_of_lane_descending(theta, n_actions)
    else:
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, F32), (candidates, k + 1)))
        up, down = wq_of_lane(theta, t, n_actions), wq_of_lane_descending(theta, t, n_actions)
    keep = np.nonzero(first_max(up) != first_max(down))[0][:rows]
    assert keep.size == rows, "only %d order-sensitive rows among %d" % (keep.size, candidates)
    return np.ascontiguousarray(theta[keep])


# ---- M-IQN with three equal maxima: the order of the soft sum, given the device's logf(3) -----------------------------------------

THREE = (5, 20, 63)             # the actions whose Q^next are bit-equal maxima


def three_maxima_case(seed, n, m, n_act=64, stride=64, batch=6):
    """tgt_next f32[B][N'][S] of multiples of 1/8: the columns THREE hold different values of magnitude up to 512 whose sums
    over the fractions are equal (every partial sum is exact, so Q^next is bit-equal), every other column lies 1000 lower.
    Then e = (1, 1, 1), s = 3, pi = fl(1 / 3) three times and lp = -(tau_e * logf(3)) for all three, and soft_j is a sum
    of three terms of mixed magnitude: its order shows.  tgt_cur: the taken action leads by 400 (lp == 0: no bonus)."""
    assert m >= 2 and n_act > max(THREE)
    rs = np.random.RandomState(seed)
    tgt = np.full((batch, m, stride), POISON, F32)
    tgt[:, :, :n_act] = rs.randint(-64, 65, size=(batch, m, n_act)) / 8. - 1000.
    cols = rs.randint(-4096, 4097, size=(batch, m, 3)) / 8.
    cols[:, m - 1, 1:] += (cols[:, :, :1].sum(axis=1) - cols[:, :, 1:].sum(axis=1))
    assert np.abs(cols).max() < 2 ** 16 and (cols.sum(axis=1) == cols.sum(axis=1)[:, :1]).all()
    tgt[:, :, list(THREE)] = cols
    pred, cur = _blocks(rs, batch, n, n_act, stride), _blocks(rs, batch, m, n_act, stride)
    act = rs.randint(0, n_act, size=batch).astype(np.uint8)
    cur[np.arange(batch), :, act] += F32(400)
    term = np.zeros(batch, np.uint8)
    term[0] = 1
    return dict(pred=pred, tau=rs.uniform(0.02, 0.98, size=(batch, n)).astype(F32), tgt=tgt, cur=cur, pol=None, act=act,
                ret=(rs.randn(batch) * 3).astype(F32), term=term, isw=(rs.rand(batch) + 0.1).astype(F32))


def three_maxima_targets(c, gamma_n, tau_e, alpha, log3, descending=False):
    """T [B][N'] of mloss_kernel on three_maxima_case, with log3 standing for the device's logf(3.f) (fp32)."""
    q = q_of_lane(c["tgt"], c["tgt"].shape[2])
    assert all((bits(q[:, a]) == bits(q[:, THREE[0]])).all() for a in THREE)
    pi = F32(1) / F32(3)
    lp = F32(0) - F32(tau_e) * F32(log3)
    soft = np.zeros(c["tgt"].shape[:2], F32)
    for a in (THREE[::-1] if descending else THREE):
        soft = soft + pi * (c["tgt"][:, :, a] - lp)
    keep = np.where(c["term"] != 0, F32(0), F32(1))
    bonus = F32(alpha) * F32(0)
    return (c["ret"] + bonus)[:, None] + keep[:, None] * (F32(gamma_n) * soft)
