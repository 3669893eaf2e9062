"""TEST INFRASTRUCTURE for PQN (csrc/layernorm.hip: arl_ln_relu_fwd / _bwd, csrc/qlambda_scan.hip: arl_qlambda_scan,
csrc/dqn.hip: arl_q_regress_loss, AtariPqnPolicy, PQN).  The reference has none of it, so the yardsticks are
restatements of include/accel_rl_hip.h's text in NumPy / float64 torch, sharing no code with the kernels:

  ln_relu_fwd64 / ln_relu_bwd64     LayerNorm + rectifier in float64; the backward pass takes the mask as an input
  ln_fwd_bound / ln_bwd_bound       the first-order error bounds of DESIGN.md 22 (u = 2^-24), from the header's
                                    summation order (ln_shape restates the header's dispatch table)
  qlambda_scan64                    the Q(lambda) walk, operation for operation (the kernel equals it bit for bit)
  q_regress64 / q_regress32         the regression loss in float64 with arl_dqn_loss's bound for a plain row
                                    (tests/drq_ref.py's, k = m = 1, no dueling merge, exact target), and in fp32
                                    operation for operation
  ref_params / ref_q                the float64 torch network on the reference layout, for whole-step checks

Bounds, with D = 4 V + log2(LPR) the additions an element of a row sum passes through, n = width, per row:
  A1 = sum |z_j|, c_j = z_j - mean, C1 = sum |c_j|, Q = sum c_j^2, v = Q / n, s = v + eps, r = s^-1/2
  mean     E_mu = u (D A1 / n + |mean|)                       (the sum, the division)
  c_j      E_c  = E_mu + u |c_j|
  Q        E_Q  = 2 E_mu C1 + (3 + D) u Q                     (2 |c_j| E_c + u c_j^2 per square, D u Q for the sum)
  s        E_s  = E_Q / n + u v + u s                         (the division, the sum with eps)
  rstd     E_r  = r (E_s / (2 s) + 4 u)                       (sqrtf and the division: 2 u each allowed)
  xhat_j   E_x  = r E_mu + |xhat_j| (E_s / (2 s) + 6 u)       (E_c r + |c_j| E_r + the product's u)
  y_j      E_y  = |gamma_j| E_x + u |gamma_j xhat_j| + u |a_j|,  a_j = gamma_j xhat_j + beta_j   (max(0, .) is 1-Lipschitz)
Backward, h_j = g_j gamma_j, H1 = sum |h_j|, P1 = sum |h_j xhat_j|, m1 = sum h / n, m2 = sum h xhat / n,
t_j = (h_j - m1) - xhat_j m2, with the forward's fp32 stats (so xhat carries E_x, rstd E_r):
  m1       E_1  = (D + 1) u H1 / n + u |m1|
  m2       E_2  = (sum |h_j| E_x,j + (D + 2) u P1) / n + u |m2|
  t_j      E_t  = u |h_j| + E_1 + u |h_j - m1| + E_x |m2| + |xhat_j| E_2 + u |xhat_j m2| + u |t_j|
  dz_j     E_dz = r E_t + E_r |t_j| + u |dz_j|
  dgamma_j sum_rows (|g| E_x + u |g xhat|) + Dc u sum_rows |g xhat|;   dbeta_j  Dc u sum_rows |g|
  with Dc = iters + RPB + (grid < 128 ? ceil(grid / 16) + 15 : ceil(grid / 64) + 63) the additions a term of a column
  sum passes through (per-slot walk, slots of a block, arl_fold_many's groups and their fold)."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


# ---- LayerNorm + rectifier ----------------------------------------------------------------------------------------

def ln_stats64(z, eps):
    z = np.asarray(z, np.float64)
    mean = z.mean(axis=1, keepdims=True)
    var = ((z - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    return mean, rstd, (z - mean) * rstd


def ln_relu_fwd64(z, gamma, beta, eps):
    """-> (y, mean [rows], rstd [rows]) in float64 from fp32 inputs."""
    mean, rstd, xhat = ln_stats64(z, eps)
    a = np.asarray(gamma, np.float64) * xhat + np.asarray(beta, np.float64)
    return np.maximum(a, 0.0), mean[:, 0], rstd[:, 0]


def ln_relu_bwd64(dy, mask, z, gamma, eps):
    """-> (dz, dgamma, dbeta); mask: bool [rows][width], the rectifier's y > 0 (an input: no element is excluded)."""
    _, rstd, xhat = ln_stats64(z, eps)
    g = np.where(mask, np.asarray(dy, np.float64), 0.0)
    h = g * np.asarray(gamma, np.float64)
    m1 = h.mean(axis=1, keepdims=True)
    m2 = (h * xhat).mean(axis=1, keepdims=True)
    return rstd * (h - m1 - xhat * m2), (g * xhat).sum(axis=0), g.sum(axis=0)


def ln_shape(rows, width):
    """The header's dispatch: (LPR, V, grid, iters, D, Dc)."""
    lpr = 8 if width <= 32 else 16 if width <= 64 else 64
    v = 1 if width <= 256 else 2 if width <= 512 else 4
    rpb = 256 // lpr
    blocks = -(-rows // rpb)
    grid = min(blocks, 256)
    iters = -(-blocks // grid)
    fold = -(-grid // 16) + 15 if grid < 128 else -(-grid // 64) + 63
    return lpr, v, grid, iters, 4 * v + int(np.log2(lpr)), iters + rpb + fold


def _ln_terms(z, eps, depth):
    z = np.asarray(z, np.float64)
    n = z.shape[1]
    mean, rstd, xhat = ln_stats64(z, eps)
    c = z - mean
    a1, c1 = np.abs(z).sum(axis=1, keepdims=True), np.abs(c).sum(axis=1, keepdims=True)
    q = (c * c).sum(axis=1, keepdims=True)
    v = q / n
    s = v + float(np.float32(eps))
    e_mu = U * (depth * a1 / n + np.abs(mean))
    e_q = 2 * e_mu * c1 + (3 + depth) * U * q
    e_s = e_q / n + U * v + U * s
    e_r = rstd * (e_s / (2 * s) + 4 * U)
    e_x = rstd * e_mu + np.abs(xhat) * (e_s / (2 * s) + 6 * U)
    return dict(mean=mean, rstd=rstd, xhat=xhat, e_mu=e_mu, e_r=e_r, e_x=e_x)


def ln_fwd_bound(z, gamma, beta, eps):
    """-> (E_y [rows][width], E_mean [rows], E_rstd [rows])."""
    depth = ln_shape(*np.shape(z))[4]
    t = _ln_terms(z, eps, depth)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    gx = gamma * t["xhat"]
    e_y = np.abs(gamma) * t["e_x"] + U * np.abs(gx) + U * np.abs(gx + beta)
    return e_y, t["e_mu"][:, 0], t["e_r"][:, 0]


def ln_bwd_bound(dy, mask, z, gamma, eps):
    """-> (E_dz [rows][width], E_dgamma [width], E_dbeta [width])."""
    rows, n = np.shape(z)
    depth, col_depth = ln_shape(rows, n)[4:]
    t = _ln_terms(z, eps, depth)
    xhat, e_x, rstd, e_r = t["xhat"], t["e_x"], t["rstd"], t["e_r"]
    g = np.where(mask, np.asarray(dy, np.float64), 0.0)
    h = g * np.asarray(gamma, np.float64)
    hx = h * xhat
    m1, m2 = h.mean(axis=1, keepdims=True), hx.mean(axis=1, keepdims=True)
    tt = (h - m1) - xhat * m2
    e_1 = (depth + 1) * U * np.abs(h).sum(axis=1, keepdims=True) / n + U * np.abs(m1)
    e_2 = ((np.abs(h) * e_x).sum(axis=1, keepdims=True) + (depth + 2) * U * np.abs(hx).sum(axis=1, keepdims=True)) / n + \
        U * np.abs(m2)
    e_t = U * np.abs(h) + e_1 + U * np.abs(h - m1) + e_x * np.abs(m2) + np.abs(xhat) * e_2 + U * np.abs(xhat * m2) + \
        U * np.abs(tt)
    e_dz = rstd * e_t + e_r * np.abs(tt) + U * np.abs(rstd * tt)
    gx = np.abs(g * xhat)
    e_dg = (np.abs(g) * e_x + U * gx).sum(axis=0) + col_depth * U * gx.sum(axis=0)
    e_db = col_depth * U * np.abs(g).sum(axis=0)
    return e_dz, e_dg, e_db


# ---- Q(lambda) ----------------------------------------------------------------------------------------------------

def qlambda_scan64(q, q_last, n_actions, rewards, dones, discount, lam):
    """q f32[n_env][T][S], q_last f32[n_env][S], rewards f32[n_env][T], dones [n_env][T] -> returns f32[n_env][T]:
    the header's walk in float64, one Python float operation per stated operation."""
    n_env, horizon = rewards.shape
    b = np.concatenate([q[:, 1:, :n_actions].max(axis=2), q_last[:, None, :n_actions].max(axis=2)], axis=1)
    out = np.zeros((n_env, horizon), np.float32)
    discount, lam = float(discount), float(lam)
    for e in range(n_env):
        big_r = 0.0
        for t in range(horizon - 1, -1, -1):
            bt = float(b[e, t])
            if t == horizon - 1:
                nxt = discount * bt
            else:
                nxt = discount * (bt + lam * (big_r - bt))
            big_r = float(rewards[e, t]) + (0.0 if dones[e, t] else nxt)
            out[e, t] = np.float32(big_r)
    return out


# ---- regression loss ------------------------------------------------------------------------------------------------

def q_regress64(q, idx, actions, returns, n_actions, delta_clip):
    """float64 on the same fp32 inputs -> dict(dq [B][A], rows, td, dq_tol [B], rows_tol, td_tol, ok): arl_dqn_loss's bound
    for a plain row with an exact target (E_q = E_y = 0: E_d = u |d|)."""
    bsz = q.shape[0]
    src = np.arange(bsz) if idx is None else np.asarray(idx)
    act = np.minimum(actions[src].astype(np.int64), n_actions - 1)
    cl = 0. if delta_clip is None else float(np.float32(delta_clip))
    ar = np.arange(bsz)
    d = returns[src].astype(np.float64) - q[ar, act].astype(np.float64)
    ad = np.abs(d)
    e_d = U * ad
    w = 1.0 / bsz
    if cl > 0:
        ok = np.abs(ad - cl) > 2 * e_d
        hub = ad > cl
        loss = np.where(hub, cl * (ad - cl / 2), 0.5 * d * d)
        slope = np.where(hub, np.sign(d) * cl, d)
    else:
        ok, hub = np.ones(bsz, bool), np.zeros(bsz, bool)
        loss, slope = 0.5 * d * d, d
    p = np.minimum(ad, cl) if cl > 0 else ad
    gq = -(w * slope)
    dq = np.zeros((bsz, n_actions))
    dq[ar, act] = gq
    return dict(dq=dq, rows=w * loss, td=p, ok=ok, dq_tol=np.where(hub, 0., w * e_d) + 5 * U * np.abs(gq),
                rows_tol=w * (np.abs(slope) * e_d + 5 * U * loss), td_tol=e_d + U * p)


def q_regress32(q, idx, actions, returns, n_actions, delta_clip):
    """arl_q_regress_loss in fp32, in the header's order -> (dq f32[B][S], loss_rows f32[B], td_abs f32[B])."""
    bsz, stride = q.shape
    src = np.arange(bsz) if idx is None else np.asarray(idx)
    act = np.minimum(actions[src].astype(np.int64), n_actions - 1)
    cl = np.float32(0. if delta_clip is None else delta_clip)
    ar = np.arange(bsz)
    w = np.float32(1) / np.float32(bsz)
    d = returns[src] - q[ar, act]
    ad = np.abs(d)
    loss, slope = np.float32(0.5) * (d * d), d.copy()
    if cl > 0:
        hub = ad > cl
        loss = np.where(hub, cl * (ad - cl / np.float32(2)), loss)
        slope = np.where(hub, np.where(d > 0, cl, -cl), slope)
    dq = np.zeros((bsz, stride), np.float32)
    dq[ar, act] = -(w * slope)
    return dq, (w * loss).astype(np.float32), (np.minimum(ad, cl) if cl > 0 else ad).astype(np.float32)


# ---- the float64 network on the reference layout ------------------------------------------------------------------

def ref_params(policy, flat_bucket):
    """The reference-layout tensors of a bucket, float64, requiring gradients (policy._ref_shapes' order)."""
    fl = policy.bucket_to_reference(flat_bucket)
    out, pos = [], 0
    for shape in policy._ref_shapes:
        m = int(np.prod(shape))
        out.append(torch.from_numpy(fl[pos:pos + m].reshape(shape).astype(np.float64)).requires_grad_())
        pos += m
    return out


def _ln_relu_torch(z, gamma, beta, eps, dim):
    mean = z.mean(dim=dim, keepdim=True)
    var = ((z - mean) ** 2).mean(dim=dim, keepdim=True)
    shape = [1] * z.dim()
    shape[dim] = -1
    return F.relu(gamma.view(shape) * ((z - mean) / torch.sqrt(var + eps)) + beta.view(shape))


def ref_q(rp, spec, x, eps):
    """Plain float64 torch: x [B, C, H, W] scaled observations -> Q [B, A].  rp: conv (W, b).., hidden (W, b).., output
    (W, b), then (gamma, beta) per conv layer and per hidden layer; conv W (out, in, kh, kw) of a true convolution, dense W
    (in, out) on (c, h, w)-ordered inputs; a conv activation is normalised over its channels, a dense one over its units."""
    n_conv, n_hid = len(spec["conv_filters"]), len(spec["hidden_sizes"])
    ln = 2 * (n_conv + n_hid + 1)
    eps = float(np.float32(eps))
    k = 0
    for i in range(n_conv):
        z = F.conv2d(x, rp[k].flip(2, 3), rp[k + 1], stride=spec["conv_strides"][i], padding=tuple(spec["conv_pads"][i]))
        x = _ln_relu_torch(z, rp[ln + 2 * i], rp[ln + 2 * i + 1], eps, 1)
        k += 2
    x = x.flatten(1)
    for j in range(n_hid):
        x = _ln_relu_torch(x @ rp[k] + rp[k + 1], rp[ln + 2 * (n_conv + j)], rp[ln + 2 * (n_conv + j) + 1], eps, 1)
        k += 2
    return x @ rp[k] + rp[k + 1]
