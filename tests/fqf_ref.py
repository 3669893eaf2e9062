"""Shared by tests/test_fqf_host.py and tests/test_fqf_gpu.py: float64 restatements of arl_fqf_fractions, arl_fqf_act's
weighted action values and arl_fqf_loss (include/accel_rl_hip.h, "Fully parameterized quantile functions"), the input
cases of the loss tests, and the derived error bounds (repeated in DESIGN.md, section 17).

Bounds, EPS = 2^-24 (one fp32 rounding), every reference built from the kernel's own fp32 inputs cast up, so only that
launch's roundings count; no intermediate is subnormal at the tests' magnitudes.

Fractions, from logits with spread C = max_k l_k - min_k l_k; expf / logf at the OpenCL full-profile 3 ulp:
  c_k = l_k - v rounds once (|c_k| EPS, which expf turns into a relative error); s is a butterfly (6 additions):
      e_k relative (C + 3) EPS;  s relative (C + 9) EPS;  q_k relative (2 C + 13) EPS  ->  atol (2 C + 16) EPS q_k
  tau_i is a chain of at most N additions of those q (sum <= 1)        ->  atol (N + 2 C + 18) EPS  (tau_hat likewise)
  logq_k = c_k - logf(s): C EPS + (C + 9) EPS + 3 EPS ln N + (C + ln N) EPS  ->  atol (3 C + 32) EPS
  H = -sum q_k logq_k (a butterfly, sum_k q_k |logq_k| = H <= ln N)    ->  atol ((2 C + 23) ln N + 3 C + 32) EPS

Loss.  dtheta, loss_rows, priorities: the bound of tests/test_iqn_gpu.py with N' = N.
dlogits, per sample b and column k, with R_b = sum_{i=1}^{N-1} (|2 pred_mid(i) - pred(i)| + |pred(i - 1)|) >= sum_i |g_i|:
  g_i: two subtractions, sum_i |delta g_i| <= 2 EPS R_b;  G: N - 1 products (tau_i <= 1) and a chain of N - 2 additions,
  |delta G| <= (N + 1) EPS R_b;  S_k: a chain of at most N - 2 additions, |delta S_k| <= N EPS R_b;  S_k - G (|.| <= 2 R_b), its
  product with q_k, the sum of the two terms, w_b (one division) and the product with it: (2 + 2 + 2 + 4) EPS R_b more;
  the entropy term ent_coef (q_k (logq_k + H)): three roundings of its own, then the same sum and w_b:
      atol_bk = EPS w_b q_k [ (2 N + 16) R_b + 8 ent_coef (|logq_k| + H_b) ]
  frac_rows[b] = w_b G:  atol_b = (N + 4) EPS w_b R_b.
"""
import numpy as np
import torch

EPS = 2.0 ** -24
POISON = 1e9                    # what the padding columns of every input hold: they must be ignored


# ---- fractions ----------------------------------------------------------------------------------------------------

def ref_fractions(logits):
    """logits float64 [B][N] (a torch tensor, possibly part of an autograd graph) -> dict(tau [B][N + 1], tau_hat [B][N],
    q, logq [B][N], H [B]), everything differentiable."""
    assert logits.dtype == torch.float64
    c = logits - logits.max(dim=1, keepdim=True).values
    logq = c - torch.log(torch.exp(c).sum(dim=1, keepdim=True))
    q = torch.exp(logq)
    tau = torch.cat([torch.zeros_like(q[:, :1]), torch.cumsum(q, dim=1)], dim=1)
    tau = torch.cat([tau[:, :-1], torch.ones_like(q[:, :1])], dim=1)        # tau_N = 1 exactly
    return dict(tau=tau, tau_hat=0.5 * (tau[:, :-1] + tau[:, 1:]), q=q, logq=logq, H=-(q * logq).sum(dim=1))


def fraction_bounds(logits, n):
    """(q relative factor, tau atol, logq atol, H atol) for fp32 logits [B][n], per the derivation above."""
    spread = float((logits.max(axis=1) - logits.min(axis=1)).max())
    ln_n = np.log(max(n, 2))
    return ((2 * spread + 16) * EPS, (n + 2 * spread + 18) * EPS, (3 * spread + 32) * EPS,
            ((2 * spread + 23) * ln_n + 3 * spread + 32) * EPS)


def ref_weighted_q(theta, tau):
    """theta float64 [B][N][A], tau float64 [B][N + 1] -> Q [B][A] = sum_j (tau_{j+1} - tau_j) theta(j, a)."""
    return ((tau[:, 1:] - tau[:, :-1])[:, :, None] * theta).sum(dim=1)


# ---- fraction loss ------------------------------------------------------------------------------------------------

def ref_dlogits(q, logq, H, tau, g, w, ent_coef):
    """The closed form of arl_fqf_loss in float64.  q, logq [B][N], H [B], tau [B][N + 1], g [B][N - 1] (g_1 .. g_{N-1}),
    w [B].  Returns (dlogits [B][N], frac_rows [B] = w G)."""
    b, n = q.shape
    G = (g * tau[:, 1:n]).sum(dim=1)
    S = torch.zeros_like(q)                                     # S_k = sum_{i = k + 1}^{N - 1} g_i
    if n > 1:
        S[:, :n - 1] = torch.flip(torch.cumsum(torch.flip(g, dims=[1]), dim=1), dims=[1])
    d = w[:, None] * (q * (S - G[:, None]) + ent_coef * q * (logq + H[:, None]))
    return d, w * G


def wasserstein_1(quantile_fn, tau, points=20001):
    """sum_i integral over [tau_i, tau_{i+1}] of |F^-1(omega) - F^-1(tau_hat_i)|, trapezoids on `points` nodes per
    interval; differentiable in tau (the nodes move with the interval's ends).  tau float64 [N + 1]."""
    s = torch.linspace(0., 1., points, dtype=torch.float64)
    lo, hi = tau[:-1, None], tau[1:, None]
    omega = lo + s[None, :] * (hi - lo)
    f = (quantile_fn(omega) - quantile_fn(0.5 * (lo + hi))).abs()
    return (0.5 * (f[:, 1:] + f[:, :-1]).sum(dim=1) / (points - 1) * (hi - lo)[:, 0]).sum()


# ---- quantile loss (arl_iqn_loss's formulas with the weighted selection) ------------------------------------------------

def ref_fqf_loss(pred, mid, fr, tgt, pol, act, ret, term, isw, gamma_n, kappa, ent_coef):
    """float64.  pred [B][N][A] (may require grad), mid [B][N - 1][A] or None, fr = dict(tau, tau_hat, q, logq, H) as
    ref_fractions returns (here: the kernel's fp32 inputs cast up), tgt / pol [B][N][A] (pol None: not double DQN).
    Returns a dict: rows (differentiable in pred), loss_b, dth (closed form), T, a_next, margin, w, g, R, dlogits, frac."""
    b, n, n_act = pred.shape
    ar = torch.arange(b)
    tau, tau_hat = fr["tau"], fr["tau_hat"]
    qsel = ref_weighted_q(pol if pol is not None else tgt, tau)
    a_next = qsel.argmax(dim=1)
    margin = float("inf")
    if n_act > 1:
        top2 = torch.topk(qsel, 2, dim=1).values
        margin = (top2[:, 0] - top2[:, 1]).min().item()
    keep = 1. - term.double()
    T = ret.double()[:, None] + keep[:, None] * (gamma_n * tgt[ar, :, a_next])          # [B][j]
    th = pred[ar, :, act.long()]                                                        # [B][i]
    u = T[:, None, :] - th[:, :, None]                                                  # [B][i][j]
    ind = (u < 0).double()                                                              # u == 0: not negative
    wt = (tau_hat[:, :, None] - ind).abs().detach()
    if kappa > 0:
        au = u.abs()
        rho = wt * torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa
        dth = -(wt * u.clamp(-kappa, kappa) / kappa).sum(dim=2)
    else:
        rho = wt * u.abs()
        dth = -(tau_hat[:, :, None] - ind).sum(dim=2)
    loss_b = rho.sum(dim=(1, 2)) / n
    w = (isw.double() if isw is not None else torch.ones(b, dtype=torch.float64)) / b
    thd = th.detach()
    if n > 1:
        two_mid = 2. * mid[ar, :, act.long()]                                           # [B][N - 1]
        g = (two_mid - thd[:, 1:]) - thd[:, :-1]
        R = ((two_mid - thd[:, 1:]).abs() + thd[:, :-1].abs()).sum(dim=1)
    else:
        g, R = torch.zeros(b, 0, dtype=torch.float64), torch.zeros(b, dtype=torch.float64)
    dlogits, frac = ref_dlogits(fr["q"], fr["logq"], fr["H"], tau, g, w, ent_coef)
    return dict(rows=w * loss_b, loss_b=loss_b.detach(), dth=(dth * (w / n)[:, None]).detach(), T=T.detach(),
                a_next=a_next, margin=margin, w=w, g=g, R=R, dlogits=dlogits, frac=frac)


def dlogits_atol(ref, fr, n, ent_coef):
    """atol_bk of the derivation above, [B][N], and frac_rows' atol_b, [B]."""
    a = EPS * ref["w"][:, None] * fr["q"] * ((2 * n + 16) * ref["R"][:, None] +
                                             8 * ent_coef * (fr["logq"].abs() + fr["H"][:, None]))
    return a, (n + 4) * EPS * ref["w"] * ref["R"]


# ---- input cases --------------------------------------------------------------------------------------------------

def block(rs, batch, r, n_act, stride, scale=2.):
    t = (rs.randn(batch, r, stride) * scale).astype(np.float32)
    t[:, :, n_act:] = POISON
    return t


def selecting(rs, t, n_act, weights):
    """tests/test_iqn_gpu.py:_selecting under the FQF selection's weights (float64 [B][R], rows summing to 1): every
    action column of block `t` [B][R][S] is centred in its WEIGHTED mean over the fractions, given a weighted mean in
    [-0.4, 0.4], and one randomly chosen action gets +1.0 at every fraction: the margin of the weighted Q is at least
    1 - 0.8 = 0.2 (up to the fp32 rounding of the centring; the callers assert it on every sample)."""
    batch = t.shape[0]
    mean = (weights[:, :, None] * t[:, :, :n_act].astype(np.float64)).sum(axis=1, keepdims=True)
    t[:, :, :n_act] -= mean.astype(np.float32)
    t[:, :, :n_act] += rs.uniform(-0.4, 0.4, size=(batch, 1, n_act)).astype(np.float32)
    chosen = rs.randint(0, n_act, size=batch)
    t[np.arange(batch), :, chosen] += np.float32(1.0)
    return chosen
