"""NumPy float64 restatements of the two PopArt entry points (include/accel_rl_hip.h, "PopArt"), each in the order its
text states; written from the header's text, sharing no code with csrc/popart.hip.  Scalars are np.float64 throughout, so
every operation rounds as the device's float64 does (no fused multiply-add).  The workgroup's summation order is the one
the RND restatement already spells out (rnd_ref._workgroup_sum)."""
import numpy as np

from rnd_ref import _workgroup_sum

F32, F64 = np.float32, np.float64
INIT_STATS = (0., 1., 1., 0.)


def denorm(value_n, last_n, stats):
    """value_n f32 [R], last_n f32 [N], stats (mu, nu, sigma, n_updates) -> (value f32 [R], last_value f32 [N])"""
    mu, sigma = F64(stats[0]), F64(stats[2])
    return ((sigma * value_n.astype(F64) + mu).astype(F32), (sigma * last_n.astype(F64) + mu).astype(F32))


def step(returns, advantages, valids, beta, sigma_min, sigma_max, stats, w_value, b_value):
    """returns f32 [R], advantages f32 [R] or None, valids i8 [R] or None, w_value f32 [hid], b_value f32 [1] ->
    (returns', advantages' or None, stats' f64 [4], w_value', b_value', diag2 f32 [2]); no argument is written."""
    beta, sigma_min, sigma_max = F64(beta), F64(sigma_min), F64(sigma_max)
    mu, nu, sigma, n_upd = (F64(s) for s in stats)
    valid = np.ones(returns.shape, bool) if valids is None else valids != 0
    g = returns.astype(F64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        # 1. (a skipped row adds nothing: the zero it adds here leaves every partial sum's bits as they are)
        cnt = _workgroup_sum(np.where(valid, F64(1.), F64(0.)))
        s1 = _workgroup_sum(np.where(valid, g, F64(0.)))
        s2 = _workgroup_sum(np.where(valid, g * g, F64(0.)))
        m1, m2 = s1 / cnt, s2 / cnt
    ok = bool(cnt > 0 and np.isfinite(m1) and np.isfinite(m2))
    w_new, b_new = w_value.copy(), b_value.copy()
    mu_n, sigma_n = mu, sigma
    stats_new = np.array([mu, nu, sigma, n_upd], dtype=F64)
    if ok:
        # 2.
        mu_n = (F64(1.) - beta) * mu + beta * m1
        nu_n = (F64(1.) - beta) * nu + beta * m2
        var = nu_n - mu_n * mu_n
        var = var if var > 0 else F64(0.)
        sd = np.sqrt(var)
        sd = sd if sd > sigma_min else sigma_min
        sd = sd if sd < sigma_max else sigma_max
        sigma_n = sd
        stats_new = np.array([mu_n, nu_n, sigma_n, n_upd + F64(1.)], dtype=F64)
        # 3.
        ratio = sigma / sigma_n
        # (rounded to the arrays' own type: float32 on the device; the host tests also walk float64 weights)
        w_new = (w_value.astype(F64) * ratio).astype(w_value.dtype)
        b_new = np.array([((sigma * F64(b_value[0]) + mu) - mu_n) / sigma_n], dtype=F64).astype(b_value.dtype)
    # 4.
    with np.errstate(over="ignore", invalid="ignore"):
        ret_new = np.where(valid, ((g - mu_n) / sigma_n).astype(F32), F32(0.)).astype(F32)
        adv_new = None if advantages is None else \
            np.where(valid, (advantages.astype(F64) / sigma_n).astype(F32), F32(0.)).astype(F32)
    diag = np.array([mu_n, sigma_n], dtype=F64).astype(F32)
    return ret_new, adv_new, stats_new, w_new, b_new, diag


def unnormalized_head(h, w_value, b_value, stats):
    """float64: sigma (h . w + b) + mu for hidden rows h f64 [B, hid] -- what the preservation step keeps."""
    mu, sigma = F64(stats[0]), F64(stats[2])
    return sigma * (h.astype(F64) @ w_value.astype(F64) + F64(b_value[0])) + mu
