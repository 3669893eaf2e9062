"""NumPy float64 restatements of the four RND entry points (include/accel_rl_hip.h, "Random network distillation"), each
in the order its text states; written from the header's text, sharing no code with csrc/rnd.hip.  Scalars are np.float64
throughout, so every operation rounds as the device's float64 does (no fused multiply-add)."""
import numpy as np

F64 = np.float64
VAR_EPS = F64(1e-8)


def next_frames(observations, extra_observations, n_env, horizon):
    """u8 [n_env * horizon, H, W]: the newest plane of the observation that follows every transition."""
    obs = observations.reshape((n_env, horizon) + observations.shape[1:])
    nxt = np.concatenate([obs[:, 1:], extra_observations[:, None]], axis=1)
    return nxt.reshape((n_env * horizon,) + observations.shape[1:])[:, -1]


def chan_merge(na, mean, m2, nb, mean_b, m2_b):
    """(count', mean', m2') -- arrays or scalars, elementwise"""
    na, nb = F64(na), F64(nb)
    w = nb / (na + nb)
    delta = mean_b - mean
    return na + nb, mean + delta * w, (m2 + m2_b) + ((delta * delta) * na) * w


def obs_stats(frames, count, mean, m2):
    """frames u8 [R, H, W]; count float, mean / m2 f64 [H * W] -> the merged state"""
    r = frames.shape[0]
    x = frames.reshape(r, -1).astype(np.uint64)
    sx, sxx = x.sum(axis=0, dtype=np.uint64), (x * x).sum(axis=0, dtype=np.uint64)
    num = np.uint64(r) * sxx - sx * sx
    nb = F64(r)
    mean_b = sx.astype(F64) / nb
    m2_b = num.astype(F64) / nb
    return chan_merge(count, mean, m2, nb, mean_b, m2_b)


def obs_prepare(frames, count, mean, m2):
    """f32 [B, H, W, 4] from u8 frames [B, H, W]"""
    b = frames.shape[0]
    sd = np.sqrt(m2 / F64(count) + VAR_EPS)
    z = (frames.reshape(b, -1).astype(F64) - mean) / sd
    z = np.minimum(np.maximum(z, F64(-5.)), F64(5.))
    out = np.zeros(frames.shape + (4,), np.float32)
    out[..., 0] = z.astype(np.float32).reshape(frames.shape)
    return out


def _halving(v):
    """a wave's 64 lane values added by halving shuffles, offsets 32 .. 1: lane 0's result"""
    v = np.array(v, dtype=F64)
    off = 32
    while off:
        v = v + np.concatenate([v[off:], np.zeros(off, F64)])      # (lanes past the end: what they add never reaches lane 0)
        off >>= 1
    return v[0]


def _workgroup_sum(values):
    """thread t of 1 024 adds positions t, t + 1 024, ... ascending; waves by halving shuffles; 16 waves in wave order"""
    values = np.asarray(values, dtype=F64)
    n = values.size
    pad = np.zeros((n + 1023) // 1024 * 1024, F64)
    pad[:n] = values
    per = np.zeros(1024, F64)
    for row in pad.reshape(-1, 1024):
        per = per + row
    if n < 1024:                 # (threads past the end hold their initial 0.0, which the padding already is)
        pass
    total = F64(0.)
    for w in range(16):
        total = total + _halving(per[64 * w:64 * w + 64])
    return total


def error(pred, targ, want_grad):
    """pred, targ f32 [B, E] -> err f32 [B] (, dpred f32 [B, E], loss f32)"""
    b, e = pred.shape
    d = pred.astype(F64) - targ.astype(F64)
    sq = d * d
    lanes = np.zeros((b, 64), F64)
    for k in range((e // 4 + 63) // 64):
        for j in range(4):
            cols = 4 * (np.arange(64) + 64 * k) + j
            ok = cols < e
            lanes[:, ok] = lanes[:, ok] + sq[:, cols[ok]]
    off = 32
    v = lanes
    while off:
        v = v + np.concatenate([v[:, off:], np.zeros((b, off), F64)], axis=1)
        off >>= 1
    err = (v[:, 0] / F64(e)).astype(np.float32)
    if not want_grad:
        return err
    dpred = ((F64(2.) * d) / (F64(e) * F64(b))).astype(np.float32)
    loss = np.float32(_workgroup_sum(err.astype(F64)) / F64(b))
    return err, dpred, loss


def reward_mix(err, r_ext, rho, moments, gamma_int, c_ext, c_int):
    """err, r_ext f32 [N, T]; rho f64 [N]; moments (count, mean, m2) -> r_mix f32 [N, T], rho', moments', diag2 f32[2]"""
    n, t = err.shape
    gamma_int, c_ext, c_int = F64(gamma_int), F64(c_ext), F64(c_int)
    rho = np.array(rho, dtype=F64)
    v = np.zeros((n, t), F64)
    e64 = err.astype(F64)
    for s in range(t):
        rho = gamma_int * rho + e64[:, s]
        v[:, s] = rho
    flat = v.reshape(-1)
    m = F64(n * t)
    mean_b = _workgroup_sum(flat) / m
    dev = flat - mean_b
    m2_b = _workgroup_sum(dev * dev)
    count, mean, m2 = chan_merge(moments[0], F64(moments[1]), F64(moments[2]), m, mean_b, m2_b)
    sd = np.sqrt(m2 / count + VAR_EPS)
    a = c_ext * r_ext.astype(F64)
    b = c_int * (e64 / sd)
    r_mix = np.where(b == 0, a, a + b).astype(np.float32)
    diag = np.array([_workgroup_sum(e64.reshape(-1)) / m, sd], dtype=F64).astype(np.float32)
    return r_mix, rho, np.array([count, mean, m2], dtype=F64), diag
