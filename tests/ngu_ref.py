"""NumPy float64 restatements of csrc/episodic.hip (include/accel_rl_hip.h states the expressions): plain loops, the
kernels' operation order."""
import numpy as np

F32, F64 = np.float32, np.float64


def _dist(a, b):
    d = F64(0.0)
    for x, y in zip(a, b):
        diff = F64(x) - F64(y)
        d = d + diff * diff
    return d


def knn(emb, dones, mem, n_ins, k):
    """emb f32[n_env, T, E], dones [n_env, T], mem f32[n_env, M, E], n_ins i32[n_env] -> (knn f64[n_env * T, k], m i32[n_env
    * T], mem, n_ins): the sequential definition -- search the ring, then insert, row by row."""
    n_env, T, E = emb.shape
    M = mem.shape[1]
    mem, n_ins = mem.copy(), n_ins.copy()
    out, m = np.full((n_env * T, k), np.inf, F64), np.zeros(n_env * T, np.int32)
    for n in range(n_env):
        for t in range(T):
            if dones[n, t]:
                mem[n], n_ins[n] = 0, 0
            else:
                held = range(max(0, n_ins[n] - M), n_ins[n])
                d = sorted(_dist(emb[n, t], mem[n, i % M]) for i in held)[:k]
                out[n * T + t, :len(d)], m[n * T + t] = d, len(d)
            mem[n, n_ins[n] % M] = emb[n, t]
            n_ins[n] += 1
    return out, m, mem, n_ins


def _block_sum(per_thread):
    """arl::block_sum_d of 1 024 threads: every wave by halving shuffles (offsets 32 .. 1), then the waves in order"""
    x = np.asarray(per_thread, F64).reshape(16, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        x[:, :off] = x[:, :off] + x[:, off:2 * off]
    s = F64(0.0)
    for w in range(16):
        s = s + x[w, 0]
    return s


def _strided(values):
    """thread t's sum of values[t], values[t + 1024], ... in ascending order, for t = 0 .. 1023"""
    acc = np.zeros(1024, F64)
    for j, v in enumerate(values):
        acc[j % 1024] = acc[j % 1024] + F64(v)
    return acc


def mix(knn_d, m, err, r_ext, dist_mean, err_moments, eps, c, xi, s_max, mod_clip, c_ext, c_int):
    """-> (r_mix f32[rows], dist_mean, err_moments, diag f32[3])"""
    rows = m.size
    dist_mean, err_moments = dist_mean.copy(), err_moments.copy()
    acc = np.zeros(1024, F64)
    for j in range(rows):
        for i in range(m[j]):
            acc[j % 1024] = acc[j % 1024] + knn_d[j, i]
    S, nb = _block_sum(acc), F64(m.sum())           # (the count is a sum of small integers: exact in any order)
    mean = dist_mean[1]
    if nb > 0:
        w = nb / (dist_mean[0] + nb)
        mean = mean + (S / nb - mean) * w
        dist_mean[:] = dist_mean[0] + nb, mean
    mu = sd = None
    if err is not None:
        nr = F64(rows)
        mean_e = _block_sum(_strided(err)) / nr
        m2_e = _block_sum(_strided([(F64(e) - mean_e) * (F64(e) - mean_e) for e in err]))
        na = err_moments[0]
        w = nr / (na + nr)
        delta = mean_e - err_moments[1]
        mu = err_moments[1] + delta * w
        m2 = (err_moments[2] + m2_e) + ((delta * delta) * na) * w
        err_moments[:] = na + nr, mu, m2
        sd = np.sqrt(m2 / (na + nr) + 1e-8)
    denom = max(mean, F64(1e-8))
    r_mix, r_epi, mod = np.zeros(rows, F32), np.zeros(rows, F64), np.ones(rows, F64)
    for j in range(rows):
        if m[j] > 0:
            ks = F64(0.0)
            for i in range(m[j]):
                ks = ks + eps / (max(knn_d[j, i] / denom - xi, F64(0.0)) + eps)
            s = np.sqrt(ks) + c
            r_epi[j] = 0.0 if s > s_max else 1.0 / s
        if err is not None:
            mod[j] = min(max(1.0 + (F64(err[j]) - mu) / sd, 1.0), mod_clip)
        a, b = c_ext * F64(r_ext[j]), c_int * (r_epi[j] * mod[j])
        r_mix[j] = F32(a if b == 0 else a + b)
    nr = F64(rows)
    diag = np.array([_block_sum(_strided(r_epi)) / nr, _block_sum(_strided(mod)) / nr, mean]).astype(F32)
    return r_mix, dist_mean, err_moments, diag
