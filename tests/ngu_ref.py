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


# ---- what tests/test_ngu_curl_limits_{gpu,host}.py add ---------------------------------------------------------------------

FOLD_AT = 1 << 30


def fold(n_ins, M):
    """the header's rule for the append: a count past 2^30 becomes M + count mod M (the same slots, the ring still full)"""
    n_ins = np.asarray(n_ins)
    return np.where(n_ins > FOLD_AT, M + n_ins % M, n_ins).astype(n_ins.dtype)


def knn_fast(emb, dones, mem, n_ins, k, fold_counts=True):
    """knn() vectorised over environments and candidates, a loop over the rollout's rows alone: the distance to EVERY slot
    of the ring (e ascending, d = d + diff * diff, no product of norms), the slots that hold nothing set to +inf, sorted.
    Entry i lives in slot i mod M, so with fewer than M entries the held slots are 0 .. n_ins - 1.  fold_counts: an env
    without a done in this rollout whose count is past 2^30 has it folded (with a done the count restarts anyway)."""
    n_env, T, E = emb.shape
    M = mem.shape[1]
    mem, n_ins = mem.copy(), n_ins.copy()
    if fold_counts:
        quiet = ~(dones != 0).any(axis=1)
        n_ins[quiet] = fold(n_ins[quiet], M)
    out, m = np.full((n_env, T, k), np.inf, F64), np.zeros((n_env, T), np.int32)
    slots, envs, kk = np.arange(M), np.arange(n_env), min(k, M)
    for t in range(T):
        done = dones[:, t] != 0
        mem[done], n_ins[done] = 0, 0
        q = emb[:, t].astype(F64)
        d = np.zeros((n_env, M), F64)
        for e in range(E):
            diff = q[:, e, None] - mem[:, :, e].astype(F64)
            d = d + diff * diff
        held = np.minimum(n_ins, M)
        d[slots[None, :] >= held[:, None]] = np.inf
        d[done] = np.inf
        out[:, t, :kk] = np.sort(d, axis=1)[:, :kk]
        m[:, t] = np.where(done, 0, np.minimum(held, k))
        mem[envs, n_ins % M] = emb[:, t]
        n_ins += 1
    return out.reshape(n_env * T, k), m.reshape(-1), mem, n_ins


def limit_rollouts(shape, n_calls, dones_at=(), p_done=0.0, seed=0):
    """[(emb, dones)] per call.  dones_at: (call, env, row) triples; p_done: drawn dones in every env but the first and the
    last.  From two rows on every call repeats an embedding (row 1 = row 0), and every call after the first repeats the
    last one of the call before, across the carried ring: distances of exactly 0.  (A rollout of one row repeats nothing.)"""
    n, t, m, k, e = shape
    rs = np.random.RandomState(sum(shape) + seed)
    calls, prev = [], None
    for call in range(n_calls):
        emb = rs.randn(n, t, e).astype(F32)
        dones = (rs.rand(n, t) < p_done).astype(np.uint8)
        dones[0], dones[n - 1] = 0, 0
        for c, env, row in dones_at:
            if c == call:
                dones[env, row] = 1
        if t > 1:
            emb[:, 1] = emb[:, 0]
        if prev is not None and t > 1:
            emb[:, 0] = prev[:, t - 1]
        calls.append((emb, dones))
        prev = emb
    return calls


# the 4096 x 4096 case's planted rows of its second call: (query row, the rollout rows that hold its planted neighbours)
LANE_ROW, LANE_NEIGHBOURS = 2000, tuple(5 + 64 * i for i in range(16))      # sixteen rows, all 5 mod 64: one lane's
DUP_ROW, DUP_ROWS = 3000, tuple(1 + 7 * j for j in range(20))               # twenty bitwise copies, twenty lanes
KNN_LIMIT_NAMES = ("scans", "full-4096", "short-ring", "long-ring", "width-28", "width-32", "envs-65535", "fold")


def knn_limit_case(name):
    """-> dict(shape, calls [(emb, dones)], mem0, ins0): the rollouts of one arl_epi_knn limits case and the carried
    state they start from (zeros but for "fold")."""
    mem0 = ins0 = None
    if name == "scans":             # env 0: dones at 70 and 270, the last past one trip of 64 lanes and of 256 threads
        shape = (2, 300, 8, 3, 4)
        calls = limit_rollouts(shape, 2, dones_at=((0, 0, 70), (0, 0, 270)))
    elif name == "full-4096":
        shape = (1, 4096, 4096, 16, 4)
        calls = limit_rollouts(shape, 2)
        emb = calls[1][0][0]
        emb[LANE_ROW] = 100.0       # far from everything else; neighbour i at distance ((i + 1) / 4)^2, exact in fp32
        for i, r in enumerate(LANE_NEIGHBOURS):
            emb[r] = emb[LANE_ROW]
            emb[r, 0] += F32(0.25 * (i + 1))
        emb[DUP_ROW] = np.array([-50.0, 20.5, 3.25, -7.0], F32)
        for r in DUP_ROWS:
            emb[r] = emb[DUP_ROW]
    elif name == "short-ring":      # a ring of 5 under a rollout of 4096: t0 >= M for all tiles but the first two
        shape = (1, 4096, 5, 5, 4)
        calls = limit_rollouts(shape, 2)
    elif name == "long-ring":       # 27 rows in three calls into a ring of 4096; env 1 restarts once
        shape = (3, 9, 4096, 16, 128)
        calls = limit_rollouts(shape, 3, dones_at=((1, 1, 4),))
    elif name in ("width-28", "width-32"):
        shape = (2, 70, 130, 16, int(name[-2:]))
        calls = limit_rollouts(shape, 3, dones_at=((0, 0, 0), (1, 0, 35), (2, 0, 69)))
    elif name == "envs-65535":      # one row, one slot; env 1234 has a done in the second call, env 7 meets its own row again
        shape = (65535, 1, 1, 1, 4)
        calls = limit_rollouts(shape, 3, dones_at=((1, 1234, 0),))
        calls[1][0][7] = calls[0][0][7]
    elif name == "fold":            # M = 6 is no power of two: a plain `mod M` and `M + mod M` part ways at once
        shape = (3, 4, 6, 6, 4)
        calls = limit_rollouts(shape, 3, dones_at=((0, 2, 1),))
        mem0 = np.random.RandomState(6).randn(3, 6, 4).astype(F32)             # the ring is full, as the counts say
        ins0 = np.array([FOLD_AT, FOLD_AT + 3, FOLD_AT + 3], np.int32)
    else:
        raise KeyError(name)
    n, t, m, k, e = shape
    if mem0 is None:
        mem0, ins0 = np.zeros((n, m, e), F32), np.zeros(n, np.int32)
    return dict(shape=shape, calls=calls, mem0=mem0, ins0=ins0)


MIX_PAR = dict(eps=1e-3, c=1e-3, xi=8e-3, s_max=8., mod_clip=5.)
MIX_COEFS = ((2., 1.), (2., 0.5), (1., 0.))     # (c_ext, c_int) of the three carried calls
MIX_LIMIT_ROWS, MIX_LIMIT_K = (1024, 1025, 3000), (16, 1)
MIX_PLANTED = ("all-m-zero", "m-above-k", "zero-distances", "tiny-distances", "s-max-split", "modulator", "xi-large")


def _ascending(rs, rows, k, m):
    d = np.sort(rs.chisquare(4, size=(rows, k)), axis=1)
    d[np.arange(k)[None, :] >= m[:, None]] = np.inf
    return d


def mix_rows_case(rows, k, with_err):
    """three calls' inputs [dict(knn, m, err, r_ext)]: ascending rows padded with +inf, every m in 0 .. k"""
    rs = np.random.RandomState(rows + 7 * k + with_err)
    calls = []
    for _ in range(3):
        m = rs.randint(0, k + 1, size=rows).astype(np.int32)
        m[0], m[rows - 1] = 0, k
        knn_d = _ascending(rs, rows, k, m)
        knn_d[rows - 1, 0] = 0.0                                    # a revisit
        r_ext = rs.randn(rows).astype(F32)
        r_ext[0] = F32(-0.0)
        calls.append(dict(knn=knn_d, m=m, err=(rs.rand(rows) * 2).astype(F32) if with_err else None, r_ext=r_ext))
    return calls


def mix_planted_case(name):
    """-> dict(k, knn, m (as the kernel is given it), err, r_ext, par, dist0, mom0, c_ext, c_int): one call each"""
    rs = np.random.RandomState(len(name) + 31 * MIX_PLANTED.index(name))
    rows, k = 40, 4
    par, dist0, mom0, err = dict(MIX_PAR), np.array([7.0, 0.3]), np.zeros(3), None
    m = rs.randint(1, k + 1, size=rows).astype(np.int32)
    if name == "all-m-zero":
        m[:] = 0
    elif name == "m-above-k":
        m[::3], m[1::3] = k + 5, 2 ** 31 - 1
    elif name == "s-max-split":     # j distances of 0 give s = sqrt(j + ...) + c: above s_max = 2 from j = 4 on
        k, par["s_max"] = 8, 2.0
        m = rs.randint(1, k + 1, size=rows).astype(np.int32)
    elif name == "modulator":       # a heavy tail: errors below the mean, above it, and many deviations above it
        rows = 2000
        m = rs.randint(0, k + 1, size=rows).astype(np.int32)
        err = np.exp(2.0 * rs.randn(rows)).astype(F32)
        mom0 = np.array([500.0, 1.5, 900.0])
    elif name == "xi-large":
        par["xi"] = 1e6
    knn_d = _ascending(rs, rows, k, np.minimum(m, k))
    if name == "zero-distances":    # a first call on distances of 0: the running mean is 0
        knn_d[np.isfinite(knn_d)], dist0 = 0.0, np.zeros(2)
    elif name == "tiny-distances":  # a mean of 1e-12: the clamp, not the mean, is the divisor; xi = 0 lets it show
        knn_d, dist0, par["xi"] = knn_d * 1e-12, np.zeros(2), 0.0
    elif name == "s-max-split":
        for j in range(rows):
            knn_d[j, :min(j % (k + 1), m[j])] = 0.0
    r_ext = rs.randn(rows).astype(F32)
    return dict(k=k, knn=knn_d, m=m, err=err, r_ext=r_ext, par=par, dist0=dist0, mom0=mom0, c_ext=2.0, c_int=1.0)


# ---- arl_invdyn_loss_parts ---------------------------------------------------------------------------------------------------

INVDYN_LDS_BYTES = 159 * 1024


def invdyn_lds_floats(width, hidden, n_actions):
    """the kernel's LDS layout: W1 [2E][H + 1], W2 [H][A | 1], x [32][2E + 1], hid and d hid [32][H + 1], logits [32][65]"""
    e2 = 2 * width
    return e2 * (hidden + 1) + hidden * (n_actions | 1) + 32 * (e2 + 1) + 2 * 32 * (hidden + 1) + 32 * 65


def invdyn_a_max(width, hidden):
    """the largest n_actions in 2 .. 64 whose layout fits (None: none does)"""
    fits = [a for a in range(2, 65) if 4 * invdyn_lds_floats(width, hidden, a) <= INVDYN_LDS_BYTES]
    return max(fits) if fits else None


def invdyn_logits64(host, b):
    e, w1, b1, w2, b2 = (np.asarray(a, F32).astype(F64) for a in host)
    return np.maximum(e.reshape(b, -1) @ w1 + b1, 0.0) @ w2 + b2


def invdyn_case(b, sizes, weights="mask", over=False, ones_from=None):
    """-> (host [e, w1, b1, w2, b2] float64, action bytes u8[b], weight float64[b]) with the feature test's scalings; the
    first seed whose float64 logits keep 1e-4 between every row's two largest (the arg-max is decided).
    weights: "mask" (0 / 1, pairs from ones_from on all 1), "sum0.3" / "sum1.7" (fractions with that sum), "last-only".
    over: some action bytes are n_actions and 255, which the kernel reads as n_actions - 1."""
    e_w, h_w, n_act = sizes
    for seed in range(b + e_w + h_w + n_act, 1 << 30):
        rs = np.random.RandomState(seed)
        host = [rs.randn(2 * b, e_w), rs.randn(2 * e_w, h_w) / np.sqrt(2 * e_w), rs.randn(h_w) * 0.1,
                rs.randn(h_w, n_act) / np.sqrt(h_w), rs.randn(n_act) * 0.1]
        top = np.sort(invdyn_logits64(host, b), axis=1)
        if (top[:, -1] - top[:, -2]).min() > 1e-4:
            break
    actions = rs.randint(0, n_act, size=b).astype(np.uint8)
    if over:
        actions[::5], actions[1::5] = n_act, 255
    if weights == "mask":
        weight = (rs.rand(b) < 0.7).astype(F64)
        if ones_from is not None:
            weight[ones_from:] = 1.0
    elif weights == "last-only":
        weight = np.zeros(b)
        weight[b - 1] = 1.0
    else:
        weight = rs.rand(b) + 0.1
        weight = (weight * (float(weights[3:]) / weight.sum())).astype(F32).astype(F64)
    return host, actions, weight
