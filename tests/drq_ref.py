"""TEST INFRASTRUCTURE for DrQ (csrc/replay.hip: arl_replay_extract_shift, csrc/dqn.hip: arl_drq_loss).  The reference has
neither, so the yardsticks are restatements of include/accel_rl_hip.h's text, sharing no code with the kernels:

  philox4x32_10 / shift_offsets / shifted_extract   integer NumPy: the offsets' Philox stream and the shifted gather
  emu_drq32    arl_drq_loss operation for operation in fp32 (the library is built with -ffp-contract=off and the loss
               calls no transcendental, so NumPy's float32 arithmetic reproduces it bit for bit)
  ref_drq64    the same loss in float64, with the error bound below

Error bound of arl_drq_loss against float64 on the same fp32 inputs, u = 2^-24 (one rounding, relative), first order in
u, from the stated operation order.  R(row) = max |entry| of a row's A (+ 1) valid columns, N = max_i |next_q_i|,
Y = |returns_b| + gamma_n N, P = max_v p_v:
  merged q of a row   E_q = 0 (plain: the entry itself) or (A + 5) u R (dueling: A roundings in the mean, of terms
                      bounded by R; one in adv - mean, a value <= 2 R; one in val + (...), a value <= 3 R)
  nbar                E_n = mean_i E_q(next row i) + k u N    (k - 1 additions of partial sums <= k N, divided by k;
                      the division's own rounding u N)
  y                   E_y = gamma_n (E_n + u N) + u Y         (the product, then the sum)
  d_v                 E_d = E_y + E_q(q row v) + u |d_v|
  td_abs              E_td = mean_v E_d + m u P               (as nbar)
  w loss_v            E_l = w (s_v E_d + 5 u loss_v),  s_v = |d loss / d d| = min(|d_v|, delta_clip) or |d_v|
                      (two roundings inside the loss, two in w = (isw / B) / m, one in the product)
  loss_rows           sum_v E_l + (m - 1) u sum_v w loss_v
  dq entries          E_g = w E_d + 5 u |gq|   (w E_d where the slope is d_v; w: 2, the product: 1, the merge: 2 roundings)
Both sides must take the same branch: the comparison needs every selecting row's largest merged q to lead the second by
more than 4 E_q (any gap > 0 for plain rows) and | |d_v| - delta_clip | > 2 E_d; `ref_drq64` returns that mask."""
import numpy as np

EPS = 2.0 ** -24
MASK = 0xFFFFFFFF
AUG_STREAM = 0xA5D3F1C7         # include/accel_rl_hip.h: ARL_AUG_PHILOX_STREAM
IQN_STREAM = 0xC9514E31
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """Random123's Philox4x32 with 10 rounds.  ctr: four arrays (or ints) of values < 2^32, key: two -> uint64[..., 4]."""
    c = [np.asarray(x, np.uint64) & np.uint64(MASK) for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for i in range(10):
        if i > 0:
            k0, k1 = (k0 + _W0) & MASK, (k1 + _W1) & MASK
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return np.stack(c, axis=-1)


def shift_offsets(seed, call, j, v, pad):
    """(dx, dy) of view v of sample j (arrays broadcast) at extraction `call`; pad 0: no draw."""
    if pad == 0:
        z = np.zeros(np.broadcast(np.asarray(j), np.asarray(v)).shape, np.int64)
        return z, z.copy()
    call &= (1 << 64) - 1                                       # two's complement int64
    w = philox4x32_10((j, v, call & MASK, call >> 32), (seed & MASK, AUG_STREAM))
    span = np.uint64(2 * pad + 1)
    dx = ((w[..., 0] * span) >> np.uint64(32)).astype(np.int64) - pad
    dy = ((w[..., 1] * span) >> np.uint64(32)).astype(np.int64) - pad
    return dx, dy


def shifted_extract(store, size, n_stack, reward_horizon, frame_h, frame_w, env_idxs, step_idxs, pad, m_obs, k_next, seed,
                    call):
    """store: NumPy copies of the ring arrays (frames u8[n_env][ring][frame_bytes], n_blanks, acts, returns, terminals).
    -> obs u8[m_obs B][F][H][W], next_obs u8[k_next B][F][H][W] (view-major), actions, returns, terminals [B], and the
    (dx, dy) of every view, [m_obs + k_next][B]."""
    b = len(env_idxs)
    frames = store["frames"].reshape(store["frames"].shape[:2] + (frame_h, frame_w))
    out = [np.zeros((m_obs * b, n_stack, frame_h, frame_w), np.uint8), np.zeros((k_next * b, n_stack, frame_h, frame_w), np.uint8)]
    offs = np.zeros((m_obs + k_next, b, 2), np.int64)
    for v in range(m_obs + k_next):
        nxt = v >= m_obs
        for j, (e, s) in enumerate(zip(env_idxs, step_idxs)):
            i = (s + reward_horizon) % size if nxt else s
            stack = frames[e, i:i + n_stack].copy()
            stack[:store["n_blanks"][e, i]] = 0
            dx, dy = (int(x) for x in shift_offsets(seed, call, j, v, pad))
            offs[v, j] = dx, dy
            ys = np.clip(np.arange(frame_h) + dy, 0, frame_h - 1)
            xs = np.clip(np.arange(frame_w) + dx, 0, frame_w - 1)
            out[nxt][(v - m_obs if nxt else v) * b + j] = stack[:, ys][:, :, xs]
    e, s = np.asarray(env_idxs), np.asarray(step_idxs)
    return out[0], out[1], store["acts"][e, s], store["returns"][e, s], store["terminals"][e, s], offs


# ---- the loss --------------------------------------------------------------------------------------------------------

def q_stride(n_act, dueling):
    return (n_act + int(dueling) + 3) // 4 * 4 + 4              # always some padding columns


def drq_case(seed, n_act, batch, k, m, dueling, double, weighted, delta_clip=1.0, special=False):
    """fp32 inputs of one launch; the padding columns hold 1e9 and must be ignored.  special: rows b % 5 == 0 sit at
    |d| == delta_clip exactly (terminal, q(action) = 0.5, return 0.5 +- delta_clip), rows b % 5 == 1 have two equal
    maxima in every selecting row (B == 1: row 0 is both)."""
    rs = np.random.RandomState(seed)
    s, cols = q_stride(n_act, dueling), n_act + int(dueling)
    c = dict(n_act=n_act, batch=batch, k=k, m=m, dueling=dueling, stride=s)

    def rows(n):
        x = np.full((n * batch, s), 1e9, np.float32)
        x[:, :cols] = (rs.randn(n * batch, cols) * 2).astype(np.float32)
        return x
    c["q"], c["nxt"], c["pol"] = rows(m), rows(k), rows(k) if double else None
    c["act"] = rs.randint(0, n_act, batch).astype(np.uint8)
    c["ret"] = rs.randn(batch).astype(np.float32)
    c["term"] = (rs.rand(batch) < 0.3).astype(np.uint8)
    c["isw"] = (rs.rand(batch) + 0.1).astype(np.float32) if weighted else None
    if special:
        for b in range(batch):
            if b % 5 == 0 and delta_clip > 0:
                c["term"][b] = 1
                c["ret"][b] = np.float32(0.5 + (delta_clip if (b // 5) % 2 == 0 else -delta_clip))
                for v in range(m):
                    c["q"][v * batch + b, :cols] = 0.
                    c["q"][v * batch + b, n_act if dueling else c["act"][b]] = 0.5
            if (b % 5 == 1 or batch == 1) and n_act > 1:
                for key in ("nxt", "pol"):
                    if c[key] is not None:
                        for i in range(k):
                            row = c[key][i * batch + b]
                            first, second = rs.choice(n_act, 2, replace=False)
                            row[first] = row[second] = np.float32(row[:n_act].max() + 1)
    return c


def _merged32(x, n, dueling):
    """q_at of every action of the rows x f32[R][S]: row[n] + (row[a] - mean), mean = (sequential sum) / n."""
    if not dueling:
        return x[:, :n].copy()
    tot = np.zeros(len(x), np.float32)
    for a in range(n):
        tot = tot + x[:, a]
    mean = tot / np.float32(n)
    return x[:, n:n + 1] + (x[:, :n] - mean[:, None])


def _tail32(c, y, w, delta_clip):
    """dqn_td_row of every (view, sample): -> (w loss [m][B], p [m][B], dq [m B][S])."""
    n, bsz, m, duel, s = c["n_act"], c["batch"], c["m"], c["dueling"], c["stride"]
    cl = np.float32(delta_clip)
    ar = np.arange(bsz)
    wl, p, dq = np.zeros((m, bsz), np.float32), np.zeros((m, bsz), np.float32), np.zeros((m * bsz, s), np.float32)
    for v in range(m):
        q = _merged32(c["q"][v * bsz:(v + 1) * bsz], n, duel)[ar, c["act"]]
        d = y - q
        ad = np.abs(d)
        loss, slope = np.float32(0.5) * (d * d), d.copy()
        if cl > 0:
            hub = ad > cl
            loss = np.where(hub, cl * (ad - cl / np.float32(2)), loss)
            slope = np.where(hub, np.where(d > 0, cl, -cl), slope)
        gq = -(w * slope)
        block = dq[v * bsz:(v + 1) * bsz]
        if not duel:
            block[ar, c["act"]] = gq
        else:
            share = gq / np.float32(n)
            block[:, :n] = -share[:, None]
            block[ar, c["act"]] = gq - share
            block[:, n] = gq
        wl[v] = w * loss
        p[v] = np.minimum(ad, cl) if cl > 0 else ad
    return wl, p, dq


def _next32(c, i):
    n, bsz, duel = c["n_act"], c["batch"], c["dueling"]
    tgt = _merged32(c["nxt"][i * bsz:(i + 1) * bsz], n, duel)
    sel = tgt if c["pol"] is None else _merged32(c["pol"][i * bsz:(i + 1) * bsz], n, duel)
    return tgt[np.arange(bsz), np.argmax(sel, axis=1)]          # np.argmax: the first maximum


def emu_drq32(c, gamma_n, delta_clip):
    """arl_drq_loss in fp32, in the header's order -> (dq f32[m B][S], loss_rows f32[B], td_abs f32[B])."""
    bsz, k, m = c["batch"], c["k"], c["m"]
    nbar = _next32(c, 0)
    if k > 1:
        for i in range(1, k):
            nbar = nbar + _next32(c, i)
        nbar = nbar / np.float32(k)
    keep = np.where(c["term"] != 0, np.float32(0), np.float32(1))
    y = c["ret"] + keep * (np.float32(gamma_n) * nbar)
    isw = np.ones(bsz, np.float32) if c["isw"] is None else c["isw"]
    w = (isw / np.float32(bsz)) / np.float32(m)
    wl, p, dq = _tail32(c, y, w, 0. if delta_clip is None else delta_clip)
    rows, td = wl[0].copy(), p[0].copy()
    for v in range(1, m):
        rows, td = rows + wl[v], td + p[v]
    return dq, rows, td / np.float32(m)


def emu_dqn32(c, gamma_n, delta_clip):
    """arl_dqn_loss in fp32 (k = m = 1 rows), written on its own: w = isw / B, nothing is averaged."""
    assert c["k"] == c["m"] == 1
    bsz = c["batch"]
    keep = np.where(c["term"] != 0, np.float32(0), np.float32(1))
    y = c["ret"] + keep * (np.float32(gamma_n) * _next32(c, 0))
    isw = np.ones(bsz, np.float32) if c["isw"] is None else c["isw"]
    wl, p, dq = _tail32(c, y, isw / np.float32(bsz), 0. if delta_clip is None else delta_clip)
    return dq, wl[0], p[0]


def _merged64(x, n, dueling):
    x = x.astype(np.float64)
    if not dueling:
        return x[:, :n]
    return x[:, n:n + 1] + (x[:, :n] - x[:, :n].mean(axis=1, keepdims=True))


def ref_drq64(c, gamma_n, delta_clip):
    """float64 on the same fp32 inputs -> dict(dq [m B][A (+ 1)], rows, td, and their bounds dq_tol [m B], rows_tol,
    td_tol, `ok` bool[B]: the samples whose branches cannot differ between fp32 and float64 -- module docstring)."""
    n, bsz, k, m, duel = c["n_act"], c["batch"], c["k"], c["m"], c["dueling"]
    cols = n + int(duel)
    cl = 0. if delta_clip is None else float(delta_clip)
    g = float(np.float32(gamma_n))
    ar = np.arange(bsz)
    eq = lambda x: (n + 5) * EPS * np.abs(x[:, :cols]).max(axis=1) if duel else np.zeros(len(x))      # noqa: E731
    ok = np.ones(bsz, bool)
    nq, e_next = np.zeros((k, bsz)), np.zeros((k, bsz))
    for i in range(k):
        blk = c["nxt"][i * bsz:(i + 1) * bsz]
        sel_raw = blk if c["pol"] is None else c["pol"][i * bsz:(i + 1) * bsz]
        tgt, sel = _merged64(blk, n, duel), _merged64(sel_raw, n, duel)
        if n > 1:
            top = np.sort(sel, axis=1)
            ok &= (top[:, -1] - top[:, -2]) > 4 * eq(sel_raw)
        nq[i] = tgt[ar, np.argmax(sel, axis=1)]
        e_next[i] = eq(blk)
    big_n = np.abs(nq).max(axis=0)
    nbar = nq.sum(axis=0) / k
    e_n = e_next.mean(axis=0) + k * EPS * big_n
    keep = (c["term"] == 0).astype(np.float64)
    ret = c["ret"].astype(np.float64)
    y = ret + keep * (g * nbar)
    e_y = g * (e_n + EPS * big_n) + EPS * (np.abs(ret) + g * big_n)
    isw = np.ones(bsz) if c["isw"] is None else c["isw"].astype(np.float64)
    w = isw / bsz / m
    dq = np.zeros((m * bsz, cols))
    rows, td, rows_tol, e_d_sum, p_max = np.zeros(bsz), np.zeros(bsz), np.zeros(bsz), np.zeros(bsz), np.zeros(bsz)
    dq_tol = np.zeros(m * bsz)
    wl_abs = np.zeros(bsz)
    for v in range(m):
        blk = c["q"][v * bsz:(v + 1) * bsz]
        d = y - _merged64(blk, n, duel)[ar, c["act"]]
        ad = np.abs(d)
        e_d = e_y + eq(blk) + EPS * ad
        if cl > 0:
            ok &= np.abs(ad - cl) > 2 * e_d
            hub = ad > cl
            loss = np.where(hub, cl * (ad - cl / 2), 0.5 * d * d)
            slope = np.where(hub, np.sign(d) * cl, d)
        else:
            hub = np.zeros(bsz, bool)
            loss, slope = 0.5 * d * d, d
        p = np.minimum(ad, cl) if cl > 0 else ad
        gq = -(w * slope)
        block = dq[v * bsz:(v + 1) * bsz]
        if not duel:
            block[ar, c["act"]] = gq
        else:
            block[:, :n] = -(gq / n)[:, None]
            block[ar, c["act"]] = gq - gq / n
            block[:, n] = gq
        dq_tol[v * bsz:(v + 1) * bsz] = np.where(hub, 0., w * e_d) + 5 * EPS * np.abs(gq)
        rows += w * loss
        wl_abs += np.abs(w * loss)
        rows_tol += w * (np.abs(slope) * e_d + 5 * EPS * loss)
        td += p
        e_d_sum += e_d
        p_max = np.maximum(p_max, p)
    rows_tol += (m - 1) * EPS * wl_abs
    return dict(dq=dq, rows=rows, td=td / m, dq_tol=dq_tol, rows_tol=rows_tol, td_tol=e_d_sum / m + m * EPS * p_max, ok=ok)
