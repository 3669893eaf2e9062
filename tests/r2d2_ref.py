"""TEST INFRASTRUCTURE for R2D2 (csrc/r2d2.hip, algos/dqn/replay_buffers/sequence.py).  The reference has no R2D2: these
are float64 NumPy restatements of include/accel_rl_hip.h's statements, written for the tests, operation for operation
(sums are sequential loops, never np.sum's pairwise order).

  h64 / h_inv64          the invertible value rescaling and its inverse (h_inv_closed_form64: the form that cancels)
  merged64               rows f32[R][stride] -> the (dueling-merged) action values f64[R][A]
  r2d2_loss64            arl_r2d2_loss: dict(dq, td_abs, loss_rows, priorities) rounded once to float32, plus d, x, z (f64)
  loss_case              random inputs of one shape with the planted rows the GPU test asserts
  within_one_ulp         got == want or its float32 neighbour
  brute_sampleable       which sequence slots can be sampled, from a simulation of the ring in global time
  SeqModel               arl_seq_store / arl_seq_prepare in NumPy
  LIMIT_SHAPES, limits_loss_case, seq_written_slots, seq_t0       the cases of tests/test_r2d2_vmpo_sacd_limits_*.py
"""
import numpy as np


def _sign(x):
    return np.where(x > 0.0, 1.0, np.where(x < 0.0, -1.0, 0.0))


def h64(z, eps):
    z = np.asarray(z, np.float64)
    return _sign(z) * (np.sqrt(np.abs(z) + 1.0) - 1.0) + eps * z


def h_inv64(x, eps):
    x = np.asarray(x, np.float64)
    s = np.sqrt(1.0 + (4.0 * eps) * ((np.abs(x) + 1.0) + eps))
    dl = (2.0 * np.abs(x)) / ((s + 1.0) + 2.0 * eps)
    return _sign(x) * (dl * (dl + 2.0))


def h_inv_closed_form64(x, eps):
    """the inverse as the paper's closed form is usually written; u * u - 1.0 cancels for |x| << 1 (absolute error about
    2^-53 / (2 eps)), which is why h_inv64 -- and the kernel -- evaluate the same function as dl (dl + 2)."""
    x = np.asarray(x, np.float64)
    s = np.sqrt(1.0 + (4.0 * eps) * ((np.abs(x) + 1.0) + eps))
    u = (s - 1.0) / (2.0 * eps)
    return _sign(x) * (u * u - 1.0)


def merged64(rows, n_actions, dueling):
    rows = np.asarray(rows, np.float32).astype(np.float64)
    adv = rows[:, :n_actions]
    if not dueling:
        return adv.copy()
    s = np.zeros(rows.shape[0])
    for a in range(n_actions):
        s = s + adv[:, a]
    mean = s / float(n_actions)
    return rows[:, n_actions:n_actions + 1] + (adv - mean[:, None])


def first_argmax(q):
    return np.argmax(q, axis=1)                     # numpy returns the first maximum


def r2d2_loss64(q, q_tgt, actions, returns, terminals, is_weights, batch, burn_in, train_len, n, n_actions, dueling,
                gamma_n, eps, eta):
    U = burn_in + train_len + n
    stride = q.shape[1]
    qm, tm = merged64(q, n_actions, dueling), merged64(q_tgt, n_actions, dueling)
    t_rows = (np.arange(batch)[:, None] * U + burn_in + np.arange(train_len)[None, :]).reshape(-1)
    a_star = first_argmax(qm[t_rows + n])
    x = tm[t_rows + n, a_star]
    hinv = h_inv64(x, eps) if eps > 0 else x
    ret = np.asarray(returns, np.float32).astype(np.float64)[t_rows]
    z = ret + np.where(np.asarray(terminals)[t_rows] != 0, 0.0, gamma_n * hinv)
    y = h64(z, eps) if eps > 0 else z
    act = np.minimum(np.asarray(actions)[t_rows].astype(np.int64), n_actions - 1)
    d = (y - qm[t_rows, act]).reshape(batch, train_len)
    ad = np.abs(d)
    w = (np.ones(batch) if is_weights is None else np.asarray(is_weights, np.float32).astype(np.float64)) / float(
        batch * train_len)
    sum_sq, sum_abs, mx = np.zeros(batch), np.zeros(batch), np.zeros(batch)
    for t in range(train_len):                                      # time order, from 0.0
        sum_sq = sum_sq + 0.5 * (d[:, t] * d[:, t])
        sum_abs = sum_abs + ad[:, t]
        mx = np.maximum(mx, ad[:, t])
    loss_rows = w * sum_sq
    prio = eta * mx + (1.0 - eta) * (sum_abs / float(train_len))
    dq = np.zeros((batch * U, stride), np.float32)
    gq = -(w[:, None] * d)
    gq = gq.reshape(-1)
    if dueling:
        share = gq / float(n_actions)
        dq[t_rows, :n_actions] = (-share).astype(np.float32)[:, None]
        dq[t_rows, act] = (gq - share).astype(np.float32)
        dq[t_rows, n_actions] = gq.astype(np.float32)
    else:
        dq[t_rows, act] = gq.astype(np.float32)
    return dict(dq=dq, td_abs=ad.astype(np.float32), loss_rows=loss_rows.astype(np.float32),
                priorities=prio.astype(np.float32), d=d, x=x.reshape(batch, train_len), z=z.reshape(batch, train_len),
                a_star=a_star.reshape(batch, train_len), t_rows=t_rows)


def within_one_ulp(got, want):
    """elementwise: got equals want or one of want's float32 neighbours (signed zeros compare equal)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    up, down = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
    return (got == want) | (got == up) | (got == down)


PAD = np.float32(1e9)


def loss_case(seed, batch, burn_in, train_len, n, n_actions, stride, dueling, gamma_n):
    """Random rows with plants.  Train step 0 and train step train_len - 1 of sequence 0 are terminal; sequence 0's first
    next-row is an integer-valued online row whose maximum is tied between the first and the last action (an exact tie:
    the first wins); the first train step of the last sequence has x == 0 exactly and return 0 (so z == 0); one sequence
    carries |q| ~ 1e4; the last train row's action byte is 200.  Padding columns hold 1e9.  In a shape too small to keep
    the plants apart they fall on the same rows; the restatement reads whatever results."""
    rng = np.random.RandomState(seed)
    U = burn_in + train_len + n
    rows = batch * U
    width = n_actions + (1 if dueling else 0)
    q = np.full((rows, stride), PAD, np.float32)
    qt = np.full((rows, stride), PAD, np.float32)
    q[:, :width] = rng.randn(rows, width).astype(np.float32) * 3
    qt[:, :width] = rng.randn(rows, width).astype(np.float32) * 3
    actions = rng.randint(0, n_actions, rows).astype(np.uint8)
    returns = rng.randn(rows).astype(np.float32)
    terminals = (rng.rand(rows) < 0.1).astype(np.uint8)
    isw = (0.25 + 0.75 * rng.rand(batch)).astype(np.float32)
    if batch >= 2:                                              # |q| ~ 1e4 in sequence 1
        sl = slice(U, 2 * U)
        q[sl, :width] *= np.float32(3e3)
        qt[sl, :width] *= np.float32(3e3)
        returns[sl] *= np.float32(1e2)
    first, last = burn_in, burn_in + train_len - 1
    terminals[first] = 1
    terminals[last] = 1
    # the tie: integer-valued online row at (sequence 0, first train step + n); with dueling the advantages are integers
    # whose mean is an integer too (the row sums to a multiple of A), value 2
    r = first + n
    tie = np.zeros(width, np.float32)
    tie[:n_actions] = -float(n_actions)
    tie[0] = tie[n_actions - 1] = 7.0
    if dueling:
        tie[:n_actions] = 0.0
        tie[0] = tie[n_actions - 1] = float(n_actions)          # mean is 2 (A >= 2) or A (A == 1): exact
        tie[n_actions] = 2.0
    q[r, :width] = tie
    # x == 0 and z == 0: (last sequence, first train step) -- the online next-row prefers action 0, whose target value is 0
    b = batch - 1
    t0 = b * U + first
    if b > 0:                                                   # (b == 0: the row is the tie row, where action 0 wins too)
        on = np.zeros(width, np.float32)
        on[:n_actions] = -1.0
        on[0] = 1.0
        q[t0 + n, :width] = on
        terminals[t0] = 0
    tg = np.zeros(width, np.float32)                            # dueling: all zero, every merged value is 0
    if not dueling:
        tg[1:n_actions] = 5.0
    qt[t0 + n, :width] = tg
    returns[t0] = 0.0
    actions[batch * U - n - 1] = 200                            # the last train row: an action byte past the row
    return dict(q=q, q_tgt=qt, actions=actions, returns=returns, terminals=terminals, is_weights=isw)


# ---- the sequence layer ---------------------------------------------------------------------------------------------------

def brute_sampleable(written, size, S, U, n_stack, n):
    """bool[size / S]: slot k (first step at ring index k * S) can be sampled after `written` steps per environment.
    Simulated in global time: ring index p holds the newest step tau < written with tau % size == p; a frame of time
    tau' is still there iff tau' >= written - size (before the ring is full that covers tau' < 0, the blank history
    before the first step ever; from the moment it is full the memory counts the frames ahead of the write cursor as
    lost, as the reference's uniform sampler does -- at written == size exactly that gives up one slot a lap early,
    which a function of the cursor alone cannot tell from the laps after it).  A slot is
    sampleable iff its U steps are in the ring at consecutive times, the n_stack - 1 frames before its first step are
    still there, and the n-step returns of its train rows (every row but the last n) are complete: the return of time
    tau is final once tau + n - 1 < written."""
    out = np.zeros(size // S, bool)
    holds = {}
    for tau in range(max(0, written - size), written):
        holds[tau % size] = tau
    for k in range(size // S):
        times = [holds.get((k * S + t) % size) for t in range(U)]
        if any(t is None for t in times):
            continue
        if any(times[t] != times[0] + t for t in range(U)):
            continue
        if any(tp < written - size for tp in range(times[0] - (n_stack - 1), times[0])):
            continue
        if any(times[t] + n - 1 >= written for t in range(U - n)):
            continue
        out[k] = True
    return out


class SeqModel(object):
    """arl_seq_store / arl_seq_prepare on host arrays."""

    def __init__(self, n_env, size, S, hidden, n_state):
        self.n_env, self.size, self.S = n_env, size, S
        self.stores = [np.full((n_env, size // S, hidden), np.nan, np.float32) for _ in range(n_state)]
        self.ring = np.full((n_env, size), 255, np.uint8)

    def store(self, states, resets, horizon, idx):
        for e in range(self.n_env):
            for t in range(horizon):
                p = (idx + t) % self.size
                self.ring[e, p] = resets[e * horizon + t]
                if p % self.S == 0:
                    for s, st in enumerate(states):
                        self.stores[s][e, p // self.S] = st[e * horizon + t]

    def prepare(self, env, slot, U):
        env_rows = np.repeat(np.asarray(env, np.int32), U)
        step_rows = ((np.asarray(slot, np.int64)[:, None] * self.S + np.arange(U)[None, :]) % self.size).astype(np.int32)
        step_rows = step_rows.reshape(-1)
        resets = self.ring[env_rows, step_rows]
        states = [st[np.asarray(env), np.asarray(slot)] for st in self.stores]
        return env_rows, step_rows, states, resets


# ---- the limits tests (tests/test_r2d2_vmpo_sacd_limits_gpu.py / _host.py) -------------------------------------------------

# (batch, burn_in, train_len, n, A, stride, dueling): all three limits at once with the value column in the last float of
# the row | A = 255 dueling at the tight stride | A = 255 plain | one train step behind the longest burn-in | a block
# index above 65535
LIMIT_SHAPES = [(2, 1024, 1024, 16, 3, 4, 1), (2, 0, 1023, 1, 255, 256, 1), (3, 5, 129, 2, 255, 256, 0),
                (1, 1024, 1, 16, 2, 4, 0), (70000, 0, 1, 1, 1, 4, 0)]
BIG_RETURN = np.float32(1e6)


def limits_loss_case(seed, batch, burn_in, train_len, n, n_actions, stride, dueling, gamma_n):
    """loss_case with two more plants.  The last train row's action byte is 255 (past the row for every A).  Sequence 0's
    last train step -- terminal already -- gets the return 1e6, so that the largest |d| of the sequence sits at train step
    train_len - 1 (y = h(1e6) ~ 2e3 with eps = 1e-3, 1e6 without; the next largest |d| of sequence 0 is the tie row's,
    n_actions + 7 at most; tests/test_r2d2_vmpo_sacd_limits_host.py asserts the margin): a walk
    of the staged errors that stops short, or a maximum that misses the last entry, shows in loss_rows and priorities.
    Left out where that row is the z == 0 plant (batch == 1 and train_len == 1: the only |d| is the last one anyway)."""
    c = loss_case(seed, batch, burn_in, train_len, n, n_actions, stride, dueling, gamma_n)
    U = burn_in + train_len + n
    c["actions"][batch * U - n - 1] = 255
    last = burn_in + train_len - 1
    if last != (batch - 1) * U + burn_in:
        c["returns"][last] = BIG_RETURN
    return c


def seq_t0(S, idx):
    """the first step of a batch whose ring index is a multiple of S (include/accel_rl_hip.h: ((idx + t) mod size) % S == 0;
    size % S == 0)."""
    t = 0
    while (idx + t) % S:
        t += 1
    return t


def seq_written_slots(size, S, horizon, idx):
    """the set of state slots SeqModel.store writes for one environment (read off a NaN-filled store)."""
    m = SeqModel(1, size, S, 4, 1)
    m.store([np.ones((horizon, 4), np.float32)], np.zeros(horizon, np.uint8), horizon, idx)
    return set(np.flatnonzero(~np.isnan(m.stores[0][0, :, 0])).tolist())
