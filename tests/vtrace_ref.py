"""TEST INFRASTRUCTURE for IMPALA's V-trace (csrc/vtrace_scan.hip: arl_vtrace_scan).  The reference has no V-trace: the
yardsticks are restatements of include/accel_rl_hip.h's text (itself written from Espeholt et al. 2018 as recalled) in
NumPy float64, sharing no code with the kernel:

  ratios64     ratio = ((double) p + 1e-8) / ((double) m + 1e-8) of the taken action (a byte >= n_actions reads the last)
  vtrace_walk  the header's walk, operation for operation, one NumPy float64 operation per stated operation, vectorised
               over the envs only (elementwise float64 NumPy arithmetic is IEEE arithmetic: the same bits as a Python
               float loop per env); returns the UNROUNDED float64 (vs, adv) and the stats
  vtrace_ref   the same rounded to fp32 once: what the kernel must equal bit for bit
  gae64        float64 GAE(lambda), rounded to fp32 once: the on-policy identity's other side
"""
import numpy as np


def ratios64(prob, old_prob, actions):
    """prob, old_prob f32[n_env][T][A], actions u8[n_env][T] -> ratio f64[n_env][T]."""
    n_act = prob.shape[2]
    a = np.minimum(actions.astype(np.int64), n_act - 1)[..., None]
    p = np.take_along_axis(prob, a, axis=2)[..., 0].astype(np.float64)
    m = np.take_along_axis(old_prob, a, axis=2)[..., 0].astype(np.float64)
    return (p + 1e-8) / (m + 1e-8)


def vtrace_walk(ratio, values, last_values, rewards, dones, discount, lam, rho_bar, c_bar, pg_rho_bar):
    """ratio f64[n_env][T]; values, rewards f32[n_env][T]; last_values f32[n_env]; dones [n_env][T] ->
    (vs f64[n_env][T], adv f64[n_env][T], stats f32[n_env][2])."""
    n_env, horizon = rewards.shape
    discount, lam, rho_bar, c_bar, pg_rho_bar = (np.float64(x) for x in (discount, lam, rho_bar, c_bar, pg_rho_bar))
    v64, r64 = values.astype(np.float64), rewards.astype(np.float64)
    vs_out, adv_out = np.zeros((n_env, horizon), np.float64), np.zeros((n_env, horizon), np.float64)
    acc_next = np.zeros(n_env, np.float64)
    v_next = last_values.astype(np.float64)
    vs_next = v_next.copy()
    ratio_sum = np.zeros(n_env, np.float64)
    for t in range(horizon - 1, -1, -1):
        rt = ratio[:, t]
        rho = np.where(rt < rho_bar, rt, rho_bar)
        cw = np.where(rt < c_bar, rt, c_bar)
        pg = np.where(rt < pg_rho_bar, rt, pg_rho_bar)
        g = np.where(dones[:, t] != 0, np.float64(0.0), discount)
        r, v = r64[:, t], v64[:, t]
        q_v = r + g * v_next
        delta = rho * (q_v - v)
        acc = delta + ((g * (lam * cw)) * acc_next)
        vs = v + acc
        adv = pg * ((r + g * vs_next) - v)
        vs_out[:, t], adv_out[:, t] = vs, adv
        ratio_sum = ratio_sum + rt
        acc_next, vs_next, v_next = acc, vs, v
    stats = np.stack([ratio_sum.astype(np.float32), (ratio > rho_bar).sum(axis=1).astype(np.float32)], axis=1)
    return vs_out, adv_out, stats


def vtrace_ref(prob, old_prob, actions, values, last_values, rewards, dones, discount, lam, rho_bar, c_bar, pg_rho_bar):
    """-> (returns f32[n_env][T], advantages f32[n_env][T], stats f32[n_env][2]): arl_vtrace_scan's outputs."""
    vs, adv, stats = vtrace_walk(ratios64(prob, old_prob, actions), values, last_values, rewards, dones, discount, lam,
                                 rho_bar, c_bar, pg_rho_bar)
    return vs.astype(np.float32), adv.astype(np.float32), stats


def gae64(values, last_values, rewards, dones, discount, lam):
    """Float64 GAE(lambda) on the fp32 inputs -> (advantages f32, returns f32 = (float) (adv + V)), each rounded once:
    delta_t = r_t + g_t V_{t+1} - V_t, A_t = delta_t + g_t lambda A_{t+1}, g_t = 0 at a done."""
    n_env, horizon = rewards.shape
    v64, r64 = values.astype(np.float64), rewards.astype(np.float64)
    adv = np.zeros((n_env, horizon), np.float64)
    a_next, v_next = np.zeros(n_env, np.float64), last_values.astype(np.float64)
    for t in range(horizon - 1, -1, -1):
        g = np.where(dones[:, t] != 0, 0.0, float(discount))
        a_next = r64[:, t] + g * v_next - v64[:, t] + g * float(lam) * a_next
        adv[:, t] = a_next
        v_next = v64[:, t]
    return adv.astype(np.float32), (adv + v64).astype(np.float32)


def rollout(seed, n_env, horizon, n_act, p_done=0.15, on_policy=False):
    """A random rollout: softmax policies a little apart (ratios on both sides of 1), values, rewards, dones."""
    rs = np.random.RandomState(seed)

    def softmax(z):
        z = np.exp(z - z.max(axis=2, keepdims=True))
        return (z / z.sum(axis=2, keepdims=True)).astype(np.float32)
    logits = rs.randn(n_env, horizon, n_act)
    prob = softmax(logits)
    old_prob = prob.copy() if on_policy else softmax(logits + 0.7 * rs.randn(n_env, horizon, n_act))
    return dict(prob=prob, old_prob=old_prob, actions=rs.randint(0, n_act, (n_env, horizon)).astype(np.uint8),
                values=rs.randn(n_env, horizon).astype(np.float32), last_values=rs.randn(n_env).astype(np.float32),
                rewards=rs.randn(n_env, horizon).astype(np.float32),
                dones=(rs.rand(n_env, horizon) < p_done).astype(np.uint8))
