// What the value-based loss and action kernels of csrc/dqn.hip, csrc/iqn.hip, csrc/fqf.hip and csrc/sac.hip share: the wave
// butterflies, the first maximum over a staged row of Q values, the lane-per-sample row helpers (dueling merge, first maximum,
// soft-max sums, the TD loss of one error), one term of the pairwise quantile-Huber loss, the fixed-order combine of
// the four waves' partial sums, the epsilon-greedy serve tail of the wave-per-sample action kernels, and -- for the kernels
// whose quantiles are strided by a_stride (iqn.hip, fqf.hip) -- the argument record, its host-side checks, the staging of
// the taken action's quantiles and of the targets T_j, and everything after them (loss_tail).  Internal; every device
// function is inlined into its callers, which are compiled with -ffp-contract=off: the operations and their order are
// part of the kernels' stated results (include/accel_rl_hip.h) -- do not re-associate them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arl_common.h"

namespace arlq {

__device__ __forceinline__ float wave_max(float x) {          // butterfly: lane ^ 32, ^ 16, ... ^ 1
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
    return x;
}
__device__ __forceinline__ float wave_sum(float x) {          // butterfly, as wave_max
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// first maximum of q[0 .. n_actions): every lane walks the same LDS row (broadcast reads) and gets the same answer
__device__ __forceinline__ int first_max(const float* q, int n_actions) {
    int best = 0;
    float best_q = q[0];
    for (int a = 1; a < n_actions; ++a) {
        const float v = q[a];
        if (v > best_q) { best_q = v; best = a; }
    }
    return best;
}

// ---- rows f32[stride] of action values (csrc/dqn.hip) or of actor logits (csrc/sac.hip), the first n entries valid ----
// dueling: the row holds n advantages followed by the value; q_a = val + (adv_a - mean adv)
__device__ __forceinline__ float row_mean(const float* row, int n) {
    float sum = 0.f;
    for (int a = 0; a < n; ++a) sum += row[a];
    return sum / (float)n;
}
__device__ __forceinline__ float q_at(const float* row, int a, int n, bool dueling, float mean) {
    return dueling ? row[n] + (row[a] - mean) : row[a];
}
__device__ __forceinline__ int first_argmax(const float* row, int n, bool dueling) {
    const float mean = dueling ? row_mean(row, n) : 0.f;
    int best = 0;
    float best_q = q_at(row, 0, n, dueling, mean);
    for (int a = 1; a < n; ++a) {
        const float q = q_at(row, a, n, dueling, mean);
        if (q > best_q) { best_q = q; best = a; }
    }
    return best;
}

// v = max_a q_a, s = sum_a expf((q_a - v) / tau_e) (a ascending, from 0) and tl = tau_e logf(s) of one row:
// tau_e log pi_a = (q_a - v) - tl.  (tau_e == 1: the division and the product are exact)
struct SoftRow { float v, s, tl; };
__device__ __forceinline__ SoftRow soft_row(const float* row, int n, bool dueling, float mean, float tau_e) {
    SoftRow r;
    r.v = q_at(row, 0, n, dueling, mean);
    for (int a = 1; a < n; ++a) r.v = fmaxf(r.v, q_at(row, a, n, dueling, mean));
    r.s = 0.f;
    for (int a = 0; a < n; ++a) r.s += expf((q_at(row, a, n, dueling, mean) - r.v) / tau_e);
    r.tl = tau_e * logf(r.s);
    return r;
}

// The TD error d = y - q under the threshold c (c <= 0: squared loss): the loss 0.5 d^2 or c (|d| - c / 2), its slope in
// d, and the priority |d| (clipped to c when c > 0)
struct TdLoss { float loss, slope, p; };
__device__ __forceinline__ TdLoss td_loss(float d, float c) {
    const float ad = fabsf(d);
    float loss = 0.5f * (d * d), slope = d;                                // d loss / d d
    if (c > 0.f && ad > c) {                                               // Huber (:157-160)
        loss = c * (ad - c / 2.f);
        slope = d > 0.f ? c : -c;
    }
    return {loss, slope, c > 0.f ? fminf(ad, c) : ad};                     // :165
}

// the sizes arl_dqn_loss and the entry points that state "sizes as arl_dqn_loss" accept
inline bool q_sizes_ok(int64_t batch, int n_actions, int stride, int dueling) {
    return !(batch <= 0 || n_actions <= 0 || n_actions > 255 || stride < n_actions + (dueling != 0) || (stride & 3));
}

// One term of the pairwise quantile-Huber loss at u = T_j - theta_i and fraction tau (of theta_i): rt the loss term, gt
// its slope in u (d rt / d theta_i = -gt).  kappa == 0: plain quantile regression.
__device__ __forceinline__ void quantile_huber_term(float u, float tau, float kappa, float& gt, float& rt) {
    const float ind = u < 0.f ? 1.f : 0.f;
    const float wt = fabsf(tau - ind);
    if (kappa > 0.f) {
        const float au = fabsf(u);
        const float l = au <= kappa ? 0.5f * (u * u) : kappa * (au - 0.5f * kappa);
        rt = wt * l / kappa;
        gt = wt * fminf(fmaxf(u, -kappa), kappa) / kappa;
    } else {
        rt = wt * fabsf(u);
        gt = tau - ind;
    }
}

// the four waves' partial sums of one lane, in the fixed order ((p0 + p1) + p2) + p3
__device__ __forceinline__ float combine4(const float (*s)[64], int lane) {
    return ((s[0][lane] + s[1][lane]) + s[2][lane]) + s[3][lane];
}

// Serve tail of a wave-per-sample action kernel (lanes are actions): the override, if any, takes the greedy action's
// place in the one-hot row; greedy[b] keeps the greedy one.
__device__ __forceinline__ void serve_wave(int g, int64_t b, int lane, int n_actions, const int32_t* override_or_null,
                                           float* onehot, uint8_t* greedy) {
    int act = g;
    if (override_or_null && override_or_null[b] >= 0) act = override_or_null[b];
    if (lane < n_actions) onehot[b * n_actions + lane] = lane == act ? 1.f : 0.f;
    if (lane == 0 && greedy) greedy[b] = (uint8_t)g;
}

// Arguments of the loss kernels whose quantiles are strided by a_stride (arl_iqn_loss; arl_miqn_loss and arl_fqf_loss
// extend it).
struct IqnLossArgs {
    const float* pred;              // online net on obs                  [B][N][S]
    const float* tau_pred;          // its fractions                      [B][N]
    const float* tgt_next;          // target net on next_obs             [B][N'][S]
    const float* pol_next;          // online net on next_obs (double DQN) or null
    const uint8_t* actions;         // [B]
    const float* returns;           // [B] n-step discounted return
    const uint8_t* terminals;       // [B]
    const float* is_weights;        // [B] or null
    float* dtheta;                  // [B][N][S]
    float* loss_rows;               // [B] per-sample (weighted) loss / B
    float* priorities;              // [B] clip(unweighted loss, 1e-6, 1e6)
    int64_t* state;                 // (seed, counter) or null
    int64_t advance;
    int64_t batch;
    int n_actions, n, n_target, stride;
    float gamma_n, kappa;           // kappa == 0: plain quantile regression
};

// Second half of loss_kernel, mloss_kernel (csrc/iqn.hip) and fqf_loss_kernel (csrc/fqf.hip), entered by all 256 threads
// once s_t (the targets T_j), s_pred and s_tau (the taken action's predicted quantiles and their fractions) are staged and
// the barrier is passed: the N x N' phase, the four-way combine, loss and priority, the dtheta write and the counter
// advance.
__device__ __forceinline__ void loss_tail(const IqnLossArgs& a, int lane, int wave, int act, const float* s_t,
                                          const float* s_pred, const float* s_tau, float* s_d, float (*s_g)[64],
                                          float (*s_r)[64]) {
    const int64_t b = blockIdx.x;
    const int n = a.n, m = a.n_target, S = a.stride;
    const float kappa = a.kappa;
    float g = 0.f, r = 0.f;
    if (lane < n) {
        const float th = s_pred[lane], tau = s_tau[lane];
        for (int j = wave; j < m; j += 4) {
            float gt, rt;
            quantile_huber_term(s_t[j] - th, tau, kappa, gt, rt);
            g += gt;
            r += rt;
        }
    }
    s_g[wave][lane] = g;
    s_r[wave][lane] = r;
    __syncthreads();
    const float wgt = (a.is_weights ? a.is_weights[b] : 1.f) / (float)a.batch;
    if (wave == 0) {
        const float gs = combine4(s_g, lane), rs = combine4(s_r, lane);
        s_d[lane] = lane < n ? -(wgt / (float)m * gs) : 0.f;    // d loss / d theta(lane, act)
        const float loss_b = wave_sum(lane < n ? rs : 0.f) / (float)m;
        if (lane == 0) {
            a.loss_rows[b] = wgt * loss_b;
            a.priorities[b] = fminf(fmaxf(loss_b, 1e-6f), 1e6f);
        }
    }
    __syncthreads();
    float* dl = a.dtheta + b * n * S;
    for (int o = threadIdx.x; o < n * S; o += 256) {            // row o / S (a fraction), column o % S (an action or padding)
        const int i = o / S;
        dl[o] = o - i * S == act ? s_d[i] : 0.f;
    }
    if (a.state && b == 0 && threadIdx.x == 0) a.state[1] += a.advance;    // the update's passes have drawn
}

// wave 1 of the three loss kernels: the taken action's predicted quantiles and their fractions, lane = predicted fraction
__device__ __forceinline__ void stage_taken(const IqnLossArgs& a, int lane, int act, float* s_pred, float* s_tau) {
    const int64_t b = blockIdx.x;
    const int n = a.n, S = a.stride;
    s_pred[lane] = lane < n ? a.pred[(b * n + lane) * S + act] : 0.f;
    s_tau[lane] = lane < n ? a.tau_pred[b * n + lane] : 0.f;
}

// wave 0 of loss_kernel and fqf_loss_kernel once a* is known: T_j = returns_b + keep * (gamma_n * theta_tgt(j, a*)), lane = j
__device__ __forceinline__ void stage_targets(const IqnLossArgs& a, int lane, int a_next, float* s_t) {
    const int64_t b = blockIdx.x;
    const int m = a.n_target, S = a.stride;
    const float keep = a.terminals[b] ? 0.f : 1.f;
    s_t[lane] = lane < m ? a.returns[b] + keep * (a.gamma_n * a.tgt_next[(b * m + lane) * S + a_next]) : 0.f;
}

inline bool theta_sizes_ok(int64_t batch, int n_actions, int fractions, int stride) {
    return batch >= 1 && batch <= 0x7fffffffLL && n_actions >= 1 && n_actions <= 64 && fractions >= 1 &&
           fractions <= ARL_IQN_MAX_FRACTIONS && stride >= n_actions && (stride & 3) == 0 && stride <= (1 << 20);
}

const char* const THETA_SIZES = "need 1 <= batch < 2^31, 1 <= n_actions <= 64, 1 <= fractions <= 64, "
                                "n_actions <= a_stride <= 2^20 and a_stride % 4 == 0";

// The checks and fields that arl_iqn_loss and arl_miqn_loss share, in the order both state them; `fn` names the entry
// point in the message.  ptrs_ok: every mandatory pointer of the caller is non-null.
inline int fill_iqn_loss(IqnLossArgs& a, const char* fn, bool ptrs_ok, const float* pred, const float* tau_pred,
                         const float* tgt_next, const uint8_t* actions, const float* returns, const uint8_t* terminals,
                         const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t n, int32_t n_target,
                         int32_t a_stride, float gamma_n, float kappa, float* dtheta, float* loss_rows,
                         float* priorities, int64_t* state_or_null, int64_t advance) {
    const char* msg = nullptr;
    if (!ptrs_ok) msg = "null pointer";
    else if (!(theta_sizes_ok(batch, n_actions, n, a_stride) && theta_sizes_ok(batch, n_actions, n_target, a_stride)))
        msg = THETA_SIZES;
    else if (!(kappa >= 0.f && kappa <= 3.0e38f)) msg = "kappa must be finite and >= 0";
    if (msg) {
        arl::set_error("%s: %s", fn, msg);
        return ARL_E_ARG;
    }
    a.pred = pred; a.tau_pred = tau_pred; a.tgt_next = tgt_next; a.actions = actions; a.returns = returns;
    a.terminals = terminals; a.is_weights = is_weights_or_null; a.dtheta = dtheta; a.loss_rows = loss_rows;
    a.priorities = priorities; a.state = state_or_null; a.advance = advance; a.batch = batch; a.n_actions = n_actions;
    a.n = n; a.n_target = n_target; a.stride = a_stride; a.gamma_n = gamma_n; a.kappa = kappa;
    return 0;
}

}  // namespace arlq
