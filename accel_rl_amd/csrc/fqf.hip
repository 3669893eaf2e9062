// Fully parameterized quantile functions (FQF, Yang et al. 2019) for gfx950: what AtariFqfPolicy adds to the implicit
// quantile network of csrc/iqn.hip, whose embedding (given mode), merge and dense passes it reuses.  Formulas and summation
// orders are stated in include/accel_rl_hip.h ("Fully parameterized quantile functions"); design notes in DESIGN.md, 17.
//
//   arl_fqf_fractions  soft-max of the proposal layer's logits -> cumulative fractions tau, midpoints tau_hat, the inner
//                      fractions tau_1 .. tau_{N-1} (compact), q, log q and the entropy; one wave per sample
//   arl_fqf_act        Q_a = sum_k (tau_{k+1} - tau_k) theta(k, a), first maximum, override, one-hot row
//   arl_fqf_loss       greedy next action under the weighted Q, targets T_j, then arl_iqn_loss's N x N phase (loss_tail);
//                      meanwhile wave 2 takes the gradient of the fraction loss w.r.t. the logits; one workgroup per sample
//
// Plain fp32 C++ (compiled with -ffp-contract=off), wave64, no atomics, no generator: every launch is deterministic.

#include "arl_common.h"
#include "q_loss_dev.h"

namespace {

using namespace arlq;

// One wave per sample, lane = fraction.  Maximum and exp sum: butterflies over the 64 lanes; the cumulative sum: every lane
// walks k = 0 .. N - 1 in the same order (q_k broadcast from lane k) and keeps the two values on either side of its own.
__global__ __launch_bounds__(256) void fractions_kernel(const float* __restrict__ logits, int64_t batch, int n,
                                                        int n_stride, float* __restrict__ tau,
                                                        float* __restrict__ tau_hat, float* __restrict__ tau_mid,
                                                        float* __restrict__ q_out, float* __restrict__ logq_out,
                                                        float* __restrict__ entropy) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= batch) return;                                     // (a whole wave: no barrier below)
    const bool in = lane < n;
    const float l = in ? logits[b * n_stride + lane] : -INFINITY;
    const float v = wave_max(l);
    const float c = in ? l - v : 0.f;
    const float e = in ? expf(c) : 0.f;
    const float s = wave_sum(e);
    const float q = e / s;
    const float lq = c - logf(s);                               // finite where q underflows to 0
    const float h = 0.f - wave_sum(in ? q * lq : 0.f);
    float t = 0.f, lo = 0.f, hi = 0.f;
    for (int k = 0; k < n; ++k) {
        const float qk = __shfl(q, k, 64);
        const float t1 = k == n - 1 ? 1.f : fminf(t + qk, 1.f);
        if (k == lane) { lo = t; hi = t1; }
        t = t1;
    }
    if (in) {
        tau[b * (n + 1) + lane] = lo;
        if (lane == n - 1) tau[b * (n + 1) + n] = hi;           // exactly 1
        tau_hat[b * n + lane] = 0.5f * (lo + hi);
        if (tau_mid && lane >= 1) tau_mid[b * (n - 1) + lane - 1] = lo;
        if (q_out) q_out[b * n + lane] = q;
        if (logq_out) logq_out[b * n + lane] = lq;
    }
    if (entropy && lane == 0) entropy[b] = h;
}

// Q_a of action `lane` under theta_b f32[k][stride] with the weights w_j = tau_b[j + 1] - tau_b[j]: j ascending, from 0
__device__ __forceinline__ float wq_of_lane(const float* theta_b, const float* tau_b, int lane, int n_actions, int k,
                                            int stride) {
    if (lane >= n_actions) return 0.f;
    float s = 0.f;
    for (int j = 0; j < k; ++j) s += (tau_b[j + 1] - tau_b[j]) * theta_b[(int64_t)j * stride + lane];
    return s;
}

// one wave per sample, lanes are actions (arl_iqn_act's kernel with the weighted sum)
__global__ __launch_bounds__(256) void fqf_act_kernel(const float* __restrict__ theta, const float* __restrict__ tau,
                                                      const int32_t* __restrict__ override_or_null, int64_t batch,
                                                      int n_actions, int k, int stride, float* __restrict__ onehot,
                                                      uint8_t* __restrict__ greedy) {
    __shared__ float s_q[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    s_q[wave][lane] = b < batch ? wq_of_lane(theta + b * k * stride, tau + b * (k + 1), lane, n_actions, k, stride) : 0.f;
    __syncthreads();
    if (b < batch) serve_wave(first_max(s_q[wave], n_actions), b, lane, n_actions, override_or_null, onehot, greedy);
}

// (n_target == n; state == NULL: nothing is drawn)
struct FqfLossArgs : IqnLossArgs {
    const float* pred_mid;          // online net on obs at tau_1 .. tau_{N-1}    [B][N-1][S] (null when N == 1)
    const float* tau;               // [B][N+1]
    const float* q;                 // [B][N]
    const float* logq;              // [B][N]
    const float* entropy;           // [B]
    float* dlogits;                 // [B][n_stride]
    float* frac_rows;               // [B]
    int n_stride;
    float ent_coef;
};

// One workgroup per sample.  loss_kernel of csrc/iqn.hip with the weighted Q in the selection, N' = N and tau_pred =
// tau_hat; wave 2, idle there, takes the fraction loss: lane i = inner fraction i (1 .. N - 1) holds g_i, then every lane
// walks i = 1 .. N - 1 (g_i and tau_i broadcast from lane i) for G and its own suffix sum S_lane.
__global__ __launch_bounds__(256) void fqf_loss_kernel(const FqfLossArgs a) {
    __shared__ float s_q[64], s_t[64], s_pred[64], s_tau[64], s_d[64], s_g[4][64], s_r[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;                               // (grid = batch exactly)
    const int A = a.n_actions, n = a.n, S = a.stride;
    int act = a.actions[b];
    act = act < A ? act : A - 1;                                // an action the net does not have: never out of bounds
    const float* tau_b = a.tau + b * (n + 1);
    float mid = 0.f, tau_i = 0.f, qk = 0.f, lq = 0.f;
    if (wave == 0) {
        const float* sel = (a.pol_next ? a.pol_next : a.tgt_next) + b * n * S;
        s_q[lane] = wq_of_lane(sel, tau_b, lane, A, n, S);
    } else if (wave == 1) {
        stage_taken(a, lane, act, s_pred, s_tau);
    } else if (wave == 2) {
        if (lane >= 1 && lane < n) {
            mid = a.pred_mid[(b * (n - 1) + lane - 1) * S + act];
            tau_i = tau_b[lane];
        }
        if (lane < n) {
            qk = a.q[b * n + lane];
            lq = a.logq[b * n + lane];
        }
    }
    __syncthreads();
    if (wave == 0) {
        stage_targets(a, lane, first_max(s_q, A), s_t);
    } else if (wave == 2) {
        const float g = lane >= 1 && lane < n ? (2.f * mid - s_pred[lane]) - s_pred[lane - 1] : 0.f;
        float G = 0.f, Sk = 0.f;
        for (int i = 1; i < n; ++i) {
            const float gi = __shfl(g, i, 64), ti = __shfl(tau_i, i, 64);
            G += gi * ti;
            if (i > lane) Sk += gi;
        }
        const float wgt = (a.is_weights ? a.is_weights[b] : 1.f) / (float)a.batch;
        const float d = wgt * (qk * (Sk - G) + a.ent_coef * (qk * (lq + a.entropy[b])));
        float* dl = a.dlogits + b * a.n_stride;
        for (int o = lane; o < a.n_stride; o += 64) dl[o] = o < n ? d : 0.f;    // (o < n <= 64: o == lane)
        if (lane == 0) a.frac_rows[b] = wgt * G;
    }
    __syncthreads();
    loss_tail(a, lane, wave, act, s_t, s_pred, s_tau, s_d, s_g, s_r);
}

bool logit_sizes_ok(int64_t batch, int n, int n_stride) {
    return batch >= 1 && batch <= 0x7fffffffLL && n >= 1 && n <= ARL_IQN_MAX_FRACTIONS && n_stride >= n &&
           (n_stride & 3) == 0 && n_stride <= (1 << 20) && batch * (n + 1) <= 0x7fffffffLL;
}

const char* const LOGIT_SIZES = "need 1 <= batch, batch x (fractions + 1) < 2^31, 1 <= fractions <= 64, "
                                "fractions <= n_stride <= 2^20 and n_stride % 4 == 0";

}  // namespace

extern "C" int arl_fqf_fractions(const float* logits, int64_t batch, int32_t n, int32_t n_stride, float* tau,
                                 float* tau_hat, float* tau_mid_or_null, float* q_or_null, float* logq_or_null,
                                 float* entropy_or_null, void* stream) {
    ARL_REQUIRE(logits && tau && tau_hat, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(logit_sizes_ok(batch, n, n_stride), ARL_E_ARG, LOGIT_SIZES);
    ARL_REQUIRE(arl::aligned16(logits), ARL_E_ALIGN, "16-byte alignment");
    hipLaunchKernelGGL(fractions_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, batch,
                       n, n_stride, tau, tau_hat, tau_mid_or_null, q_or_null, logq_or_null, entropy_or_null);
    return arl::check_launch("fqf fractions_kernel");
}

extern "C" int arl_fqf_act(const float* theta, const float* tau, const int32_t* override_or_null, int64_t batch,
                           int32_t n_actions, int32_t k, int32_t a_stride, float* onehot, uint8_t* greedy_or_null,
                           void* stream) {
    ARL_REQUIRE(theta && tau && onehot, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(theta_sizes_ok(batch, n_actions, k, a_stride), ARL_E_ARG, THETA_SIZES);
    ARL_REQUIRE(batch * ((int64_t)k + 1) <= 0x7fffffffLL, ARL_E_ARG, LOGIT_SIZES);
    hipLaunchKernelGGL(fqf_act_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream, theta, tau,
                       override_or_null, batch, n_actions, k, a_stride, onehot, greedy_or_null);
    return arl::check_launch("fqf act_kernel");
}

extern "C" int arl_fqf_loss(const float* pred, const float* pred_mid_or_null, const float* tau, const float* tau_hat,
                            const float* q, const float* logq, const float* entropy, const float* tgt_next,
                            const float* pol_next_or_null, const uint8_t* actions, const float* returns,
                            const uint8_t* terminals, const float* is_weights_or_null, int64_t batch, int32_t n_actions,
                            int32_t n, int32_t a_stride, int32_t n_stride, float gamma_n, float kappa, float ent_coef,
                            float* dtheta, float* loss_rows, float* priorities, float* dlogits, float* frac_rows,
                            void* stream) {
    FqfLossArgs a = {};
    const bool ptrs_ok = pred && (pred_mid_or_null || n == 1) && tau && tau_hat && q && logq && entropy && tgt_next &&
                         actions && returns && terminals && dtheta && loss_rows && priorities && dlogits && frac_rows;
    int rc = fill_iqn_loss(a, __func__, ptrs_ok, pred, tau_hat, tgt_next, actions, returns, terminals, is_weights_or_null,
                           batch, n_actions, n, n, a_stride, gamma_n, kappa, dtheta, loss_rows, priorities, nullptr, 0);
    if (rc) return rc;
    ARL_REQUIRE(logit_sizes_ok(batch, n, n_stride), ARL_E_ARG, LOGIT_SIZES);
    ARL_REQUIRE(ent_coef >= 0.f && ent_coef <= 3.0e38f, ARL_E_ARG, "ent_coef must be finite and >= 0");
    ARL_REQUIRE(arl::aligned16(dlogits), ARL_E_ALIGN, "16-byte alignment");
    a.pol_next = pol_next_or_null; a.pred_mid = pred_mid_or_null; a.tau = tau; a.q = q; a.logq = logq;
    a.entropy = entropy; a.dlogits = dlogits; a.frac_rows = frac_rows; a.n_stride = n_stride; a.ent_coef = ent_coef;
    hipLaunchKernelGGL(fqf_loss_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("fqf loss_kernel");
}
