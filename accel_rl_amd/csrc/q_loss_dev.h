// What the value-based loss and action kernels of csrc/dqn.hip and csrc/iqn.hip share: the wave butterflies, the first
// maximum over a staged row of Q values, one term of the pairwise quantile-Huber loss, the fixed-order combine of the four
// waves' partial sums, and the epsilon-greedy serve tail of the wave-per-sample action kernels.  Internal; every
// function is inlined into its callers, which are compiled with -ffp-contract=off: the operations and their order are
// part of the kernels' stated results (include/accel_rl_hip.h) -- do not re-associate them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace arlq
