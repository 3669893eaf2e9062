// Q(lambda) returns of an on-policy Q-learner (PQN, Gallici et al. 2024; not in the reference): arl_qlambda_scan.
// (A source of its own next to scan.hip: the committed counter records of the GAE / n-step scans are keyed to that
// file's hash, tests/test_host_logic.py, and nothing of theirs changes here.)
// One wave (a 64-thread block) per env.  Parallel part: lane l takes the steps t = l, l + 64, ..: the fp32 maximum of the
// first n_actions entries of the bootstrap row of step t (q row (e, t + 1), or q_last row e for the last step), read as
// float4s, into LDS next to the step's reward and done flag.  Sequential part: lane 0 walks t = T - 1 .. 0 with R in
// float64, the expression of accel_rl_hip.h operation for operation (no contraction), leaving (float) R in LDS; the
// lanes then store the env's returns together.  LDS: 9 bytes per step (<= 36 KiB at the horizon limit of 4096).
#include "arl_common.h"

namespace {

constexpr int QL_MAX_ACTIONS = 64;

__global__ __launch_bounds__(64) void qlambda_scan_kernel(const float* __restrict__ q, const float* __restrict__ q_last,
                                                          const float* __restrict__ rewards,
                                                          const uint8_t* __restrict__ dones, double discount,
                                                          double lambda, int T, int n_actions, int stride,
                                                          float* __restrict__ returns) {
    extern __shared__ float ql_lds[];
    float* boot = ql_lds;                    // [T] b_t
    float* rr = ql_lds + T;                  // [T] r_t, then (float) R_t
    uint8_t* dd = reinterpret_cast<uint8_t*>(ql_lds + 2 * (int64_t)T);     // [T] done_t
    const int64_t e = blockIdx.x;
    const int lane = threadIdx.x;
    const int n4 = (n_actions + 3) >> 2;
    for (int t = lane; t < T; t += 64) {
        const float* row = t + 1 < T ? q + (e * T + t + 1) * stride : q_last + e * stride;
        const float4* row4 = reinterpret_cast<const float4*>(row);
        float m = row[0];
        for (int k = 0; k < n4; ++k) {
            const float4 v = row4[k];
            const int a0 = 4 * k;
            m = fmaxf(m, v.x);
            if (a0 + 1 < n_actions) m = fmaxf(m, v.y);
            if (a0 + 2 < n_actions) m = fmaxf(m, v.z);
            if (a0 + 3 < n_actions) m = fmaxf(m, v.w);
        }
        boot[t] = m;
        rr[t] = rewards[e * T + t];
        dd[t] = dones[e * T + t];
    }
    __syncthreads();
    if (lane == 0) {
        double R = 0.0;
        for (int t = T - 1; t >= 0; --t) {
            const double b = (double)boot[t];
            const double next = t == T - 1 ? discount * b : discount * (b + lambda * (R - b));
            R = (double)rr[t] + (dd[t] ? 0.0 : next);
            rr[t] = (float)R;
        }
    }
    __syncthreads();
    for (int t = lane; t < T; t += 64) returns[e * T + t] = rr[t];
}

}  // namespace

extern "C" int arl_qlambda_scan(const float* q, const float* q_last, const float* rewards, const uint8_t* dones,
                                double discount, double lambda, int64_t n_env, int32_t horizon, int32_t n_actions,
                                int32_t q_stride, float* returns, void* stream) {
    ARL_REQUIRE(q && q_last && rewards && dones && returns, ARL_E_ARG, "null pointer");
    ARL_ENV_SCAN_SIZES(n_env, horizon);
    ARL_REQUIRE(n_actions >= 1 && n_actions <= QL_MAX_ACTIONS, ARL_E_RANGE, "1 <= n_actions <= 64");
    ARL_ENV_SCAN_Q_STRIDE(q_stride, n_actions);
    ARL_REQUIRE(arl::unit_interval(discount) && arl::unit_interval(lambda), ARL_E_ARG,
                "discount and lambda must lie in [0, 1]");
    ARL_REQUIRE(arl::aligned16(q) && arl::aligned16(q_last) && arl::aligned4(rewards) && arl::aligned4(returns),
                ARL_E_ALIGN, "q and q_last 16-byte, rewards and returns 4-byte aligned");
    const int64_t steps = n_env * horizon;
    const arl::Span in[4] = {{q, steps * q_stride * 4}, {q_last, n_env * q_stride * 4}, {rewards, steps * 4}, {dones, steps}};
    const arl::Span out[1] = {{returns, steps * 4}};
    if (!arl::check_disjoint(__func__, in, 4, out, 1)) return ARL_E_ARG;
    hipLaunchKernelGGL(qlambda_scan_kernel, dim3((unsigned)n_env), dim3(64), (size_t)horizon * 9 + 16, (hipStream_t)stream,
                       q, q_last, rewards, dones, discount, lambda, (int)horizon, (int)n_actions, (int)q_stride, returns);
    return arl::check_launch("qlambda_scan_kernel");
}
