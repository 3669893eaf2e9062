// V-trace value targets and policy-gradient advantages of an off-policy actor-critic learner (IMPALA, Espeholt et al.
// 2018; not in the reference): arl_vtrace_scan.
// (A source of its own next to scan.hip, as qlambda_scan.hip is: the committed counter records of the GAE / n-step scans
// are keyed to that file's hash, tests/test_host_logic.py, and nothing of theirs changes here.)
// One wave (a 64-thread block) per env, the rollout walked in chunks of VT_CHUNK steps from its end so that the staging
// area is a fixed 17 KiB of LDS whatever the horizon.  Per chunk -- parallel part: lane l takes the chunk's steps l,
// l + 64, ..: p = prob[row][a], m = old_prob[row][a], the float64 ratio (the one division of a step), r_t, V_t and
// done_t into LDS.  Sequential part: lane 0 walks the chunk's steps downwards in float64, the expressions of
// accel_rl_hip.h operation for operation (no contraction), carrying acc_next, vs_next and v_next in registers across
// steps and chunks (never the rounded floats), and leaves (float) vs and (float) adv where r_t and V_t stood.  The lanes
// then store the chunk's results together.  An associative scan would change the rounding; none is used.
#include "arl_common.h"

namespace {

constexpr int VT_CHUNK = 1024;

__global__ __launch_bounds__(64) void vtrace_scan_kernel(
    const float* __restrict__ prob, const float* __restrict__ old_prob, const uint8_t* __restrict__ actions,
    const float* __restrict__ values, const float* __restrict__ last_values, const float* __restrict__ rewards,
    const uint8_t* __restrict__ dones, double discount, double lambda, double rho_bar, double c_bar, double pg_rho_bar,
    int T, int n_actions, float* __restrict__ returns, float* __restrict__ advantages, float* __restrict__ stats) {
    __shared__ double ratio_s[VT_CHUNK];     // ratio_t
    __shared__ float rr[VT_CHUNK];           // r_t, then (float) vs_t
    __shared__ float vv[VT_CHUNK];           // V_t, then (float) adv_t
    __shared__ uint8_t dd[VT_CHUNK];         // done_t
    const int64_t e = blockIdx.x;
    const int64_t row0 = e * T;
    const int lane = threadIdx.x;
    // lane 0's carry (the other lanes hold the same initial values and never touch them again)
    double acc_next = 0.0, v_next = (double)last_values[e], vs_next = v_next, ratio_sum = 0.0;
    int n_clipped = 0;
    for (int hi = T; hi > 0; hi -= VT_CHUNK) {
        const int lo = hi > VT_CHUNK ? hi - VT_CHUNK : 0;
        const int len = hi - lo;
        for (int i = lane; i < len; i += 64) {
            const int64_t row = row0 + lo + i;
            int a = actions[row];
            a = a < n_actions - 1 ? a : n_actions - 1;
            const double p = (double)prob[row * n_actions + a], m = (double)old_prob[row * n_actions + a];
            ratio_s[i] = (p + 1e-8) / (m + 1e-8);
            rr[i] = rewards[row];
            vv[i] = values[row];
            dd[i] = dones[row];
        }
        __syncthreads();
        if (lane == 0) {
            for (int i = len - 1; i >= 0; --i) {
                const double ratio = ratio_s[i], r = (double)rr[i], v = (double)vv[i];
                const double rho = ratio < rho_bar ? ratio : rho_bar;
                const double cw = ratio < c_bar ? ratio : c_bar;
                const double pg = ratio < pg_rho_bar ? ratio : pg_rho_bar;
                const double g = dd[i] ? 0.0 : discount;
                const double q_v = r + g * v_next;
                const double delta = rho * (q_v - v);
                const double acc = delta + ((g * (lambda * cw)) * acc_next);
                const double vs = v + acc;
                const double adv = pg * ((r + g * vs_next) - v);
                rr[i] = (float)vs;
                vv[i] = (float)adv;
                ratio_sum = ratio_sum + ratio;
                n_clipped += ratio > rho_bar ? 1 : 0;
                acc_next = acc;
                vs_next = vs;
                v_next = v;
            }
        }
        __syncthreads();
        for (int i = lane; i < len; i += 64) {
            returns[row0 + lo + i] = rr[i];
            advantages[row0 + lo + i] = vv[i];
        }
        __syncthreads();                     // the next chunk's loads overwrite what these stores read
    }
    if (stats && lane == 0) {
        stats[2 * e] = (float)ratio_sum;
        stats[2 * e + 1] = (float)n_clipped;
    }
}

}  // namespace

extern "C" int arl_vtrace_scan(const float* prob, const float* old_prob, const uint8_t* actions, const float* values,
                               const float* last_values, const float* rewards, const uint8_t* dones, double discount,
                               double lambda, double rho_bar, double c_bar, double pg_rho_bar, int64_t n_env,
                               int32_t horizon, int32_t n_actions, float* returns, float* advantages,
                               float* stats_or_null, void* stream) {
    ARL_REQUIRE(prob && old_prob && actions && values && last_values && rewards && dones && returns && advantages,
                ARL_E_ARG, "null pointer");
    ARL_ENV_SCAN_SIZES(n_env, horizon);
    ARL_REQUIRE(n_actions >= 1 && n_actions <= ARL_MAX_ACTIONS, ARL_E_RANGE, "1 <= n_actions <= 18");
    ARL_REQUIRE(arl::unit_interval(discount) && arl::unit_interval(lambda), ARL_E_ARG,
                "discount and lambda must lie in [0, 1]");
    ARL_REQUIRE(arl::finite_positive(rho_bar) && arl::finite_positive(c_bar) && arl::finite_positive(pg_rho_bar),
                ARL_E_ARG, "rho_bar, c_bar and pg_rho_bar must be finite and > 0");
    const int64_t steps = n_env * horizon;
    const arl::Span in[7] = {
        {prob, steps * n_actions * 4}, {old_prob, steps * n_actions * 4}, {actions, steps}, {values, steps * 4},
        {last_values, n_env * 4}, {rewards, steps * 4}, {dones, steps}};
    const arl::Span out[3] = {{returns, steps * 4}, {advantages, steps * 4}, {stats_or_null, n_env * 8}};
    if (!arl::check_disjoint(__func__, in, 7, out, 3)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned4(prob) && arl::aligned4(old_prob) && arl::aligned4(values) && arl::aligned4(last_values) &&
                arl::aligned4(rewards) && arl::aligned4(returns) && arl::aligned4(advantages) &&
                arl::aligned4(stats_or_null), ARL_E_ALIGN, "every float pointer must be 4-byte aligned");
    hipLaunchKernelGGL(vtrace_scan_kernel, dim3((unsigned)n_env), dim3(64), 0, (hipStream_t)stream, prob, old_prob,
                       actions, values, last_values, rewards, dones, discount, lambda, rho_bar, c_bar, pg_rho_bar,
                       (int)horizon, (int)n_actions, returns, advantages, stats_or_null);
    return arl::check_launch("vtrace_scan_kernel");
}
