// PopArt (adaptive value normalisation; single task) for gfx950: the two stages it adds between the rollout and the
// optimiser step of an actor-critic whose value output is a NORMALISED value.
//
//   arl_popart_denorm   (float) (sigma n + mu) of the recorded and of the bootstrap values, one streaming launch
//   arl_popart_step     batch moments of the return targets -> running statistics -> the head's value row and bias
//                       rewritten so that sigma n + mu of every state stays what it was -> returns (and advantages)
//                       normalised in place; one workgroup, one launch
//
// include/accel_rl_hip.h states every expression and order.  float64 from the promoted inputs on, every output rounded
// once; no float atomics, no process-wide state; compiled with -ffp-contract=off.

#include <cmath>

#include "arl_optim_dev.h"

namespace {

constexpr int DENORM_THREADS = 256;
constexpr int STEP_THREADS = 1024;

__global__ __launch_bounds__(DENORM_THREADS) void popart_denorm_kernel(const float* __restrict__ value_n, int64_t rows,
                                                                      const float* __restrict__ last_n, int64_t n_last,
                                                                      const double* __restrict__ stats,
                                                                      float* __restrict__ value,
                                                                      float* __restrict__ last_value) {
    const double mu = stats[0], sigma = stats[2];
    const int64_t total = rows + n_last, stride = (int64_t)gridDim.x * DENORM_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * DENORM_THREADS + threadIdx.x; i < total; i += stride) {
        if (i < rows) value[i] = (float)(sigma * (double)value_n[i] + mu);
        else last_value[i - rows] = (float)(sigma * (double)last_n[i - rows] + mu);
    }
}

__global__ __launch_bounds__(STEP_THREADS) void popart_step_kernel(float* __restrict__ returns, float* __restrict__ adv,
                                                                  const int8_t* __restrict__ valids, int64_t rows,
                                                                  double beta, double sigma_min, double sigma_max,
                                                                  double* __restrict__ stats, float* __restrict__ w_value,
                                                                  float* __restrict__ b_value, int hid,
                                                                  float* __restrict__ diag) {
    __shared__ double s_red[STEP_THREADS / 64];
    const int tid = threadIdx.x;
    // every thread takes the statistics before thread 0 rewrites them (the reductions' barriers lie in between)
    const double mu = stats[0], nu = stats[1], sigma = stats[2], n_upd = stats[3];
    // 1. the batch's moments over the valid rows
    double c = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t i = tid; i < rows; i += STEP_THREADS) {
        if (valids && valids[i] == 0) continue;
        const double g = (double)returns[i];
        c += 1.0;
        s1 += g;
        s2 += g * g;
    }
    const double cnt = arl::block_sum_d(c, s_red);
    const double S1 = arl::block_sum_d(s1, s_red);
    const double S2 = arl::block_sum_d(s2, s_red);
    const double m1 = S1 / cnt, m2 = S2 / cnt;
    // 2. the statistics (every thread the same arithmetic on the same values)
    const bool ok = cnt > 0.0 && isfinite(m1) && isfinite(m2);
    double mu_n = mu, sigma_n = sigma;
    if (ok) {
        mu_n = (1.0 - beta) * mu + beta * m1;
        const double nu_n = (1.0 - beta) * nu + beta * m2;
        double var = nu_n - mu_n * mu_n;
        var = var > 0.0 ? var : 0.0;
        double sd = sqrt(var);
        sd = sd > sigma_min ? sd : sigma_min;
        sd = sd < sigma_max ? sd : sigma_max;
        sigma_n = sd;
        // 3. the head's value row and bias: sigma' n' + mu' = sigma n + mu for every hidden row
        const double ratio = sigma / sigma_n;
        for (int j = tid; j < hid; j += STEP_THREADS) w_value[j] = (float)((double)w_value[j] * ratio);
        if (tid == 0) {
            b_value[0] = (float)(((sigma * (double)b_value[0] + mu) - mu_n) / sigma_n);
            stats[0] = mu_n;
            stats[1] = nu_n;
            stats[2] = sigma_n;
            stats[3] = n_upd + 1.0;
        }
    }
    if (tid == 0) {
        diag[0] = (float)mu_n;
        diag[1] = (float)sigma_n;
    }
    // 4. the targets the loss sees, in place
    for (int64_t i = tid; i < rows; i += STEP_THREADS) {
        const bool valid = !valids || valids[i] != 0;
        returns[i] = valid ? (float)(((double)returns[i] - mu_n) / sigma_n) : 0.f;
        if (adv) adv[i] = valid ? (float)((double)adv[i] / sigma_n) : 0.f;
    }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int arl_popart_denorm(const float* value_n, int64_t rows, const float* last_n, int64_t n_last,
                                 const double* stats, float* value, float* last_value, void* stream) {
    ARL_REQUIRE(value_n && last_n && stats && value && last_value, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(rows >= 1 && rows <= ARL_POPART_MAX_ROWS && n_last >= 1 && n_last <= rows, ARL_E_RANGE,
                "1 <= rows <= 2^22, 1 <= n_last <= rows");
    const int64_t rb = rows * 4, lb = n_last * 4;
    ARL_REQUIRE(!arl::overlap(value, rb, value_n, rb) && !arl::overlap(value, rb, last_n, lb) &&
                    !arl::overlap(last_value, lb, value_n, rb) && !arl::overlap(last_value, lb, last_n, lb) &&
                    !arl::overlap(value, rb, last_value, lb),
                ARL_E_ARG, "value and last_value must not overlap an input or each other");
    ARL_REQUIRE(arl::aligned4(value_n) && arl::aligned4(last_n) && arl::aligned4(value) && arl::aligned4(last_value) &&
                    aligned8(stats),
                ARL_E_ALIGN, "float pointers 4-byte, stats 8-byte aligned");
    hipLaunchKernelGGL(popart_denorm_kernel, dim3(arl::stream_grid(rows + n_last, DENORM_THREADS)), dim3(DENORM_THREADS),
                       0, (hipStream_t)stream, value_n, rows, last_n, n_last, stats, value, last_value);
    return arl::check_launch("popart_denorm_kernel");
}

extern "C" int arl_popart_step(float* returns, float* advantages_or_null, const int8_t* valids_or_null, int64_t rows,
                               double beta, double sigma_min, double sigma_max, double* stats, float* w_value,
                               float* b_value, int32_t hid, float* diag2, void* stream) {
    ARL_REQUIRE(returns && stats && w_value && b_value && diag2, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(arl::unit_interval(beta), ARL_E_ARG, "beta must lie in [0, 1]");
    ARL_REQUIRE(std::isfinite(sigma_min) && std::isfinite(sigma_max) && sigma_min > 0.0 && sigma_min <= sigma_max,
                ARL_E_ARG, "0 < sigma_min <= sigma_max, both finite");
    ARL_REQUIRE(rows >= 1 && rows <= ARL_POPART_MAX_ROWS, ARL_E_RANGE, "1 <= rows <= 2^22");
    ARL_REQUIRE(hid >= 1 && hid <= ARL_POPART_MAX_HID, ARL_E_RANGE, "1 <= hid <= 65536");
    ARL_REQUIRE(!advantages_or_null || !arl::overlap(returns, rows * 4, advantages_or_null, rows * 4), ARL_E_ARG,
                "returns and advantages must not overlap");
    ARL_REQUIRE(arl::aligned4(returns) && arl::aligned4(advantages_or_null) && arl::aligned4(w_value) &&
                    arl::aligned4(b_value) && arl::aligned4(diag2) && aligned8(stats),
                ARL_E_ALIGN, "float pointers 4-byte, stats 8-byte aligned");
    hipLaunchKernelGGL(popart_step_kernel, dim3(1), dim3(STEP_THREADS), 0, (hipStream_t)stream, returns,
                       advantages_or_null, valids_or_null, rows, beta, sigma_min, sigma_max, stats, w_value, b_value,
                       (int)hid, diag2);
    return arl::check_launch("popart_step_kernel");
}
