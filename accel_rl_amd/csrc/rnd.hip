// Random network distillation (RND; single value head, one reward stream) for gfx950: the streaming and scan stages the
// exploration bonus adds around the two conv trunks, which run on the contraction kernels.
//
//   arl_rnd_obs_stats    running per-pixel mean / variance of the newest plane of every NEXT observation: exact integer
//                        sums over the batch, Chan's merge in float64
//   arl_rnd_obs_prepare  clamp((x - mean) / sqrt(m2 / count + 1e-8), -5, 5) of those frames -> f32 NHWC, channels 1..3 zero
//   arl_rnd_error        err[b] = mean_e (pred - targ)^2 in float64, its gradient and the mean over the rows
//   arl_rnd_reward_mix   per-env discounted running sum of err -> running moments -> r_mix = c_ext r_ext + c_int err / std
//
// include/accel_rl_hip.h states every expression and order.  float64 from the promoted inputs on, every output rounded
// once; no float atomics, no process-wide state; compiled with -ffp-contract=off.

#include <cmath>

#include "arl_optim_dev.h"

namespace {

constexpr int RND_THREADS = 256;
constexpr int MIX_THREADS = 1024;
constexpr double RND_VAR_EPS = 1e-8;

// the newest plane of the observation that FOLLOWS transition `row` = n * T + t of an env-major rollout
__device__ __forceinline__ const uint8_t* next_frame(const uint8_t* obs, const uint8_t* extra, int64_t row, int T, int C,
                                                     int64_t hw) {
    const int64_t n = row / T;
    const int t = (int)(row - n * T);
    return t + 1 < T ? obs + ((row + 1) * C + (C - 1)) * hw : extra + (n * C + (C - 1)) * hw;
}

// Chan's merge of (nb, mean_b, m2_b) into (na, mean, m2); the caller writes the new count na + nb
__device__ __forceinline__ void chan_merge(double na, double nb, double mean_b, double m2_b, double& mean, double& m2) {
    const double w = nb / (na + nb);
    const double delta = mean_b - mean;
    mean = mean + delta * w;
    m2 = (m2 + m2_b) + ((delta * delta) * na) * w;
}

// ---------------------------------------------------------------- observation statistics

// grid (pixel groups, splits): split z sums rows z, z + splits, ... of V adjacent pixels per thread into
// part[z][0 = sum x | 1 = sum x^2][pixel]; integers, so neither the split nor the order shows in the result.
template <int V>
__global__ __launch_bounds__(RND_THREADS) void rnd_stats_partial_kernel(const uint8_t* __restrict__ obs,
                                                                       const uint8_t* __restrict__ extra, int64_t rows,
                                                                       int T, int C, int64_t hw,
                                                                       const double* __restrict__ count,
                                                                       unsigned long long* __restrict__ part,
                                                                       double* __restrict__ count_old) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) count_old[0] = count[0];
    const int64_t p = ((int64_t)blockIdx.x * RND_THREADS + threadIdx.x) * V;
    if (p >= hw) return;
    unsigned long long sx[V], sxx[V];
#pragma unroll
    for (int v = 0; v < V; ++v) sx[v] = sxx[v] = 0ull;
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const uint8_t* f = next_frame(obs, extra, r, T, C, hw) + p;
        uint32_t word;
        if (V == 4) word = *reinterpret_cast<const uint32_t*>(f);
        else word = f[0];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const unsigned long long x = (word >> (8 * v)) & 255u;
            sx[v] += x;
            sxx[v] += x * x;
        }
    }
    unsigned long long* out = part + (int64_t)blockIdx.y * 2 * hw;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        out[p + v] = sx[v];
        out[hw + p + v] = sxx[v];
    }
}

__global__ __launch_bounds__(RND_THREADS) void rnd_stats_merge_kernel(const unsigned long long* __restrict__ part,
                                                                     int splits, int64_t rows, int64_t hw,
                                                                     const double* __restrict__ count_old,
                                                                     double* __restrict__ count, double* __restrict__ mean,
                                                                     double* __restrict__ m2) {
    const int64_t p = (int64_t)blockIdx.x * RND_THREADS + threadIdx.x;
    const double na = count_old[0], nb = (double)rows;
    if (p == 0) count[0] = na + nb;
    if (p >= hw) return;
    unsigned long long sx = 0ull, sxx = 0ull;
    for (int z = 0; z < splits; ++z) {
        sx += part[(int64_t)z * 2 * hw + p];
        sxx += part[(int64_t)z * 2 * hw + hw + p];
    }
    // rows <= 2^24: rows * sxx <= 2^48 * 65025 < 2^64, and >= sx^2 (Cauchy-Schwarz)
    const unsigned long long num = (unsigned long long)rows * sxx - sx * sx;
    const double mean_b = (double)sx / nb;
    const double m2_b = (double)num / nb;
    double mu = mean[p], s = m2[p];
    chan_merge(na, nb, mean_b, m2_b, mu, s);
    mean[p] = mu;
    m2[p] = s;
}

// ---------------------------------------------------------------- network input

// grid (pixel blocks, row groups): a thread owns one pixel, forms its deviation once and walks rows y, y + gridDim.y, ...
__global__ __launch_bounds__(RND_THREADS) void rnd_prepare_kernel(const uint8_t* __restrict__ obs,
                                                                 const uint8_t* __restrict__ extra,
                                                                 const int32_t* __restrict__ idx, int64_t batch, int T,
                                                                 int C, int64_t hw, const double* __restrict__ count,
                                                                 const double* __restrict__ mean,
                                                                 const double* __restrict__ m2, float4* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * RND_THREADS + threadIdx.x;
    if (p >= hw) return;
    const double mu = mean[p];
    const double sd = sqrt(m2[p] / count[0] + RND_VAR_EPS);
    for (int64_t b = blockIdx.y; b < batch; b += gridDim.y) {
        const int64_t row = idx ? (int64_t)idx[b] : b;
        const double x = (double)next_frame(obs, extra, row, T, C, hw)[p];
        double z = (x - mu) / sd;
        z = z < -5.0 ? -5.0 : z;
        z = z > 5.0 ? 5.0 : z;
        out[b * hw + p] = make_float4((float)z, 0.f, 0.f, 0.f);
    }
}

// ---------------------------------------------------------------- prediction error

// One wave per row, rows wave, wave + (waves of the grid), ...  Lane l adds the four elements of its float4s l, l + 64,
// ... in ascending order; the wave adds by halving shuffles (offsets 32 .. 1).
__global__ __launch_bounds__(RND_THREADS) void rnd_error_kernel(const float* __restrict__ pred,
                                                               const float* __restrict__ targ, int64_t batch, int E,
                                                               float* __restrict__ err, float* __restrict__ dpred) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (RND_THREADS / 64);
    const double e_d = (double)E, scale = e_d * (double)batch;
    for (int64_t b = (int64_t)blockIdx.x * (RND_THREADS / 64) + (threadIdx.x >> 6); b < batch; b += waves) {
        const float4* p4 = reinterpret_cast<const float4*>(pred + b * E);
        const float4* t4 = reinterpret_cast<const float4*>(targ + b * E);
        float4* g4 = dpred ? reinterpret_cast<float4*>(dpred + b * E) : nullptr;
        double acc = 0.0;
        for (int i = lane; i < E / 4; i += 64) {
            const float4 p = p4[i], t = t4[i];
            const double d0 = (double)p.x - (double)t.x, d1 = (double)p.y - (double)t.y;
            const double d2 = (double)p.z - (double)t.z, d3 = (double)p.w - (double)t.w;
            acc += d0 * d0;
            acc += d1 * d1;
            acc += d2 * d2;
            acc += d3 * d3;
            if (g4)
                g4[i] = make_float4((float)((2.0 * d0) / scale), (float)((2.0 * d1) / scale), (float)((2.0 * d2) / scale),
                                    (float)((2.0 * d3) / scale));
        }
        const double s = arl::wave_sum_d(acc);
        if (lane == 0) err[b] = (float)(s / e_d);
    }
}

// one workgroup: thread t adds err[t], err[t + 1024], ... (promoted) in ascending order; block_sum_d's order
__global__ __launch_bounds__(MIX_THREADS) void rnd_loss_kernel(const float* __restrict__ err, int64_t batch,
                                                              float* __restrict__ loss) {
    __shared__ double s_red[MIX_THREADS / 64];
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < batch; b += MIX_THREADS) s += (double)err[b];
    const double S = arl::block_sum_d(s, s_red);
    if (threadIdx.x == 0) loss[0] = (float)(S / (double)batch);
}

// ---------------------------------------------------------------- reward mix

__global__ __launch_bounds__(MIX_THREADS) void rnd_reward_mix_kernel(const float* __restrict__ err,
                                                                    const float* __restrict__ r_ext, int n_env, int T,
                                                                    double* __restrict__ rho, double* __restrict__ moments,
                                                                    double gamma, double c_ext, double c_int,
                                                                    float* __restrict__ r_mix, float* __restrict__ diag,
                                                                    double* __restrict__ ret) {
    __shared__ double s_red[MIX_THREADS / 64];
    __shared__ double s_sd;
    const int tid = threadIdx.x;
    const int64_t total = (int64_t)n_env * T;
    // 1. the running discounted sum of the bonus, per env in time order (not reset at dones)
    for (int n = tid; n < n_env; n += MIX_THREADS) {
        double r = rho[n];
        for (int t = 0; t < T; ++t) {
            r = gamma * r + (double)err[(int64_t)n * T + t];
            ret[(int64_t)n * T + t] = r;
        }
        rho[n] = r;
    }
    __syncthreads();
    // 2. the batch's moments, two passes
    double s = 0.0, se = 0.0;
    for (int64_t j = tid; j < total; j += MIX_THREADS) {
        s += ret[j];
        se += (double)err[j];
    }
    const double S1 = arl::block_sum_d(s, s_red);
    const double SE = arl::block_sum_d(se, s_red);
    const double nb = (double)total;
    const double mean_b = S1 / nb;
    double q = 0.0;
    for (int64_t j = tid; j < total; j += MIX_THREADS) {
        const double d = ret[j] - mean_b;
        q += d * d;
    }
    const double m2_b = arl::block_sum_d(q, s_red);
    // 3. merged into the running moments BEFORE this batch is normalised
    if (tid == 0) {
        const double na = moments[0];
        double mu = moments[1], m2 = moments[2];
        chan_merge(na, nb, mean_b, m2_b, mu, m2);
        const double cnt = na + nb;
        moments[0] = cnt;
        moments[1] = mu;
        moments[2] = m2;
        const double sd = sqrt(m2 / cnt + RND_VAR_EPS);
        s_sd = sd;
        diag[0] = (float)(SE / nb);
        diag[1] = (float)sd;
    }
    __syncthreads();
    const double sd = s_sd;
    // 4. the mixed reward; a zero bonus term leaves the extrinsic one as it is (the sign of a zero included)
    for (int64_t j = tid; j < total; j += MIX_THREADS) {
        const double a = c_ext * (double)r_ext[j];
        const double b = c_int * ((double)err[j] / sd);
        r_mix[j] = (float)(b == 0.0 ? a : a + b);
    }
}

int check_frames(const void* obs, const void* extra, int64_t n_env, int32_t horizon, int32_t c, int32_t h, int32_t w) {
    ARL_REQUIRE(obs && extra, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n_env >= 1 && horizon >= 1 && horizon <= ARL_RND_MAX_HORIZON && n_env * horizon <= ARL_RND_MAX_ROWS,
                ARL_E_RANGE, "1 <= n_env, 1 <= horizon <= 4096, n_env * horizon <= 2^24");
    ARL_REQUIRE(c >= 1 && c <= 1024 && h >= 1 && w >= 1 && (int64_t)h * w <= ARL_RND_MAX_PIXELS, ARL_E_RANGE,
                "1 <= channels <= 1024, 1 <= h * w <= 2^24");
    return 0;
}

}  // namespace

extern "C" int64_t arl_rnd_obs_stats_workspace_bytes(int32_t h, int32_t w) {
    if (h < 1 || w < 1 || (int64_t)h * w > ARL_RND_MAX_PIXELS) return 0;
    return ((int64_t)2 * ARL_RND_STATS_SPLITS * h * w + 2) * 8;
}

extern "C" int arl_rnd_obs_stats(const uint8_t* observations, const uint8_t* extra_observations, int64_t n_env,
                                 int32_t horizon, int32_t channels, int32_t h, int32_t w, double* count, double* mean,
                                 double* m2, void* workspace, void* stream) {
    int rc = check_frames(observations, extra_observations, n_env, horizon, channels, h, w);
    if (rc) return rc;
    ARL_REQUIRE(count && mean && m2 && workspace, ARL_E_ARG, "null pointer");
    ARL_REQUIRE((reinterpret_cast<uintptr_t>(count) & 7u) == 0 && (reinterpret_cast<uintptr_t>(mean) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(m2) & 7u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
                ARL_E_ALIGN, "count, mean, m2 and workspace must be 8-byte aligned");
    const int64_t hw = (int64_t)h * w, rows = n_env * horizon;
    const int splits = (int)(rows < ARL_RND_STATS_SPLITS ? rows : ARL_RND_STATS_SPLITS);
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    double* count_old = reinterpret_cast<double*>(part + (int64_t)2 * ARL_RND_STATS_SPLITS * hw);
    hipStream_t s = (hipStream_t)stream;
    // four pixels per lane where every frame starts on a 4-byte boundary
    const bool vec = hw % 4 == 0 && arl::aligned4(observations) && arl::aligned4(extra_observations);
    if (vec) {
        const dim3 grid((unsigned)((hw / 4 + RND_THREADS - 1) / RND_THREADS), (unsigned)splits);
        hipLaunchKernelGGL(rnd_stats_partial_kernel<4>, grid, dim3(RND_THREADS), 0, s, observations, extra_observations,
                           rows, horizon, channels, hw, count, part, count_old);
    } else {
        const dim3 grid((unsigned)((hw + RND_THREADS - 1) / RND_THREADS), (unsigned)splits);
        hipLaunchKernelGGL(rnd_stats_partial_kernel<1>, grid, dim3(RND_THREADS), 0, s, observations, extra_observations,
                           rows, horizon, channels, hw, count, part, count_old);
    }
    rc = arl::check_launch("rnd_stats_partial_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(rnd_stats_merge_kernel, dim3((unsigned)((hw + RND_THREADS - 1) / RND_THREADS)), dim3(RND_THREADS),
                       0, s, part, splits, rows, hw, count_old, count, mean, m2);
    return arl::check_launch("rnd_stats_merge_kernel");
}

extern "C" int arl_rnd_obs_prepare(const uint8_t* observations, const uint8_t* extra_observations,
                                   const int32_t* idx_or_null, int64_t batch, int64_t n_env, int32_t horizon,
                                   int32_t channels, int32_t h, int32_t w, const double* count, const double* mean,
                                   const double* m2, float* out, void* stream) {
    int rc = check_frames(observations, extra_observations, n_env, horizon, channels, h, w);
    if (rc) return rc;
    ARL_REQUIRE(count && mean && m2 && out, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(batch >= 1 && batch <= ARL_RND_MAX_ROWS, ARL_E_RANGE, "1 <= batch <= 2^24");
    ARL_REQUIRE(idx_or_null || batch <= n_env * horizon, ARL_E_RANGE, "without idx: batch <= n_env * horizon");
    ARL_REQUIRE(arl::aligned16(out) && (!idx_or_null || arl::aligned4(idx_or_null)) &&
                    (reinterpret_cast<uintptr_t>(count) & 7u) == 0 && (reinterpret_cast<uintptr_t>(mean) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(m2) & 7u) == 0,
                ARL_E_ALIGN, "out 16-byte, idx 4-byte, count / mean / m2 8-byte aligned");
    const int64_t hw = (int64_t)h * w;
    const int64_t pix_blocks = (hw + RND_THREADS - 1) / RND_THREADS;
    int64_t groups = (2048 + pix_blocks - 1) / pix_blocks;           // about 2048 workgroups in all
    if (groups > batch) groups = batch;
    hipLaunchKernelGGL(rnd_prepare_kernel, dim3((unsigned)pix_blocks, (unsigned)groups), dim3(RND_THREADS), 0,
                       (hipStream_t)stream, observations, extra_observations, idx_or_null, batch, horizon, channels, hw,
                       count, mean, m2, reinterpret_cast<float4*>(out));
    return arl::check_launch("rnd_prepare_kernel");
}

extern "C" int arl_rnd_error(const float* pred, const float* targ, int64_t batch, int32_t width, int32_t want_grad,
                             float* err, float* dpred, float* loss, void* stream) {
    ARL_REQUIRE(pred && targ && err, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(!want_grad || (dpred && loss), ARL_E_ARG, "want_grad needs dpred and loss");
    ARL_REQUIRE(batch >= 1 && batch <= ARL_RND_MAX_ROWS, ARL_E_RANGE, "1 <= batch <= 2^24");
    ARL_REQUIRE(width >= 4 && width <= ARL_RND_MAX_WIDTH && width % 4 == 0, ARL_E_RANGE,
                "width a multiple of 4 in 4 .. 2^16");
    ARL_REQUIRE(arl::aligned16(pred) && arl::aligned16(targ) && arl::aligned4(err) &&
                    (!want_grad || (arl::aligned16(dpred) && arl::aligned4(loss))),
                ARL_E_ALIGN, "pred, targ and dpred 16-byte, err and loss 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rnd_error_kernel, dim3(arl::stream_grid(batch, RND_THREADS / 64)), dim3(RND_THREADS), 0, s, pred,
                       targ, batch, (int)width, err, want_grad ? dpred : nullptr);
    int rc = arl::check_launch("rnd_error_kernel");
    if (rc || !want_grad) return rc;
    hipLaunchKernelGGL(rnd_loss_kernel, dim3(1), dim3(MIX_THREADS), 0, s, err, batch, loss);
    return arl::check_launch("rnd_loss_kernel");
}

extern "C" int arl_rnd_reward_mix(const float* err, const float* r_ext, int64_t n_env, int32_t horizon, double* rho,
                                  double* moments, double gamma_int, double c_ext, double c_int, float* r_mix,
                                  float* diag2, void* workspace, void* stream) {
    ARL_REQUIRE(err && r_ext && rho && moments && r_mix && diag2 && workspace, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(gamma_int) && gamma_int >= 0.0 && gamma_int <= 1.0 && std::isfinite(c_ext) &&
                    std::isfinite(c_int),
                ARL_E_ARG, "gamma_int in [0, 1], c_ext and c_int finite");
    ARL_REQUIRE(n_env >= 1 && n_env <= ARL_RND_MIX_MAX_ENVS && horizon >= 1 && horizon <= ARL_RND_MAX_HORIZON &&
                    n_env * horizon <= ARL_RND_MIX_MAX_ROWS,
                ARL_E_RANGE, "1 <= n_env <= 2^20, 1 <= horizon <= 4096, n_env * horizon <= 2^22");
    ARL_REQUIRE(r_mix != err && r_mix != r_ext, ARL_E_ARG, "r_mix must not be an input");
    ARL_REQUIRE(arl::aligned4(err) && arl::aligned4(r_ext) && arl::aligned4(r_mix) && arl::aligned4(diag2) &&
                    (reinterpret_cast<uintptr_t>(rho) & 7u) == 0 && (reinterpret_cast<uintptr_t>(moments) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
                ARL_E_ALIGN, "float pointers 4-byte, rho / moments / workspace 8-byte aligned");
    hipLaunchKernelGGL(rnd_reward_mix_kernel, dim3(1), dim3(MIX_THREADS), 0, (hipStream_t)stream, err, r_ext, (int)n_env,
                       (int)horizon, rho, moments, gamma_int, c_ext, c_int, r_mix, diag2, static_cast<double*>(workspace));
    return arl::check_launch("rnd_reward_mix_kernel");
}
