// LayerNorm + rectifier between the contraction launches of a Q-network (PQN, Gallici et al. 2024; the reference has
// none): row-wise over z f32[rows][width] in contiguous memory (NHWC conv activation: rows = B * Ho * Wo, width = K;
// dense layer: rows = B, width = units).
//
//   arl_ln_relu_fwd    y = max(0, gamma * xhat + beta), stats = (mean, rstd); z is kept (the backward pass recomputes
//                      xhat from z and stats)
//   arl_ln_relu_bwd    dz (in place over dy or elsewhere), per-workgroup partial sums of dgamma / dbeta, folded by
//                      arl_fold_many (now, or by the caller's fold list)
//
// Both are streaming kernels: every element is read once as part of a float4 and lives in registers from there on.
// Lanes and summation order (stated in include/accel_rl_hip.h; DESIGN.md 22 derives the error bound from it):
//   a row is held by LPR consecutive lanes of one wave, V float4s per lane: lane l of the row holds the float4s
//   number v * LPR + l (v = 0 .. V - 1) of the row.
//        width   4 ..  32 :  LPR  8, V 1   (8 rows per wave)
//               36 ..  64 :  LPR 16, V 1   (4 rows per wave)
//               68 .. 256 :  LPR 64, V 1   (one wave per row)
//              260 .. 512 :  LPR 64, V 2
//              516 .. 1024:  LPR 64, V 4
//   a row sum: per lane s = q_0, then s = s + q_v for v = 1 .. V - 1, with q_v = ((x + y) + z) + w of float4 v (0 for a
//   float4 past the row's end); then a butterfly over the LPR lanes, s = s + s[lane ^ off] for off = LPR / 2, LPR / 4,
//   .. 1 (both partners compute the same sum: every lane of the row ends with the same bits).
//   a column sum (dgamma, dbeta): a block of 256 threads holds RPB = 256 / LPR row slots; slot k of block b walks the
//   rows b * RPB + k + i * grid * RPB (i ascending) and adds each row's term to its accumulator in that order; the
//   block's RPB accumulators are added in slot order (slot 0 first) into ONE partial row per block; arl_fold_many
//   adds the grid (<= 256) partial rows in its own fixed order.  No atomics anywhere.
//   (The forward leaves no partials and no result of it depends on the grid: it takes up to 2048 blocks.)
#include "arl_common.h"

#include <math.h>

namespace {

constexpr int LN_THREADS = 256, LN_MAX_GRID = 256, LN_MAX_WIDTH = 1024;
constexpr int LN_FWD_MAX_GRID = 2048;       // the forward leaves no per-block partials: as many blocks as fill the chip

__device__ __forceinline__ float quad_sum(const float4 v) { return ((v.x + v.y) + v.z) + v.w; }

template <int LPR>
__device__ __forceinline__ float row_sum(float s) {
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, LPR);
    return s;
}

struct LnSlot { int l, slot; };
template <int LPR>
__device__ __forceinline__ LnSlot ln_slot() {
    LnSlot s;
    s.l = threadIdx.x % LPR;
    s.slot = threadIdx.x / LPR;          // wave-major: a wave's 64 / LPR rows are consecutive slots
    return s;
}

template <int LPR, int V>
__global__ __launch_bounds__(LN_THREADS) void ln_relu_fwd_kernel(const float4* __restrict__ z,
                                                                 const float4* __restrict__ gamma,
                                                                 const float4* __restrict__ beta, int64_t rows, int w4,
                                                                 float width_f, float eps, int iters,
                                                                 float4* __restrict__ y, float2* __restrict__ stats) {
    constexpr int RPB = LN_THREADS / LPR;
    const LnSlot t = ln_slot<LPR>();
    float4 gm[V], bt[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int c = v * LPR + t.l;
        gm[v] = c < w4 ? gamma[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        bt[v] = c < w4 ? beta[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int it = 0; it < iters; ++it) {                 // (uniform trip count: every lane takes part in the butterflies)
        const int64_t row = ((int64_t)it * gridDim.x + blockIdx.x) * RPB + t.slot;
        const bool live = row < rows;
        float4 zv[V];
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = v * LPR + t.l;
            zv[v] = (live && c < w4) ? z[row * w4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
            s = v == 0 ? quad_sum(zv[v]) : s + quad_sum(zv[v]);
        }
        const float mean = row_sum<LPR>(s) / width_f;
        float ss = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = v * LPR + t.l;
            float4 d = make_float4(zv[v].x - mean, zv[v].y - mean, zv[v].z - mean, zv[v].w - mean);
            if (!(c < w4)) d = make_float4(0.f, 0.f, 0.f, 0.f);
            zv[v] = d;
            const float4 q = make_float4(d.x * d.x, d.y * d.y, d.z * d.z, d.w * d.w);
            ss = v == 0 ? quad_sum(q) : ss + quad_sum(q);
        }
        const float var = row_sum<LPR>(ss) / width_f;
        const float rstd = 1.f / sqrtf(var + eps);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = v * LPR + t.l;
            if (live && c < w4) {
                const float4 d = zv[v];
                float4 o;
                o.x = fmaxf(0.f, gm[v].x * (d.x * rstd) + bt[v].x);
                o.y = fmaxf(0.f, gm[v].y * (d.y * rstd) + bt[v].y);
                o.z = fmaxf(0.f, gm[v].z * (d.z * rstd) + bt[v].z);
                o.w = fmaxf(0.f, gm[v].w * (d.w * rstd) + bt[v].w);
                y[row * w4 + c] = o;
            }
        }
        if (live && t.l == 0) stats[row] = make_float2(mean, rstd);
    }
}

// MASKED: dy comes multiplied by the rectifier mask (masked-out entries +0): y is not read
template <int LPR, int V, bool MASKED>
__global__ __launch_bounds__(LN_THREADS) void ln_relu_bwd_kernel(const float4* dy,
                                                                 const float4* __restrict__ y,
                                                                 const float4* __restrict__ z,
                                                                 const float2* __restrict__ stats,
                                                                 const float4* __restrict__ gamma, int64_t rows, int w4,
                                                                 float width_f, int iters, float4* dz,      // (dz may be dy)
                                                                 float4* __restrict__ part_g, float4* __restrict__ part_b) {
    constexpr int RPB = LN_THREADS / LPR;
    __shared__ float4 lds[2][V][LN_THREADS];
    const LnSlot t = ln_slot<LPR>();
    float4 gm[V], acc_g[V], acc_b[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int c = v * LPR + t.l;
        gm[v] = c < w4 ? gamma[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        acc_g[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        acc_b[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int it = 0; it < iters; ++it) {
        const int64_t row = ((int64_t)it * gridDim.x + blockIdx.x) * RPB + t.slot;
        const bool live = row < rows;
        const float2 st = live ? stats[row] : make_float2(0.f, 0.f);
        const float mean = st.x, rstd = st.y;
        float4 h[V], xh[V];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = v * LPR + t.l;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f), x = g;
            if (live && c < w4) {
                const int64_t i = row * w4 + c;
                g = dy[i];
                const float4 zz = z[i];
                if (!MASKED) {
                    const float4 a = y[i];
                    g.x = a.x > 0.f ? g.x : 0.f; g.y = a.y > 0.f ? g.y : 0.f;
                    g.z = a.z > 0.f ? g.z : 0.f; g.w = a.w > 0.f ? g.w : 0.f;
                }
                x = make_float4((zz.x - mean) * rstd, (zz.y - mean) * rstd, (zz.z - mean) * rstd, (zz.w - mean) * rstd);
                acc_g[v].x += g.x * x.x; acc_g[v].y += g.y * x.y; acc_g[v].z += g.z * x.z; acc_g[v].w += g.w * x.w;
                acc_b[v].x += g.x; acc_b[v].y += g.y; acc_b[v].z += g.z; acc_b[v].w += g.w;
            }
            xh[v] = x;
            h[v] = make_float4(g.x * gm[v].x, g.y * gm[v].y, g.z * gm[v].z, g.w * gm[v].w);
            const float4 p = make_float4(h[v].x * x.x, h[v].y * x.y, h[v].z * x.z, h[v].w * x.w);
            s1 = v == 0 ? quad_sum(h[v]) : s1 + quad_sum(h[v]);
            s2 = v == 0 ? quad_sum(p) : s2 + quad_sum(p);
        }
        const float m1 = row_sum<LPR>(s1) / width_f;
        const float m2 = row_sum<LPR>(s2) / width_f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = v * LPR + t.l;
            if (live && c < w4) {
                float4 o;
                o.x = rstd * ((h[v].x - m1) - xh[v].x * m2);
                o.y = rstd * ((h[v].y - m1) - xh[v].y * m2);
                o.z = rstd * ((h[v].z - m1) - xh[v].z * m2);
                o.w = rstd * ((h[v].w - m1) - xh[v].w * m2);
                dz[row * w4 + c] = o;
            }
        }
    }
    // the block's RPB row slots -> one partial row, slot 0 first
#pragma unroll
    for (int v = 0; v < V; ++v) {
        lds[0][v][threadIdx.x] = acc_g[v];
        lds[1][v][threadIdx.x] = acc_b[v];
    }
    __syncthreads();
    if (t.slot == 0) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = v * LPR + t.l;
            if (c < w4) {
                float4 sg = lds[0][v][t.l], sb = lds[1][v][t.l];
                for (int k = 1; k < RPB; ++k) {
                    const float4 a = lds[0][v][k * LPR + t.l], b = lds[1][v][k * LPR + t.l];
                    sg.x += a.x; sg.y += a.y; sg.z += a.z; sg.w += a.w;
                    sb.x += b.x; sb.y += b.y; sb.z += b.z; sb.w += b.w;
                }
                part_g[(int64_t)blockIdx.x * w4 + c] = sg;
                part_b[(int64_t)blockIdx.x * w4 + c] = sb;
            }
        }
    }
}

struct LnShape { int lpr, v, grid, iters; };
LnShape ln_shape(int64_t rows, int width, int max_grid) {
    LnShape s;
    s.lpr = width <= 32 ? 8 : width <= 64 ? 16 : 64;
    s.v = width <= 256 ? 1 : width <= 512 ? 2 : 4;
    const int rpb = LN_THREADS / s.lpr;
    const int64_t blocks = (rows + rpb - 1) / rpb;
    s.grid = (int)(blocks < max_grid ? blocks : max_grid);
    s.iters = (int)((blocks + s.grid - 1) / s.grid);
    return s;
}

int check_ln(int64_t rows, int32_t width) {
    if (rows < 1 || rows > INT32_MAX || width < 4 || width > LN_MAX_WIDTH || (width & 3)) {
        arl::set_error("layernorm: need 1 <= rows <= 2^31 - 1 and width a multiple of 4 in 4 .. 1024");
        return ARL_E_RANGE;
    }
    return 0;
}

// KERNEL(LPR, V): the instantiation's name
#define ARL_LN_DISPATCH(KERNEL, shape, ...)                                                                   \
    do {                                                                                                      \
        const dim3 g_((unsigned)(shape).grid), b_(LN_THREADS);                                                \
        if ((shape).lpr == 8) hipLaunchKernelGGL((KERNEL(8, 1)), g_, b_, 0, s, __VA_ARGS__);                  \
        else if ((shape).lpr == 16) hipLaunchKernelGGL((KERNEL(16, 1)), g_, b_, 0, s, __VA_ARGS__);           \
        else if ((shape).v == 1) hipLaunchKernelGGL((KERNEL(64, 1)), g_, b_, 0, s, __VA_ARGS__);              \
        else if ((shape).v == 2) hipLaunchKernelGGL((KERNEL(64, 2)), g_, b_, 0, s, __VA_ARGS__);              \
        else hipLaunchKernelGGL((KERNEL(64, 4)), g_, b_, 0, s, __VA_ARGS__);                                  \
    } while (0)
#define ARL_LN_FWD(L_, V_) ln_relu_fwd_kernel<L_, V_>
#define ARL_LN_BWD(L_, V_) ln_relu_bwd_kernel<L_, V_, false>
#define ARL_LN_BWD_MASKED(L_, V_) ln_relu_bwd_kernel<L_, V_, true>

}  // namespace

extern "C" int64_t arl_ln_bwd_workspace_bytes(void) { return (int64_t)2 * LN_MAX_GRID * LN_MAX_WIDTH * sizeof(float); }

extern "C" int arl_ln_relu_fwd(const float* z, const float* gamma, const float* beta, int64_t rows, int32_t width,
                               float eps, float* y, float* stats, void* stream) {
    ARL_REQUIRE(z && gamma && beta && y && stats, ARL_E_ARG, "null pointer");
    int rc = check_ln(rows, width);
    if (rc) return rc;
    ARL_REQUIRE(eps > 0.f && eps <= 3.0e38f, ARL_E_ARG, "eps must be finite and > 0");
    ARL_REQUIRE(y != z, ARL_E_ARG, "y must not be z (z is kept for the backward pass)");
    ARL_REQUIRE(arl::aligned16(z) && arl::aligned16(gamma) && arl::aligned16(beta) && arl::aligned16(y) &&
                arl::aligned16(stats), ARL_E_ALIGN, "16-byte alignment");
    const LnShape sh = ln_shape(rows, width, LN_FWD_MAX_GRID);
    hipStream_t s = (hipStream_t)stream;
    ARL_LN_DISPATCH(ARL_LN_FWD, sh, (const float4*)z, (const float4*)gamma, (const float4*)beta, rows,
                    (int)(width >> 2), (float)width, eps, sh.iters, (float4*)y, (float2*)stats);
    return arl::check_launch("ln_relu_fwd_kernel");
}

extern "C" int arl_ln_relu_bwd(const float* dy, const float* y, const float* z, const float* stats, const float* gamma,
                               int64_t rows, int32_t width, int32_t dy_masked, float* dz, float* dgamma, float* dbeta,
                               void* workspace, arl_fold_item* items2_or_null, void* stream) {
    ARL_REQUIRE(dy && y && z && stats && gamma && dz && dgamma && dbeta && workspace, ARL_E_ARG, "null pointer");
    int rc = check_ln(rows, width);
    if (rc) return rc;
    ARL_REQUIRE(dy_masked == 0 || dy_masked == 1, ARL_E_ARG, "dy_masked must be 0 or 1");
    ARL_REQUIRE(arl::aligned16(dy) && arl::aligned16(y) && arl::aligned16(z) && arl::aligned16(stats) &&
                arl::aligned16(gamma) && arl::aligned16(dz) && arl::aligned16(dgamma) && arl::aligned16(dbeta) &&
                arl::aligned16(workspace), ARL_E_ALIGN, "16-byte alignment");
    const LnShape sh = ln_shape(rows, width, LN_MAX_GRID);
    float* part_g = (float*)workspace;
    float* part_b = part_g + (int64_t)sh.grid * width;
    hipStream_t s = (hipStream_t)stream;
    if (dy_masked)          // dy is taken as it comes and y is not read: a quarter of the kernel's reads less
        ARL_LN_DISPATCH(ARL_LN_BWD_MASKED, sh, (const float4*)dy, (const float4*)y, (const float4*)z, (const float2*)stats,
                        (const float4*)gamma, rows, (int)(width >> 2), (float)width, sh.iters, (float4*)dz,
                        (float4*)part_g, (float4*)part_b);
    else
        ARL_LN_DISPATCH(ARL_LN_BWD, sh, (const float4*)dy, (const float4*)y, (const float4*)z, (const float2*)stats,
                        (const float4*)gamma, rows, (int)(width >> 2), (float)width, sh.iters, (float4*)dz,
                        (float4*)part_g, (float4*)part_b);
    rc = arl::check_launch("ln_relu_bwd_kernel");
    arl_fold_item local[2];
    arl_fold_item* it = items2_or_null ? items2_or_null : local;
    it[0].part = part_g; it[0].out = dgamma; it[0].total = width; it[0].splits = sh.grid; it[0].valid = 0;
    it[1].part = part_b; it[1].out = dbeta; it[1].total = width; it[1].splits = sh.grid; it[1].valid = 0;
    if (rc || items2_or_null) return rc;
    return arl_fold_many(local, 2, stream);
}
