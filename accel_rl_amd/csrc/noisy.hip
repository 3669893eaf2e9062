// Noisy dense layers (NoisyNets, factorized Gaussian noise) for gfx950: everything noise-specific of
// AtariNoisyNetDqnPolicy (policies/dqn/layers/noisy_layer.py:15-147 of the reference).  The four matrix products of a layer
// (x W, (x f(e_in)) W_sigma and their gradients) run on the MFMA entry points of mfma_conv.hip; this file holds what sits
// between them:
//
//   arl_noisy_normals       the generator, one layer's e_in or e_out into caller buffers (tests, tools)
//   arl_noisy_noise         the noise of every noisy layer of one forward pass in one launch: f(e_in), f(e_out), and
//                           x * f(e_in) for the layer whose input already exists
//   arl_noisy_dense_combine y = [x W + b] + f(e_out) * ([xs W_sigma + b_sigma]) (+ relu), folding both products' split
//                           partial sums itself; writes the next layer's h * f(e_in); may advance the pass counter
//   arl_noisy_dense_bwd_prep g2 = g * f(e_out), db = sum_rows g, db_sigma = sum_rows g2 (fixed order, no atomics)
//   arl_noisy_dense_bwd_dx  dx = dx_w + f(e_in) * dx_sigma (both already masked by the rectifier of the layer below)
//
// For AtariNoisyNetCatDqnPolicy (dueling: the two streams' hidden layers stacked into one 2H layer, each with its own e_in):
//   arl_noisy_draws         a pass's noise as a list of (layer, which) draws, each into a column range of a wider buffer
//   arl_noisy_duel_combine  arl_noisy_dense_combine with one sigma product per stream, each folded into its own columns
//   arl_noisy_duel_bwd_prep arl_noisy_dense_bwd_prep writing g2 as two contiguous per-stream blocks
//   arl_noisy_duel_bwd_dx   dx = dx_w + f(e_in_lo) * dx_sigma_lo + f(e_in_hi) * dx_sigma_hi
//
// Generator (stated exactly in include/accel_rl_hip.h): Philox4x32-10, key (seed, 2 layer + which), counter
// (element / 4, row group, call counter lo, call counter hi); Box-Muller in double on the words' top 24 bits.
// fp32 elsewhere, compiled with -ffp-contract=off.

#include "arl_common.h"
#include "philox_dev.h"

namespace arlc {
int fold_wide_from();           // mfma_conv.hip: the split count from which a fold sums 64-way (fold_slot)
}

namespace {

using arlp::philox4x32_10;           // philox_dev.h (shared with csrc/iqn.hip)

// the four normals of block q (elements 4q .. 4q + 3) of one (layer, which, row group, call) stream
__device__ __forceinline__ void normals4(uint64_t seed, uint64_t counter, int stream_id, uint32_t group, uint32_t q,
                                         float e[4], uint32_t w[4]) {
    w[0] = q; w[1] = group; w[2] = (uint32_t)counter; w[3] = (uint32_t)(counter >> 32);
    philox4x32_10(w, (uint32_t)seed, (uint32_t)stream_id);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const double u1 = ((double)(w[2 * p] >> 8) + 0.5) * (1.0 / 16777216.0);
        const double u2 = ((double)(w[2 * p + 1] >> 8) + 0.5) * (1.0 / 16777216.0);
        const double r = sqrt(-2.0 * log(u1));
        double s, c;
        sincospi(2.0 * u2, &s, &c);
        e[2 * p] = (float)(r * c);
        e[2 * p + 1] = (float)(r * s);
    }
}

__device__ __forceinline__ float fsgn_sqrt(float e) {     // f(e) = sgn(e) sqrt(|e|)   (noisy_layer.py:10-11)
    const float r = sqrtf(fabsf(e));
    return e > 0.f ? r : (e < 0.f ? -r : 0.f);
}

__global__ __launch_bounds__(256) void normals_kernel(uint64_t seed, uint64_t counter, int stream_id, int64_t rows,
                                                      int width, int rows_per_draw, float* __restrict__ e_out,
                                                      float* __restrict__ f_out, uint32_t* __restrict__ words) {
    const int nq = (width + 3) / 4;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * nq) return;
    const int64_t r = t / nq;
    const int q = (int)(t - r * nq);
    float e[4];
    uint32_t w[4];
    normals4(seed, counter, stream_id, (uint32_t)(r / rows_per_draw), (uint32_t)q, e, w);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int j = 4 * q + l;
        if (j >= width) break;
        const int64_t o = r * width + j;
        if (e_out) e_out[o] = e[l];
        if (f_out) f_out[o] = fsgn_sqrt(e[l]);
        if (words) words[o] = w[l];
    }
}

// ---- one forward pass's noise: segment s = (layer, which) covers rows x (stride / 4) blocks of 4 elements
struct NoiseSeg {
    float* f;               // f32[rows][stride]
    const float* x;         // which == 0: the layer input or null
    float* xs;              // which == 0: x * f(e_in)
    int width, stride, pitch, stream_id;   // stride: elements written per row (zeros from width on); pitch: row pitch
    int64_t block0;         // first thread of this segment
};
struct NoiseArgs {
    NoiseSeg seg[ARL_NOISY_MAX_DRAWS];
    int n_seg, rows_per_draw;
    int64_t rows, total;
    const int64_t* state;
};

__global__ __launch_bounds__(256) void noise_kernel(const NoiseArgs a) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.total) return;
    int s = 0;
    while (s + 1 < a.n_seg && t >= a.seg[s + 1].block0) ++s;
    const NoiseSeg& g = a.seg[s];
    const int nq = g.stride >> 2;
    const int64_t u = t - g.block0;
    const int64_t r = u / nq;
    const int q = (int)(u - r * nq);
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (4 * q < g.width) {
        float e[4];
        uint32_t w[4];
        normals4((uint64_t)a.state[0], (uint64_t)a.state[1], g.stream_id, (uint32_t)(r / a.rows_per_draw), (uint32_t)q,
                 e, w);
#pragma unroll
        for (int l = 0; l < 4; ++l) f[l] = 4 * q + l < g.width ? fsgn_sqrt(e[l]) : 0.f;
    }
    const int64_t o = r * g.pitch + 4 * q;
    *reinterpret_cast<float4*>(g.f + o) = make_float4(f[0], f[1], f[2], f[3]);
    if (g.x) {
        const float4 xv = *reinterpret_cast<const float4*>(g.x + o);
        *reinterpret_cast<float4*>(g.xs + o) = make_float4(xv.x * f[0], xv.y * f[1], xv.z * f[2], xv.w * f[3]);
    }
}

// fold_splits_kernel's sum of element i (mfma_conv.hip: zgn groups, group k sums splits k, k + zgn, ...; then
// s_0 + s_1 + ... + s_{zgn-1}), operation for operation, then the bias
__device__ __forceinline__ float folded(const arl_fold_item& it, int zgn, int64_t i, const float* bias, int u) {
    if (it.splits <= 0) return it.part[i];          // finished (bias applied by the product's own launch)
    float s = 0.f;
    for (int k = 0; k < zgn; ++k) {
        float sk = 0.f;
        for (int z = k; z < it.splits; z += zgn) sk += it.part[(int64_t)z * it.total + i];
        s = k == 0 ? sk : s + sk;
    }
    if (bias) s += bias[u];
    return s;
}

__global__ __launch_bounds__(256) void combine_kernel(const arl_fold_item pw, const arl_fold_item ps, int zgn_w,
                                                      int zgn_s, const float* __restrict__ bias,
                                                      const float* __restrict__ b_sigma, const float* __restrict__ feout,
                                                      int64_t rows, int units, int relu, float* __restrict__ y,
                                                      const float* __restrict__ fein_next, float* __restrict__ xs_next,
                                                      int64_t* state_advance) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (state_advance && i == 0) state_advance[1] += 1;     // read only by this pass's noise launch, which has run
    if (i >= rows * units) return;
    const int u = (int)(i % units);
    const float a = folded(pw, zgn_w, i, bias, u);
    const float s = folded(ps, zgn_s, i, b_sigma, u);
    float v = a + feout[i] * s;
    if (relu) v = fmaxf(v, 0.f);
    y[i] = v;
    if (xs_next) xs_next[i] = v * fein_next[i];
}

__global__ __launch_bounds__(256) void bwd_prep_kernel(const float* __restrict__ g, const float* __restrict__ feout,
                                                       int64_t rows, int units, float* __restrict__ g2,
                                                       float* __restrict__ db, float* __restrict__ db_sigma) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= units) return;
    float s = 0.f, s2 = 0.f;
    for (int64_t r = 0; r < rows; ++r) {                     // rows in order: a fixed summation order
        const float gv = g[r * units + u];
        const float g2v = gv * feout[r * units + u];
        g2[r * units + u] = g2v;
        s += gv;
        s2 += g2v;
    }
    db[u] = s;
    db_sigma[u] = s2;
}

__global__ __launch_bounds__(256) void bwd_dx_kernel(const float4* __restrict__ dx_w, const float4* __restrict__ dx_s,
                                                     const float4* __restrict__ fein, int64_t n4, float4* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 a = dx_w[i], s = dx_s[i], f = fein[i];
    dx[i] = make_float4(a.x + f.x * s.x, a.y + f.y * s.y, a.z + f.z * s.z, a.w + f.w * s.w);
}

// The stacked 2H hidden layer of a dueling network (units 0 .. split-1 advantage stream, split .. units-1 value stream):
// one W product over all units, one sigma product per stream (its own x * f(e_in)), each folded into its own columns.
__global__ __launch_bounds__(256) void duel_combine_kernel(const arl_fold_item pw, const arl_fold_item ps_lo,
                                                           const arl_fold_item ps_hi, int zgn_w, int zgn_lo, int zgn_hi,
                                                           const float* __restrict__ bias,
                                                           const float* __restrict__ b_sigma,
                                                           const float* __restrict__ feout, int64_t rows, int units,
                                                           int split, int relu, float* __restrict__ y,
                                                           const float* __restrict__ fein_next,
                                                           float* __restrict__ xs_next, int64_t* state_advance) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (state_advance && i == 0) state_advance[1] += 1;     // read only by this pass's noise launch, which has run
    if (i >= rows * units) return;
    const int64_t r = i / units;
    const int u = (int)(i - r * units);
    const float a = folded(pw, zgn_w, i, bias, u);
    const float s = u < split ? folded(ps_lo, zgn_lo, r * split + u, b_sigma, u)
                              : folded(ps_hi, zgn_hi, r * (units - split) + (u - split), b_sigma, u);
    float v = a + feout[i] * s;
    if (relu) v = fmaxf(v, 0.f);
    y[i] = v;
    if (xs_next) xs_next[i] = v * fein_next[i];
}

__global__ __launch_bounds__(256) void duel_bwd_prep_kernel(const float* __restrict__ g, const float* __restrict__ feout,
                                                            int64_t rows, int units, int split, float* __restrict__ g2_lo,
                                                            float* __restrict__ g2_hi, float* __restrict__ db,
                                                            float* __restrict__ db_sigma) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= units) return;
    const bool lo = u < split;
    const int w2 = lo ? split : units - split, c = lo ? u : u - split;
    float* g2 = lo ? g2_lo : g2_hi;
    float s = 0.f, s2 = 0.f;
    for (int64_t r = 0; r < rows; ++r) {                     // rows in order, as bwd_prep_kernel
        const float gv = g[r * units + u];
        const float g2v = gv * feout[r * units + u];
        g2[r * w2 + c] = g2v;
        s += gv;
        s2 += g2v;
    }
    db[u] = s;
    db_sigma[u] = s2;
}

__global__ __launch_bounds__(256) void duel_bwd_dx_kernel(const float4* __restrict__ dx_w, const float4* __restrict__ s0,
                                                          const float4* __restrict__ f0, const float4* __restrict__ s1,
                                                          const float4* __restrict__ f1, int64_t n4,
                                                          float4* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 a = dx_w[i], p = s0[i], e = f0[i], q = s1[i], h = f1[i];
    dx[i] = make_float4((a.x + e.x * p.x) + h.x * q.x, (a.y + e.y * p.y) + h.y * q.y, (a.z + e.z * p.z) + h.z * q.z,
                        (a.w + e.w * p.w) + h.w * q.w);
}

inline unsigned grid_for(int64_t n) { return (unsigned)((n + 255) / 256); }

bool fold_item_ok(const arl_fold_item* it, int64_t total) {
    return it && it->part && it->splits >= 0 && it->splits <= 4096 && (it->splits == 0 || it->total == total);
}

}  // namespace

extern "C" int arl_noisy_normals(int64_t seed, int64_t counter, int32_t layer, int32_t which, int64_t rows,
                                 int32_t width, int32_t rows_per_draw, float* e_or_null, float* f_or_null,
                                 uint32_t* words_or_null, void* stream) {
    ARL_REQUIRE(e_or_null || f_or_null || words_or_null, ARL_E_ARG, "null pointer: no output buffer");
    ARL_REQUIRE(rows > 0 && width > 0 && rows_per_draw > 0, ARL_E_ARG, "non-positive size");
    ARL_REQUIRE(layer >= 0 && layer < (1 << 30) && (which == 0 || which == 1), ARL_E_ARG, "layer < 0 or which not 0 / 1");
    ARL_REQUIRE(rows <= ((int64_t)1 << 40) / width, ARL_E_RANGE, "rows x width too large");
    const int64_t n = rows * ((width + 3) / 4);
    hipLaunchKernelGGL(normals_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (uint64_t)seed,
                       (uint64_t)counter, 2 * layer + which, rows, width, rows_per_draw, e_or_null, f_or_null,
                       words_or_null);
    return arl::check_launch("normals_kernel");
}

extern "C" int arl_noisy_noise(const int64_t* state, const arl_noisy_layer* layers, int32_t n_layers, int64_t rows,
                               int32_t rows_per_draw, void* stream) {
    ARL_REQUIRE(state && layers, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n_layers > 0 && rows > 0 && rows_per_draw > 0, ARL_E_ARG, "non-positive size");
    ARL_REQUIRE(n_layers <= ARL_NOISY_MAX_LAYERS, ARL_E_RANGE, "more than ARL_NOISY_MAX_LAYERS layers");
    NoiseArgs a = {};
    int64_t total = 0;
    for (int l = 0; l < n_layers; ++l) {
        const arl_noisy_layer& L = layers[l];
        ARL_REQUIRE(L.fein && L.feout && (!L.x || L.xs), ARL_E_ARG, "null pointer in a layer");
        ARL_REQUIRE(L.fan_in > 0 && L.units > 0 && L.out_stride >= L.units && L.layer >= 0 && L.layer < (1 << 30),
                    ARL_E_ARG, "layer sizes / layer index");
        ARL_REQUIRE(L.fan_in % 4 == 0 && L.out_stride % 4 == 0, ARL_E_RANGE, "fan_in / out_stride not multiples of 4");
        ARL_REQUIRE(arl::aligned16(L.fein) && arl::aligned16(L.feout) && (!L.x || (arl::aligned16(L.x) &&
                    arl::aligned16(L.xs))), ARL_E_ALIGN, "16-byte alignment");
        ARL_REQUIRE(rows <= ((int64_t)1 << 40) / L.fan_in && rows <= ((int64_t)1 << 40) / L.out_stride, ARL_E_RANGE,
                    "rows x fan_in / out_stride too large");
        for (int which = 0; which < 2; ++which) {
            NoiseSeg& g = a.seg[a.n_seg++];
            g.f = which ? L.feout : L.fein;
            g.x = which ? nullptr : L.x;
            g.xs = which ? nullptr : L.xs;
            g.width = which ? L.units : L.fan_in;
            g.stride = g.pitch = which ? L.out_stride : L.fan_in;
            g.stream_id = 2 * L.layer + which;
            g.block0 = total;
            total += rows * (g.stride / 4);
        }
    }
    a.rows = rows; a.rows_per_draw = rows_per_draw; a.total = total; a.state = state;
    hipLaunchKernelGGL(noise_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("noise_kernel");
}

extern "C" int arl_noisy_dense_combine(const arl_fold_item* w_prod, const float* bias_or_null,
                                       const arl_fold_item* sigma_prod, const float* b_sigma_or_null,
                                       const float* feout, int64_t rows, int32_t units, int32_t relu, float* y,
                                       const float* fein_next_or_null, float* xs_next_or_null,
                                       int64_t* state_or_null, void* stream) {
    ARL_REQUIRE(w_prod && sigma_prod && feout && y, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(rows > 0 && units > 0, ARL_E_ARG, "non-positive size");
    ARL_REQUIRE(!fein_next_or_null == !xs_next_or_null, ARL_E_ARG, "fein_next and xs_next: both or neither");
    ARL_REQUIRE(fold_item_ok(w_prod, rows * units) && fold_item_ok(sigma_prod, rows * units), ARL_E_ARG,
                "fold items: null part or total != rows x units");
    const int wide = arlc::fold_wide_from();
    const int zw = w_prod->splits >= wide ? 64 : 16, zs = sigma_prod->splits >= wide ? 64 : 16;
    hipLaunchKernelGGL(combine_kernel, dim3(grid_for(rows * units)), dim3(256), 0, (hipStream_t)stream, *w_prod,
                       *sigma_prod, zw, zs, bias_or_null, b_sigma_or_null, feout, rows, units, relu, y,
                       fein_next_or_null, xs_next_or_null, state_or_null);
    return arl::check_launch("combine_kernel");
}

extern "C" int arl_noisy_dense_bwd_prep(const float* g, const float* feout, int64_t rows, int32_t units, float* g2,
                                        float* db, float* db_sigma, void* stream) {
    ARL_REQUIRE(g && feout && g2 && db && db_sigma, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(rows > 0 && units > 0, ARL_E_ARG, "non-positive size");
    hipLaunchKernelGGL(bwd_prep_kernel, dim3(grid_for(units)), dim3(256), 0, (hipStream_t)stream, g, feout, rows, units,
                       g2, db, db_sigma);
    return arl::check_launch("bwd_prep_kernel");
}

extern "C" int arl_noisy_dense_bwd_dx(const float* dx_w, const float* dx_sigma, const float* fein, int64_t rows,
                                      int32_t fan_in, float* dx, void* stream) {
    ARL_REQUIRE(dx_w && dx_sigma && fein && dx, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(rows > 0 && fan_in > 0, ARL_E_ARG, "non-positive size");
    ARL_REQUIRE(fan_in % 4 == 0, ARL_E_RANGE, "fan_in not a multiple of 4");
    ARL_REQUIRE(arl::aligned16(dx_w) && arl::aligned16(dx_sigma) && arl::aligned16(fein) && arl::aligned16(dx),
                ARL_E_ALIGN, "16-byte alignment");
    const int64_t n4 = rows * fan_in / 4;
    hipLaunchKernelGGL(bwd_dx_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, (const float4*)dx_w,
                       (const float4*)dx_sigma, (const float4*)fein, n4, (float4*)dx);
    return arl::check_launch("bwd_dx_kernel");
}

extern "C" int arl_noisy_draws(const int64_t* state, const arl_noisy_draw* draws, int32_t n_draws, int64_t rows,
                               int32_t rows_per_draw, void* stream) {
    ARL_REQUIRE(state && draws, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n_draws > 0 && rows > 0 && rows_per_draw > 0, ARL_E_ARG, "non-positive size");
    ARL_REQUIRE(n_draws <= ARL_NOISY_MAX_DRAWS, ARL_E_RANGE, "more than ARL_NOISY_MAX_DRAWS draws");
    NoiseArgs a = {};
    int64_t total = 0;
    for (int d = 0; d < n_draws; ++d) {
        const arl_noisy_draw& D = draws[d];
        ARL_REQUIRE(D.f && (!D.x || D.xs) && (!D.x || D.which == 0), ARL_E_ARG,
                    "null pointer in a draw (or x given for an e_out draw)");
        ARL_REQUIRE(D.width > 0 && D.pitch >= D.width && D.layer >= 0 && D.layer < (1 << 30) &&
                    (D.which == 0 || D.which == 1), ARL_E_ARG, "draw sizes / layer / which");
        ARL_REQUIRE(D.width % 4 == 0 && D.pitch % 4 == 0, ARL_E_RANGE, "width / pitch not multiples of 4");
        ARL_REQUIRE(arl::aligned16(D.f) && (!D.x || (arl::aligned16(D.x) && arl::aligned16(D.xs))), ARL_E_ALIGN,
                    "16-byte alignment");
        ARL_REQUIRE(rows <= ((int64_t)1 << 40) / D.pitch, ARL_E_RANGE, "rows x pitch too large");
        NoiseSeg& g = a.seg[a.n_seg++];
        g.f = D.f; g.x = D.x; g.xs = D.xs;
        g.width = g.stride = D.width;
        g.pitch = D.pitch;
        g.stream_id = 2 * D.layer + D.which;
        g.block0 = total;
        total += rows * (D.width / 4);
    }
    a.rows = rows; a.rows_per_draw = rows_per_draw; a.total = total; a.state = state;
    hipLaunchKernelGGL(noise_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("noise_kernel (draws)");
}

extern "C" int arl_noisy_duel_combine(const arl_fold_item* w_prod, const float* bias_or_null,
                                      const arl_fold_item* sigma_lo, const arl_fold_item* sigma_hi,
                                      const float* b_sigma_or_null, const float* feout, int64_t rows, int32_t units,
                                      int32_t split, int32_t relu, float* y, const float* fein_next_or_null,
                                      float* xs_next_or_null, int64_t* state_or_null, void* stream) {
    ARL_REQUIRE(w_prod && sigma_lo && sigma_hi && feout && y, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(rows > 0 && units > 0 && split > 0 && split < units, ARL_E_ARG, "non-positive size or split not in (0, units)");
    ARL_REQUIRE(!fein_next_or_null == !xs_next_or_null, ARL_E_ARG, "fein_next and xs_next: both or neither");
    ARL_REQUIRE(fold_item_ok(w_prod, rows * units) && fold_item_ok(sigma_lo, rows * split) &&
                fold_item_ok(sigma_hi, rows * (units - split)), ARL_E_ARG,
                "fold items: null part or total != rows x (units, split, units - split)");
    const int wide = arlc::fold_wide_from();
    const int zw = w_prod->splits >= wide ? 64 : 16, zl = sigma_lo->splits >= wide ? 64 : 16,
              zh = sigma_hi->splits >= wide ? 64 : 16;
    hipLaunchKernelGGL(duel_combine_kernel, dim3(grid_for(rows * units)), dim3(256), 0, (hipStream_t)stream, *w_prod,
                       *sigma_lo, *sigma_hi, zw, zl, zh, bias_or_null, b_sigma_or_null, feout, rows, units, split, relu,
                       y, fein_next_or_null, xs_next_or_null, state_or_null);
    return arl::check_launch("duel_combine_kernel");
}

extern "C" int arl_noisy_duel_bwd_prep(const float* g, const float* feout, int64_t rows, int32_t units, int32_t split,
                                       float* g2_lo, float* g2_hi, float* db, float* db_sigma, void* stream) {
    ARL_REQUIRE(g && feout && g2_lo && g2_hi && db && db_sigma, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(rows > 0 && units > 0 && split > 0 && split < units, ARL_E_ARG, "non-positive size or split not in (0, units)");
    hipLaunchKernelGGL(duel_bwd_prep_kernel, dim3(grid_for(units)), dim3(256), 0, (hipStream_t)stream, g, feout, rows,
                       units, split, g2_lo, g2_hi, db, db_sigma);
    return arl::check_launch("duel_bwd_prep_kernel");
}

extern "C" int arl_noisy_duel_bwd_dx(const float* dx_w, const float* dx_sigma_lo, const float* fein_lo,
                                     const float* dx_sigma_hi, const float* fein_hi, int64_t rows, int32_t fan_in,
                                     float* dx, void* stream) {
    ARL_REQUIRE(dx_w && dx_sigma_lo && fein_lo && dx_sigma_hi && fein_hi && dx, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(rows > 0 && fan_in > 0, ARL_E_ARG, "non-positive size");
    ARL_REQUIRE(fan_in % 4 == 0, ARL_E_RANGE, "fan_in not a multiple of 4");
    ARL_REQUIRE(arl::aligned16(dx_w) && arl::aligned16(dx_sigma_lo) && arl::aligned16(fein_lo) &&
                arl::aligned16(dx_sigma_hi) && arl::aligned16(fein_hi) && arl::aligned16(dx), ARL_E_ALIGN,
                "16-byte alignment");
    const int64_t n4 = rows * fan_in / 4;
    hipLaunchKernelGGL(duel_bwd_dx_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, (const float4*)dx_w,
                       (const float4*)dx_sigma_lo, (const float4*)fein_lo, (const float4*)dx_sigma_hi,
                       (const float4*)fein_hi, n4, (float4*)dx);
    return arl::check_launch("duel_bwd_dx_kernel");
}
