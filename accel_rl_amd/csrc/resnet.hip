// What the IMPALA residual network (Espeholt et al. 2018; the reference has none) needs between the contraction launches:
//
//   arl_maxpool3s2_fwd   3 x 3 / stride 2 / pad 1 max pooling of an NHWC activation; also writes max(y, 0) (the input of
//                        the next convolution and its rectifier mask) and the window position of every maximum
//   arl_maxpool3s2_bwd   its backward pass as a gather over the input elements (no atomics)
//   arl_add_relu         sum = a + b [, relu = max(sum, 0)]: the residual sum forward, g + dx backward
//   arl_gather_scale_obs_nhwc_any   the scaled f32 NHWC input of a first convolution from u8 NCHW observations of any
//                        plane size and channel count (arl_gather_scale_obs_nhwc takes four planes of a multiple of
//                        16 bytes: every Atari frame; this one the rest, a byte per load)
//
// All are streaming kernels on float32: one float4 (four consecutive channels) per thread and step of a grid-stride
// walk, 64-bit indexing, plain vector stores, no LDS, no atomics; every output element is a function of the inputs alone
// (no partial sums, nothing depends on the grid), so two launches give the same bits.  The order of every comparison
// and addition is stated in include/accel_rl_hip.h.
#include "arl_common.h"

#include <math.h>

namespace {

constexpr int RN_THREADS = 256;
constexpr int RN_MAX_CHANNELS = 1024, RN_MAX_SIDE = 1 << 16, RN_MAX_BATCH = 1 << 20;

// t = q * d + r; the 32-bit division where t fits (it does for every shape of the networks here)
__device__ __forceinline__ void split_index(int64_t t, int d, int64_t& q, int& r) {
    if ((uint64_t)t <= 0xffffffffull) {
        const uint32_t tt = (uint32_t)t, dd = (uint32_t)d;
        q = (int64_t)(tt / dd);
        r = (int)(tt % dd);
    } else {
        q = t / d;
        r = (int)(t % d);
    }
}

__device__ __forceinline__ float relu1(float v) { return v > 0.f ? v : 0.f; }
__device__ __forceinline__ float4 relu4(const float4 v) { return make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)); }

__device__ __forceinline__ void take_max(float v, int pos, float& best, int& arg) {
    if (v > best) {                 // strict: the first maximum in row-major window order keeps its place
        best = v;
        arg = pos;
    }
}

__global__ __launch_bounds__(RN_THREADS) void maxpool3s2_fwd_kernel(const float4* __restrict__ z, int in_h, int in_w,
                                                                    int out_h, int out_w, int c4, int64_t total,
                                                                    float4* __restrict__ y, float4* __restrict__ y_relu,
                                                                    uint32_t* __restrict__ arg) {
    const int64_t step = (int64_t)gridDim.x * RN_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x; t < total; t += step) {
        int64_t p, q, b;
        int c, ox, oy;
        split_index(t, c4, p, c);
        split_index(p, out_w, q, ox);
        split_index(q, out_h, b, oy);
        const float ninf = -INFINITY;
        float4 best = make_float4(ninf, ninf, ninf, ninf);
        int ax = 0, ay = 0, az = 0, aw = 0;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if (iy < 0 || iy >= in_h) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if (ix < 0 || ix >= in_w) continue;
                const float4 v = z[((b * in_h + iy) * in_w + ix) * c4 + c];
                const int pos = 3 * ky + kx;
                take_max(v.x, pos, best.x, ax);
                take_max(v.y, pos, best.y, ay);
                take_max(v.z, pos, best.z, az);
                take_max(v.w, pos, best.w, aw);
            }
        }
        y[t] = best;
        if (y_relu) y_relu[t] = relu4(best);
        if (arg) arg[t] = (uint32_t)ax | (uint32_t)ay << 8 | (uint32_t)az << 16 | (uint32_t)aw << 24;
    }
}

__device__ __forceinline__ void add_term(bool hit, float d, float& acc, bool& have) {
    if (hit) {
        acc = have ? acc + d : d;
        have = true;
    }
}

__global__ __launch_bounds__(RN_THREADS) void maxpool3s2_bwd_kernel(const float4* __restrict__ dy,
                                                                    const uint32_t* __restrict__ arg, int in_h, int in_w,
                                                                    int out_h, int out_w, int c4, int64_t total,
                                                                    float4* __restrict__ dz) {
    const int64_t step = (int64_t)gridDim.x * RN_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x; t < total; t += step) {
        int64_t p, q, b;
        int c, j, i;
        split_index(t, c4, p, c);
        split_index(p, in_w, q, j);
        split_index(q, in_h, b, i);
        // the windows that contain (i, j): oy in [i / 2, (i + 1) / 2], ox in [j / 2, (j + 1) / 2], inside the output
        const int oy_hi = min((i + 1) >> 1, out_h - 1), ox_hi = min((j + 1) >> 1, out_w - 1);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        bool hx = false, hy = false, hz = false, hw = false;
        for (int oy = i >> 1; oy <= oy_hi; ++oy) {
            for (int ox = j >> 1; ox <= ox_hi; ++ox) {
                const uint32_t pos = (uint32_t)(3 * (i - 2 * oy + 1) + (j - 2 * ox + 1));
                const int64_t o = ((b * out_h + oy) * out_w + ox) * c4 + c;
                const uint32_t a = arg[o];
                if (((a & 0xffu) == pos) | ((a >> 8 & 0xffu) == pos) | ((a >> 16 & 0xffu) == pos) | ((a >> 24) == pos)) {
                    const float4 d = dy[o];
                    add_term((a & 0xffu) == pos, d.x, acc.x, hx);
                    add_term((a >> 8 & 0xffu) == pos, d.y, acc.y, hy);
                    add_term((a >> 16 & 0xffu) == pos, d.z, acc.z, hz);
                    add_term((a >> 24) == pos, d.w, acc.w, hw);
                }
            }
        }
        dz[t] = acc;
    }
}

// a, b and sum may be the same buffers: a thread reads its own float4s before it writes them and touches no other
template <bool RELU>
__global__ __launch_bounds__(RN_THREADS) void add_relu_kernel(const float4* a, const float4* b, int64_t n4, float4* sum,
                                                              float4* __restrict__ relu) {
    const int64_t step = (int64_t)gridDim.x * RN_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x; t < n4; t += step) {
        const float4 u = a[t], v = b[t];
        const float4 s = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
        sum[t] = s;
        if (RELU) relu[t] = relu4(s);
    }
}

// one thread per pixel and group of four output channels; with four planes or fewer consecutive threads read
// consecutive bytes of every plane
__global__ __launch_bounds__(RN_THREADS) void gather_nhwc_any_kernel(const uint8_t* __restrict__ obs,
                                                                     const int32_t* __restrict__ idx, int channels,
                                                                     int plane, int c4, float scale, int64_t total,
                                                                     float4* __restrict__ out) {
    const int64_t step = (int64_t)gridDim.x * RN_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x; t < total; t += step) {
        int64_t p, b;
        int c, pix;
        split_index(t, c4, p, c);
        split_index(p, plane, b, pix);
        const uint8_t* row = obs + (idx ? (int64_t)idx[b] : b) * channels * plane + pix;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ch = 4 * c + k;
            v[k] = ch < channels ? (float)row[(int64_t)ch * plane] * scale : 0.f;
        }
        out[t] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

int check_pool(int64_t batch, int32_t in_h, int32_t in_w, int32_t channels) {
    if (batch < 1 || batch > RN_MAX_BATCH || in_h < 1 || in_h > RN_MAX_SIDE || in_w < 1 || in_w > RN_MAX_SIDE ||
        channels < 4 || channels > RN_MAX_CHANNELS || (channels & 3)) {
        arl::set_error("maxpool3s2: need 1 <= batch <= 2^20, 1 <= in_h, in_w <= 2^16 and channels a multiple of 4 in "
                       "4 .. 1024");
        return ARL_E_RANGE;
    }
    return 0;
}

}  // namespace

extern "C" int arl_maxpool3s2_fwd(const float* z, int64_t batch, int32_t in_h, int32_t in_w, int32_t channels, float* y,
                                  float* y_relu_or_null, uint8_t* arg_or_null, void* stream) {
    ARL_REQUIRE(z && y, ARL_E_ARG, "null pointer");
    int rc = check_pool(batch, in_h, in_w, channels);
    if (rc) return rc;
    ARL_REQUIRE(y != z && y_relu_or_null != z && y_relu_or_null != y, ARL_E_ARG, "z, y and y_relu must be three buffers");
    ARL_REQUIRE(arl::aligned16(z) && arl::aligned16(y) && arl::aligned16(y_relu_or_null) && arl::aligned4(arg_or_null),
                ARL_E_ALIGN, "16-byte alignment (arg: 4-byte)");
    const int out_h = (in_h - 1) / 2 + 1, out_w = (in_w - 1) / 2 + 1, c4 = channels >> 2;
    const int64_t total = batch * out_h * out_w * c4;
    hipLaunchKernelGGL(maxpool3s2_fwd_kernel, dim3(arl::stream_grid(total, RN_THREADS)), dim3(RN_THREADS), 0,
                       (hipStream_t)stream, (const float4*)z, (int)in_h, (int)in_w, out_h, out_w, c4, total, (float4*)y,
                       (float4*)y_relu_or_null, (uint32_t*)arg_or_null);
    return arl::check_launch("maxpool3s2_fwd_kernel");
}

extern "C" int arl_maxpool3s2_bwd(const float* dy, const uint8_t* arg, int64_t batch, int32_t in_h, int32_t in_w,
                                  int32_t channels, float* dz, void* stream) {
    ARL_REQUIRE(dy && arg && dz, ARL_E_ARG, "null pointer");
    int rc = check_pool(batch, in_h, in_w, channels);
    if (rc) return rc;
    ARL_REQUIRE(dz != dy, ARL_E_ARG, "dz must not be dy");
    ARL_REQUIRE(arl::aligned16(dy) && arl::aligned16(dz) && arl::aligned4(arg), ARL_E_ALIGN,
                "16-byte alignment (arg: 4-byte)");
    const int out_h = (in_h - 1) / 2 + 1, out_w = (in_w - 1) / 2 + 1, c4 = channels >> 2;
    const int64_t total = batch * in_h * in_w * c4;
    hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3(arl::stream_grid(total, RN_THREADS)), dim3(RN_THREADS), 0,
                       (hipStream_t)stream, (const float4*)dy, (const uint32_t*)arg, (int)in_h, (int)in_w, out_h, out_w, c4,
                       total, (float4*)dz);
    return arl::check_launch("maxpool3s2_bwd_kernel");
}

extern "C" int arl_gather_scale_obs_nhwc_any(const uint8_t* obs, const int32_t* idx_or_null, int64_t batch,
                                             int32_t channels, int32_t plane_bytes, float scale, float* out, void* stream) {
    ARL_REQUIRE(obs && out, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(batch >= 1 && batch <= ((int64_t)1 << 24) && channels >= 1 && channels <= RN_MAX_CHANNELS &&
                plane_bytes >= 1 && plane_bytes <= (1 << 24), ARL_E_RANGE,
                "need 1 <= batch <= 2^24, 1 <= channels <= 1024, 1 <= plane_bytes <= 2^24");
    ARL_REQUIRE(arl::aligned4(idx_or_null) && arl::aligned16(out), ARL_E_ALIGN, "idx 4-byte, out 16-byte aligned");
    const int c4 = (channels + 3) >> 2;
    const int64_t total = batch * plane_bytes * c4;
    hipLaunchKernelGGL(gather_nhwc_any_kernel, dim3(arl::stream_grid(total, RN_THREADS)), dim3(RN_THREADS), 0,
                       (hipStream_t)stream, obs, idx_or_null, (int)channels, (int)plane_bytes, c4, scale, total, (float4*)out);
    return arl::check_launch("gather_nhwc_any_kernel");
}

extern "C" int arl_add_relu(const float* a, const float* b, int64_t n, float* sum, float* relu_or_null, void* stream) {
    ARL_REQUIRE(a && b && sum, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n >= 4 && n <= ((int64_t)1 << 40) && !(n & 3), ARL_E_RANGE, "n must be a multiple of 4 in 4 .. 2^40");
    ARL_REQUIRE(relu_or_null != a && relu_or_null != b && relu_or_null != sum, ARL_E_ARG,
                "relu must be a buffer of its own");
    ARL_REQUIRE(arl::aligned16(a) && arl::aligned16(b) && arl::aligned16(sum) && arl::aligned16(relu_or_null), ARL_E_ALIGN,
                "16-byte alignment");
    const int64_t n4 = n >> 2;
    const dim3 grid(arl::stream_grid(n4, RN_THREADS)), block(RN_THREADS);
    if (relu_or_null)
        hipLaunchKernelGGL(add_relu_kernel<true>, grid, block, 0, (hipStream_t)stream, (const float4*)a, (const float4*)b,
                           n4, (float4*)sum, (float4*)relu_or_null);
    else
        hipLaunchKernelGGL(add_relu_kernel<false>, grid, block, 0, (hipStream_t)stream, (const float4*)a, (const float4*)b,
                           n4, (float4*)sum, (float4*)nullptr);
    return arl::check_launch("add_relu_kernel");
}
