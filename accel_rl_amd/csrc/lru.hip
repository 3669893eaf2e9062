// The linear recurrent unit (LRU) over TIME, forward and backward, for gfx950: the memory of the LRU policy
// (policies/atari_lru_policy.py; Orvieto et al. 2023's diagonal complex recurrence with S5's in-scan resets).
//
//   arl_lru_params      lam = exp(-exp(nu) + i theta), gam = sqrt(1 - |lam|^2): float64, rounded once
//   arl_lru_fwd         h_t = keep_t (lam (.) prev_t) + gam (.) u_t per segment and complex channel, every step of a
//                       segment in one launch
//   arl_lru_bwd         g_t = dH_t + keep_(t+1) (conj(lam) (.) g_(t+1)), du = gam (.) g, and per segment one partial of
//                       d lam and d gam
//   arl_lru_param_fold  the partials added in ascending segment order, then the chain rule to d nu and d theta in float64
//
// One work item is one (segment, block of 64 channels); lane = channel, so a wave reads one step's 64 (re, im) pairs as
// one contiguous 512-byte piece of a row, 8 bytes per lane.  Workgroups of four waves walk the items grid-stride.  The
// segment's flags are staged once into LDS (T bytes), keep_t is then a wave-uniform read.
//   below ARL_LRU_CHUNK_MIN steps   every wave owns an item and runs the serial recurrence, the loads of the next
//                                   LRU_AHEAD steps issued ahead of the dependent multiply-add chain
//   from ARL_LRU_CHUNK_MIN steps    the four waves share an item: the time axis is cut into four chunks of ceil(T / 4)
//                                   steps, a reduce-then-scan through LDS.  Pass 1: a chunk from a zero carry, of which
//                                   only the summary (end state B, multiplier A) is kept -- the chunk as the affine map
//                                   c -> A c + B, A = lam multiplied in once per kept step, exact zero once a reset cuts
//                                   the chunk.  One barrier.  Every wave composes its carry-in from h0 and the summaries
//                                   of the chunks before it, in ascending order; pass 2 reruns the chunk from that carry
//                                   and stores.  The backward mirrors it in reverse time.
// One writer per output element, no atomics, nothing depends on the grid: two launches, or two grid sizes, give the same
// bits; reset NULL stages zeros, so an all-zero flag array gives its bits.  The path is a function of T alone.
// Compiled with -ffp-contract=off and without packed fp32 instructions.
#include "arl_common.h"

#include <math.h>

namespace {

constexpr int LRU_THREADS = 256, LRU_WAVES = 4, LRU_LANES = 64;
constexpr int LRU_AHEAD = 8;            // steps whose loads are in flight before the chain that consumes them
constexpr int LRU_FOLD_AHEAD = 16;      // segments whose partials are in flight in the fold

int g_lru_path = 0;                     // arl_dev_lru_force_path: 0 = by T, 1 = serial, 2 = chunked

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {           // a b
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) {          // conj(a) b
    return make_float2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}

// sF[t] = whether step t of segment seg carries a flag, t < T; threads first, first + stride, ..
__device__ __forceinline__ void stage_flags(uint8_t* sF, const uint8_t* __restrict__ reset, const int32_t* __restrict__ idx,
                                            int64_t seg, int T, int first, int stride) {
    for (int t = first; t < T; t += stride) {
        uint8_t f = 0;
        if (reset) {
            const int64_t r = seg * T + t;
            f = reset[idx ? (int64_t)idx[r] : r] != 0;
        }
        sF[t] = f;
    }
}

// Steps t0 .. t1 - 1 of one channel from the carry h (u and h_all point at the channel's element of step 0, row = the row
// stride in float2).  STORE: every step's state goes to h_all.  MULT: a = the multiplier of the steps.
template <bool STORE, bool MULT>
__device__ __forceinline__ void fwd_steps(const float2* __restrict__ u, float2* __restrict__ h_all, const uint8_t* sF, int t0,
                                          int t1, int64_t row, bool on, float2 lam, float gam, float2& h, float2& a) {
    for (int tb = t0; tb < t1; tb += LRU_AHEAD) {
        float2 uu[LRU_AHEAD];
#pragma unroll
        for (int k = 0; k < LRU_AHEAD; ++k) {
            uu[k] = make_float2(0.f, 0.f);
            if (on && tb + k < t1) uu[k] = u[(int64_t)(tb + k) * row];
        }
#pragma unroll
        for (int k = 0; k < LRU_AHEAD; ++k) {
            const int t = tb + k;
            if (t < t1) {                       // (wave-uniform)
                const bool keep = t == 0 || sF[t - 1] == 0;
                const float2 in = make_float2(gam * uu[k].x, gam * uu[k].y);
                if (keep) {
                    const float2 p = cmul(lam, h);
                    h = make_float2(p.x + in.x, p.y + in.y);
                    if (MULT) a = cmul(lam, a);
                } else {                        // the carry takes no part
                    h = in;
                    if (MULT) a = make_float2(0.f, 0.f);
                }
                if (STORE && on) h_all[(int64_t)t * row] = h;
            }
        }
    }
}

// (h0 and h_last are not __restrict__: they may be one buffer)
__global__ __launch_bounds__(LRU_THREADS) void lru_fwd_kernel(const float2* __restrict__ u, const float* __restrict__ lam,
                                                              const float* __restrict__ gam, const float2* h0,
                                                              const uint8_t* __restrict__ reset,
                                                              const int32_t* __restrict__ idx, float2* __restrict__ h_all,
                                                              float2* h_last, int64_t items, int n_blk, int T, int N,
                                                              int chunked) {
    __shared__ uint8_t sF[LRU_WAVES][ARL_LRU_MAX_STEPS];
    __shared__ float4 sSum[LRU_WAVES][LRU_LANES];       // (B re, B im, A re, A im)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float2 one = make_float2(1.f, 0.f);
    if (!chunked) {
        for (int64_t base = (int64_t)blockIdx.x * LRU_WAVES; base < items; base += (int64_t)gridDim.x * LRU_WAVES) {
            const int64_t item = base + wave;
            const bool live = item < items;
            const int64_t seg = live ? item / n_blk : 0;
            const int c = (int)(item - seg * n_blk) * LRU_LANES + lane;
            const bool on = live && c < N;
            __syncthreads();                    // the flags of the item before have been read
            if (live) stage_flags(sF[wave], reset, idx, seg, T, lane, LRU_LANES);
            __syncthreads();
            const float2 l = on ? make_float2(lam[2 * c], lam[2 * c + 1]) : make_float2(0.f, 0.f);
            const float gm = on ? gam[c] : 0.f;
            float2 h = on ? h0[seg * N + c] : make_float2(0.f, 0.f);
            const int64_t off = seg * T * N + c;
            fwd_steps<true, false>(u + off, h_all + off, sF[wave], 0, live ? T : 0, N, on, l, gm, h, one);
            if (on && h_last) h_last[seg * N + c] = h;
        }
        return;
    }
    const int len = (T + LRU_WAVES - 1) / LRU_WAVES;
    const int t0 = wave * len < T ? wave * len : T, t1 = t0 + len < T ? t0 + len : T;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t seg = item / n_blk;
        const int c = (int)(item - seg * n_blk) * LRU_LANES + lane;
        const bool on = c < N;
        __syncthreads();                        // the flags and summaries of the item before have been read
        stage_flags(sF[0], reset, idx, seg, T, tid, LRU_THREADS);
        const float2 l = on ? make_float2(lam[2 * c], lam[2 * c + 1]) : make_float2(0.f, 0.f);
        const float gm = on ? gam[c] : 0.f;
        const float2 start = on ? h0[seg * N + c] : make_float2(0.f, 0.f);      // every wave, before wave 3 may write it
        const int64_t off = seg * T * N + c;
        __syncthreads();
        float2 b = make_float2(0.f, 0.f), a = make_float2(1.f, 0.f);
        if (wave < LRU_WAVES - 1) fwd_steps<false, true>(u + off, h_all + off, sF[0], t0, t1, N, on, l, gm, b, a);
        sSum[wave][lane] = make_float4(b.x, b.y, a.x, a.y);
        __syncthreads();
        float2 h = start;
        for (int j = 0; j < wave; ++j) {        // the carry into this chunk: chunk 0's map, then chunk 1's, ..
            const float4 s = sSum[j][lane];
            const float2 p = cmul(make_float2(s.z, s.w), h);
            h = make_float2(p.x + s.x, p.y + s.y);
        }
        fwd_steps<true, false>(u + off, h_all + off, sF[0], t0, t1, N, on, l, gm, h, one);
        if (wave == LRU_WAVES - 1 && on && h_last) h_last[seg * N + c] = h;
    }
}

// Steps t1 - 1 .. t0 of one channel in reverse time from the carry g (= g of step t1; the pointers as in fwd_steps).
// OUT: du, and the chunk's sums dl (d lam) and dg (d gam) from 0.f in the order of the walk; otherwise a = the
// multiplier of the steps.
template <bool OUT>
__device__ __forceinline__ void bwd_steps(const float2* dh, const float2* __restrict__ u, const float2* __restrict__ h_all,
                                          float2 start, float2* du, const uint8_t* sF, int t0, int t1, int T, int64_t row,
                                          bool on, float2 lam, float gam, float2& g, float2& a, float2& dl, float& dg) {
    const float2 zero = make_float2(0.f, 0.f);
    for (int tb = t1 - 1; tb >= t0; tb -= LRU_AHEAD) {
        float2 d[LRU_AHEAD], uu[LRU_AHEAD], pp[LRU_AHEAD];
#pragma unroll
        for (int k = 0; k < LRU_AHEAD; ++k) {
            const int t = tb - k;
            const bool ld = on && t >= t0;
            d[k] = uu[k] = zero;
            pp[k] = start;
            if (ld) d[k] = dh[(int64_t)t * row];
            if (OUT && ld) uu[k] = u[(int64_t)t * row];
            if (OUT && ld && t > 0) pp[k] = h_all[(int64_t)(t - 1) * row];
        }
#pragma unroll
        for (int k = 0; k < LRU_AHEAD; ++k) {
            const int t = tb - k;
            if (t >= t0) {                      // (wave-uniform)
                const bool keep_next = t + 1 < T && sF[t] == 0;
                if (keep_next) {
                    const float2 p = cmulc(lam, g);
                    g = make_float2(d[k].x + p.x, d[k].y + p.y);
                    if (!OUT) a = cmulc(lam, a);
                } else {                        // no gradient crosses a reset, none enters after the last step
                    g = d[k];
                    if (!OUT) a = zero;
                }
                if (OUT) {
                    if (on) du[(int64_t)t * row] = make_float2(gam * g.x, gam * g.y);
                    if (t == 0 || sF[t - 1] == 0) {
                        const float2 q = cmulc(pp[k], g);
                        dl = make_float2(dl.x + q.x, dl.y + q.y);
                    }
                    dg = dg + (uu[k].x * g.x + uu[k].y * g.y);
                }
            }
        }
    }
}

// (dh and du are not __restrict__: they may be one buffer; a thread reads its element before it writes it)
__global__ __launch_bounds__(LRU_THREADS) void lru_bwd_kernel(const float2* __restrict__ u, const float2* __restrict__ h_all,
                                                              const float2* __restrict__ h0, const float* __restrict__ lam,
                                                              const float* __restrict__ gam, const float2* dh,
                                                              const uint8_t* __restrict__ reset,
                                                              const int32_t* __restrict__ idx, float2* du,
                                                              float* __restrict__ dlam_parts, float* __restrict__ dgam_parts,
                                                              int64_t items, int n_blk, int T, int N, int chunked) {
    __shared__ uint8_t sF[LRU_WAVES][ARL_LRU_MAX_STEPS];
    __shared__ float4 sSum[LRU_WAVES][LRU_LANES];       // (B re, B im, A re, A im)
    __shared__ float4 sPart[LRU_WAVES][LRU_LANES];      // (d lam re, d lam im, d gam, -)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float2 zero = make_float2(0.f, 0.f);
    float2 one = make_float2(1.f, 0.f);
    if (!chunked) {
        for (int64_t base = (int64_t)blockIdx.x * LRU_WAVES; base < items; base += (int64_t)gridDim.x * LRU_WAVES) {
            const int64_t item = base + wave;
            const bool live = item < items;
            const int64_t seg = live ? item / n_blk : 0;
            const int c = (int)(item - seg * n_blk) * LRU_LANES + lane;
            const bool on = live && c < N;
            __syncthreads();                    // the flags of the item before have been read
            if (live) stage_flags(sF[wave], reset, idx, seg, T, lane, LRU_LANES);
            __syncthreads();
            const float2 l = on ? make_float2(lam[2 * c], lam[2 * c + 1]) : make_float2(0.f, 0.f);
            const float gm = on ? gam[c] : 0.f;
            const float2 start = on ? h0[seg * N + c] : make_float2(0.f, 0.f);
            const int64_t off = seg * T * N + c;
            float2 g = zero, dl = zero;
            float dg = 0.f;
            bwd_steps<true>(dh + off, u + off, h_all + off, start, du + off, sF[wave], 0, live ? T : 0, T, N, on, l, gm, g, one,
                            dl, dg);
            if (on) {
                dlam_parts[2 * (seg * N + c)] = dl.x;
                dlam_parts[2 * (seg * N + c) + 1] = dl.y;
                dgam_parts[seg * N + c] = dg;
            }
        }
        return;
    }
    const int len = (T + LRU_WAVES - 1) / LRU_WAVES;
    const int t0 = wave * len < T ? wave * len : T, t1 = t0 + len < T ? t0 + len : T;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t seg = item / n_blk;
        const int c = (int)(item - seg * n_blk) * LRU_LANES + lane;
        const bool on = c < N;
        __syncthreads();                        // the flags, summaries and partials of the item before have been read
        stage_flags(sF[0], reset, idx, seg, T, tid, LRU_THREADS);
        const float2 l = on ? make_float2(lam[2 * c], lam[2 * c + 1]) : make_float2(0.f, 0.f);
        const float gm = on ? gam[c] : 0.f;
        const float2 start = on ? h0[seg * N + c] : make_float2(0.f, 0.f);
        const int64_t off = seg * T * N + c;
        __syncthreads();
        float2 b = zero, a = make_float2(1.f, 0.f), dl = zero;
        float dg = 0.f;
        if (wave > 0) bwd_steps<false>(dh + off, u + off, h_all + off, start, du + off, sF[0], t0, t1, T, N, on, l, gm, b, a, dl, dg);
        sSum[wave][lane] = make_float4(b.x, b.y, a.x, a.y);
        __syncthreads();
        float2 g = zero;
        for (int j = LRU_WAVES - 1; j > wave; --j) {    // the carry into this chunk: chunk 3's map, then chunk 2's, ..
            const float4 s = sSum[j][lane];
            const float2 p = cmul(make_float2(s.z, s.w), g);
            g = make_float2(p.x + s.x, p.y + s.y);
        }
        bwd_steps<true>(dh + off, u + off, h_all + off, start, du + off, sF[0], t0, t1, T, N, on, l, gm, g, one, dl, dg);
        sPart[wave][lane] = make_float4(dl.x, dl.y, dg, 0.f);
        __syncthreads();
        if (wave == 0 && on) {                  // chunk 0's partial + chunk 1's + chunk 2's + chunk 3's
            float4 acc = sPart[0][lane];
            for (int j = 1; j < LRU_WAVES; ++j) {
                const float4 p = sPart[j][lane];
                acc = make_float4(acc.x + p.x, acc.y + p.y, acc.z + p.z, 0.f);
            }
            dlam_parts[2 * (seg * N + c)] = acc.x;
            dlam_parts[2 * (seg * N + c) + 1] = acc.y;
            dgam_parts[seg * N + c] = acc.z;
        }
    }
}

__global__ __launch_bounds__(LRU_THREADS) void lru_params_kernel(const float* __restrict__ nu, const float* __restrict__ theta,
                                                                 int N, float* __restrict__ lam, float* __restrict__ gam) {
    const int j = blockIdx.x * LRU_THREADS + threadIdx.x;
    if (j >= N) return;
    const double e = exp((double)nu[j]), mag = exp(-e), th = (double)theta[j];
    lam[2 * j] = (float)(mag * cos(th));
    lam[2 * j + 1] = (float)(mag * sin(th));
    gam[j] = (float)sqrt(-expm1(-2.0 * e));     // 1 - |lam|^2 without the cancellation
}

__global__ __launch_bounds__(LRU_THREADS) void lru_param_fold_kernel(const float* __restrict__ dlam_parts,
                                                                     const float* __restrict__ dgam_parts,
                                                                     const float* __restrict__ nu, const float* __restrict__ theta,
                                                                     int64_t n_seg, int N, float* __restrict__ dnu,
                                                                     float* __restrict__ dtheta) {
    const int j = blockIdx.x * LRU_THREADS + threadIdx.x;
    if (j >= N) return;
    float dl_re = 0.f, dl_im = 0.f, dg = 0.f;
    for (int64_t s0 = 0; s0 < n_seg; s0 += LRU_FOLD_AHEAD) {    // the loads of 16 segments in flight, the sums one chain
        float re[LRU_FOLD_AHEAD], im[LRU_FOLD_AHEAD], gg[LRU_FOLD_AHEAD];
#pragma unroll
        for (int k = 0; k < LRU_FOLD_AHEAD; ++k) {
            const int64_t s = s0 + k < n_seg ? s0 + k : n_seg - 1;
            re[k] = dlam_parts[2 * (s * N + j)];
            im[k] = dlam_parts[2 * (s * N + j) + 1];
            gg[k] = dgam_parts[s * N + j];
        }
#pragma unroll
        for (int k = 0; k < LRU_FOLD_AHEAD; ++k) {
            if (s0 + k < n_seg) {
                dl_re += re[k];
                dl_im += im[k];
                dg += gg[k];
            }
        }
    }
    const double e = exp((double)nu[j]), mag = exp(-e), th = (double)theta[j];
    const double l_re = mag * cos(th), l_im = mag * sin(th), gm = sqrt(-expm1(-2.0 * e));
    dtheta[j] = (float)(-l_im * (double)dl_re + l_re * (double)dl_im);
    dnu[j] = (float)(-e * (l_re * (double)dl_re + l_im * (double)dl_im) + (double)dg * e * (mag * mag) / gm);
}

int check_lru(int64_t n_seg, int32_t T, int32_t N) {
    if (n_seg < 1 || n_seg > ARL_ATTN_MAX_BATCH || T < 1 || T > ARL_LRU_MAX_STEPS || N < 2 || N > ARL_LRU_MAX_STATE || (N & 1)) {
        arl::set_error("linear recurrence: need 1 <= n_seg <= 2^24, 1 <= T <= %d, state_size even in 2 .. %d",
                       ARL_LRU_MAX_STEPS, ARL_LRU_MAX_STATE);
        return ARL_E_RANGE;
    }
    return 0;
}

bool lru_chunked(int32_t T) { return g_lru_path == 0 ? T >= ARL_LRU_CHUNK_MIN : g_lru_path == 2; }

unsigned lru_grid(int64_t items, bool chunked) {
    const int64_t blocks = chunked ? items : (items + LRU_WAVES - 1) / LRU_WAVES;
    return (unsigned)(blocks < ARL_LRU_MAX_GRID ? blocks : ARL_LRU_MAX_GRID);
}

}  // namespace

extern "C" void arl_dev_lru_force_path(int32_t path) { g_lru_path = (path == 1 || path == 2) ? path : 0; }

extern "C" int arl_lru_params(const float* nu, const float* theta, int32_t state_size, float* lam, float* gam, void* stream) {
    ARL_REQUIRE(nu && theta && lam && gam, ARL_E_ARG, "null pointer");
    int rc = check_lru(1, 1, state_size);
    if (rc) return rc;
    const int64_t n = (int64_t)state_size * 4;
    const arl::Span in[2] = {{nu, n}, {theta, n}};
    const arl::Span outs[2] = {{lam, 2 * n}, {gam, n}};
    if (!arl::check_disjoint("arl_lru_params", in, 2, outs, 2)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned4(nu) && arl::aligned4(theta) && arl::aligned4(gam) && arl::aligned4(lam), ARL_E_ALIGN,
                "4-byte alignment");
    hipLaunchKernelGGL(lru_params_kernel, dim3((state_size + LRU_THREADS - 1) / LRU_THREADS), dim3(LRU_THREADS), 0,
                       (hipStream_t)stream, nu, theta, (int)state_size, lam, gam);
    return arl::check_launch("lru_params_kernel");
}

extern "C" int arl_lru_fwd(const float* u, const float* lam, const float* gam, const float* h0, const uint8_t* reset_or_null,
                           const int32_t* idx_or_null, int64_t n_seg, int32_t seg_len, int32_t state_size, float* h_all,
                           float* h_last_or_null, void* stream) {
    ARL_REQUIRE(u && lam && gam && h0 && h_all, ARL_E_ARG, "null pointer");
    int rc = check_lru(n_seg, seg_len, state_size);
    if (rc) return rc;
    const int64_t n_u = n_seg * seg_len * state_size * 8, n_h = n_seg * state_size * 8, n = (int64_t)state_size * 4;
    const bool in_place = h_last_or_null == h0;         // a thread reads its element of h0 before any writes it
    const arl::Span in[6] = {{u, n_u}, {lam, 2 * n}, {gam, n}, {reset_or_null, reset_or_null ? n_seg * seg_len : 0},
                             {idx_or_null, idx_or_null ? n_seg * seg_len * 4 : 0}, {h0, in_place ? 0 : n_h}};
    const arl::Span outs[2] = {{h_all, n_u}, {h_last_or_null, n_h}};
    if (!arl::check_disjoint("arl_lru_fwd", in, 6, outs, 2)) return ARL_E_ARG;
    ARL_REQUIRE(!arl::overlap(h_all, n_u, h0, n_h), ARL_E_ARG, "h_all must not overlap h0");
    ARL_REQUIRE(arl::aligned16(u) && arl::aligned16(h0) && arl::aligned16(h_all) && arl::aligned16(h_last_or_null) &&
                    arl::aligned4(lam) && arl::aligned4(gam) && arl::aligned4(idx_or_null),
                ARL_E_ALIGN, "u, h0, h_all and h_last 16-byte, lam, gam and idx 4-byte aligned");
    const int n_blk = (state_size + LRU_LANES - 1) / LRU_LANES;
    const int64_t items = n_seg * n_blk;
    const bool chunked = lru_chunked(seg_len);
    hipLaunchKernelGGL(lru_fwd_kernel, dim3(lru_grid(items, chunked)), dim3(LRU_THREADS), 0, (hipStream_t)stream,
                       (const float2*)u, lam, gam, (const float2*)h0, reset_or_null, idx_or_null, (float2*)h_all,
                       (float2*)h_last_or_null, items, n_blk, (int)seg_len, (int)state_size, chunked ? 1 : 0);
    return arl::check_launch("lru_fwd_kernel");
}

extern "C" int arl_lru_bwd(const float* u, const float* h_all, const float* h0, const float* lam, const float* gam,
                           const float* dh, const uint8_t* reset_or_null, const int32_t* idx_or_null, int64_t n_seg,
                           int32_t seg_len, int32_t state_size, float* du, float* dlam_parts, float* dgam_parts, void* stream) {
    ARL_REQUIRE(u && h_all && h0 && lam && gam && dh && du && dlam_parts && dgam_parts, ARL_E_ARG, "null pointer");
    int rc = check_lru(n_seg, seg_len, state_size);
    if (rc) return rc;
    const int64_t n_u = n_seg * seg_len * state_size * 8, n_h = n_seg * state_size * 8, n = (int64_t)state_size * 4;
    const bool in_place = du == dh;                     // a thread reads its element of dh before it writes it
    const arl::Span in[8] = {{u, n_u}, {h_all, n_u}, {h0, n_h}, {lam, 2 * n}, {gam, n},
                             {reset_or_null, reset_or_null ? n_seg * seg_len : 0},
                             {idx_or_null, idx_or_null ? n_seg * seg_len * 4 : 0}, {dh, in_place ? 0 : n_u}};
    const arl::Span outs[3] = {{du, n_u}, {dlam_parts, n_h}, {dgam_parts, n_h / 2}};
    if (!arl::check_disjoint("arl_lru_bwd", in, 8, outs, 3)) return ARL_E_ARG;
    ARL_REQUIRE(!arl::overlap(dlam_parts, n_h, dh, n_u) && !arl::overlap(dgam_parts, n_h / 2, dh, n_u), ARL_E_ARG,
                "the partials must not overlap dh");
    ARL_REQUIRE(arl::aligned16(u) && arl::aligned16(h_all) && arl::aligned16(h0) && arl::aligned16(dh) && arl::aligned16(du) &&
                    arl::aligned4(lam) && arl::aligned4(dlam_parts) && arl::aligned4(gam) && arl::aligned4(idx_or_null) &&
                    arl::aligned4(dgam_parts),
                ARL_E_ALIGN, "u, h_all, h0, dh and du 16-byte, lam, gam, idx and the partials 4-byte aligned");
    const int n_blk = (state_size + LRU_LANES - 1) / LRU_LANES;
    const int64_t items = n_seg * n_blk;
    const bool chunked = lru_chunked(seg_len);
    hipLaunchKernelGGL(lru_bwd_kernel, dim3(lru_grid(items, chunked)), dim3(LRU_THREADS), 0, (hipStream_t)stream,
                       (const float2*)u, (const float2*)h_all, (const float2*)h0, lam, gam, (const float2*)dh,
                       reset_or_null, idx_or_null, (float2*)du, dlam_parts, dgam_parts, items, n_blk, (int)seg_len,
                       (int)state_size, chunked ? 1 : 0);
    return arl::check_launch("lru_bwd_kernel");
}

extern "C" int arl_lru_param_fold(const float* dlam_parts, const float* dgam_parts, const float* nu, const float* theta,
                                  int64_t n_seg, int32_t state_size, float* dnu, float* dtheta, void* stream) {
    ARL_REQUIRE(dlam_parts && dgam_parts && nu && theta && dnu && dtheta, ARL_E_ARG, "null pointer");
    int rc = check_lru(n_seg, 1, state_size);
    if (rc) return rc;
    const int64_t n = (int64_t)state_size * 4;
    const arl::Span in[4] = {{dlam_parts, n_seg * 2 * n}, {dgam_parts, n_seg * n}, {nu, n}, {theta, n}};
    const arl::Span outs[2] = {{dnu, n}, {dtheta, n}};
    if (!arl::check_disjoint("arl_lru_param_fold", in, 4, outs, 2)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned4(dlam_parts) && arl::aligned4(dgam_parts) && arl::aligned4(nu) && arl::aligned4(theta) &&
                    arl::aligned4(dnu) && arl::aligned4(dtheta),
                ARL_E_ALIGN, "4-byte alignment");
    hipLaunchKernelGGL(lru_param_fold_kernel, dim3((state_size + LRU_THREADS - 1) / LRU_THREADS), dim3(LRU_THREADS), 0,
                       (hipStream_t)stream, dlam_parts, dgam_parts, nu, theta, n_seg, (int)state_size, dnu, dtheta);
    return arl::check_launch("lru_param_fold_kernel");
}
