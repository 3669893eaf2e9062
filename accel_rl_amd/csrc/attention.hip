// Multi-head self-attention over the positions of one feature map, forward and backward, for gfx950: the core of the
// relational policy (Zambaldi et al. 2018; policies/atari_relational_policy.py), and the two streaming kernels that
// append and strip its coordinate channels.
//
//   arl_attn_fwd            S = scale Q K^T, P = softmax_j(S), O = P V per sample and head [, lse = logsumexp_j S]
//   arl_attn_bwd            S again (the forward's instructions), P = exp(S - lse), D_i = sum_e dO_ie O_ie,
//                           dV = P^T dO, dP = dO V^T, dS = scale P o (dP - D), dQ = dS K, dK = dS^T Q
//   arl_attn_tiled_fwd/_bwd the same for 65 .. 256 positions: 64-row tiles around an online soft-max (further down)
//   arl_entity_coords_fwd   y = [x, (2 j - (w - 1)) / (w - 1), (2 i - (h - 1)) / (h - 1), 0, 0] along the channels
//   arl_entity_coords_bwd   g_in = g + d_y[..., :C] [, +0 where mask <= 0]
//
// Attention.  One work item is one (sample, head); a workgroup of four waves walks the items grid-stride (item g,
// g + grid, ...), and an item's whole attention lives in the LDS of its compute unit: Q, K, V (and dO) as [64][d + 1]
// tiles, S / P (and dS) as [64][65].  Every row stride is odd, so an operand read down a column (P^T, dS^T, K^T, V^T)
// is as conflict-free as one along a row.  Rows from N up are zeros in every tile and in P and dS, and the reductions
// over positions stop at N.  All six products run on v_mfma_f32_32x32x2_f32, operands as they are: S, dP and dS are
// 2 x 2 blocks of 32 x 32, one per wave; a [64][d] product (O, dV, dQ, dK) is 2 x 2 blocks too where d > 32, and where
// d <= 32 its two blocks deal the reduction out in halves (positions 0 .. 31 and 32 .. 63) to two waves each: the
// second half's partial goes through a tile that is free at that point and is added to the first's.  The soft-max and
// D_i take four threads per row, each walking every fourth column (every fourth float4) in ascending order, the four
// partial sums added as ((p0 + p1) + p2) + p3.  Every output element has one writer: plain vector stores, no atomics,
// no partial sums in global memory; nothing depends on the grid, and two runs give the same bits.  P never leaves LDS.
// The streaming kernels are csrc/resnet.hip's kind: one float4 per thread and step, no LDS.
// Compiled with -ffp-contract=off and without packed fp32 instructions.
#include "arl_common.h"
#include "attention_dev.h"

#include <math.h>

namespace {

__global__ __launch_bounds__(AT_THREADS, 2) void attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                              float* __restrict__ lse, int64_t items, int N, int H, int d,
                                                              float scale) {
    extern __shared__ float lds[];
    const int ld = d + 1, tile = AT_POS * ld;
    float* sQ = lds;                            // [64][d + 1]; after S: the second halves' partial of O
    float* sK = sQ + tile;
    float* sV = sK + tile;
    float* sS = sV + tile;                      // [64][65]  S, then exp(S - max)
    float* sInv = sS + AT_SBLK;                 // [64]      1 / sum_j exp(S_ij - max_i)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
    const int64_t HD = (int64_t)H * d;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / H;
        const int h = (int)(item - b * H);
        const float* base = qkv + b * N * 3 * HD + (int64_t)h * d;
        __syncthreads();                        // the item before has been read
        load_tile(sQ, base, 3 * HD, N, d, ld, tid);
        load_tile(sK, base + HD, 3 * HD, N, d, ld, tid);
        load_tile(sV, base + 2 * HD, 3 * HD, N, d, ld, tid);
        __syncthreads();
        {
            const int rb = (wave >> 1) * 32, cb = (wave & 1) * 32;
            const f32x16 acc = qk_block(sQ, sK, ld, d, rb, cb, lane);
#pragma unroll
            for (int v = 0; v < 16; ++v) sS[(rb + acc_row(v, lane)) * AT_LS + cb + l31] = scale * acc[v];
        }
        __syncthreads();
        {                                       // soft-max: row tid / 4, columns tid % 4, + 4, ..
            const int i = tid >> 2, q = tid & 3;
            float* s = sS + i * AT_LS;
            float m = -INFINITY, p = 0.f;
            if (i < N) {
                for (int j = q; j < N; j += 4) m = fmaxf(m, s[j]);
            }
            m = fmaxf(m, __shfl_xor(m, 1, 64));
            m = fmaxf(m, __shfl_xor(m, 2, 64));
            if (i < N) {
                for (int j = q; j < N; j += 4) {
                    const float e = expf(s[j] - m);
                    s[j] = e;
                    p += e;
                }
                for (int j = N + q; j < AT_POS; j += 4) s[j] = 0.f;
            } else {
                for (int j = q; j < AT_POS; j += 4) s[j] = 0.f;
            }
            const float l = row_sum4(p, lane);
            if (q == 0) {
                sInv[i] = i < N ? 1.f / l : 0.f;
                if (lse && i < N) lse[item * N + i] = m + logf(l);
            }
        }
        __syncthreads();
        float* o = out + b * N * HD + (int64_t)h * d;
        pos_product(d, N, sQ, ld, wave, lane, [&](int i, int k) { return sS[i * AT_LS + k]; },
                    [&](int k, int e) { return e < d ? sV[k * ld + e] : 0.f; },
                    [&](int i, int e, float v) { if (i < N) o[i * HD + e] = v * sInv[i]; });
    }
}

__global__ __launch_bounds__(AT_THREADS, 2) void attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                              const float* __restrict__ lse, const float* __restrict__ dout,
                                                              float* __restrict__ dqkv, int64_t items, int N, int H, int d,
                                                              float scale) {
    extern __shared__ float lds[];
    const int ld = d + 1, tile = AT_POS * ld;
    float* sQ = lds;
    float* sK = sQ + tile;
    float* sV = sK + tile;                      // after dP: the second halves' partial of dK
    float* sG = sV + tile;                      // dO; after dP: the second halves' partial of dQ
    float* sP = sG + tile;                      // [64][65]
    float* sdS = sP + AT_SBLK;                  // [64][65]; before dS: the second halves' partial of dV
    float* sLse = sdS + AT_SBLK;                // [64]
    float* sD = sLse + AT_POS;                  // [64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
    const int rb = (wave >> 1) * 32, cb = (wave & 1) * 32;      // this wave's block of S, dP and dS
    const int64_t HD = (int64_t)H * d;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / H;
        const int h = (int)(item - b * H);
        const int64_t off = b * N * 3 * HD + (int64_t)h * d;
        __syncthreads();                        // the item before has been read
        load_tile(sQ, qkv + off, 3 * HD, N, d, ld, tid);
        load_tile(sK, qkv + off + HD, 3 * HD, N, d, ld, tid);
        load_tile(sV, qkv + off + 2 * HD, 3 * HD, N, d, ld, tid);
        load_tile(sG, dout + b * N * HD + (int64_t)h * d, HD, N, d, ld, tid);
        if (tid < AT_POS) sLse[tid] = tid < N ? lse[item * N + tid] : 0.f;
        __syncthreads();
        {                                       // D_i: row tid / 4, float4s tid % 4, + 4, ..; the products added one by one
            const int i = tid >> 2, q = tid & 3;
            float p = 0.f;
            if (i < N) {
                const float* o = out + (b * N + i) * HD + (int64_t)h * d;
                const float* g = sG + i * ld;
                for (int c = 4 * q; c < d; c += 16) {
                    const float4 ov = *reinterpret_cast<const float4*>(o + c);
                    p += g[c] * ov.x;
                    p += g[c + 1] * ov.y;
                    p += g[c + 2] * ov.z;
                    p += g[c + 3] * ov.w;
                }
            }
            const float s = row_sum4(p, lane);
            if (q == 0) sD[i] = s;
        }
        {                                       // P = exp(S - lse), zeros from N on
            const f32x16 acc = qk_block(sQ, sK, ld, d, rb, cb, lane);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = rb + acc_row(v, lane), j = cb + l31;
                sP[i * AT_LS + j] = (i < N && j < N) ? expf(scale * acc[v] - sLse[i]) : 0.f;
            }
        }
        __syncthreads();
        float* dq = dqkv + off;
        float* dk = dq + HD;
        float* dv = dk + HD;
        // dV = P^T dO
        pos_product(d, N, sdS, ld, wave, lane, [&](int j, int i) { return sP[i * AT_LS + j]; },
                    [&](int i, int e) { return e < d ? sG[i * ld + e] : 0.f; },
                    [&](int j, int e, float v) { if (j < N) dv[j * 3 * HD + e] = v; });
        __syncthreads();                        // dV's partial has been read
        {                                       // dP = dO V^T, dS = scale (P (dP - D))
            f32x16 acc = {};
            acc = mm32(acc, 0, d, lane, [&](int i, int e) { return sG[(rb + i) * ld + e]; },
                       [&](int e, int j) { return sV[(cb + j) * ld + e]; });
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = rb + acc_row(v, lane), j = cb + l31;
                sdS[i * AT_LS + j] = scale * (sP[i * AT_LS + j] * (acc[v] - sD[i]));
            }
        }
        __syncthreads();                        // dS is whole; dO and V have been read
        // dQ = dS K
        pos_product(d, N, sG, ld, wave, lane, [&](int i, int j) { return sdS[i * AT_LS + j]; },
                    [&](int j, int e) { return e < d ? sK[j * ld + e] : 0.f; },
                    [&](int i, int e, float v) { if (i < N) dq[i * 3 * HD + e] = v; });
        // dK = dS^T Q
        pos_product(d, N, sV, ld, wave, lane, [&](int j, int i) { return sdS[i * AT_LS + j]; },
                    [&](int i, int e) { return e < d ? sQ[i * ld + e] : 0.f; },
                    [&](int j, int e, float v) { if (j < N) dk[j * 3 * HD + e] = v; });
    }
}

// ---- more than 64 positions: 64-row tiles streamed around an online soft-max ---------------------------------------------
//
// The same tiles, products and thread layouts as above, with N up to ARL_ATTN_TILED_MAX_POS = 4 tiles of 64 rows.
// Forward: one item is (sample, head, query tile).  Q is loaded once; the key tiles pass through sK / sV in ascending
// order, each one's 64 x 64 score block through sS; per row a running maximum m and sum l live in LDS, and the item's
// unnormalised O stays in the MFMA accumulators, scaled by alpha = exp(m_old - m_new) before every tile's x V is added
// by the same chain.  Where d <= 32 the waves 2 and 3 take the second 32 keys of EVERY tile and keep their partial to
// the end: one addition, first halves + second halves, per item.  Backward: one item is (sample, head); lse, D and a
// [N_pad][d + 1] tile of dQ are resident in LDS; key tiles outside, query tiles inside, both ascending; dK_j and dV_j
// stay in the accumulators over the inner loop (d <= 32: halves of the query tile, kept apart to the end as above) and
// each tile pair's dS K_j goes into the dQ tile, stored at j = 0 and added after.  dS is written over P in place: the
// thread that owns a dP accumulator element owns that element of P.

constexpr int AT_TILES = ARL_ATTN_TILED_MAX_POS / AT_POS;

__global__ __launch_bounds__(AT_THREADS, 2) void attn_tiled_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                    float* __restrict__ lse, int64_t items, int N, int H,
                                                                    int d, float scale) {
    extern __shared__ float lds[];
    const int ld = d + 1, tile = AT_POS * ld;
    float* sQ = lds;                            // [64][d + 1]; after the last tile: the second halves' partial of O
    float* sK = sQ + tile;
    float* sV = sK + tile;
    float* sS = sV + tile;                      // [64][65]  S, then exp(S - m)
    float* sM = sS + AT_SBLK;                   // [64]      the running maximum
    float* sL = sM + AT_POS;                    // [64]      the running sum
    float* sA = sL + AT_POS;                    // [64]      this tile's alpha
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
    const int tiles = (N + AT_POS - 1) / AT_POS;
    const bool halves = d <= 32;
    // O: block (wave / 2, wave % 2) of [64][64], or row block wave % 2 over the keys [32 (wave / 2), + 32) of each tile
    const int orb = (halves ? wave & 1 : wave >> 1) * 32, ocb = halves ? 0 : (wave & 1) * 32, okb = halves ? (wave >> 1) * 32 : 0;
    const int64_t HD = (int64_t)H * d;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t bh = item / tiles, b = bh / H;
        const int h = (int)(bh - b * H), q0 = (int)(item - bh * tiles) * AT_POS;
        const float* base = qkv + b * N * 3 * HD + (int64_t)h * d;
        __syncthreads();                        // the item before has been read
        load_tile(sQ, base + (int64_t)q0 * 3 * HD, 3 * HD, N - q0, d, ld, tid);
        if (tid < AT_POS) {
            sM[tid] = -INFINITY;
            sL[tid] = 0.f;
        }
        f32x16 acc = {};
        for (int k0 = 0; k0 < N; k0 += AT_POS) {
            const int kn = N - k0 < AT_POS ? N - k0 : AT_POS;
            __syncthreads();                    // the tile before has been read; Q, m and l are whole
            load_tile(sK, base + (int64_t)k0 * 3 * HD + HD, 3 * HD, kn, d, ld, tid);
            load_tile(sV, base + (int64_t)k0 * 3 * HD + 2 * HD, 3 * HD, kn, d, ld, tid);
            __syncthreads();
            {
                const int rb = (wave >> 1) * 32, cb = (wave & 1) * 32;
                const f32x16 s = qk_block(sQ, sK, ld, d, rb, cb, lane);
#pragma unroll
                for (int v = 0; v < 16; ++v) sS[(rb + acc_row(v, lane)) * AT_LS + cb + l31] = scale * s[v];
            }
            __syncthreads();
            {                                   // row tid / 4, columns tid % 4, + 4, ..; rows from N up hold zeros: finite
                const int i = tid >> 2, q = tid & 3;
                float* s = sS + i * AT_LS;
                const float m_old = sM[i], l_old = sL[i];
                float m = m_old, p = 0.f;
                for (int j = q; j < kn; j += 4) m = fmaxf(m, s[j]);
                m = fmaxf(m, __shfl_xor(m, 1, 64));
                m = fmaxf(m, __shfl_xor(m, 2, 64));
                for (int j = q; j < kn; j += 4) {
                    const float e = expf(s[j] - m);
                    s[j] = e;
                    p += e;
                }
                for (int j = kn + q; j < AT_POS; j += 4) s[j] = 0.f;
                const float lt = row_sum4(p, lane);
                if (q == 0) {
                    const float alpha = expf(m_old - m);        // the first tile: exp(-inf) = 0, and l_old = 0
                    sA[i] = alpha;
                    sM[i] = m;
                    sL[i] = alpha * l_old + lt;
                }
            }
            __syncthreads();
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[v] = acc[v] * sA[orb + acc_row(v, lane)];
            const int ke = halves ? (kn < okb + 32 ? kn : okb + 32) : kn;
            acc = mm32(acc, okb, ke, lane, [&](int i, int k) { return sS[(orb + i) * AT_LS + k]; },
                       [&](int k, int e) { return ocb + e < d ? sV[k * ld + ocb + e] : 0.f; });
        }
        if (lse && tid < AT_POS && q0 + tid < N) lse[bh * N + q0 + tid] = sM[tid] + logf(sL[tid]);
        float* o = out + (b * N + q0) * HD + (int64_t)h * d;
        if (halves) {
            if (wave >= 2 && l31 < d) {         // (every wave is past its last read of Q: the barrier after S)
#pragma unroll
                for (int v = 0; v < 16; ++v) sQ[(orb + acc_row(v, lane)) * ld + l31] = acc[v];
            }
            __syncthreads();
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[v] = acc[v] + sQ[(orb + acc_row(v, lane)) * ld + (l31 < d ? l31 : 0)];
        }
        if (ocb + l31 < d && !(halves && wave >= 2)) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = orb + acc_row(v, lane);
                if (q0 + i < N) o[i * HD + ocb + l31] = acc[v] * (1.f / sL[i]);
            }
        }
    }
}

__global__ __launch_bounds__(AT_THREADS) void attn_tiled_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                                 const float* __restrict__ lse, const float* __restrict__ dout,
                                                                 float* __restrict__ dqkv, int64_t items, int N, int H, int d,
                                                                 float scale) {
    extern __shared__ float lds[];
    const int ld = d + 1, tile = AT_POS * ld, npad = (N + AT_POS - 1) / AT_POS * AT_POS;
    float* sdQ = lds;                           // [N_pad][d + 1]
    float* sQ = sdQ + npad * ld;                // after the inner loop: the second halves' partial of dK
    float* sK = sQ + tile;
    float* sV = sK + tile;
    float* sG = sV + tile;                      // dO; after dP: the second halves' partial of dS K; at last that of dV
    float* sP = sG + tile;                      // [64][65]  P, then dS
    float* sLse = sP + AT_SBLK;                 // [N_pad]
    float* sD = sLse + npad;                    // [N_pad]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
    const int rb = (wave >> 1) * 32, cb = (wave & 1) * 32;      // this wave's block of S, dP and dS
    const int64_t HD = (int64_t)H * d;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / H;
        const int h = (int)(item - b * H);
        const int64_t off = b * N * 3 * HD + (int64_t)h * d, ooff = b * N * HD + (int64_t)h * d;
        __syncthreads();                        // the item before has been read
        for (int i = tid; i < npad; i += AT_THREADS) sLse[i] = i < N ? lse[item * N + i] : 0.f;
        for (int i0 = 0; i0 < N; i0 += AT_POS) {        // D_i: row tid / 4, float4s tid % 4, + 4, ..; added one by one
            const int i = i0 + (tid >> 2), q = tid & 3;
            float p = 0.f;
            if (i < N) {
                const float* o = out + ooff + i * HD;
                const float* g = dout + ooff + i * HD;
                for (int c = 4 * q; c < d; c += 16) {
                    const float4 ov = *reinterpret_cast<const float4*>(o + c), gv = *reinterpret_cast<const float4*>(g + c);
                    p += gv.x * ov.x;
                    p += gv.y * ov.y;
                    p += gv.z * ov.z;
                    p += gv.w * ov.w;
                }
            }
            const float s = row_sum4(p, lane);
            if (q == 0) sD[i] = s;
        }
        float* dq = dqkv + off;
        for (int k0 = 0; k0 < N; k0 += AT_POS) {
            const int kn = N - k0 < AT_POS ? N - k0 : AT_POS;
            __syncthreads();                    // the key tile before has been read
            load_tile(sK, qkv + off + (int64_t)k0 * 3 * HD + HD, 3 * HD, kn, d, ld, tid);
            load_tile(sV, qkv + off + (int64_t)k0 * 3 * HD + 2 * HD, 3 * HD, kn, d, ld, tid);
            f32x16 dk = {}, dv = {};
            for (int i0 = 0; i0 < N; i0 += AT_POS) {
                const int in = N - i0 < AT_POS ? N - i0 : AT_POS;
                __syncthreads();                // the query tile before has been read
                load_tile(sQ, qkv + off + (int64_t)i0 * 3 * HD, 3 * HD, in, d, ld, tid);
                load_tile(sG, dout + ooff + (int64_t)i0 * HD, HD, in, d, ld, tid);
                __syncthreads();
                {                               // P = exp(S - lse), zeros from N on in both indices
                    const f32x16 acc = qk_block(sQ, sK, ld, d, rb, cb, lane);
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int i = rb + acc_row(v, lane), j = cb + l31;
                        sP[i * AT_LS + j] = (i < in && j < kn) ? expf(scale * acc[v] - sLse[i0 + i]) : 0.f;
                    }
                }
                __syncthreads();
                // dV_j += P^T dO_i
                dv = pos_accumulate(dv, d, in, wave, lane, [&](int j, int i) { return sP[i * AT_LS + j]; },
                                    [&](int i, int e) { return e < d ? sG[i * ld + e] : 0.f; });
                f32x16 dp = {};                 // dP = dO_i V_j^T
                dp = mm32(dp, 0, d, lane, [&](int i, int e) { return sG[(rb + i) * ld + e]; },
                          [&](int e, int j) { return sV[(cb + j) * ld + e]; });
                __syncthreads();                // P and dO have been read
#pragma unroll
                for (int v = 0; v < 16; ++v) {  // dS = scale (P (dP - D)) over P
                    const int i = rb + acc_row(v, lane), j = cb + l31;
                    sP[i * AT_LS + j] = scale * (sP[i * AT_LS + j] * (dp[v] - sD[i0 + i]));
                }
                __syncthreads();
                // dK_j += dS^T Q_i
                dk = pos_accumulate(dk, d, in, wave, lane, [&](int j, int i) { return sP[i * AT_LS + j]; },
                                    [&](int i, int e) { return e < d ? sQ[i * ld + e] : 0.f; });
                // dQ_i (+)= dS K_j
                float* t = sdQ + i0 * ld;
                const bool first = k0 == 0;
                pos_product(d, kn, sG, ld, wave, lane, [&](int i, int j) { return sP[i * AT_LS + j]; },
                            [&](int j, int e) { return e < d ? sK[j * ld + e] : 0.f; },
                            [&](int i, int e, float v) { t[i * ld + e] = first ? v : t[i * ld + e] + v; });
            }
            __syncthreads();                    // the last query tile has been read
            pos_store(dk, d, kn, sQ, ld, dq + (int64_t)k0 * 3 * HD + HD, 3 * HD, wave, lane);
            pos_store(dv, d, kn, sG, ld, dq + (int64_t)k0 * 3 * HD + 2 * HD, 3 * HD, wave, lane);
        }
        __syncthreads();                        // dQ is whole
        const int d4 = d >> 2;
        for (int i = tid; i < N * d4; i += AT_THREADS) {
            const int r = i / d4, c = (i - r * d4) * 4;
            const float* s = sdQ + r * ld + c;
            *reinterpret_cast<float4*>(dq + (int64_t)r * 3 * HD + c) = make_float4(s[0], s[1], s[2], s[3]);
        }
    }
}

// ---- the coordinate channels -------------------------------------------------------------------------------------------

constexpr int EC_MAX_CHANNELS = 1024, EC_MAX_SIDE = 1 << 16, EC_MAX_BATCH = 1 << 20;

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

__device__ __forceinline__ float coord(int pos, int side) {
    return side > 1 ? (float)(2 * pos - (side - 1)) / (float)(side - 1) : 0.f;
}

__global__ __launch_bounds__(AT_THREADS) void entity_coords_fwd_kernel(const float4* __restrict__ x, int h, int w, int c4,
                                                                       int64_t total, float4* __restrict__ y) {
    const int64_t step = (int64_t)gridDim.x * AT_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x; t < total; t += step) {
        int64_t p, q, b;
        int c, j, i;
        split_index(t, c4 + 1, p, c);
        if (c < c4) {
            y[t] = x[p * c4 + c];
        } else {
            split_index(p, w, q, j);
            split_index(q, h, b, i);
            y[t] = make_float4(coord(j, w), coord(i, h), 0.f, 0.f);
        }
    }
}

// g and g_in may be one buffer: a thread reads its own float4 before it writes it and touches no other
__global__ __launch_bounds__(AT_THREADS) void entity_coords_bwd_kernel(const float4* g, const float4* __restrict__ dy,
                                                                       const float4* __restrict__ mask, int c4,
                                                                       int64_t total, float4* g_in) {
    const int64_t step = (int64_t)gridDim.x * AT_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x; t < total; t += step) {
        int64_t p;
        int c;
        split_index(t, c4, p, c);
        const float4 u = g[t], v = dy[p * (c4 + 1) + c];
        float4 s = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
        if (mask) {
            const float4 m = mask[t];
            s = make_float4(m.x > 0.f ? s.x : 0.f, m.y > 0.f ? s.y : 0.f, m.z > 0.f ? s.z : 0.f, m.w > 0.f ? s.w : 0.f);
        }
        g_in[t] = s;
    }
}

int check_attn(int64_t batch, int32_t n_pos, int32_t n_heads, int32_t head_dim, int32_t max_pos = ARL_ATTN_MAX_POS) {
    if (batch < 1 || batch > ARL_ATTN_MAX_BATCH || n_pos < 1 || n_pos > max_pos || head_dim < 4 ||
        head_dim > ARL_ATTN_MAX_HEAD_DIM || (head_dim & 3) || n_heads < 1 ||
        (int64_t)n_heads * head_dim > ARL_ATTN_MAX_WIDTH) {
        arl::set_error("attention: need 1 <= batch <= 2^24, 1 <= n_pos <= %d, head_dim a multiple of 4 in 4 .. 64, "
                       "n_heads >= 1 and n_heads * head_dim <= 256", max_pos);
        return ARL_E_RANGE;
    }
    return 0;
}

size_t attn_lds_bytes(int d, bool bwd) {
    return ((size_t)(bwd ? 4 : 3) * AT_POS * (d + 1) + (bwd ? 2 : 1) * AT_SBLK + (bwd ? 2 : 1) * AT_POS) * sizeof(float);
}

size_t attn_tiled_lds_bytes(int n_pos, int d, bool bwd) {
    const size_t npad = (size_t)(n_pos + AT_POS - 1) / AT_POS * AT_POS;
    return bwd ? ((npad + 4 * AT_POS) * (d + 1) + AT_SBLK + 2 * npad) * sizeof(float)
               : ((size_t)3 * AT_POS * (d + 1) + AT_SBLK + 3 * AT_POS) * sizeof(float);
}


int check_coords(int64_t batch, int32_t h, int32_t w, int32_t channels) {
    if (batch < 1 || batch > EC_MAX_BATCH || h < 1 || h > EC_MAX_SIDE || w < 1 || w > EC_MAX_SIDE || channels < 4 ||
        channels > EC_MAX_CHANNELS || (channels & 3)) {
        arl::set_error("entity_coords: need 1 <= batch <= 2^20, 1 <= h, w <= 2^16 and channels a multiple of 4 in 4 .. 1024");
        return ARL_E_RANGE;
    }
    return 0;
}

}  // namespace

extern "C" int arl_attn_fwd(const float* qkv, float* out, float* lse_or_null, int64_t batch, int32_t n_pos, int32_t n_heads,
                            int32_t head_dim, float scale, void* stream) {
    ARL_REQUIRE(qkv && out, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(scale), ARL_E_ARG, "scale must be finite");
    int rc = check_attn(batch, n_pos, n_heads, head_dim);
    if (rc) return rc;
    const int64_t items = batch * n_heads, n_out = batch * n_pos * n_heads * head_dim;
    const arl::Span in[1] = {{qkv, 3 * n_out * 4}};
    const arl::Span outs[2] = {{out, n_out * 4}, {lse_or_null, items * n_pos * 4}};
    if (!arl::check_disjoint("arl_attn_fwd", in, 1, outs, 2)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned16(qkv) && arl::aligned16(out) && arl::aligned4(lse_or_null), ARL_E_ALIGN,
                "qkv and out 16-byte, lse 4-byte aligned");
    const size_t lds = attn_lds_bytes(head_dim, false);
    rc = raise_lds(reinterpret_cast<const void*>(attn_fwd_kernel), lds, "attn_fwd_kernel");
    if (rc) return rc;
    const unsigned grid = (unsigned)(items < ARL_ATTN_MAX_GRID ? items : ARL_ATTN_MAX_GRID);
    hipLaunchKernelGGL(attn_fwd_kernel, dim3(grid), dim3(AT_THREADS), lds, (hipStream_t)stream, qkv, out, lse_or_null,
                       items, (int)n_pos, (int)n_heads, (int)head_dim, scale);
    return arl::check_launch("attn_fwd_kernel");
}

extern "C" int arl_attn_bwd(const float* qkv, const float* out, const float* lse, const float* dout, float* dqkv,
                            int64_t batch, int32_t n_pos, int32_t n_heads, int32_t head_dim, float scale, void* stream) {
    ARL_REQUIRE(qkv && out && lse && dout && dqkv, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(scale), ARL_E_ARG, "scale must be finite");
    int rc = check_attn(batch, n_pos, n_heads, head_dim);
    if (rc) return rc;
    const int64_t items = batch * n_heads, n_out = batch * n_pos * n_heads * head_dim;
    const arl::Span in[4] = {{qkv, 3 * n_out * 4}, {out, n_out * 4}, {lse, items * n_pos * 4}, {dout, n_out * 4}};
    const arl::Span outs[1] = {{dqkv, 3 * n_out * 4}};
    if (!arl::check_disjoint("arl_attn_bwd", in, 4, outs, 1)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned16(qkv) && arl::aligned16(out) && arl::aligned16(dout) && arl::aligned16(dqkv) &&
                    arl::aligned4(lse), ARL_E_ALIGN, "qkv, out, dout and dqkv 16-byte, lse 4-byte aligned");
    const size_t lds = attn_lds_bytes(head_dim, true);
    rc = raise_lds(reinterpret_cast<const void*>(attn_bwd_kernel), lds, "attn_bwd_kernel");
    if (rc) return rc;
    const unsigned grid = (unsigned)(items < ARL_ATTN_MAX_GRID ? items : ARL_ATTN_MAX_GRID);
    hipLaunchKernelGGL(attn_bwd_kernel, dim3(grid), dim3(AT_THREADS), lds, (hipStream_t)stream, qkv, out, lse, dout, dqkv,
                       items, (int)n_pos, (int)n_heads, (int)head_dim, scale);
    return arl::check_launch("attn_bwd_kernel");
}

extern "C" int arl_attn_tiled_fwd(const float* qkv, float* out, float* lse_or_null, int64_t batch, int32_t n_pos,
                                  int32_t n_heads, int32_t head_dim, float scale, void* stream) {
    ARL_REQUIRE(qkv && out, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(scale), ARL_E_ARG, "scale must be finite");
    int rc = check_attn(batch, n_pos, n_heads, head_dim, ARL_ATTN_TILED_MAX_POS);
    if (rc) return rc;
    const int64_t heads = batch * n_heads, items = heads * ((n_pos + AT_POS - 1) / AT_POS),
                  n_out = batch * n_pos * n_heads * head_dim;
    const arl::Span in[1] = {{qkv, 3 * n_out * 4}};
    const arl::Span outs[2] = {{out, n_out * 4}, {lse_or_null, heads * n_pos * 4}};
    if (!arl::check_disjoint("arl_attn_tiled_fwd", in, 1, outs, 2)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned16(qkv) && arl::aligned16(out) && arl::aligned4(lse_or_null), ARL_E_ALIGN,
                "qkv and out 16-byte, lse 4-byte aligned");
    const size_t lds = attn_tiled_lds_bytes(n_pos, head_dim, false);
    rc = raise_lds(reinterpret_cast<const void*>(attn_tiled_fwd_kernel), lds, "attn_tiled_fwd_kernel");
    if (rc) return rc;
    const unsigned grid = (unsigned)(items < ARL_ATTN_MAX_GRID ? items : ARL_ATTN_MAX_GRID);
    hipLaunchKernelGGL(attn_tiled_fwd_kernel, dim3(grid), dim3(AT_THREADS), lds, (hipStream_t)stream, qkv, out, lse_or_null,
                       items, (int)n_pos, (int)n_heads, (int)head_dim, scale);
    return arl::check_launch("attn_tiled_fwd_kernel");
}

extern "C" int arl_attn_tiled_bwd(const float* qkv, const float* out, const float* lse, const float* dout, float* dqkv,
                                  int64_t batch, int32_t n_pos, int32_t n_heads, int32_t head_dim, float scale,
                                  void* stream) {
    ARL_REQUIRE(qkv && out && lse && dout && dqkv, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(scale), ARL_E_ARG, "scale must be finite");
    int rc = check_attn(batch, n_pos, n_heads, head_dim, ARL_ATTN_TILED_MAX_POS);
    if (rc) return rc;
    const int64_t items = batch * n_heads, n_out = batch * n_pos * n_heads * head_dim;
    const arl::Span in[4] = {{qkv, 3 * n_out * 4}, {out, n_out * 4}, {lse, items * n_pos * 4}, {dout, n_out * 4}};
    const arl::Span outs[1] = {{dqkv, 3 * n_out * 4}};
    if (!arl::check_disjoint("arl_attn_tiled_bwd", in, 4, outs, 1)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned16(qkv) && arl::aligned16(out) && arl::aligned16(dout) && arl::aligned16(dqkv) &&
                    arl::aligned4(lse), ARL_E_ALIGN, "qkv, out, dout and dqkv 16-byte, lse 4-byte aligned");
    const size_t lds = attn_tiled_lds_bytes(n_pos, head_dim, true);
    rc = raise_lds(reinterpret_cast<const void*>(attn_tiled_bwd_kernel), lds, "attn_tiled_bwd_kernel");
    if (rc) return rc;
    const unsigned grid = (unsigned)(items < ARL_ATTN_MAX_GRID ? items : ARL_ATTN_MAX_GRID);
    hipLaunchKernelGGL(attn_tiled_bwd_kernel, dim3(grid), dim3(AT_THREADS), lds, (hipStream_t)stream, qkv, out, lse, dout,
                       dqkv, items, (int)n_pos, (int)n_heads, (int)head_dim, scale);
    return arl::check_launch("attn_tiled_bwd_kernel");
}

extern "C" int arl_entity_coords_fwd(const float* x, int64_t batch, int32_t h, int32_t w, int32_t channels, float* y,
                                     void* stream) {
    ARL_REQUIRE(x && y, ARL_E_ARG, "null pointer");
    int rc = check_coords(batch, h, w, channels);
    if (rc) return rc;
    const int64_t pixels = batch * h * w;
    ARL_REQUIRE(!arl::overlap(x, pixels * channels * 4, y, pixels * (channels + 4) * 4), ARL_E_ARG, "y must not overlap x");
    ARL_REQUIRE(arl::aligned16(x) && arl::aligned16(y), ARL_E_ALIGN, "16-byte alignment");
    const int c4 = channels >> 2;
    const int64_t total = pixels * (c4 + 1);
    hipLaunchKernelGGL(entity_coords_fwd_kernel, dim3(arl::stream_grid(total, AT_THREADS)), dim3(AT_THREADS), 0,
                       (hipStream_t)stream, (const float4*)x, (int)h, (int)w, c4, total, (float4*)y);
    return arl::check_launch("entity_coords_fwd_kernel");
}

extern "C" int arl_entity_coords_bwd(const float* g, const float* d_y, const float* mask_or_null, int64_t batch, int32_t h,
                                     int32_t w, int32_t channels, float* g_in, void* stream) {
    ARL_REQUIRE(g && d_y && g_in, ARL_E_ARG, "null pointer");
    int rc = check_coords(batch, h, w, channels);
    if (rc) return rc;
    const int64_t pixels = batch * h * w, n = pixels * channels * 4;
    ARL_REQUIRE(!arl::overlap(g_in, n, d_y, pixels * (channels + 4) * 4) &&
                    !(mask_or_null && arl::overlap(g_in, n, mask_or_null, n)) &&
                    (g_in == g || !arl::overlap(g_in, n, g, n)),
                ARL_E_ARG, "g_in must not overlap d_y or mask, and g only as the same buffer");
    ARL_REQUIRE(arl::aligned16(g) && arl::aligned16(d_y) && arl::aligned16(mask_or_null) && arl::aligned16(g_in),
                ARL_E_ALIGN, "16-byte alignment");
    const int c4 = channels >> 2;
    const int64_t total = pixels * c4;
    hipLaunchKernelGGL(entity_coords_bwd_kernel, dim3(arl::stream_grid(total, AT_THREADS)), dim3(AT_THREADS), 0,
                       (hipStream_t)stream, (const float4*)g, (const float4*)d_y, (const float4*)mask_or_null, c4, total,
                       (float4*)g_in);
    return arl::check_launch("entity_coords_bwd_kernel");
}
