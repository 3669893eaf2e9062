// Windowed causal multi-head attention over TIME, forward and backward, for gfx950: the memory of the attention-memory
// policy (policies/atari_attn_memory_policy.py; Transformer-XL's cached segment, GTrXL's use of it in RL).
//
//   arl_tattn_fwd       per segment and head: T queries against a context of L = M + T rows (M stored embeddings' K / V,
//                       then the segment's own); query t sees the context rows c with age a = M + t - c in 0 .. M;
//                       s = scale q.k + rel[h][a] for a live entry, rel[h][a] alone for a dead one (older than the last
//                       reset before t), P = softmax over the window, O = sum over the live entries of P v
//   arl_tattn_bwd       S again (the forward's instructions), P = exp(S - lse), D, dV, dP, dS, dQ, dK; per item one
//                       partial of d rel
//   arl_tattn_rel_fold  d rel = the partials added in ascending segment order
//   arl_tattn_shift     serving: window = [state ; e], state <- window[1:]   (float4 streaming, csrc/resnet.hip's kind)
//
// One work item is one (segment, head); a workgroup of four waves walks the items grid-stride.  T <= 64, so the queries
// are ONE tile of csrc/attention.hip's kind and only the context is tiled (at most two tiles of 64 rows): the forward is
// attn_tiled_fwd_kernel's online soft-max with Q and K / V read from different tensors, and band, liveness and rel
// applied as the scores leave the accumulators; the backward keeps dO, Q and the dQ sums resident, and since there is
// one query tile every context tile's dK / dV is whole after one pass.  Tiles, products, thread layouts and the orders of
// summation are attention_dev.h's.  The per-row reset horizon R_t comes from one ballot over the segment's flags.  The
// union of the T windows is the whole context, so no context tile lies outside every window: none is skipped.
// One writer per output element, no atomics, nothing depends on the grid: two launches give the same bits.
// Compiled with -ffp-contract=off and without packed fp32 instructions.
#include "arl_common.h"
#include "attention_dev.h"

#include <math.h>

namespace {

constexpr int TA_REL = ARL_TATTN_MAX_MEM + 4;   // floats reserved for one head's rel row

// sR[t] = R_t = 1 + the last r < t whose flag is set, 0 if none (t < T <= 64); called by every thread of wave 0
__device__ __forceinline__ void reset_rows(int* sR, const uint8_t* __restrict__ reset, const int32_t* __restrict__ idx,
                                           int64_t seg, int T, int lane) {
    bool f = false;
    if (reset && lane < T) {
        const int64_t r = seg * T + lane;
        f = reset[idx ? (int64_t)idx[r] : r] != 0;
    }
    const unsigned long long before = __ballot(f) & ((1ull << lane) - 1ull);
    sR[lane] = before ? 64 - __clzll((long long)before) : 0;
}

// the score of query i against context row c (this wave's accumulator element qk), and whether the entry is live;
// -inf outside the window.  Both passes form it with these instructions.
__device__ __forceinline__ float band_score(float qk, float scale, int i, int c, int M, int Ri, const float* sRel, bool& live) {
    const int a = M + i - c;
    live = Ri == 0 || c >= M + Ri;
    if (a < 0 || a > M) return -INFINITY;
    return live ? scale * qk + sRel[a] : sRel[a];
}

__global__ __launch_bounds__(AT_THREADS, 2) void tattn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                               const float* __restrict__ rel, const uint8_t* __restrict__ reset,
                                                               const int32_t* __restrict__ idx, float* __restrict__ out,
                                                               float* __restrict__ lse, int64_t items, int T, int M, int H,
                                                               int d, float scale) {
    extern __shared__ float lds[];
    const int ld = d + 1, tile = AT_POS * ld, L = M + T;
    float* sQ = lds;                            // [64][d + 1]; after the last tile: the second halves' partial of O
    float* sK = sQ + tile;
    float* sV = sK + tile;
    float* sS = sV + tile;                      // [64][65]  S, then exp(S - m) of the live entries
    float* sM = sS + AT_SBLK;                   // [64]      the running maximum
    float* sL = sM + AT_POS;                    // [64]      the running sum
    float* sA = sL + AT_POS;                    // [64]      this tile's alpha
    float* sRel = sA + AT_POS;                  // [M + 1]   rel[h]
    int* sR = reinterpret_cast<int*>(sRel + TA_REL);    // [64]  R_t
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
    const bool halves = d <= 32;
    const int orb = (halves ? wave & 1 : wave >> 1) * 32, ocb = halves ? 0 : (wave & 1) * 32;
    const int64_t HD = (int64_t)H * d;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t s = item / H;
        const int h = (int)(item - s * H);
        const float* kb = kv + s * L * 2 * HD + (int64_t)h * d;
        __syncthreads();                        // the item before has been read
        load_tile(sQ, q + s * T * HD + (int64_t)h * d, HD, T, d, ld, tid);
        if (wave == 0) {
            sM[lane] = -INFINITY;
            sL[lane] = 0.f;
            reset_rows(sR, reset, idx, s, T, lane);
        }
        for (int a = tid; a <= M; a += AT_THREADS) sRel[a] = rel[h * (M + 1) + a];
        f32x16 acc = {};
        for (int k0 = 0; k0 < L; k0 += AT_POS) {
            const int kn = L - k0 < AT_POS ? L - k0 : AT_POS;
            __syncthreads();                    // the tile before has been read; Q, m, l, R and rel are whole
            load_tile(sK, kb + (int64_t)k0 * 2 * HD, 2 * HD, kn, d, ld, tid);
            load_tile(sV, kb + (int64_t)k0 * 2 * HD + HD, 2 * HD, kn, d, ld, tid);
            __syncthreads();
            {
                const int rb = (wave >> 1) * 32, cb = (wave & 1) * 32;
                const f32x16 sc = qk_block(sQ, sK, ld, d, rb, cb, lane);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int i = rb + acc_row(v, lane);
                    bool live;
                    sS[i * AT_LS + cb + l31] = band_score(sc[v], scale, i, k0 + cb + l31, M, sR[i], sRel, live);
                }
            }
            __syncthreads();
            {                                   // row tid / 4, columns tid % 4, + 4, ..
                const int i = tid >> 2, qd = tid & 3;
                float* sr = sS + i * AT_LS;
                if (i < T) {                    // (uniform over the four threads of a row)
                    // context row i lies in tile 0 and in row i's window: m is finite from the first tile on
                    const float m_old = sM[i], l_old = sL[i];
                    const int first_live = sR[i] == 0 ? 0 : M + sR[i];
                    float m = m_old, p = 0.f;
                    for (int j = qd; j < kn; j += 4) m = fmaxf(m, sr[j]);
                    m = fmaxf(m, __shfl_xor(m, 1, 64));
                    m = fmaxf(m, __shfl_xor(m, 2, 64));
                    for (int j = qd; j < kn; j += 4) {
                        const float e = expf(sr[j] - m);
                        p += e;
                        sr[j] = k0 + j >= first_live ? e : 0.f;         // a dead entry's value is zero
                    }
                    for (int j = kn + qd; j < AT_POS; j += 4) sr[j] = 0.f;
                    const float lt = row_sum4(p, lane);
                    if (qd == 0) {
                        const float alpha = expf(m_old - m);            // the first tile: exp(-inf) = 0, and l_old = 0
                        sA[i] = alpha;
                        sM[i] = m;
                        sL[i] = alpha * l_old + lt;
                    }
                } else {
                    for (int j = qd; j < AT_POS; j += 4) sr[j] = 0.f;
                    if (qd == 0) sA[i] = 0.f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[v] = acc[v] * sA[orb + acc_row(v, lane)];
            acc = pos_accumulate(acc, d, kn, wave, lane, [&](int i, int k) { return sS[i * AT_LS + k]; },
                                 [&](int k, int e) { return e < d ? sV[k * ld + e] : 0.f; });
        }
        if (lse && tid < T) lse[item * T + tid] = sM[tid] + logf(sL[tid]);
        float* o = out + s * T * HD + (int64_t)h * d;
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
                if (i < T) o[i * HD + ocb + l31] = acc[v] * (1.f / sL[i]);
            }
        }
    }
}

// (launch bounds of two workgroups per compute unit cost this kernel 44 bytes of scratch per lane: one, and none)
__global__ __launch_bounds__(AT_THREADS) void tattn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                               const float* __restrict__ rel, const uint8_t* __restrict__ reset,
                                                               const int32_t* __restrict__ idx, const float* __restrict__ out,
                                                               const float* __restrict__ lse, const float* __restrict__ dout,
                                                               float* __restrict__ dq, float* __restrict__ dkv,
                                                               float* __restrict__ drel_parts, int64_t items, int T, int M,
                                                               int H, int d, float scale) {
    extern __shared__ float lds[];
    const int ld = d + 1, tile = AT_POS * ld, L = M + T;
    float* sQ = lds;
    float* sG = sQ + tile;                      // dO
    float* sdQ = sG + tile;                     // the dQ sums, resident until whole
    float* sK = sdQ + tile;                     // after dQ: the second halves' partial of dV
    float* sV = sK + tile;                      // after dP: the second halves' partial of dS K, then that of dK
    float* sP = sV + tile;                      // [64][65]  P of the live entries, then their scale dS
    float* sW = sP + AT_SBLK;                   // [64][65]  P (dP - D) of every entry in the window: d rel's terms
    float* sLse = sW + AT_SBLK;                 // [64]
    float* sD = sLse + AT_POS;                  // [64]
    float* sRel = sD + AT_POS;                  // [M + 1]
    int* sR = reinterpret_cast<int*>(sRel + TA_REL);    // [64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
    const int rb = (wave >> 1) * 32, cb = (wave & 1) * 32;      // this wave's block of S, dP and dS
    const int64_t HD = (int64_t)H * d;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t s = item / H;
        const int h = (int)(item - s * H);
        const int64_t qoff = s * T * HD + (int64_t)h * d, koff = s * L * 2 * HD + (int64_t)h * d;
        __syncthreads();                        // the item before has been read
        load_tile(sQ, q + qoff, HD, T, d, ld, tid);
        load_tile(sG, dout + qoff, HD, T, d, ld, tid);
        if (wave == 0) {
            sLse[lane] = lane < T ? lse[item * T + lane] : 0.f;
            reset_rows(sR, reset, idx, s, T, lane);
        }
        for (int a = tid; a <= M; a += AT_THREADS) sRel[a] = rel[h * (M + 1) + a];
        {                                       // D_i: row tid / 4, float4s tid % 4, + 4, ..; the products added one by one
            const int i = tid >> 2, qd = tid & 3;
            float p = 0.f;
            if (i < T) {
                const float* o = out + qoff + i * HD;
                const float* g = dout + qoff + i * HD;
                for (int c = 4 * qd; c < d; c += 16) {
                    const float4 ov = *reinterpret_cast<const float4*>(o + c), gv = *reinterpret_cast<const float4*>(g + c);
                    p += gv.x * ov.x;
                    p += gv.y * ov.y;
                    p += gv.z * ov.z;
                    p += gv.w * ov.w;
                }
            }
            const float t = row_sum4(p, lane);
            if (qd == 0) sD[i] = t;
        }
        float drel = 0.f;                       // thread a <= M: the sum of this item's P (dP - D) at age a, t ascending
        for (int k0 = 0; k0 < L; k0 += AT_POS) {
            const int kn = L - k0 < AT_POS ? L - k0 : AT_POS;
            __syncthreads();                    // the context tile before has been read
            load_tile(sK, kv + koff + (int64_t)k0 * 2 * HD, 2 * HD, kn, d, ld, tid);
            load_tile(sV, kv + koff + (int64_t)k0 * 2 * HD + HD, 2 * HD, kn, d, ld, tid);
            __syncthreads();
            f32x16 pf;                          // P of every entry in the window, dead ones included
            unsigned live_bits = 0;
            {
                const f32x16 sc = qk_block(sQ, sK, ld, d, rb, cb, lane);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int i = rb + acc_row(v, lane), j = cb + l31;
                    bool live;
                    const float x = band_score(sc[v], scale, i, k0 + j, M, sR[i], sRel, live);
                    pf[v] = (i < T && j < kn) ? expf(x - sLse[i]) : 0.f;        // expf(-inf) = 0 outside the window
                    live_bits |= (live ? 1u : 0u) << v;
                    sP[i * AT_LS + j] = live ? pf[v] : 0.f;
                }
            }
            __syncthreads();
            // dV_j = P^T dO over the live entries
            f32x16 dv = {};
            dv = pos_accumulate(dv, d, T, wave, lane, [&](int j, int i) { return sP[i * AT_LS + j]; },
                                [&](int i, int e) { return e < d ? sG[i * ld + e] : 0.f; });
            f32x16 dp = {};                     // dP = dO V_j^T
            dp = mm32(dp, 0, d, lane, [&](int i, int e) { return sG[(rb + i) * ld + e]; },
                      [&](int e, int j) { return sV[(cb + j) * ld + e]; });
            __syncthreads();                    // P and V have been read
#pragma unroll
            for (int v = 0; v < 16; ++v) {      // dS = P (dP - D), a dead entry's dP is zero; scale dS of the live over P
                const int i = rb + acc_row(v, lane), j = cb + l31;
                const bool live = (live_bits >> v) & 1u;
                const float ds = pf[v] * ((live ? dp[v] : 0.f) - sD[i]);
                sW[i * AT_LS + j] = ds;
                sP[i * AT_LS + j] = live ? scale * ds : 0.f;
            }
            __syncthreads();
            if (tid <= M) {
                for (int t = 0; t < T; ++t) {
                    const int j = M + t - tid - k0;
                    if (j >= 0 && j < kn) drel += sW[t * AT_LS + j];
                }
            }
            // dK_j = dS^T Q
            f32x16 dk = {};
            dk = pos_accumulate(dk, d, T, wave, lane, [&](int j, int i) { return sP[i * AT_LS + j]; },
                                [&](int i, int e) { return e < d ? sQ[i * ld + e] : 0.f; });
            // dQ (+)= dS K_j
            const bool first = k0 == 0;
            pos_product(d, kn, sV, ld, wave, lane, [&](int i, int j) { return sP[i * AT_LS + j]; },
                        [&](int j, int e) { return e < d ? sK[j * ld + e] : 0.f; },
                        [&](int i, int e, float v) { sdQ[i * ld + e] = first ? v : sdQ[i * ld + e] + v; });
            __syncthreads();                    // K and dQ's partial have been read
            float* dkp = dkv + koff + (int64_t)k0 * 2 * HD;
            pos_store(dk, d, kn, sV, ld, dkp, 2 * HD, wave, lane);
            pos_store(dv, d, kn, sK, ld, dkp + HD, 2 * HD, wave, lane);
        }
        __syncthreads();                        // dQ is whole
        const int d4 = d >> 2;
        for (int i = tid; i < T * d4; i += AT_THREADS) {
            const int r = i / d4, c = (i - r * d4) * 4;
            const float* t = sdQ + r * ld + c;
            *reinterpret_cast<float4*>(dq + qoff + (int64_t)r * HD + c) = make_float4(t[0], t[1], t[2], t[3]);
        }
        if (tid <= M) drel_parts[item * (M + 1) + tid] = drel;
    }
}

// drel[k] = parts[0][k] + parts[1][k] + .. in ascending segment order, k over n_heads (M + 1)
__global__ __launch_bounds__(AT_THREADS) void tattn_rel_fold_kernel(const float* __restrict__ parts, int64_t n_seg, int width,
                                                                   float* __restrict__ drel) {
    const int k = blockIdx.x * AT_THREADS + threadIdx.x;
    if (k >= width) return;
    float acc = 0.f;
    for (int64_t s = 0; s < n_seg; ++s) acc += parts[s * width + k];
    drel[k] = acc;
}

// one thread per (env, float4 column) walks the M + 1 slots in ascending order: it reads slot m before it writes slot
// m - 1 and touches no other thread's elements, so the state shifts in place
__global__ __launch_bounds__(AT_THREADS) void tattn_shift_kernel(float4* state, const float4* __restrict__ e, int64_t total,
                                                                int M, int e4, float4* __restrict__ window,
                                                                float4* __restrict__ prev) {
    const int64_t step = (int64_t)gridDim.x * AT_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x; t < total; t += step) {
        const int64_t b = t / e4;
        const int c = (int)(t - b * e4);
        float4* st = state + b * M * e4 + c;
        float4* w = window + b * (M + 1) * e4 + c;
        for (int m = 0; m <= M; ++m) {
            const float4 v = m < M ? st[(int64_t)m * e4] : e[t];
            w[(int64_t)m * e4] = v;
            if (m < M && prev) prev[b * M * e4 + (int64_t)m * e4 + c] = v;
            if (m > 0) st[(int64_t)(m - 1) * e4] = v;
        }
    }
}

int check_tattn(int64_t n_seg, int32_t T, int32_t M, int32_t H, int32_t d) {
    if (n_seg < 1 || n_seg > ARL_ATTN_MAX_BATCH || T < 1 || T > ARL_TATTN_MAX_STEPS || M < 1 || M > ARL_TATTN_MAX_MEM ||
        d < 4 || d > ARL_ATTN_MAX_HEAD_DIM || (d & 3) || H < 1 || (int64_t)H * d > ARL_ATTN_MAX_WIDTH) {
        arl::set_error("windowed attention: need 1 <= n_seg <= 2^24, 1 <= seg_len <= %d, 1 <= mem_len <= %d, head_dim a "
                       "multiple of 4 in 4 .. 64, n_heads >= 1 and n_heads * head_dim <= 256", ARL_TATTN_MAX_STEPS,
                       ARL_TATTN_MAX_MEM);
        return ARL_E_RANGE;
    }
    return 0;
}

size_t tattn_lds_bytes(int d, bool bwd) {
    return ((size_t)(bwd ? 5 : 3) * AT_POS * (d + 1) + (bwd ? 2 : 1) * AT_SBLK + (bwd ? 3 : 4) * AT_POS + TA_REL) * sizeof(float);
}

}  // namespace

extern "C" int arl_tattn_fwd(const float* q, const float* kv, const float* rel, const uint8_t* reset_or_null,
                             const int32_t* idx_or_null, int64_t n_seg, int32_t seg_len, int32_t mem_len, int32_t n_heads,
                             int32_t head_dim, float scale, float* out, float* lse_or_null, void* stream) {
    ARL_REQUIRE(q && kv && rel && out, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(scale), ARL_E_ARG, "scale must be finite");
    int rc = check_tattn(n_seg, seg_len, mem_len, n_heads, head_dim);
    if (rc) return rc;
    const int64_t items = n_seg * n_heads, n_q = n_seg * seg_len * n_heads * head_dim,
                  n_kv = n_seg * (mem_len + seg_len) * 2 * n_heads * head_dim;
    const arl::Span in[5] = {{q, n_q * 4}, {kv, n_kv * 4}, {rel, (int64_t)n_heads * (mem_len + 1) * 4},
                             {reset_or_null, reset_or_null ? n_seg * seg_len : 0},
                             {idx_or_null, idx_or_null ? n_seg * seg_len * 4 : 0}};
    const arl::Span outs[2] = {{out, n_q * 4}, {lse_or_null, items * seg_len * 4}};
    if (!arl::check_disjoint("arl_tattn_fwd", in, 5, outs, 2)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned16(q) && arl::aligned16(kv) && arl::aligned16(out) && arl::aligned4(rel) &&
                    arl::aligned4(idx_or_null) && arl::aligned4(lse_or_null), ARL_E_ALIGN,
                "q, kv and out 16-byte, rel, idx and lse 4-byte aligned");
    const size_t lds = tattn_lds_bytes(head_dim, false);
    rc = raise_lds(reinterpret_cast<const void*>(tattn_fwd_kernel), lds, "tattn_fwd_kernel");
    if (rc) return rc;
    const unsigned grid = (unsigned)(items < ARL_ATTN_MAX_GRID ? items : ARL_ATTN_MAX_GRID);
    hipLaunchKernelGGL(tattn_fwd_kernel, dim3(grid), dim3(AT_THREADS), lds, (hipStream_t)stream, q, kv, rel, reset_or_null,
                       idx_or_null, out, lse_or_null, items, (int)seg_len, (int)mem_len, (int)n_heads, (int)head_dim, scale);
    return arl::check_launch("tattn_fwd_kernel");
}

extern "C" int arl_tattn_bwd(const float* q, const float* kv, const float* rel, const uint8_t* reset_or_null,
                             const int32_t* idx_or_null, const float* out, const float* lse, const float* dout, float* dq,
                             float* dkv, float* drel_parts, int64_t n_seg, int32_t seg_len, int32_t mem_len,
                             int32_t n_heads, int32_t head_dim, float scale, void* stream) {
    ARL_REQUIRE(q && kv && rel && out && lse && dout && dq && dkv && drel_parts, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(scale), ARL_E_ARG, "scale must be finite");
    int rc = check_tattn(n_seg, seg_len, mem_len, n_heads, head_dim);
    if (rc) return rc;
    const int64_t items = n_seg * n_heads, n_q = n_seg * seg_len * n_heads * head_dim,
                  n_kv = n_seg * (mem_len + seg_len) * 2 * n_heads * head_dim;
    const arl::Span in[8] = {{q, n_q * 4}, {kv, n_kv * 4}, {rel, (int64_t)n_heads * (mem_len + 1) * 4},
                             {reset_or_null, reset_or_null ? n_seg * seg_len : 0},
                             {idx_or_null, idx_or_null ? n_seg * seg_len * 4 : 0},
                             {out, n_q * 4}, {lse, items * seg_len * 4}, {dout, n_q * 4}};
    const arl::Span outs[3] = {{dq, n_q * 4}, {dkv, n_kv * 4}, {drel_parts, items * (mem_len + 1) * 4}};
    if (!arl::check_disjoint("arl_tattn_bwd", in, 8, outs, 3)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned16(q) && arl::aligned16(kv) && arl::aligned16(out) && arl::aligned16(dout) &&
                    arl::aligned16(dq) && arl::aligned16(dkv) && arl::aligned4(rel) && arl::aligned4(idx_or_null) &&
                    arl::aligned4(lse) && arl::aligned4(drel_parts), ARL_E_ALIGN,
                "q, kv, out, dout, dq and dkv 16-byte, rel, idx, lse and drel_parts 4-byte aligned");
    const size_t lds = tattn_lds_bytes(head_dim, true);
    rc = raise_lds(reinterpret_cast<const void*>(tattn_bwd_kernel), lds, "tattn_bwd_kernel");
    if (rc) return rc;
    const unsigned grid = (unsigned)(items < ARL_ATTN_MAX_GRID ? items : ARL_ATTN_MAX_GRID);
    hipLaunchKernelGGL(tattn_bwd_kernel, dim3(grid), dim3(AT_THREADS), lds, (hipStream_t)stream, q, kv, rel, reset_or_null,
                       idx_or_null, out, lse, dout, dq, dkv, drel_parts, items, (int)seg_len, (int)mem_len, (int)n_heads,
                       (int)head_dim, scale);
    return arl::check_launch("tattn_bwd_kernel");
}

extern "C" int arl_tattn_rel_fold(const float* drel_parts, int64_t n_seg, int32_t n_heads, int32_t mem_len, float* drel,
                                  void* stream) {
    ARL_REQUIRE(drel_parts && drel, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n_seg >= 1 && n_seg <= ARL_ATTN_MAX_BATCH && n_heads >= 1 && n_heads <= ARL_ATTN_MAX_WIDTH / 4 &&
                    mem_len >= 1 && mem_len <= ARL_TATTN_MAX_MEM, ARL_E_RANGE,
                "1 <= n_seg <= 2^24, 1 <= n_heads <= 64, 1 <= mem_len <= 64");
    const int width = n_heads * (mem_len + 1);
    ARL_REQUIRE(!arl::overlap(drel, (int64_t)width * 4, drel_parts, n_seg * width * 4), ARL_E_ARG,
                "drel must not overlap drel_parts");
    ARL_REQUIRE(arl::aligned4(drel_parts) && arl::aligned4(drel), ARL_E_ALIGN, "4-byte alignment");
    hipLaunchKernelGGL(tattn_rel_fold_kernel, dim3((width + AT_THREADS - 1) / AT_THREADS), dim3(AT_THREADS), 0,
                       (hipStream_t)stream, drel_parts, n_seg, width, drel);
    return arl::check_launch("tattn_rel_fold_kernel");
}

extern "C" int arl_tattn_shift(float* state, const float* e, int64_t n_env, int32_t mem_len, int32_t width, float* window,
                               float* prev_or_null, void* stream) {
    ARL_REQUIRE(state && e && window, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n_env >= 1 && n_env <= ARL_ATTN_MAX_BATCH && mem_len >= 1 && mem_len <= ARL_TATTN_MAX_MEM && width >= 4 &&
                    width <= 1024 && (width & 3) == 0, ARL_E_RANGE,
                "1 <= n_env <= 2^24, 1 <= mem_len <= 64, width a multiple of 4 in 4 .. 1024");
    const int64_t n_state = n_env * mem_len * width * 4, n_e = n_env * width * 4;
    const arl::Span in[1] = {{e, n_e}};
    const arl::Span outs[3] = {{state, n_state}, {window, n_state + n_e}, {prev_or_null, n_state}};
    if (!arl::check_disjoint("arl_tattn_shift", in, 1, outs, 3)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned16(state) && arl::aligned16(e) && arl::aligned16(window) && arl::aligned16(prev_or_null),
                ARL_E_ALIGN, "16-byte alignment");
    const int e4 = width >> 2;
    const int64_t total = n_env * e4;
    hipLaunchKernelGGL(tattn_shift_kernel, dim3(arl::stream_grid(total, AT_THREADS)), dim3(AT_THREADS), 0,
                       (hipStream_t)stream, (float4*)state, (const float4*)e, total, (int)mem_len, e4, (float4*)window,
                       (float4*)prev_or_null);
    return arl::check_launch("tattn_shift_kernel");
}
