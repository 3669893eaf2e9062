// Device helpers shared by the attention kernels (csrc/attention.hip, csrc/tattention.hip): the fp32 MFMA chain on
// 32 x 32 blocks, the [64][d + 1] tile loader, the [64][d] products over positions and the four-thread row sum.
#pragma once
#include "arl_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int AT_THREADS = 256;
constexpr int AT_POS = ARL_ATTN_MAX_POS;        // rows of every tile
constexpr int AT_LS = AT_POS + 1;               // row stride of S / P / dS
constexpr int AT_SBLK = AT_POS * AT_LS;

// D[i][j] += sum_k a(i, k) b(k, j) over kb <= k < ke (operands from ke on read as 0); i, j = 0 .. 31
template <class FA, class FB>
__device__ __forceinline__ f32x16 mm32(f32x16 acc, int kb, int ke, int lane, FA a, FB b) {
    const int l31 = lane & 31, half = lane >> 5;
    for (int k0 = kb; k0 < ke; k0 += 2) {
        const int k = k0 + half;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k < ke ? a(l31, k) : 0.f, k < ke ? b(k, l31) : 0.f, acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ int acc_row(int v, int lane) { return (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5); }

// rows 0 .. 63 of a tile from src (row n at src + n * row_stride, d floats, 16-byte aligned); rows from N up are zeros
__device__ __forceinline__ void load_tile(float* dst, const float* __restrict__ src, int64_t row_stride, int N, int d,
                                          int ld, int tid) {
    const int d4 = d >> 2;
    for (int i = tid; i < AT_POS * d4; i += AT_THREADS) {
        const int r = i / d4, c = (i - r * d4) * 4;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < N) v = *reinterpret_cast<const float4*>(src + r * row_stride + c);
        float* o = dst + r * ld + c;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
}

// this wave's 32 x 32 block (rb, cb) of Q K^T, not yet scaled: the one instruction sequence of both passes
__device__ __forceinline__ f32x16 qk_block(const float* sQ, const float* sK, int ld, int d, int rb, int cb, int lane) {
    f32x16 acc = {};
    return mm32(acc, 0, d, lane, [&](int i, int k) { return sQ[(rb + i) * ld + k]; },
                [&](int k, int j) { return sK[(cb + j) * ld + k]; });
}

// C[64][d] = A B over the positions k < kn: a(row, k), b(k, col) with row in 0 .. 63 and col in 0 .. 63 (b answers 0 for
// col >= d); emit(row, col, value) once per element with col < d.  d > 32: block (wave / 2, wave % 2).  d <= 32: row
// block wave % 2, positions [32 (wave / 2), 32 (wave / 2) + 32): waves 2 and 3 leave their partial in `part` ([64][ld],
// free at this point), waves 0 and 1 add it to theirs -- first half + second half -- and emit.  All four waves call.
template <class FA, class FB, class FE>
__device__ __forceinline__ void pos_product(int d, int kn, float* part, int ld, int wave, int lane, FA a, FB b, FE emit) {
    const int l31 = lane & 31;
    f32x16 acc = {};
    if (d > 32) {
        const int rb = (wave >> 1) * 32, cb = (wave & 1) * 32;
        acc = mm32(acc, 0, kn, lane, [&](int i, int k) { return a(rb + i, k); }, [&](int k, int j) { return b(k, cb + j); });
        if (cb + l31 < d) {
#pragma unroll
            for (int v = 0; v < 16; ++v) emit(rb + acc_row(v, lane), cb + l31, acc[v]);
        }
        return;
    }
    const int rb = (wave & 1) * 32, half = wave >> 1;
    const int kb = half * 32, ke = kn < kb + 32 ? kn : kb + 32;         // (an empty half leaves zeros)
    acc = mm32(acc, kb, ke, lane, [&](int i, int k) { return a(rb + i, k); }, [&](int k, int j) { return b(k, j); });
    if (half == 1 && l31 < d) {
#pragma unroll
        for (int v = 0; v < 16; ++v) part[(rb + acc_row(v, lane)) * ld + l31] = acc[v];
    }
    __syncthreads();
    if (half == 0 && l31 < d) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = rb + acc_row(v, lane);
            emit(r, l31, acc[v] + part[r * ld + l31]);
        }
    }
}

// ((p0 + p1) + p2) + p3 of the four threads of a row (lanes 4 r .. 4 r + 3)
__device__ __forceinline__ float row_sum4(float p, int lane) {
    const int base = lane & ~3;
    const float p0 = __shfl(p, base, 64), p1 = __shfl(p, base + 1, 64), p2 = __shfl(p, base + 2, 64),
                p3 = __shfl(p, base + 3, 64);
    return ((p0 + p1) + p2) + p3;
}

// this wave's partial of a [64][d] product whose rows and reduction run over positions: acc += sum_k a(row, k) b(k, col)
// over this wave's share of k < kn (d > 32: block (wave / 2, wave % 2), all of k; d <= 32: row block wave % 2, the k
// of [32 (wave / 2), + 32)); a(row, k) with row in 0 .. 63, b(k, col) answers 0 for col >= d
template <class FA, class FB>
__device__ __forceinline__ f32x16 pos_accumulate(f32x16 acc, int d, int kn, int wave, int lane, FA a, FB b) {
    if (d > 32) {
        const int rb = (wave >> 1) * 32, cb = (wave & 1) * 32;
        return mm32(acc, 0, kn, lane, [&](int i, int k) { return a(rb + i, k); }, [&](int k, int j) { return b(k, cb + j); });
    }
    const int rb = (wave & 1) * 32, kb = (wave >> 1) * 32, ke = kn < kb + 32 ? kn : kb + 32;
    return mm32(acc, kb, ke, lane, [&](int i, int k) { return a(rb + i, k); }, [&](int k, int j) { return b(k, j); });
}

// pos_accumulate's result to global rows (row r at dst + r * row_stride, rows below n only).  d <= 32: waves 2 and 3 leave
// theirs in `part` ([64][ld], free), waves 0 and 1 add it to theirs: first halves + second halves.  All four waves call.
__device__ __forceinline__ void pos_store(f32x16 acc, int d, int n, float* part, int ld, float* dst, int64_t row_stride,
                                          int wave, int lane) {
    const int l31 = lane & 31;
    int rb = (wave >> 1) * 32, cb = (wave & 1) * 32;
    if (d <= 32) {
        rb = (wave & 1) * 32, cb = 0;
        if (wave >= 2 && l31 < d) {
#pragma unroll
            for (int v = 0; v < 16; ++v) part[(rb + acc_row(v, lane)) * ld + l31] = acc[v];
        }
        __syncthreads();
        if (wave >= 2) return;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = acc[v] + part[(rb + acc_row(v, lane)) * ld + (l31 < d ? l31 : 0)];
    }
    if (cb + l31 < d) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = rb + acc_row(v, lane);
            if (r < n) dst[r * row_stride + cb + l31] = acc[v];
        }
    }
}

int raise_lds(const void* kernel, size_t lds, const char* what) {
    if (lds <= 65536) return 0;                 // per launch: the attribute belongs to the current device's copy
    hipError_t err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) {
        arl::set_error("hipFuncSetAttribute(%s): %s", what, hipGetErrorString(err));
        return (int)err;
    }
    return 0;
}

}  // namespace
