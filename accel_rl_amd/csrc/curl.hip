// The contrastive loss of CURL (Srinivas, Laskin, Abbeel 2020) for gfx950: InfoNCE over a minibatch with a bilinear
// similarity, forward, loss and every gradient in one launch.
//
//   arl_curl_loss_parts   P = zq W, S = P zk^T (B x B), L_i = logsumexp_j S_ij - S_ii, loss = coef mean_i L_i,
//                         G = coef / B (softmax_row(S) - I), dP = G zk, dzq = dP W^T, dW = zq^T dP,
//                         accuracy = share of rows whose first arg-max of S_i. is i
//
// A workgroup of four waves owns query-row tiles of 32 (tile g, g + grid, ...).  W stays in LDS for the life of the
// workgroup; a tile's zq and P = zq W live there too.  The keys then stream through LDS in tiles of 32 rows, TWICE: pass 1
// forms the 32 x 32 block S = P K^T and keeps, one lane per query row, the running maximum and the rescaled sum (the
// online soft-max), the diagonal logit and the first arg-max; pass 2 forms the same block again (the same instructions on
// the same operands: the same bits), turns it into G in place and adds G K into dP, which stays in the waves' accumulators
// over the key tiles.  The B x B matrix never exists: one block of it lives in LDS at a time.  The block's reduction over
// D is dealt out to the four waves in quarters (four partial blocks in LDS, added in wave order by whoever reads an
// entry), so that no wave idles behind a single 32 x 32 product.  dzq = dP W^T goes straight to global memory; the
// wave's 32 x 32 blocks of dW += zq^T dP stay in accumulators ACROSS the tiles a workgroup walks and are left in the parts
// buffer, which arl_fold_many adds over the workgroups in its fixed order.  All five products run on the fp32 MFMA chain
// (v_mfma_f32_32x32x2_f32, operands as they are): a few MFLOP, bound by the launch and the LDS traffic, not by the matrix
// rate.  Every row stride in LDS is odd, so the row-indexed and the column-indexed operand reads are both conflict-free.
// No atomics; compiled with -ffp-contract=off and without packed fp32 instructions.

#include <cmath>

#include "arl_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int CU_THREADS = 256;
constexpr int CU_TILE = ARL_CURL_TILE;          // query rows per tile = key rows per tile
constexpr int CU_GRID = ARL_CURL_MAX_PARTS;     // workgroups (= partial sums per dW element) at most
constexpr int CU_LDS = CU_TILE + 1;             // row stride of a block of S
constexpr int CU_SBLK = CU_TILE * CU_LDS;       // floats of one partial block of S
constexpr int CU_WBLK = 4;                      // dW blocks a wave owns: ceil(128 / 32)^2 / 4

struct CurlArgs {
    const float *zq, *zk, *w;
    int B, D;
    float scale, inv_b;                         // coef / B, 1 / B
    float* dzq;
    float* parts;                               // [dW | loss, acc, 0, 0], each [grid][total]
    int64_t off_loss;                           // floats from `parts` to the second block's first split
};

// D[i][j] += sum_k a(i, k) b(k, j) over kb <= k < ke (an odd count: the operands past ke read as 0); i, j = 0 .. 31
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

__global__ __launch_bounds__(CU_THREADS) void curl_kernel(const CurlArgs p) {
    extern __shared__ float lds[];
    __shared__ float s_max[CU_TILE], s_inv[CU_TILE];    // a query row's final maximum and 1 / sum
    const int D = p.D, B = p.B, ld = D + 1;     // (D % 4 == 0: the stride is odd)
    float* sW = lds;                            // [D][D + 1]
    float* sP = sW + D * ld;                    // [32][D + 1]   zq_tile W
    float* sQ = sP + CU_TILE * ld;              // [32][D + 1]   zq_tile
    float* sK = sQ + CU_TILE * ld;              // [32][D + 1]   a key tile
    float* sG = sK + CU_TILE * ld;              // [32][D + 1]   dP
    float* sS = sG + CU_TILE * ld;              // [4][32][33]   the waves' partial blocks of S; [0] becomes G
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
    const int nbD = (D + 31) >> 5, d4 = D >> 2;
    const int kq = ((d4 + 1) & ~1);             // a wave's share of the reduction over D in S: even, 4 kq >= D
    const int kb = wave * kq, ke = kb + kq < D ? kb + kq : D;
    const int c0 = wave * 32;                   // the column block of P, dP and dzq this wave owns (wave < nbD)

    for (int i = tid; i < D * D; i += CU_THREADS) sW[(i / D) * ld + i % D] = p.w[i];

    // rows r0 .. r0 + 31 of src (f32[B][D], 16-byte rows) into dst; rows past B read as 0
    auto load_tile = [&](float* dst, const float* src, int r0) {
        for (int i = tid; i < CU_TILE * d4; i += CU_THREADS) {
            const int r = i / d4, c = (i - r * d4) * 4;
            float4 v = {0.f, 0.f, 0.f, 0.f};
            if (r0 + r < B) v = *reinterpret_cast<const float4*>(src + (int64_t)(r0 + r) * D + c);
            float* o = dst + r * ld + c;
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
    };
    // this wave's partial of S = P K^T over its quarter of D (an empty quarter leaves zeros)
    auto s_partial = [&]() {
        f32x16 acc = {};
        acc = mm32(acc, kb, ke, lane, [&](int i, int k) { return sP[i * ld + k]; },
                   [&](int k, int j) { return sK[j * ld + k]; });
        float* o = sS + wave * CU_SBLK;
#pragma unroll
        for (int v = 0; v < 16; ++v) o[acc_row(v, lane) * CU_LDS + l31] = acc[v];
    };
    auto s_at = [&](int i, int j) {             // the partials in wave order: the same bits in both passes
        const float* s = sS + i * CU_LDS + j;
        return ((s[0] + s[CU_SBLK]) + s[2 * CU_SBLK]) + s[3 * CU_SBLK];
    };

    f32x16 gW[CU_WBLK];
#pragma unroll
    for (int i = 0; i < CU_WBLK; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) gW[i][v] = 0.f;
    float g_loss = 0.f, g_hit = 0.f;

    const int tiles = (B + CU_TILE - 1) / CU_TILE;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int r0 = tile * CU_TILE;
        __syncthreads();                        // the tile before has been read (and W is in place)
        load_tile(sQ, p.zq, r0);
        __syncthreads();
        // 1. P = zq_tile W
        if (wave < nbD) {
            const int col = c0 + l31;
            f32x16 acc = {};
            acc = mm32(acc, 0, D, lane, [&](int i, int k) { return sQ[i * ld + k]; },
                       [&](int k, int j) { return c0 + j < D ? sW[k * ld + c0 + j] : 0.f; });
            if (col < D) {
#pragma unroll
                for (int v = 0; v < 16; ++v) sP[acc_row(v, lane) * ld + col] = acc[v];
            }
        }
        // 2. pass 1 over the keys: the online soft-max of every query row, one lane per row
        const int gi = r0 + lane;               // (wave 0, lane < 32: this lane's query row)
        float m = -INFINITY, l = 0.f, diag = 0.f, best = -INFINITY;
        int arg = -1;
        for (int k0 = 0; k0 < B; k0 += CU_TILE) {
            __syncthreads();                    // P is written; the block before has been read
            load_tile(sK, p.zk, k0);
            __syncthreads();
            s_partial();
            __syncthreads();
            if (wave == 0 && lane < CU_TILE) {
                const int nk = B - k0 < CU_TILE ? B - k0 : CU_TILE;     // keys past B do not exist
                float tm = m;
                for (int j = 0; j < nk; ++j) {
                    const float s = s_at(lane, j);
                    if (s > best) { best = s; arg = k0 + j; }
                    if (k0 + j == gi) diag = s;
                    tm = fmaxf(tm, s);
                }
                float sum = 0.f;
                for (int j = 0; j < nk; ++j) sum += expf(s_at(lane, j) - tm);
                l = l * expf(m - tm) + sum;     // (the first block: exp(-inf) = 0)
                m = tm;
            }
        }
        if (wave == 0) {
            float loss = 0.f, hit = 0.f;
            if (lane < CU_TILE) {
                s_max[lane] = m;
                s_inv[lane] = 1.f / l;
                if (gi < B) {
                    loss = ((logf(l) + m) - diag) * p.scale;
                    hit = arg == gi ? 1.f : 0.f;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                loss += __shfl_down(loss, off, 64);
                hit += __shfl_down(hit, off, 64);
            }
            g_loss += loss;                     // (lane 0's is the one written)
            g_hit += hit;
        }
        // 3. pass 2: S again, G = coef / B (softmax - I) in place of it, dP += G K
        f32x16 accP = {};
        for (int k0 = 0; k0 < B; k0 += CU_TILE) {
            __syncthreads();                    // s_max / s_inv are written; the block and the keys before have been read
            load_tile(sK, p.zk, k0);
            __syncthreads();
            s_partial();
            __syncthreads();
            for (int e = tid; e < CU_TILE * CU_TILE; e += CU_THREADS) {
                const int i = e >> 5, j = e & 31;
                float g = 0.f;
                if (r0 + i < B && k0 + j < B)
                    g = p.scale * (expf(s_at(i, j) - s_max[i]) * s_inv[i] - (r0 + i == k0 + j ? 1.f : 0.f));
                sS[i * CU_LDS + j] = g;         // (partial 0's entry: read by this thread alone)
            }
            __syncthreads();
            if (wave < nbD)
                accP = mm32(accP, 0, CU_TILE, lane, [&](int i, int k) { return sS[i * CU_LDS + k]; },
                            [&](int k, int j) { return c0 + j < D ? sK[k * ld + c0 + j] : 0.f; });
        }
        if (wave < nbD && c0 + l31 < D) {
#pragma unroll
            for (int v = 0; v < 16; ++v) sG[acc_row(v, lane) * ld + c0 + l31] = accP[v];
        }
        __syncthreads();
        // 4. dzq_tile = dP W^T, straight to global memory
        if (wave < nbD) {
            const int col = c0 + l31;
            f32x16 acc = {};
            acc = mm32(acc, 0, D, lane, [&](int i, int k) { return sG[i * ld + k]; },
                       [&](int k, int j) { return c0 + j < D ? sW[(c0 + j) * ld + k] : 0.f; });
            if (col < D) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int r = r0 + acc_row(v, lane);
                    if (r < B) p.dzq[(int64_t)r * D + col] = acc[v];
                }
            }
        }
        // 5. dW += zq_tile^T dP: 32 x 32 blocks, block q with wave q mod 4 (rows past B are zeros in both operands)
#pragma unroll
        for (int i = 0; i < CU_WBLK; ++i) {
            const int q = wave + 4 * i;
            if (q < nbD * nbD) {
                const int rb = (q / nbD) * 32, cb = (q % nbD) * 32;
                gW[i] = mm32(gW[i], 0, CU_TILE, lane, [&](int r, int k) { return rb + r < D ? sQ[k * ld + rb + r] : 0.f; },
                             [&](int k, int j) { return cb + j < D ? sG[k * ld + cb + j] : 0.f; });
            }
        }
    }
    // this workgroup's partial sums
    const int64_t g = blockIdx.x;
    float* pW = p.parts + g * ((int64_t)D * D);
    float* pl = p.parts + p.off_loss + g * 4;
#pragma unroll
    for (int i = 0; i < CU_WBLK; ++i) {
        const int q = wave + 4 * i;
        if (q < nbD * nbD) {
            const int rb = (q / nbD) * 32, col = (q % nbD) * 32 + l31;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = rb + acc_row(v, lane);
                if (r < D && col < D) pW[(int64_t)r * D + col] = gW[i][v];
            }
        }
    }
    if (tid == 0) {                             // (lane 0 of wave 0 holds the tiles' sums)
        pl[0] = g_loss;
        pl[1] = g_hit * p.inv_b;
        pl[2] = pl[3] = 0.f;
    }
}

bool curl_width_ok(int32_t width) { return width >= 4 && width <= ARL_CURL_MAX_WIDTH && width % 4 == 0; }

size_t curl_lds_bytes(int32_t width) {
    const size_t D = (size_t)width;
    return (D * (D + 1) + 4 * CU_TILE * (D + 1) + 4 * CU_SBLK) * 4;
}

}  // namespace

extern "C" int64_t arl_curl_workspace_bytes(int32_t width) {
    return curl_width_ok(width) ? (int64_t)CU_GRID * ((int64_t)width * width + 4) * 4 : 0;
}

extern "C" int arl_curl_loss_parts(const float* zq, const float* zk, const float* w, int64_t batch, int32_t width,
                                   float coef, float* dzq, float* dw, float* loss2, void* workspace,
                                   arl_fold_item* items2_or_null, void* stream) {
    ARL_REQUIRE(zq && zk && w && dzq && dw && loss2 && workspace, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(coef), ARL_E_ARG, "coef must be finite");
    ARL_REQUIRE(curl_width_ok(width), ARL_E_RANGE, "width a multiple of 4 in 4 .. 128");
    ARL_REQUIRE(batch >= 1 && batch <= ARL_CURL_MAX_ROWS, ARL_E_RANGE, "1 <= batch <= 4096");
    ARL_REQUIRE(arl::aligned16(zq) && arl::aligned16(zk) && arl::aligned16(dzq) && arl::aligned16(dw) &&
                    arl::aligned16(loss2) && arl::aligned16(workspace) && arl::aligned4(w),
                ARL_E_ALIGN, "zq, zk, dzq, dw, loss2 and workspace 16-byte, w 4-byte aligned");
    const int64_t tiles = (batch + CU_TILE - 1) / CU_TILE;
    const int grid = (int)(tiles < CU_GRID ? tiles : CU_GRID);
    const size_t lds = curl_lds_bytes(width);
    if (lds > 65536) {                          // per launch: the attribute belongs to the current device's copy
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(curl_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) { arl::set_error("hipFuncSetAttribute(curl_kernel): %s", hipGetErrorString(err)); return (int)err; }
    }
    float* parts = static_cast<float*>(workspace);
    const int64_t totals[2] = {(int64_t)width * width, 4};
    // with `grid` splits a block's splits are contiguous from its offset: [grid][total]
    const int64_t offs[2] = {0, totals[0] * CU_GRID};
    CurlArgs a = {zq, zk, w, (int)batch, width, (float)((double)coef / (double)batch), (float)(1.0 / (double)batch),
                  dzq, parts, offs[1]};
    hipLaunchKernelGGL(curl_kernel, dim3((unsigned)grid), dim3(CU_THREADS), lds, (hipStream_t)stream, a);
    int rc = arl::check_launch("curl_kernel");
    if (rc) return rc;
    float* outs[2] = {dw, loss2};
    const int32_t valid[2] = {0, 2};
    arl_fold_item local[2];
    arl_fold_item* items = items2_or_null ? items2_or_null : local;
    for (int i = 0; i < 2; ++i) {
        items[i].part = parts + offs[i];
        items[i].out = outs[i];
        items[i].total = totals[i];
        items[i].splits = grid;
        items[i].valid = valid[i];
    }
    return items2_or_null ? 0 : arl_fold_many(local, 2, stream);
}
