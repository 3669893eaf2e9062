// The episodic novelty bonus of "Never Give Up" (Badia et al. 2020) for gfx950: a k-nearest-neighbour search of every
// rollout row against the memory of its own episode, and the kernel-and-modulator stage that turns the distances into
// the mixed reward.
//
//   arl_epi_knn   search: knn[row][0 .. m) = the m smallest squared distances between the row's embedding and the
//                 min(M, p) most recent entries of its episode, ascending; then append: mem / n_ins become the state
//                 after the rollout (two launches on one stream)
//   arl_epi_mix   running mean of the distances -> r_epi = 1 / (sqrt(sum_i eps / (dn_i + eps)) + c), times the clipped
//                 RND modulator -> r_mix = c_ext r_ext + c_int r_epi mod (one workgroup)
//
// include/accel_rl_hip.h states every expression and order.  The distance is the sum of squared differences in float64,
// not |a|^2 + |b|^2 - 2ab: near-duplicates decide the bonus and the expansion cancels there, so the search runs on the
// vector ALU and not on MFMA.  No float atomics, no process-wide state; compiled with -ffp-contract=off.

#include <cmath>

#include "arl_optim_dev.h"

namespace {

constexpr int KNN_THREADS = 256;
constexpr int KNN_WAVES = KNN_THREADS / 64;     // rows of a workgroup's tile: one per wave
constexpr int KNN_TILE = 64;                    // candidates staged per step: one per lane
constexpr int KNN_KMAX = ARL_EPI_MAX_K;
constexpr int MIX_THREADS = 1024;

__device__ __forceinline__ double wave_min_d(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double y = __shfl_xor(x, off, 64);
        x = y < x ? y : x;
    }
    return x;
}

// ---------------------------------------------------------------- search

// grid (row tiles, n_env); workgroup = KNN_WAVES waves, wave w owns row t = tile * KNN_WAVES + w of env n and keeps that
// row's embedding in registers (EMAX / 4 float4 per lane, the same in every lane).  The candidates of the tile's rows --
// the carried ring by age (age a = entry n_ins - 1 - a), then the rollout's own rows -- pass through LDS in steps of 64,
// staged once for all waves; row stride E + 1 words, so that lane l reading word e of candidate l meets no other lane's
// bank.  A lane forms the distance to its own candidate (e ascending) and keeps the 16 smallest it has seen, sorted, in
// registers; the wave then takes k times the smallest head of its 64 lists.
template <int EMAX>
__global__ __launch_bounds__(KNN_THREADS) void epi_knn_kernel(const float* __restrict__ emb,
                                                              const uint8_t* __restrict__ dones,
                                                              const float* __restrict__ mem,
                                                              const int32_t* __restrict__ n_ins, int T, int E, int M, int k,
                                                              double* __restrict__ knn, int32_t* __restrict__ m_out) {
    extern __shared__ float s_cand[];           // [KNN_TILE][E + 1]
    const int n = blockIdx.y, t0 = blockIdx.x * KNN_WAVES;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = t0 + wave;
    const bool row = t < T;
    const int stride = E + 1, e4n = E >> 2;
    const uint8_t* dn = dones + (int64_t)n * T;
    const float* emb_n = emb + (int64_t)n * T * E;
    const float* mem_n = mem + (int64_t)n * M * E;
    const int ins = n_ins[n];
    const int held = ins < M ? ins : M;         // entries the carried ring holds

    // the last done before this row (-1: none), and whether the row is one itself
    int last = -1;
    bool searches = false;
    if (row) {
        for (int r = lane; r < t; r += 64)
            if (dn[r]) last = r;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(last, off, 64);
            last = o > last ? o : last;
        }
        searches = dn[t] == 0;
    }
    // this row's candidates: carried ages [0, n_age), rollout rows [r_lo, t)
    int r_lo = t, n_age = 0;
    if (searches) {
        r_lo = last >= 0 ? last : 0;
        if (t - M > r_lo) r_lo = t - M;
        if (last < 0 && t < M) n_age = held < M - t ? held : M - t;
    }

    float4 q[EMAX / 4];
#pragma unroll
    for (int i = 0; i < EMAX / 4; ++i) {
        q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row && i < e4n) q[i] = reinterpret_cast<const float4*>(emb_n + (int64_t)t * E)[i];
    }
    double best[KNN_KMAX];
#pragma unroll
    for (int j = 0; j < KNN_KMAX; ++j) best[j] = INFINITY;

    // what the tile can need: ages below M - t0 (its first row reaches furthest back), rollout rows [t0 - M, t0 + waves - 1)
    const int age_end = t0 < M ? (held < M - t0 ? held : M - t0) : 0;
    const int roll_lo = t0 - M > 0 ? t0 - M : 0;
    const int roll_hi = (t0 + KNN_WAVES - 1 < T ? t0 + KNN_WAVES - 1 : T);      // exclusive; <= T
    for (int phase = 0; phase < 2; ++phase) {
        const int lo = phase == 0 ? 0 : roll_lo, hi = phase == 0 ? age_end : roll_hi;
        for (int c0 = lo; c0 < hi; c0 += KNN_TILE) {
            const int cn = hi - c0 < KNN_TILE ? hi - c0 : KNN_TILE;
            __syncthreads();                    // the step before has been read
            for (int i = threadIdx.x; i < cn * e4n; i += KNN_THREADS) {
                const int c = i / e4n, e4 = i - c * e4n;
                const float* src;
                if (phase == 0) {
                    int slot = (ins - 1 - (c0 + c)) % M;            // ins - 1 - age >= 0: age < held <= ins
                    src = mem_n + (int64_t)slot * E;
                } else {
                    src = emb_n + (int64_t)(c0 + c) * E;
                }
                const float4 v = reinterpret_cast<const float4*>(src)[e4];
                float* d = s_cand + c * stride + 4 * e4;
                d[0] = v.x;
                d[1] = v.y;
                d[2] = v.z;
                d[3] = v.w;
            }
            __syncthreads();
            const int c = c0 + lane;
            const bool mine = lane < cn && (phase == 0 ? c < n_age : (c >= r_lo && c < t));
            if (mine) {
                const float* b = s_cand + lane * stride;
                double d = 0.0;
#pragma unroll
                for (int i = 0; i < EMAX / 4; ++i) {
                    if (i < e4n) {
                        const double d0 = (double)q[i].x - (double)b[4 * i], d1 = (double)q[i].y - (double)b[4 * i + 1];
                        const double d2 = (double)q[i].z - (double)b[4 * i + 2], d3 = (double)q[i].w - (double)b[4 * i + 3];
                        d += d0 * d0;
                        d += d1 * d1;
                        d += d2 * d2;
                        d += d3 * d3;
                    }
                }
                if (d < best[KNN_KMAX - 1]) {
#pragma unroll
                    for (int j = 0; j < KNN_KMAX; ++j) {
                        const double lo_v = d < best[j] ? d : best[j];
                        d = d < best[j] ? best[j] : d;
                        best[j] = lo_v;
                    }
                }
            }
        }
    }
    if (!row) return;
    // the wave's k smallest: the smallest head, taken from the lowest lane that holds it
    const int64_t out_row = (int64_t)n * T + t;
    const int cand = n_age + (t - r_lo);
    const int m = cand < k ? cand : k;
    for (int j = 0; j < k; ++j) {
        const double lo_v = wave_min_d(best[0]);
        if (lane == 0) knn[out_row * k + j] = lo_v;
        const unsigned long long who = __ballot(best[0] == lo_v);
        if (lane == __ffsll((long long)who) - 1) {
#pragma unroll
            for (int i = 0; i + 1 < KNN_KMAX; ++i) best[i] = best[i + 1];
            best[KNN_KMAX - 1] = INFINITY;
        }
    }
    if (lane == 0) m_out[out_row] = m;
}

// ---------------------------------------------------------------- append

// one workgroup per env.  With a done in the rollout (the last at row L): the ring is cleared and holds rows L .. T - 1
// as entries 0 .. T - 1 - L; without one, rows 0 .. T - 1 are entries n_ins .. n_ins + T - 1.  Entry i lives in slot
// i mod M, and only the last min(M, count) entries are written: every slot at most once.
__global__ __launch_bounds__(KNN_THREADS) void epi_append_kernel(const float* __restrict__ emb,
                                                                 const uint8_t* __restrict__ dones, int T, int E, int M,
                                                                 float* __restrict__ mem, int32_t* __restrict__ n_ins) {
    __shared__ int s_last[KNN_WAVES];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t* dn = dones + (int64_t)n * T;
    int last = -1;
    for (int r = threadIdx.x; r < T; r += KNN_THREADS)
        if (dn[r]) last = r;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(last, off, 64);
        last = o > last ? o : last;
    }
    if (lane == 0) s_last[wave] = last;
    __syncthreads();
    last = s_last[0];
    for (int w = 1; w < KNN_WAVES; ++w) last = s_last[w] > last ? s_last[w] : last;
    const int ins = n_ins[n];
    __syncthreads();                            // everyone has read n_ins before it is rewritten
    const int first = last >= 0 ? last : 0;     // the rollout row that is entry `base`
    int base = last >= 0 ? 0 : ins;
    if (base > (1 << 30)) base = M + base % M;  // the same slots, the ring still full: the count never overflows
    const int count = T - first;                // new entries base .. base + count - 1
    const int e4n = E >> 2;
    float4* mem4 = reinterpret_cast<float4*>(mem + (int64_t)n * M * E);
    const float4* emb4 = reinterpret_cast<const float4*>(emb + (int64_t)n * T * E);
    const int skip = count > M ? count - M : 0;
    if (last >= 0 && count < M)                 // a new episode that does not fill the ring: the other slots read 0
        for (int i = threadIdx.x; i < (M - count) * e4n; i += KNN_THREADS)
            mem4[(int64_t)count * e4n + i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = threadIdx.x; i < (count - skip) * e4n; i += KNN_THREADS) {
        const int j = skip + i / e4n, e4 = i % e4n;
        const int slot = (int)(((int64_t)base + j) % M);
        mem4[(int64_t)slot * e4n + e4] = emb4[(int64_t)(first + j) * e4n + e4];
    }
    if (threadIdx.x == 0) n_ins[n] = base + count;
}

// ---------------------------------------------------------------- kernel, modulator, mix

__global__ __launch_bounds__(MIX_THREADS) void epi_mix_kernel(const double* __restrict__ knn, const int32_t* __restrict__ m,
                                                              const float* __restrict__ err,
                                                              const float* __restrict__ r_ext, int64_t rows, int k,
                                                              double* __restrict__ dist_mean,
                                                              double* __restrict__ err_moments, double eps, double c,
                                                              double xi, double s_max, double mod_clip, double c_ext,
                                                              double c_int, float* __restrict__ r_mix,
                                                              float* __restrict__ diag) {
    __shared__ double s_red[MIX_THREADS / 64];
    __shared__ double s_bc[3];                  // the distances' mean, the errors' mean and standard deviation
    const int tid = threadIdx.x;
    // 1. the batch's mean distance (thread t: rows t, t + 1024, ..., each row's values ascending), merged BEFORE use
    double s = 0.0, cnt = 0.0;
    for (int64_t j = tid; j < rows; j += MIX_THREADS)
        for (int i = 0; i < (m[j] < k ? m[j] : k); ++i) {
            s += knn[j * k + i];
            cnt += 1.0;
        }
    const double S = arl::block_sum_d(s, s_red);
    const double nb = arl::block_sum_d(cnt, s_red);
    // 3a. the batch's error moments, two passes
    double mean_e = 0.0, m2_e = 0.0;
    const double nr = (double)rows;
    if (err) {
        double se = 0.0;
        for (int64_t j = tid; j < rows; j += MIX_THREADS) se += (double)err[j];
        mean_e = arl::block_sum_d(se, s_red) / nr;
        double qe = 0.0;
        for (int64_t j = tid; j < rows; j += MIX_THREADS) {
            const double d = (double)err[j] - mean_e;
            qe += d * d;
        }
        m2_e = arl::block_sum_d(qe, s_red);
    }
    if (tid == 0) {
        double mean = dist_mean[1];
        if (nb > 0.0) {
            const double na = dist_mean[0];
            const double w = nb / (na + nb);
            const double delta = S / nb - mean;
            mean = mean + delta * w;
            dist_mean[0] = na + nb;
            dist_mean[1] = mean;
        }
        s_bc[0] = mean;
        if (err) {
            const double na = err_moments[0];
            const double w = nr / (na + nr);
            const double delta = mean_e - err_moments[1];
            const double mu = err_moments[1] + delta * w;
            const double m2 = (err_moments[2] + m2_e) + ((delta * delta) * na) * w;
            err_moments[0] = na + nr;
            err_moments[1] = mu;
            err_moments[2] = m2;
            s_bc[1] = mu;
            s_bc[2] = sqrt(m2 / (na + nr) + 1e-8);
        }
    }
    __syncthreads();
    const double mean = s_bc[0];
    const double denom = mean > 1e-8 ? mean : 1e-8;
    // 2 .. 4. per row
    double sr = 0.0, sm = 0.0;
    for (int64_t j = tid; j < rows; j += MIX_THREADS) {
        double r_epi = 0.0;
        const int mj = m[j] < k ? m[j] : k;
        if (mj > 0) {
            double ks = 0.0;
            for (int i = 0; i < mj; ++i) {
                double dn = knn[j * k + i] / denom - xi;
                dn = dn > 0.0 ? dn : 0.0;
                ks += eps / (dn + eps);
            }
            const double sim = sqrt(ks) + c;
            r_epi = sim > s_max ? 0.0 : 1.0 / sim;
        }
        double mod = 1.0;
        if (err) {
            const double alpha = 1.0 + ((double)err[j] - s_bc[1]) / s_bc[2];
            mod = alpha > 1.0 ? alpha : 1.0;
            mod = mod < mod_clip ? mod : mod_clip;
        }
        sr += r_epi;
        sm += mod;
        const double a = c_ext * (double)r_ext[j];
        const double b = c_int * (r_epi * mod);
        r_mix[j] = (float)(b == 0.0 ? a : a + b);
    }
    const double SR = arl::block_sum_d(sr, s_red);
    const double SM = arl::block_sum_d(sm, s_red);
    if (tid == 0) {
        diag[0] = (float)(SR / nr);
        diag[1] = (float)(SM / nr);
        diag[2] = (float)mean;
    }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int arl_epi_knn(const float* emb, const uint8_t* dones, int64_t n_env, int32_t horizon, int32_t width,
                           int32_t memory_size, int32_t k, float* mem, int32_t* n_ins, double* knn, int32_t* m,
                           void* stream) {
    ARL_REQUIRE(emb && dones && mem && n_ins && knn && m, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n_env >= 1 && horizon >= 1 && horizon <= ARL_RND_MAX_HORIZON && n_env * horizon <= ARL_RND_MAX_ROWS,
                ARL_E_RANGE, "1 <= n_env, 1 <= horizon <= 4096, n_env * horizon <= 2^24");
    ARL_REQUIRE(n_env <= 65535, ARL_E_RANGE, "n_env <= 65535 (the grid's second dimension)");
    ARL_REQUIRE(width >= 4 && width <= ARL_EPI_MAX_WIDTH && width % 4 == 0, ARL_E_RANGE, "width a multiple of 4 in 4 .. 128");
    ARL_REQUIRE(memory_size >= 1 && memory_size <= ARL_EPI_MAX_MEMORY, ARL_E_RANGE, "1 <= memory_size <= 4096");
    ARL_REQUIRE(k >= 1 && k <= ARL_EPI_MAX_K, ARL_E_RANGE, "1 <= k <= 16");
    ARL_REQUIRE(arl::aligned16(emb) && arl::aligned16(mem) && arl::aligned4(n_ins) && arl::aligned4(m) && aligned8(knn),
                ARL_E_ALIGN, "emb and mem 16-byte, knn 8-byte, n_ins and m 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((horizon + KNN_WAVES - 1) / KNN_WAVES), (unsigned)n_env);
    const size_t lds = (size_t)KNN_TILE * (width + 1) * sizeof(float);
    if (width <= 32)
        hipLaunchKernelGGL(epi_knn_kernel<32>, grid, dim3(KNN_THREADS), lds, s, emb, dones, mem, n_ins, (int)horizon,
                           (int)width, (int)memory_size, (int)k, knn, m);
    else
        hipLaunchKernelGGL(epi_knn_kernel<128>, grid, dim3(KNN_THREADS), lds, s, emb, dones, mem, n_ins, (int)horizon,
                           (int)width, (int)memory_size, (int)k, knn, m);
    int rc = arl::check_launch("epi_knn_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(epi_append_kernel, dim3((unsigned)n_env), dim3(KNN_THREADS), 0, s, emb, dones, (int)horizon,
                       (int)width, (int)memory_size, mem, n_ins);
    return arl::check_launch("epi_append_kernel");
}

extern "C" int arl_epi_mix(const double* knn, const int32_t* m, const float* err_or_null, const float* r_ext, int64_t rows,
                           int32_t k, double* dist_mean, double* err_moments, double eps, double c, double xi, double s_max,
                           double mod_clip, double c_ext, double c_int, float* r_mix, float* diag3, void* stream) {
    ARL_REQUIRE(knn && m && r_ext && dist_mean && err_moments && r_mix && diag3, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(eps) && eps > 0.0 && std::isfinite(c) && c >= 0.0 && std::isfinite(xi) && xi >= 0.0 &&
                    std::isfinite(s_max) && s_max > 0.0 && std::isfinite(mod_clip) && mod_clip >= 1.0 &&
                    std::isfinite(c_ext) && std::isfinite(c_int),
                ARL_E_ARG, "eps > 0, c >= 0, xi >= 0, s_max > 0, mod_clip >= 1, c_ext and c_int finite");
    ARL_REQUIRE(r_mix != r_ext && r_mix != err_or_null, ARL_E_ARG, "r_mix must not be an input");
    ARL_REQUIRE(rows >= 1 && rows <= ARL_RND_MIX_MAX_ROWS, ARL_E_RANGE, "1 <= rows <= 2^22");
    ARL_REQUIRE(k >= 1 && k <= ARL_EPI_MAX_K, ARL_E_RANGE, "1 <= k <= 16");
    ARL_REQUIRE(aligned8(knn) && aligned8(dist_mean) && aligned8(err_moments) && arl::aligned4(m) &&
                    arl::aligned4(r_ext) && arl::aligned4(r_mix) && arl::aligned4(diag3) &&
                    (!err_or_null || arl::aligned4(err_or_null)),
                ARL_E_ALIGN, "knn / dist_mean / err_moments 8-byte, the others 4-byte aligned");
    hipLaunchKernelGGL(epi_mix_kernel, dim3(1), dim3(MIX_THREADS), 0, (hipStream_t)stream, knn, m, err_or_null, r_ext, rows,
                       (int)k, dist_mean, err_moments, eps, c, xi, s_max, mod_clip, c_ext, c_int, r_mix, diag3);
    return arl::check_launch("epi_mix_kernel");
}

// ---------------------------------------------------------------- inverse-dynamics head
//
// arl_invdyn_loss_parts: the head that trains the embedding, forward, loss and every gradient in one launch.  Pair b is
// rows 2b, 2b + 1 of e, read as one row x_b of 2E floats.  hid = relu(x W1 + b1), logits = hid W2 + b2, the weighted
// cross-entropy against the action, and de, dW1, db1, dW2, db2.
//
// A workgroup of four waves walks row tiles of 32 pairs (tile g, g + grid, ...).  W1 [2E][H] and W2 [H][A] are loaded
// into LDS once and stay for the life of the workgroup; a tile's x, hid, d hid and logits / d logits live in LDS too, all
// with odd row strides, so that both the row-indexed and the column-indexed operand reads of the matrix instruction are
// conflict-free.  Six products run on the fp32 MFMA chain (v_mfma_f32_32x32x2_f32: operands as they are, no split
// to form and none to recombine -- the head is a few MFLOP per minibatch and is bound by its launch and its LDS traffic,
// not by the matrix rate): hidden layer, logits, hidden gradient, de, and the two weight gradients, whose 32 x 32 blocks
// a wave keeps in its accumulators ACROSS the tiles it walks.  Softmax and cross-entropy: one lane per pair.  A
// workgroup leaves its partial sums in the parts buffer; arl_fold_many adds the workgroups in its fixed order.

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int ID_THREADS = 256;
constexpr int ID_TILE = ARL_INVDYN_TILE;        // pairs per tile
constexpr int ID_GRID = ARL_INVDYN_MAX_PARTS;   // workgroups (= partial sums per gradient element) at most
constexpr int ID_LDL = 65;                      // row stride of the logits tile (n_actions <= 64)
constexpr int ID_WBLK = 4;                      // weight-gradient blocks a wave owns, per matrix

struct InvDynArgs {
    const float *e, *w1, *b1, *w2, *b2, *weight;
    const uint8_t* actions;
    int64_t batch;
    int E2, H, A;                               // 2E, hidden, actions
    float* de;
    float* parts;                               // [dW1 | db1 | dW2 | db2 | loss, acc], each [grid][total]
    int64_t off_b1, off_w2, off_b2, off_loss;   // floats from `parts` to each block's first split
    int a4;                                     // n_actions rounded up to 4
};

// D[i][j] += sum_k a(i, k) b(k, j) over k < K (K even or not: operands past K read as 0); i, j = 0 .. 31 of this block
template <class FA, class FB>
__device__ __forceinline__ f32x16 mm32(f32x16 acc, int K, int lane, FA a, FB b) {
    const int l31 = lane & 31, half = lane >> 5;
    for (int k0 = 0; k0 < K; k0 += 2) {
        const int k = k0 + half;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k < K ? a(l31, k) : 0.f, k < K ? b(k, l31) : 0.f, acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ int acc_row(int v, int lane) { return (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5); }

__global__ __launch_bounds__(ID_THREADS) void invdyn_kernel(const InvDynArgs p) {
    extern __shared__ float lds[];
    __shared__ double s_red[ID_THREADS / 64];
    const int E2 = p.E2, H = p.H, A = p.A;
    const int ldx = E2 + 1, ldh = H + 1, ld1 = H + 1, ld2 = A | 1;
    float* sW1 = lds;                           // [2E][H + 1]
    float* sW2 = sW1 + E2 * ld1;                // [H][A | 1]
    float* sX = sW2 + H * ld2;                  // [32][2E + 1]
    float* sH = sX + ID_TILE * ldx;             // [32][H + 1]   hid
    float* sD = sH + ID_TILE * ldh;             // [32][H + 1]   d loss / d (x W1 + b1)
    float* sL = sD + ID_TILE * ldh;             // [32][65]      logits, then d loss / d logits
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31;
    const int nbH = (H + 31) >> 5, nbA = (A + 31) >> 5, nbX = (E2 + 31) >> 5;

    for (int i = tid; i < E2 * H; i += ID_THREADS) sW1[(i / H) * ld1 + i % H] = p.w1[i];
    for (int i = tid; i < H * A; i += ID_THREADS) sW2[(i / A) * ld2 + i % A] = p.w2[i];
    // max(sum_b w_b, 1): every workgroup adds all weights in the same order (thread t: b = t, t + 256, ...)
    double ws = 0.0;
    for (int64_t b = tid; b < p.batch; b += ID_THREADS) ws += (double)p.weight[b];
    ws = arl::block_sum_d(ws, s_red);
    const float inv = (float)(1.0 / (ws > 1.0 ? ws : 1.0));

    f32x16 gW1[ID_WBLK], gW2[ID_WBLK];
#pragma unroll
    for (int i = 0; i < ID_WBLK; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) gW1[i][v] = gW2[i][v] = 0.f;
    float g_b1 = 0.f, g_b2 = 0.f, g_loss = 0.f, g_acc = 0.f;

    const int64_t tiles = (p.batch + ID_TILE - 1) / ID_TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b0 = tile * ID_TILE;
        __syncthreads();                        // the tile before has been read
        for (int i = tid; i < ID_TILE * E2; i += ID_THREADS) {
            const int r = i / E2, c = i - r * E2;
            sX[r * ldx + c] = b0 + r < p.batch ? p.e[(b0 + r) * E2 + c] : 0.f;
        }
        __syncthreads();
        // 1. hid = relu(x W1 + b1)
        for (int blk = wave; blk < nbH; blk += 4) {
            const int col = blk * 32 + l31;
            f32x16 acc = {};
            acc = mm32(acc, E2, lane, [&](int i, int k) { return sX[i * ldx + k]; },
                       [&](int k, int j) { return blk * 32 + j < H ? sW1[k * ld1 + blk * 32 + j] : 0.f; });
            if (col < H) {
                const float bias = p.b1[col];
#pragma unroll
                for (int v = 0; v < 16; ++v) sH[acc_row(v, lane) * ldh + col] = fmaxf(acc[v] + bias, 0.f);
            }
        }
        __syncthreads();
        // 2. logits = hid W2 + b2
        for (int blk = wave; blk < nbA; blk += 4) {
            const int col = blk * 32 + l31;
            f32x16 acc = {};
            acc = mm32(acc, H, lane, [&](int i, int k) { return sH[i * ldh + k]; },
                       [&](int k, int j) { return blk * 32 + j < A ? sW2[k * ld2 + blk * 32 + j] : 0.f; });
            if (col < A) {
                const float bias = p.b2[col];
#pragma unroll
                for (int v = 0; v < 16; ++v) sL[acc_row(v, lane) * ID_LDL + col] = acc[v] + bias;
            }
        }
        __syncthreads();
        // softmax and cross-entropy, one lane per pair; the row of logits becomes the row of their gradients
        if (wave == 0) {
            float loss = 0.f, hit = 0.f;
            if (lane < ID_TILE) {
                const int64_t b = b0 + lane;
                float* row = sL + lane * ID_LDL;
                const float w = b < p.batch ? p.weight[b] : 0.f;
                int act = b < p.batch ? (int)p.actions[b] : 0;
                act = act < A ? act : A - 1;
                float mx = row[0];
                int arg = 0;
                for (int a = 1; a < A; ++a)
                    if (row[a] > mx) { mx = row[a]; arg = a; }
                float se = 0.f;
                for (int a = 0; a < A; ++a) se += expf(row[a] - mx);
                if (w != 0.f) {
                    loss = (w * ((logf(se) + mx) - row[act])) * inv;
                    hit = arg == act ? w * inv : 0.f;
                }
                const float scale = w * inv;
                for (int a = 0; a < A; ++a) {
                    const float pa = expf(row[a] - mx) / se;
                    row[a] = w != 0.f ? scale * (pa - (a == act ? 1.f : 0.f)) : 0.f;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                loss += __shfl_down(loss, off, 64);
                hit += __shfl_down(hit, off, 64);
            }
            g_loss += loss;                     // (lane 0's is the one written)
            g_acc += hit;
        }
        __syncthreads();
        // 3. d hid = d logits W2^T, through the rectifier
        for (int blk = wave; blk < nbH; blk += 4) {
            const int col = blk * 32 + l31;
            f32x16 acc = {};
            acc = mm32(acc, A, lane, [&](int i, int k) { return sL[i * ID_LDL + k]; },
                       [&](int k, int j) { return blk * 32 + j < H ? sW2[(blk * 32 + j) * ld2 + k] : 0.f; });
            if (col < H) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int r = acc_row(v, lane);
                    sD[r * ldh + col] = sH[r * ldh + col] > 0.f ? acc[v] : 0.f;
                }
            }
        }
        __syncthreads();
        // 4. de = d pre W1^T
        for (int blk = wave; blk < nbX; blk += 4) {
            const int col = blk * 32 + l31;
            f32x16 acc = {};
            acc = mm32(acc, H, lane, [&](int i, int k) { return sD[i * ldh + k]; },
                       [&](int k, int j) { return blk * 32 + j < E2 ? sW1[(blk * 32 + j) * ld1 + k] : 0.f; });
            if (col < E2) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int64_t b = b0 + acc_row(v, lane);
                    if (b < p.batch) p.de[b * E2 + col] = acc[v];
                }
            }
        }
        // 5. dW1 += x^T d pre, dW2 += hid^T d logits: 32 x 32 blocks, block q of a matrix with wave q mod 4
#pragma unroll
        for (int i = 0; i < ID_WBLK; ++i) {
            const int q = wave + 4 * i;
            if (q < nbX * nbH) {
                const int r0 = (q / nbH) * 32, c0 = (q % nbH) * 32;
                gW1[i] = mm32(gW1[i], ID_TILE, lane, [&](int r, int k) { return r0 + r < E2 ? sX[k * ldx + r0 + r] : 0.f; },
                              [&](int k, int j) { return c0 + j < H ? sD[k * ldh + c0 + j] : 0.f; });
            }
            if (q < nbH * nbA) {
                const int r0 = (q / nbA) * 32, c0 = (q % nbA) * 32;
                gW2[i] = mm32(gW2[i], ID_TILE, lane, [&](int r, int k) { return r0 + r < H ? sH[k * ldh + r0 + r] : 0.f; },
                              [&](int k, int j) { return c0 + j < A ? sL[k * ID_LDL + c0 + j] : 0.f; });
            }
        }
        // 6. the bias gradients: thread j adds column j of the tile, rows ascending
        if (tid < H)
            for (int r = 0; r < ID_TILE; ++r) g_b1 += sD[r * ldh + tid];
        if (tid < A)
            for (int r = 0; r < ID_TILE; ++r) g_b2 += sL[r * ID_LDL + tid];
    }
    // this workgroup's partial sums
    const int64_t g = blockIdx.x;
    float* pW1 = p.parts + g * ((int64_t)E2 * H);
    float* pb1 = p.parts + p.off_b1 + g * H;
    float* pW2 = p.parts + p.off_w2 + g * ((int64_t)H * A);
    float* pb2 = p.parts + p.off_b2 + g * p.a4;
    float* pl = p.parts + p.off_loss + g * 4;
#pragma unroll
    for (int i = 0; i < ID_WBLK; ++i) {
        const int q = wave + 4 * i;
        if (q < nbX * nbH) {
            const int r0 = (q / nbH) * 32, col = (q % nbH) * 32 + l31;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = r0 + acc_row(v, lane);
                if (r < E2 && col < H) pW1[(int64_t)r * H + col] = gW1[i][v];
            }
        }
        if (q < nbH * nbA) {
            const int r0 = (q / nbA) * 32, col = (q % nbA) * 32 + l31;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = r0 + acc_row(v, lane);
                if (r < H && col < A) pW2[(int64_t)r * A + col] = gW2[i][v];
            }
        }
    }
    if (tid < H) pb1[tid] = g_b1;
    if (tid < p.a4) pb2[tid] = tid < A ? g_b2 : 0.f;
    if (tid == 0) {                             // (lane 0 of wave 0 holds the tiles' sums)
        pl[0] = g_loss;
        pl[1] = g_acc;
        pl[2] = pl[3] = 0.f;
    }
}

struct InvDynPlan { int64_t totals[5], offs[5], floats; size_t lds; };

// sizes of the parts buffer (for ID_GRID workgroups) and of the LDS; false: outside the limits
bool invdyn_plan(int32_t width, int32_t hidden, int32_t n_actions, InvDynPlan* pl) {
    if (width < 4 || width > ARL_EPI_MAX_WIDTH || width % 4 || hidden < 4 || hidden > ARL_INVDYN_MAX_HIDDEN || hidden % 4 ||
        n_actions < 2 || n_actions > ARL_INVDYN_MAX_ACTIONS)
        return false;
    const int64_t E2 = 2 * width, H = hidden, A = n_actions;
    if (((E2 + 31) / 32) * ((H + 31) / 32) > 4 * ID_WBLK) return false;
    const int64_t totals[5] = {E2 * H, H, H * A, (A + 3) / 4 * 4, 4};
    int64_t off = 0;
    for (int i = 0; i < 5; ++i) {
        pl->totals[i] = totals[i];
        pl->offs[i] = off;
        off += totals[i] * ID_GRID;
    }
    pl->floats = off;
    pl->lds = (size_t)(E2 * (H + 1) + H * (A | 1) + ID_TILE * (E2 + 1) + 2 * ID_TILE * (H + 1) + ID_TILE * ID_LDL) * 4;
    return pl->lds <= 160 * 1024 - 1024;
}

}  // namespace

extern "C" int64_t arl_invdyn_workspace_bytes(int32_t width, int32_t hidden, int32_t n_actions) {
    InvDynPlan pl;
    return invdyn_plan(width, hidden, n_actions, &pl) ? pl.floats * 4 : 0;
}

extern "C" int arl_invdyn_loss_parts(const float* e, const float* w1, const float* b1, const float* w2, const float* b2,
                                     const uint8_t* actions, const float* weight, int64_t batch, int32_t width,
                                     int32_t hidden, int32_t n_actions, float* de, float* dw1, float* db1, float* dw2,
                                     float* db2, float* loss2, void* workspace, arl_fold_item* items5_or_null,
                                     void* stream) {
    ARL_REQUIRE(e && w1 && b1 && w2 && b2 && actions && weight && de && dw1 && db1 && dw2 && db2 && loss2 && workspace,
                ARL_E_ARG, "null pointer");
    InvDynPlan pl;
    ARL_REQUIRE(invdyn_plan(width, hidden, n_actions, &pl), ARL_E_RANGE,
                "width a multiple of 4 in 4 .. 128, hidden a multiple of 4 in 4 .. 256, 2 <= n_actions <= 64, "
                "ceil(2 width / 32) ceil(hidden / 32) <= 16");
    ARL_REQUIRE(batch >= 1 && batch <= ARL_RND_MAX_ROWS, ARL_E_RANGE, "1 <= batch <= 2^24");
    ARL_REQUIRE(arl::aligned16(e) && arl::aligned16(de) && arl::aligned16(dw1) && arl::aligned16(db1) &&
                    arl::aligned16(dw2) && arl::aligned16(db2) && arl::aligned16(loss2) && arl::aligned16(workspace) &&
                    arl::aligned4(w1) && arl::aligned4(b1) && arl::aligned4(w2) && arl::aligned4(b2) && arl::aligned4(weight),
                ARL_E_ALIGN, "e, de, the gradients, loss2 and workspace 16-byte, the other float pointers 4-byte aligned");
    const int64_t tiles = (batch + ID_TILE - 1) / ID_TILE;
    const int grid = (int)(tiles < ID_GRID ? tiles : ID_GRID);
    if (pl.lds > 65536) {                       // per launch: the attribute belongs to the current device's copy
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(invdyn_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
        if (err != hipSuccess) { arl::set_error("hipFuncSetAttribute(invdyn_kernel): %s", hipGetErrorString(err)); return (int)err; }
    }
    float* parts = static_cast<float*>(workspace);
    // with `grid` splits a block's splits are contiguous from its offset: [grid][total]
    InvDynArgs a = {e, w1, b1, w2, b2, weight, actions, batch, 2 * width, hidden, n_actions, de, parts,
                    pl.offs[1], pl.offs[2], pl.offs[3], pl.offs[4], (int)pl.totals[3]};
    hipLaunchKernelGGL(invdyn_kernel, dim3((unsigned)grid), dim3(ID_THREADS), pl.lds, (hipStream_t)stream, a);
    int rc = arl::check_launch("invdyn_kernel");
    if (rc) return rc;
    float* outs[5] = {dw1, db1, dw2, db2, loss2};
    const int32_t valid[5] = {0, 0, 0, n_actions, 2};
    arl_fold_item local[5];
    arl_fold_item* items = items5_or_null ? items5_or_null : local;
    for (int i = 0; i < 5; ++i) {
        items[i].part = parts + pl.offs[i];
        items[i].out = outs[i];
        items[i].total = pl.totals[i];
        items[i].splits = grid;
        items[i].valid = valid[i];
    }
    return items5_or_null ? 0 : arl_fold_many(local, 5, stream);
}
