// Implicit quantile networks (IQN, Dabney et al. 2018) for gfx950: everything of AtariIqnPolicy that is not a matrix
// product (those run on the MFMA entry points of mfma_conv.hip).  Formulas, generator mapping and summation orders are
// stated in include/accel_rl_hip.h ("Implicit quantile networks"); design notes in DESIGN.md, section 15.
//
//   arl_iqn_embed      fractions tau (drawn: Philox4x32-10 uniforms; or given) and their 64 cosine features
//   arl_iqn_merge_fwd  x = psi (conv features, one row per sample) * phi (embedding, one row per (sample, fraction))
//   arl_iqn_merge_bwd  dphi and dpsi, both already masked by the rectifier of the layer they go to
//   arl_iqn_act        Q_a = mean over the fractions, first maximum, override, one-hot row; may advance the call counter
//   arl_iqn_loss       greedy next action, targets T_j, the N x N' quantile-Huber loss and its gradient; one workgroup
//                      per sample; may advance the call counter
//   arl_miqn_loss      Munchausen IQN (Vieillard et al. 2020): arl_iqn_loss with the soft-max targets
//                      T_j = (return + bonus) + keep * (gamma_n * sum_a pi_a (theta_tgt(j, a) - tau_e log pi_a)), pi the
//                      soft-max of the target net's Q over the actions (max and exp sum: butterflies over the lanes)
//
// Plain fp32 C++ (compiled with -ffp-contract=off), wave64, no atomics: every launch is deterministic.
// The butterflies, first_max, the quantile-Huber term, the four-way combine and the serve tail are csrc/q_loss_dev.h's, and
// so are IqnLossArgs, its host-side checks (theta_sizes_ok, fill_iqn_loss), the staging of the taken action's quantiles and
// of T_j, and loss_tail: csrc/fqf.hip runs the same quantile part.

#include "arl_common.h"
#include "philox_dev.h"
#include "q_loss_dev.h"

namespace {

using namespace arlq;

// cos(pi i tau) with the argument reduced in integers: |tau| = s 2^e, the angle in units of pi is i s 2^e.
__device__ __forceinline__ float cos_pi_i_tau(uint32_t i, float tau) {
    const uint32_t bits = __float_as_uint(tau) & 0x7fffffffu;
    const int ex = (int)(bits >> 23);
    const uint32_t s = ex ? ((bits & 0x7fffffu) | 0x800000u) : (bits & 0x7fffffu);
    const int e = (ex ? ex : 1) - 150;
    if (i == 0 || s == 0 || e >= 1) return 1.f;         // angle 0, or an even multiple of pi
    uint64_t p = (uint64_t)i * s * 4;                   // angle = p 2^-sh, p < 2^32 (times 4: the folds below stay integral)
    const int sh = 2 - e;                               // >= 2
    bool neg = false, use_sin = false;
    if (sh < 40) {                                      // (else p 2^-sh < 2^-8: first octant as it stands)
        const uint64_t half = (uint64_t)1 << sh;        // pi
        p &= (half << 1) - 1;                           // modulo 2 pi
        if (p > half) p = (half << 1) - p;              // cos(2 pi - t) = cos t
        if (p > (half >> 1)) { p = half - p; neg = true; }              // cos(pi - t) = -cos t
        if (p > (half >> 2)) { p = (half >> 1) - p; use_sin = true; }   // cos(pi / 2 - t) = sin t
    }
    const float t = ldexpf((float)p, -sh);              // in [0, 1/4]; exact when p has at most 24 significant bits
    const float v = use_sin ? sinpif(t) : cospif(t);
    return neg ? 0.f - v : v;
}

// one thread per (pair p, block of 4 features): 16 threads per pair, each writing one float4 of cosf
__global__ __launch_bounds__(256) void embed_kernel(const float* __restrict__ tau_in, const int64_t* __restrict__ state,
                                                    int64_t row0, int64_t call_offset, int64_t pairs, int r,
                                                    float* __restrict__ tau_out, float* __restrict__ cosf) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= pairs * (ARL_IQN_COS / 4)) return;
    const int64_t p = t >> 4;
    const int q = (int)(t & 15);
    float tau;
    if (tau_in) {
        tau = tau_in[p];
    } else {
        const uint64_t e = (uint64_t)(row0 * r + p);                // (row0 + row) R + r
        const uint64_t call = (uint64_t)(state[1] + call_offset);
        uint32_t w[4] = {(uint32_t)(e >> 2), 0u, (uint32_t)call, (uint32_t)(call >> 32)};
        arlp::philox4x32_10(w, (uint32_t)(uint64_t)state[0], ARL_IQN_PHILOX_STREAM);
        const uint32_t k = w[e & 3] >> 9;
        tau = (float)(2 * k + 1) * (1.0f / 16777216.0f);            // (2k + 1) < 2^24: exact
    }
    if (q == 0) tau_out[p] = tau;
    float c[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) c[l] = cos_pi_i_tau((uint32_t)(4 * q + l), tau);
    *reinterpret_cast<float4*>(cosf + p * ARL_IQN_COS + 4 * q) = make_float4(c[0], c[1], c[2], c[3]);
}

__global__ __launch_bounds__(256) void merge_fwd_kernel(const float4* __restrict__ psi, const float4* __restrict__ phi,
                                                        int64_t n4, int r, int f4, float4* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int64_t row = i / f4;
    const int c = (int)(i - row * f4);
    const float4 a = psi[(row / r) * f4 + c], b = phi[i];
    x[i] = make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

// one lane per (sample, float4 of f); the r loop stays inside the lane: a fixed summation order, nothing crosses lanes
__global__ __launch_bounds__(256) void merge_bwd_kernel(const float4* __restrict__ g, const float4* __restrict__ psi,
                                                        const float4* __restrict__ phi, int64_t batch, int r, int f4,
                                                        float4* __restrict__ dphi, float4* __restrict__ dpsi) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * f4) return;
    const int64_t b = i / f4;
    const int c = (int)(i - b * f4);
    const float4 ps = psi[i];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < r; ++k) {
        const int64_t o = (b * r + k) * f4 + c;
        const float4 gv = g[o], ph = phi[o];
        dphi[o] = make_float4(ph.x > 0.f ? gv.x * ps.x : 0.f, ph.y > 0.f ? gv.y * ps.y : 0.f,
                              ph.z > 0.f ? gv.z * ps.z : 0.f, ph.w > 0.f ? gv.w * ps.w : 0.f);
        s.x += gv.x * ph.x; s.y += gv.y * ph.y; s.z += gv.z * ph.z; s.w += gv.w * ph.w;
    }
    dpsi[i] = make_float4(ps.x > 0.f ? s.x : 0.f, ps.y > 0.f ? s.y : 0.f, ps.z > 0.f ? s.z : 0.f, ps.w > 0.f ? s.w : 0.f);
}

// Q_a of action `lane` under theta_b f32[k][stride]: rows read coalesced, k ascending, the sum starts at 0
__device__ __forceinline__ float q_of_lane(const float* theta_b, int lane, int n_actions, int k, int stride) {
    if (lane >= n_actions) return 0.f;
    float s = 0.f;
    for (int j = 0; j < k; ++j) s += theta_b[(int64_t)j * stride + lane];
    return s / (float)k;
}

// one wave per sample, lanes are actions
__global__ __launch_bounds__(256) void act_kernel(const float* __restrict__ theta,
                                                  const int32_t* __restrict__ override_or_null, int64_t batch,
                                                  int n_actions, int k, int stride, float* __restrict__ onehot,
                                                  uint8_t* __restrict__ greedy, int64_t* state, int64_t advance) {
    __shared__ float s_q[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    s_q[wave][lane] = b < batch ? q_of_lane(theta + b * k * stride, lane, n_actions, k, stride) : 0.f;
    __syncthreads();
    if (b < batch) serve_wave(first_max(s_q[wave], n_actions), b, lane, n_actions, override_or_null, onehot, greedy);
    if (state && blockIdx.x == 0 && threadIdx.x == 0) state[1] += advance;     // this pass's draws have all been made
}

// One workgroup per sample.  Q phase: wave 0, lane = action, the N' rows of the selecting net read coalesced; meanwhile wave 1
// stages the taken action's predicted quantiles and their fractions.  Then wave 0 stages T_j (lane = j).  N x N' phase: lane i =
// predicted fraction i in every wave, the j loop dealt to the waves (j = wave, wave + 4, ...: every lane reads the same T_j, a
// broadcast); the four partial sums per lane are combined in the fixed order ((p0 + p1) + p2) + p3.  All 256 threads then
// write dtheta (quantiles are strided by S here: the taken action's column, zeros elsewhere).
__global__ __launch_bounds__(256) void loss_kernel(const IqnLossArgs a) {
    __shared__ float s_q[64], s_t[64], s_pred[64], s_tau[64], s_d[64], s_g[4][64], s_r[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;                               // (grid = batch exactly)
    const int A = a.n_actions, n = a.n, m = a.n_target, S = a.stride;
    int act = a.actions[b];
    act = act < A ? act : A - 1;                                // an action the net does not have: never out of bounds
    if (wave == 0) {
        const float* sel = (a.pol_next ? a.pol_next : a.tgt_next) + b * m * S;
        s_q[lane] = q_of_lane(sel, lane, A, m, S);
    } else if (wave == 1) {
        stage_taken(a, lane, act, s_pred, s_tau);
    }
    __syncthreads();
    if (wave == 0) {
        stage_targets(a, lane, first_max(s_q, A), s_t);
    }
    __syncthreads();
    loss_tail(a, lane, wave, act, s_t, s_pred, s_tau, s_d, s_g, s_r);
}

// (a Munchausen target selects no action: pol_next's slot carries the target net on obs, [B][N'][S]; returns: the reward)
struct MiqnLossArgs : IqnLossArgs {
    float tau_e, alpha, l0;         // entropy temperature (> 0), bonus scale (>= 0), clip floor (<= 0)
};

constexpr int MIQN_TILE_ROW = 64 + 1;       // 64 actions, and odd: the lanes walking their rows meet no bank conflict

// Munchausen IQN: loss_kernel with the targets T_j = (return + bonus) + keep * (gamma_n * soft_j).  One workgroup per sample.
// Q phase: waves 0 and 2, lane = action, take Q^next and Q^cur (the N' rows read coalesced), wave 1 stages the taken action's
// predicted quantiles and their fractions, and all 256 threads stage the [N'][A] tile of tgt_next in LDS.  Soft-max phase:
// waves 0 and 2 take max and exp sum of their row as butterflies; wave 0 keeps pi_a and tau_e log pi_a, wave 2 the bonus.
// Then wave 0, lane = j, walks its row of the tile (a ascending, from 0) and stages T_j.  Then loss_tail.
__global__ __launch_bounds__(256) void mloss_kernel(const MiqnLossArgs a) {
    __shared__ float s_tile[ARL_IQN_MAX_FRACTIONS * MIQN_TILE_ROW];
    __shared__ float s_q[64], s_qc[64], s_pi[64], s_lp[64], s_bonus;
    __shared__ float s_t[64], s_pred[64], s_tau[64], s_d[64], s_g[4][64], s_r[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;                               // (grid = batch exactly)
    const int A = a.n_actions, n = a.n, m = a.n_target, S = a.stride;
    int act = a.actions[b];
    act = act < A ? act : A - 1;                                // an action the net does not have: never out of bounds
    const float* nxt = a.tgt_next + b * m * S;
    if (wave == 0) {
        s_q[lane] = q_of_lane(nxt, lane, A, m, S);
    } else if (wave == 1) {
        stage_taken(a, lane, act, s_pred, s_tau);
    } else if (wave == 2) {
        s_qc[lane] = q_of_lane(a.pol_next + b * m * S, lane, A, m, S);
    }
    for (int o = threadIdx.x; o < m * A; o += 256) {            // row o / A (a fraction), column o % A (an action)
        const int j = o / A;
        s_tile[j * MIQN_TILE_ROW + (o - j * A)] = nxt[(int64_t)j * S + (o - j * A)];
    }
    __syncthreads();
    if (wave == 0 || wave == 2) {
        const float q = wave == 0 ? s_q[lane] : s_qc[lane];
        const float v = wave_max(lane < A ? q : -INFINITY);
        const float c = q - v;
        const float e = lane < A ? expf(c / a.tau_e) : 0.f;
        const float s = wave_sum(e);
        const float lp = c - a.tau_e * logf(s);                 // tau_e log pi_a
        if (wave == 0) {
            s_pi[lane] = e / s;
            s_lp[lane] = lp;
        } else if (lane == act) {
            s_bonus = a.alpha * fminf(fmaxf(lp, a.l0), 0.f);    // on terminal rows too
        }
    }
    __syncthreads();
    if (wave == 0) {
        float soft = 0.f;                                       // sum_a pi_a (theta(j, a) - tau_e log pi_a)
        if (lane < m)
            for (int k = 0; k < A; ++k) soft += s_pi[k] * (s_tile[lane * MIQN_TILE_ROW + k] - s_lp[k]);
        const float keep = a.terminals[b] ? 0.f : 1.f;
        s_t[lane] = lane < m ? (a.returns[b] + s_bonus) + keep * (a.gamma_n * soft) : 0.f;
    }
    __syncthreads();
    loss_tail(a, lane, wave, act, s_t, s_pred, s_tau, s_d, s_g, s_r);
}

inline unsigned grid_for(int64_t n) { return (unsigned)((n + 255) / 256); }

bool merge_sizes_ok(int64_t batch, int r, int f) {
    return batch >= 1 && batch <= 0x7fffffffLL && r >= 1 && r <= ARL_IQN_MAX_FRACTIONS && f >= 4 && (f & 3) == 0 &&
           f <= (1 << 24) && batch * r <= 0x7fffffffLL && batch * r * f <= ((int64_t)1 << 40);
}

const char* const MERGE_SIZES = "need 1 <= batch, batch x r < 2^31, 1 <= r <= 64, 4 <= f <= 2^24, f % 4 == 0 and "
                                "batch x r x f <= 2^40";

}  // namespace

extern "C" int arl_iqn_embed(const float* tau_in_or_null, const int64_t* state_or_null, int64_t row0,
                             int64_t call_offset, int64_t rows, int32_t r, float* tau, float* cosf, void* stream) {
    ARL_REQUIRE(tau && cosf, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(!tau_in_or_null != !state_or_null, ARL_E_ARG, "exactly one of tau_in (given) and state (drawn)");
    ARL_REQUIRE(rows >= 1 && r >= 1 && r <= ARL_IQN_MAX_FRACTIONS && row0 >= 0 && row0 <= 0x7fffffffLL &&
                rows <= 0x7fffffffLL && (row0 + rows) * r <= 0x7fffffffLL, ARL_E_ARG,
                "need rows >= 1, row0 >= 0, 1 <= r <= 64 and (row0 + rows) x r < 2^31");
    ARL_REQUIRE(arl::aligned16(cosf), ARL_E_ALIGN, "16-byte alignment");
    const int64_t pairs = rows * r;
    hipLaunchKernelGGL(embed_kernel, dim3(grid_for(pairs * (ARL_IQN_COS / 4))), dim3(256), 0, (hipStream_t)stream,
                       tau_in_or_null, state_or_null, row0, call_offset, pairs, r, tau, cosf);
    return arl::check_launch("iqn embed_kernel");
}

extern "C" int arl_iqn_merge_fwd(const float* psi, const float* phi, int64_t batch, int32_t r, int32_t f, float* x,
                                 void* stream) {
    ARL_REQUIRE(psi && phi && x, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(merge_sizes_ok(batch, r, f), ARL_E_ARG, MERGE_SIZES);
    ARL_REQUIRE(arl::aligned16(psi) && arl::aligned16(phi) && arl::aligned16(x), ARL_E_ALIGN, "16-byte alignment");
    const int64_t n4 = batch * r * (f / 4);
    hipLaunchKernelGGL(merge_fwd_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, (const float4*)psi,
                       (const float4*)phi, n4, r, f / 4, (float4*)x);
    return arl::check_launch("iqn merge_fwd_kernel");
}

extern "C" int arl_iqn_merge_bwd(const float* g, const float* psi, const float* phi, int64_t batch, int32_t r, int32_t f,
                                 float* dphi, float* dpsi, void* stream) {
    ARL_REQUIRE(g && psi && phi && dphi && dpsi, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(merge_sizes_ok(batch, r, f), ARL_E_ARG, MERGE_SIZES);
    ARL_REQUIRE(arl::aligned16(g) && arl::aligned16(psi) && arl::aligned16(phi) && arl::aligned16(dphi) &&
                arl::aligned16(dpsi), ARL_E_ALIGN, "16-byte alignment");
    hipLaunchKernelGGL(merge_bwd_kernel, dim3(grid_for(batch * (f / 4))), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)g, (const float4*)psi, (const float4*)phi, batch, r, f / 4, (float4*)dphi,
                       (float4*)dpsi);
    return arl::check_launch("iqn merge_bwd_kernel");
}

extern "C" int arl_iqn_act(const float* theta, const int32_t* override_or_null, int64_t batch, int32_t n_actions,
                           int32_t k, int32_t a_stride, float* onehot, uint8_t* greedy_or_null, int64_t* state_or_null,
                           int64_t advance, void* stream) {
    ARL_REQUIRE(theta && onehot, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(theta_sizes_ok(batch, n_actions, k, a_stride), ARL_E_ARG, THETA_SIZES);
    hipLaunchKernelGGL(act_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream, theta,
                       override_or_null, batch, n_actions, k, a_stride, onehot, greedy_or_null, state_or_null, advance);
    return arl::check_launch("iqn act_kernel");
}

extern "C" int arl_iqn_loss(const float* pred, const float* tau_pred, const float* tgt_next,
                            const float* pol_next_or_null, const uint8_t* actions, const float* returns,
                            const uint8_t* terminals, const float* is_weights_or_null, int64_t batch, int32_t n_actions,
                            int32_t n, int32_t n_target, int32_t a_stride, float gamma_n, float kappa, float* dtheta,
                            float* loss_rows, float* priorities, int64_t* state_or_null, int64_t advance, void* stream) {
    IqnLossArgs a = {};
    const bool ptrs_ok = pred && tau_pred && tgt_next && actions && returns && terminals && dtheta && loss_rows && priorities;
    int rc = fill_iqn_loss(a, __func__, ptrs_ok, pred, tau_pred, tgt_next, actions, returns, terminals, is_weights_or_null,
                           batch, n_actions, n, n_target, a_stride, gamma_n, kappa, dtheta, loss_rows, priorities,
                           state_or_null, advance);
    if (rc) return rc;
    a.pol_next = pol_next_or_null;
    hipLaunchKernelGGL(loss_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("iqn loss_kernel");
}

extern "C" int arl_miqn_loss(const float* pred, const float* tau_pred, const float* tgt_next, const float* tgt_cur,
                             const uint8_t* actions, const float* returns, const uint8_t* terminals,
                             const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t n,
                             int32_t n_target, int32_t a_stride, float gamma_n, float kappa, float tau_e, float alpha,
                             float l0, float* dtheta, float* loss_rows, float* priorities, int64_t* state_or_null,
                             int64_t advance, void* stream) {
    MiqnLossArgs a = {};
    const bool ptrs_ok = pred && tau_pred && tgt_next && tgt_cur && actions && returns && terminals && dtheta && loss_rows &&
                         priorities;
    int rc = fill_iqn_loss(a, __func__, ptrs_ok, pred, tau_pred, tgt_next, actions, returns, terminals, is_weights_or_null,
                           batch, n_actions, n, n_target, a_stride, gamma_n, kappa, dtheta, loss_rows, priorities,
                           state_or_null, advance);
    if (rc) return rc;
    ARL_REQUIRE(tau_e > 0.f && tau_e <= 3.0e38f, ARL_E_ARG, "tau_e must be finite and > 0");
    ARL_REQUIRE(alpha >= 0.f && alpha <= 3.0e38f, ARL_E_ARG, "alpha must be finite and >= 0");
    ARL_REQUIRE(l0 <= 0.f && l0 >= -3.0e38f, ARL_E_ARG, "l0 must be finite and <= 0");
    a.pol_next = tgt_cur; a.tau_e = tau_e; a.alpha = alpha; a.l0 = l0;
    hipLaunchKernelGGL(mloss_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("iqn mloss_kernel");
}
