// Phasic policy gradient (single-network variant) for gfx950: the output stage of both phases.
//
//   arl_ppg_head_loss_parts   policy / value heads + softmax + the phase's losses and their gradients in one pass
//       ARL_PPG_POLICY  PPO's clipped surrogate, value and entropy losses; the value gradient stops at the last shared
//                       layer (dh leaves the value row out, dw_head / db_head keep it)
//       ARL_PPG_AUX     value regression + beta_clone * KL(old || new) on stored rollouts; dh takes every row
//
// A sibling of learner.hip's head_kernel<true> (same forward, same row walk, same partials for arl_fold_many), kept
// apart from it so that the existing learners' kernel is compiled from unchanged source.  All fp32; compiled with
// -ffp-contract=off.

#include <cmath>

#include "arl_common.h"
#include "head_dev.h"
#include "head_wgrad_dev.h"

namespace {

struct PpgHeadArgs {
    const float* h;          // [B][hid] post-relu hidden activations
    const float* w_head;     // [K][hid], rows 0..A-1 = pi, row A = value
    const float* b_head;     // [K]
    const uint8_t* actions;  // [n_rows]            (policy phase)
    const float* adv;        // [n_rows]            (policy phase)
    const float* ret;        // [n_rows]
    const float* old_prob;   // [n_rows][A]
    const int32_t* idx;      // [B] rows of this minibatch, or null (identity)
    const float* lr_mult;    // device scalar       (policy phase: the clip anneals with it)
    const float* inv_count;  // device scalar or null -> 1/B
    float* dout;             // [B][K] gradient wrt (logits, value)
    float* dh;               // [B][hid] gradient wrt h
    float* loss_partials;    // [gridDim][4]
    float* wpart;            // [gridDim][wstride] this workgroup's share of dW_head, or null (separate kernel)
    float* bpart;            // [gridDim][Kp]      ... of db_head                      (with wpart)
    int batch, hid, n_act, tie_rule;
    float clip_param, v_coeff, ent_coeff, beta_clone;
    int mask_dh;
    int64_t wstride;         // floats between workgroups' wpart: K * hid rounded up to 4
};

// One wave per row (looping), lanes split the hidden dimension, lane k owns action k (lane A the value): head_kernel's
// layout.  AUX selects the phase at compile time; HVT = hid / 64 when the hidden width is a multiple of 64, 0 = any.
template <bool AUX, int HVT>
__global__ __launch_bounds__(256) void ppg_head_kernel(PpgHeadArgs a) {
    constexpr int HV = HVT ? HVT : HID_MAX / 64;
    extern __shared__ __attribute__((aligned(16))) float s_w[];     // [K][hid] (+ [4][K][hid] head-gradient slices)
    __shared__ float s_loss[4][4];
    __shared__ float s_db[4][64];
    const int A = a.n_act, K = A + 1, hid = a.hid, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // a row's scalars are fetched one row ahead (idx -> action -> old probability is a chain of dependent loads)
    int m_act = 0;
    float m_adv = 0.f, m_ret = 0.f, m_old = 0.f;                     // m_old: AUX old_prob[row][lane], else old_prob[row][act]
    auto load_meta = [&](int b) {
        if (b < a.batch) {
            const int64_t row = a.idx ? (int64_t)a.idx[b] : b;
            m_ret = a.ret[row];
            if (AUX) {
                if (lane < A) m_old = a.old_prob[row * A + lane];
            } else {
                m_act = a.actions[row];
                m_adv = a.adv[row];
                m_old = a.old_prob[row * A + m_act];
            }
        }
    };
    const int waves = (gridDim.x * blockDim.x) >> 6;
    load_meta(blockIdx.x * (blockDim.x >> 6) + wave);
    if (((K * hid) & 3) || (reinterpret_cast<uintptr_t>(a.w_head) & 15)) {
        for (int i = threadIdx.x; i < K * hid; i += blockDim.x) s_w[i] = a.w_head[i];
    } else {    // stage W: independent b128 loads, four in flight per thread (named registers: an indexed array of
                // conditionally loaded float4s, or a select against a constant, goes through scratch)
        const int n4 = (K * hid) >> 2;
        const float4* src = reinterpret_cast<const float4*>(a.w_head);
        float4* dst = reinterpret_cast<float4*>(s_w);
        for (int i0 = threadIdx.x; i0 < n4; i0 += 4 * 256) {
            const int i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
            const float4 v0 = src[i0];
            float4 v1 = v0, v2 = v0, v3 = v0;
            if (i1 < n4) v1 = src[i1];
            if (i2 < n4) v2 = src[i2];
            if (i3 < n4) v3 = src[i3];
            dst[i0] = v0;
            if (i1 < n4) dst[i1] = v1;
            if (i2 < n4) dst[i2] = v2;
            if (i3 < n4) dst[i3] = v3;
        }
    }
    __syncthreads();
    const float TINY = 1e-8f;
    const float inv_n = a.inv_count ? a.inv_count[0] : 1.f / (float)a.batch;
    const float clip = AUX ? 0.f : a.clip_param * a.lr_mult[0];
    const float w = inv_n;
    float l0 = 0.f, l_v = 0.f, l_ent = 0.f;                          // l0: pi_loss | clone
    const bool fused_wgrad = a.wpart != nullptr;                     // uniform
    float* s_dw = s_w + K * hid + wave * K * hid;
    float db_lane = 0.f;
    if (fused_wgrad) {
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < HV; ++j)
                if (HVT || lane + 64 * j < hid) s_dw[k * hid + lane + 64 * j] = 0.f;
    }
    const int KH = AUX ? K : A;                                      // rows of dout that reach dh
    for (int b = blockIdx.x * (blockDim.x >> 6) + wave; b < a.batch; b += waves) {
        const int act = m_act;
        const float adv = m_adv, ret = m_ret, old = m_old;
        load_meta(b + waves);
        const float* hrow = a.h + (int64_t)b * hid;
        float hv[HV];
#pragma unroll
        for (int j = 0; j < HV; ++j) hv[j] = (HVT || lane + 64 * j < hid) ? hrow[lane + 64 * j] : 0.f;
        float v = 0.f, mx = -3.0e38f, mine = 0.f;
        for (int k = 0; k < K; ++k) {
            float sdot = 0.f;
#pragma unroll
            for (int j = 0; j < HV; ++j)
                if (HVT || lane + 64 * j < hid) sdot += hv[j] * s_w[k * hid + lane + 64 * j];
            const float o = wave_sum_f(sdot) + a.b_head[k];
            if (k < A) mx = fmaxf(mx, o); else v = o;
            mine = (lane == k) ? o : mine;
        }
        const bool is_act = lane < A;
        const float ex = is_act ? expf(mine - mx) : 0.f;
        float z = 0.f;
        for (int k = 0; k < A; ++k) z += readlane_f(ex, k);
        const float pk = ex / z;
        const float lg = is_act ? logf(pk + TINY) : 0.f;
        const float dv = 2.f * a.v_coeff * w * (v - ret);
        float dlk;
        if (AUX) {
            const float c = a.beta_clone * w;
            const float kl_k = is_act ? old * (logf(old + TINY) - lg) : 0.f;
            const float qk = is_act ? old * pk / (pk + TINY) : 0.f;
            float kl = 0.f, sq = 0.f;
            for (int k = 0; k < A; ++k) { kl += readlane_f(kl_k, k); sq += readlane_f(qk, k); }
            dlk = is_act ? c * (pk * sq - qk) : (lane == A ? dv : 0.f);
            if (lane == 0) {
                l0 += c * kl;
                l_v += a.v_coeff * w * (v - ret) * (v - ret);
            }
        } else {                                                         // head_kernel, kind 1
            const float pa = __shfl(pk, act, 64);
            const float ent_k = pk * lg;
            float gk = is_act ? a.ent_coeff * w * (lg + pk / (pk + TINY)) : 0.f;
            float ent = 0.f;
            for (int k = 0; k < A; ++k) ent -= readlane_f(ent_k, k);
            const float old_pa = old;
            const float ratio = (pa + TINY) / (old_pa + TINY);
            const float lo = 1.f - clip, hi = 1.f + clip;
            const float rc = fminf(fmaxf(ratio, lo), hi);
            const float s1 = ratio * adv, s2 = rc * adv;
            const float pi_term = fminf(s1, s2);
            const bool in_range = (ratio >= lo) && (ratio <= hi);
            float g_ratio;
            if (a.tie_rule == ARL_PPO_TIE_THEANO) {
                g_ratio = (pi_term == s1) ? adv : (in_range ? adv : 0.f);
            } else if (a.tie_rule == ARL_PPO_TIE_BOTH) {
                g_ratio = ((pi_term == s1) ? adv : 0.f) + ((pi_term == s2 && in_range) ? adv : 0.f);
            } else {
                g_ratio = in_range ? adv : (s1 < s2 ? adv : 0.f);
            }
            const float g_act = -w * g_ratio / (old_pa + TINY);
            gk += (lane == act) ? g_act : 0.f;
            const float gp = gk * pk;
            float dot = 0.f;
            for (int k = 0; k < A; ++k) dot += readlane_f(gp, k);
            dlk = is_act ? pk * (gk - dot) : (lane == A ? dv : 0.f);
            if (lane == 0) {
                l0 += -w * pi_term;
                l_v += a.v_coeff * w * (v - ret) * (v - ret);
                l_ent += -a.ent_coeff * w * ent;
            }
        }
        if (lane < K) a.dout[(int64_t)b * K + lane] = dlk;
        // dh[b][c] = sum_{k < KH} dl_k W[k][c], k in order: the policy phase stops the value row here
        float sdh[HV];
#pragma unroll
        for (int j = 0; j < HV; ++j) sdh[j] = 0.f;
        for (int k = 0; k < K; ++k) {
            const float dl_k = readlane_f(dlk, k);
            if (k < KH) {
#pragma unroll
                for (int j = 0; j < HV; ++j)
                    if (HVT || lane + 64 * j < hid) sdh[j] += dl_k * s_w[k * hid + lane + 64 * j];
            }
            if (fused_wgrad) {
#pragma unroll
                for (int j = 0; j < HV; ++j)
                    if (HVT || lane + 64 * j < hid) s_dw[k * hid + lane + 64 * j] += dl_k * hv[j];
            }
        }
        if (lane < K) db_lane += dlk;
        float* dhrow = a.dh + (int64_t)b * hid;
#pragma unroll
        for (int j = 0; j < HV; ++j) {
            const int c = lane + 64 * j;
            if (HVT || c < hid) dhrow[c] = (a.mask_dh && !(hv[j] > 0.f)) ? 0.f : sdh[j];
        }
    }
    if (lane == 0) { s_loss[wave][0] = l0; s_loss[wave][1] = l_v; s_loss[wave][2] = l_ent; s_loss[wave][3] = (l0 + l_v) + l_ent; }
    __syncthreads();
    if (threadIdx.x < 4) {
        float sl = 0.f;
        for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) sl += s_loss[wv][threadIdx.x];
        a.loss_partials[blockIdx.x * 4 + threadIdx.x] = sl;
    }
    if (fused_wgrad) {                                               // (the barrier above covers the slices too)
        s_db[wave][lane] = db_lane;
        const float* s0 = s_w + K * hid;
        float* out = a.wpart + (int64_t)blockIdx.x * a.wstride;
        for (int i = threadIdx.x; i < K * hid; i += blockDim.x)
            out[i] = ((s0[i] + s0[K * hid + i]) + s0[2 * K * hid + i]) + s0[3 * K * hid + i];
        __syncthreads();
        const int Kp = (K + 3) & ~3;
        if (threadIdx.x < Kp)
            a.bpart[(int64_t)blockIdx.x * Kp + threadIdx.x] =
                threadIdx.x < K ? ((s_db[0][threadIdx.x] + s_db[1][threadIdx.x]) + s_db[2][threadIdx.x]) + s_db[3][threadIdx.x] : 0.f;
    }
}

template <bool AUX>
int ppg_head_launch(const PpgHeadArgs& a, int grid, size_t lds, hipStream_t s) {
    int rc = 0;
#define ARL_PPG_HEAD(HVT_)                                                                                           \
    do {                                                                                                             \
        rc = head_allow_lds(ppg_head_kernel<AUX, HVT_>, lds);                                                        \
        if (rc) return rc;                                                                                           \
        hipLaunchKernelGGL((ppg_head_kernel<AUX, HVT_>), dim3(grid), dim3(256), lds, s, a);                          \
    } while (0)
    if (a.hid == 512) ARL_PPG_HEAD(8);
    else if (a.hid == 256) ARL_PPG_HEAD(4);
    else if (a.hid == 1024) ARL_PPG_HEAD(16);
    else if (a.hid == 64) ARL_PPG_HEAD(1);
    else ARL_PPG_HEAD(0);
#undef ARL_PPG_HEAD
    return arl::check_launch(AUX ? "ppg_head_kernel<aux>" : "ppg_head_kernel<policy>");
}

}  // namespace

extern "C" int arl_ppg_head_loss_parts(const float* h, const float* w_head, const float* b_head,
                                       const uint8_t* actions, const float* advantages, const float* returns,
                                       const float* old_prob, const int32_t* idx_or_null, const float* lr_mult,
                                       const float* inv_count_or_null, int64_t batch, int32_t hid, int32_t n_actions,
                                       int32_t phase, int32_t tie_rule, float clip_param, float v_loss_coeff,
                                       float ent_loss_coeff, float beta_clone, int32_t relu_mask_dh, float* dout,
                                       float* dh, float* dw_head, float* db_head, float* loss4, void* workspace,
                                       arl_fold_item* items3, void* stream) {
    ARL_REQUIRE(phase == ARL_PPG_POLICY || phase == ARL_PPG_AUX, ARL_E_ARG, "phase must be ARL_PPG_POLICY or ARL_PPG_AUX");
    ARL_REQUIRE(h && w_head && b_head && returns && old_prob && dout && dh && dw_head && db_head && loss4 &&
                    workspace && items3, ARL_E_ARG, "null pointer");
    const bool aux = phase == ARL_PPG_AUX;
    if (aux) {
        ARL_REQUIRE(std::isfinite(v_loss_coeff) && std::isfinite(beta_clone), ARL_E_ARG,
                    "v_loss_coeff and beta_clone must be finite");
    } else {
        ARL_REQUIRE(actions && advantages && lr_mult, ARL_E_ARG, "null pointer (the policy phase reads actions, advantages, lr_mult)");
        ARL_REQUIRE(tie_rule == ARL_PPO_TIE_THEANO || tie_rule == ARL_PPO_TIE_MATH || tie_rule == ARL_PPO_TIE_BOTH, ARL_E_ARG,
                    "tie_rule must be ARL_PPO_TIE_THEANO, ARL_PPO_TIE_MATH or ARL_PPO_TIE_BOTH");
        ARL_REQUIRE(std::isfinite(clip_param) && std::isfinite(v_loss_coeff) && std::isfinite(ent_loss_coeff), ARL_E_ARG,
                    "clip_param, v_loss_coeff and ent_loss_coeff must be finite");
    }
    int rc = check_head(batch, hid, n_actions);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    PpgHeadArgs a = {};
    a.h = h; a.w_head = w_head; a.b_head = b_head; a.actions = actions; a.adv = advantages; a.ret = returns;
    a.old_prob = old_prob; a.idx = idx_or_null; a.lr_mult = lr_mult; a.inv_count = inv_count_or_null;
    a.dout = dout; a.dh = dh; a.loss_partials = (float*)workspace;
    a.batch = (int)batch; a.hid = hid; a.n_act = n_actions; a.tie_rule = tie_rule;
    a.clip_param = clip_param; a.v_coeff = v_loss_coeff; a.ent_coeff = ent_loss_coeff; a.beta_clone = beta_clone;
    a.mask_dh = relu_mask_dh;
    // the sibling's grid and workspace layout (arl_pg_head_workspace_bytes): loss partials [256][4], weight partials,
    // bias partials
    const int grid = (int)((batch + 3) / 4 < 256 ? (batch + 3) / 4 : 256);
    const int K = n_actions + 1;
    const int Kp = (K + 3) & ~3;
    float* ws = (float*)workspace;
    float* part = ws + 256 * 4;
    const bool fused = K * hid <= FUSED_WGRAD_MAX;
    const int64_t kh = (int64_t)K * hid, kh4 = (kh + 3) & ~(int64_t)3;
    float* part_b = part + (fused ? (int64_t)grid : (int64_t)WG_SPLITS) * kh4;
    if (fused) { a.wpart = part; a.bpart = part_b; }
    a.wstride = kh4;
    const size_t lds = (size_t)(fused ? 5 : 1) * K * hid * 4;
    rc = aux ? ppg_head_launch<true>(a, grid, lds, s) : ppg_head_launch<false>(a, grid, lds, s);
    if (rc) return rc;
    if (!fused) {
        hipLaunchKernelGGL(head_wgrad_kernel, dim3((hid + 63) / 64, WG_SPLITS), dim3(256), 0, s, dout, h,
                           (int)batch, (int)hid, K, Kp, kh4, part, part_b);
        rc = arl::check_launch("head_wgrad_kernel");
        if (rc) return rc;
    }
    const int n_parts = fused ? grid : WG_SPLITS;
    items3[0].part = part; items3[0].out = dw_head; items3[0].total = kh4; items3[0].splits = n_parts;
    items3[1].part = part_b; items3[1].out = db_head; items3[1].total = Kp; items3[1].splits = n_parts;
    items3[2].part = ws; items3[2].out = loss4; items3[2].total = 4; items3[2].splits = grid;
    items3[0].valid = kh4 != kh ? kh : 0;              // dw_head holds K * hid floats
    items3[1].valid = K;                                // db_head holds K floats, the partials are padded to Kp
    items3[2].valid = 0;
    return 0;
}
