// The actor-critic output stage, once: policy / value heads + softmax (+ a loss and its gradients) in one pass, and the
// host side of its launch.  learner.hip (serving, A2C / PPO), ppg.hip (PPG's two phases) and vmpo.hip (V-MPO) instantiate
// it with their `Loss` types; nothing but the loss differs between them.  All fp32; compiled with -ffp-contract=off, the order of
// operations is the one include/accel_rl_hip.h states.
//
// A Loss provides
//   TRAIN, WT, NAME     compile-time: losses and gradients at all (false: probabilities and values are the output) |
//                       the launch carries weight-copy workgroups behind the head's own (below) | the name errors report
//   Loss(a)             what is uniform over the launch (the clip range)
//   load(a, row, A, lane, m)   fetch row `row`'s scalars into m (fields it leaves alone keep {0, 0, 0, valid 1, 0})
//   row(a, m, A, lane, pk, w)  lane k < A: d loss / d logit k; every lane: the row's two weighted loss terms
//   dh_rows(A)          rows of dout that reach dh
#pragma once
#include "arl_common.h"
#include "head_dev.h"
#include "head_wgrad_dev.h"
#include "dgrad_wt_dev.h"

namespace {

constexpr float HEAD_TINY = 1e-8f;                                      // categorical.py:6

struct HeadArgs {
    const float* h;          // [B][hid] post-relu hidden activations
    const float* w_head;     // [K][hid], rows 0..A-1 = pi, row A = value
    const float* b_head;     // [K]
    const uint8_t* actions;  // [n_rows]
    const float* adv;        // [n_rows]
    const float* ret;        // [n_rows]
    const float* old_prob;   // [n_rows][A]
    const int8_t* valids;    // [n_rows] or null
    const int32_t* idx;      // [B] rows of this minibatch, or null (identity)
    const float* lr_mult;    // device scalar (PPO clip anneals with it, ppo.py:46)
    const float* inv_count;  // device scalar 1/sum(valids) or null -> 1/B
    float* prob;             // [B][A]   (serving)
    float* value;            // [B]      (serving)
    float* dout;             // [B][K] gradient wrt (logits, value)
    float* dh;               // [B][hid] gradient wrt h (before the relu mask)
    float* loss_partials;    // [head_blocks][4] = the loss's two terms around the value loss, and the three's sum
    float* wpart;            // [head_blocks][wstride] this workgroup's share of dW_head[K][hid] = sum_b dout[b] x h[b], or null
    float* bpart;            // [head_blocks][Kp]      ... of db_head = sum_b dout[b]                (with wpart)
    int batch, hid, n_act, kind, tie_rule;
    float clip_param, v_coeff, ent_coeff, beta_clone;
    int mask_dh;             // dh *= (h > 0): h is a rectifier's output and the caller wants the gradient before it
    int head_blocks;         // workgroups of the head itself (a Loss::WT launch carries more: see head_kernel)
    int64_t wstride;         // floats between workgroups' wpart: K * hid rounded up to 4 (arl_fold_many folds float4s)
    const float* duals;      // device (eta, alpha): V-MPO reads its KL multiplier here, it moves inside a captured graph
};

struct HeadRow { int act; float adv, ret, valid, old; };     // old: the taken action's stored probability (PPG-aux: lane k's)
struct HeadTerms { float dl, l0, l_ent; };

// One row of A2C (a2c.py:43-46) or PPO (ppo.py:42-51) with the entropy bonus: lane k's d loss / d logit_k through the
// softmax, -w * surrogate and -c_e * w * entropy.  pk: lane k's probability (0 past the actions).
__device__ __forceinline__ HeadTerms pg_row(const HeadArgs& a, const HeadRow& r, const bool ppo, const float clip,
                                            const int A, const int lane, const float pk, const float w) {
    const float TINY = HEAD_TINY;
    const bool is_act = lane < A;
    const int act = r.act;
    const float adv = r.adv;
    const float pa = __shfl(pk, act, 64);
    // ---- d loss / d p_k : entropy term for every action (categorical.py:76-78)
    const float lg = is_act ? logf(pk + TINY) : 0.f;
    const float ent_k = pk * lg;
    float gk = is_act ? a.ent_coeff * w * (lg + pk / (pk + TINY)) : 0.f;     // d(-c_e * ent)/dp_k
    float ent = 0.f;
    for (int k = 0; k < A; ++k) ent -= readlane_f(ent_k, k);
    float pi_term, g_act;
    if (ppo) {
        const float old_pa = r.old;
        const float ratio = (pa + TINY) / (old_pa + TINY);           // categorical.py:66-70
        const float lo = 1.f - clip, hi = 1.f + clip;
        const float rc = fminf(fmaxf(ratio, lo), hi);
        const float s1 = ratio * adv, s2 = rc * adv;
        pi_term = fminf(s1, s2);
        const bool in_range = (ratio >= lo) && (ratio <= hi);
        float g_ratio;
        if (a.tie_rule == ARL_PPO_TIE_THEANO) {
            // the reference's graph as Theano >= 0.8 differentiates it: Minimum.L_op, e = eq(min, x), gives e g to
            // its FIRST argument (s1 here: T.minimum(surr_1, surr_2)) and (1 - e) g to the second -- a tie goes to
            // the first alone --, Clip.L_op passes g for lo <= r <= hi
            g_ratio = (pi_term == s1) ? adv : (in_range ? adv : 0.f);
        } else if (a.tie_rule == ARL_PPO_TIE_BOTH) {
            // Theano <= 0.7: eq(min, x) g to EVERY argument equal to the minimum -- inside the range s1 and s2 are the
            // same number and the sample counts twice
            g_ratio = ((pi_term == s1) ? adv : 0.f) + ((pi_term == s2 && in_range) ? adv : 0.f);
        } else {
            g_ratio = in_range ? adv : (s1 < s2 ? adv : 0.f);
        }
        g_act = -w * g_ratio / (old_pa + TINY);
    } else {
        pi_term = logf(pa + TINY) * adv;
        g_act = -w * adv / (pa + TINY);
    }
    gk += (lane == act) ? g_act : 0.f;
    const float gp = gk * pk;
    float dot = 0.f;
    for (int k = 0; k < A; ++k) dot += readlane_f(gp, k);
    return {pk * (gk - dot), -w * pi_term, -a.ent_coeff * w * ent};          // softmax backward
}

// one wave per row (looping); lanes split the hidden dimension.  Every per-action
// array is indexed with compile-time indices only (fully unrolled loops with
// `k < n_act` guards) so that it lives in VGPRs, not scratch.
// HVT = hid / 64 when the hidden width is a multiple of 64 (no per-lane guards: a guarded element costs an
// exec-mask save / branch / restore, and the generic kernel is mostly those), 0 = any width.
// wt (Loss::WT): the workgroups behind the head's own grid (blockIdx.x >= a.head_blocks) write the data gradients'
// k-contiguous weight copies (dgrad_wt_dev.h) -- the backward pass that follows reads them, and this launch is where a
// minibatch's parameters are final and nothing else needs the CUs (one launch less per minibatch).
template <class Loss, int HVT>
__global__ __launch_bounds__(256) void head_kernel(HeadArgs a, const arlw::DgradWtArgs wt) {
    constexpr bool TRAIN = Loss::TRAIN;
    if (Loss::WT && (int)blockIdx.x >= a.head_blocks) {
        arlw::dgrad_wt_block(wt, (int)blockIdx.x - a.head_blocks, (int)threadIdx.x);
        return;
    }
    constexpr int HV = HVT ? HVT : HID_MAX / 64;
    extern __shared__ __attribute__((aligned(16))) float s_w[];     // [K][hid] (+ [4][K][hid] head-gradient slices)
    __shared__ float s_loss[4][4];
    __shared__ float s_db[4][64];
    const int A = a.n_act, K = A + 1, hid = a.hid, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // A row's scalars hang off a three-deep chain of dependent loads (idx -> action -> old probability): they
    // are fetched one row ahead -- the first row's before the weights are even staged -- so the chain's
    // latency runs under the dot products instead of after them.
    HeadRow meta = {0, 0.f, 0.f, 1.f, 0.f};
    const Loss loss(a);
    auto load_meta = [&](int b) {
        if constexpr (TRAIN)
            if (b < a.batch) loss.load(a, a.idx ? (int64_t)a.idx[b] : b, A, lane, meta);
    };
    const int waves = (a.head_blocks * blockDim.x) >> 6;
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
    const float inv_n = TRAIN ? (a.inv_count ? a.inv_count[0] : 1.f / (float)a.batch) : 0.f;
    float l0 = 0.f, l_v = 0.f, l_ent = 0.f;
    // The head's own weight / bias gradient rides along (no second pass over dout and h): every wave adds its rows'
    // outer products dout[b] x h[b] into its LDS slice, the workgroup sums the four slices in wave order and leaves
    // ONE partial per workgroup for arl_fold_many (fixed order => deterministic).
    const bool fused_wgrad = TRAIN && a.wpart != nullptr;            // uniform
    float* s_dw = s_w + K * hid + wave * K * hid;
    float db_lane = 0.f;
    if (fused_wgrad) {
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < HV; ++j)
                if (HVT || lane + 64 * j < hid) s_dw[k * hid + lane + 64 * j] = 0.f;
    }
    for (int b = blockIdx.x * (blockDim.x >> 6) + wave; b < a.batch; b += waves) {
        const HeadRow cur = meta;
        load_meta(b + waves);                                           // next row's chain starts now
        const float* hrow = a.h + (int64_t)b * hid;
        float hv[HV];
#pragma unroll
        for (int j = 0; j < HV; ++j) hv[j] = (HVT || lane + 64 * j < hid) ? hrow[lane + 64 * j] : 0.f;
        // Lane k owns action k (lane A the value): the transcendental work is done once per action, not
        // once per lane; sums over actions stay sequential in k (readlane), i.e. in a fixed order.  The loops
        // over k are real loops (K is uniform): unrolled to the 19-action maximum they were mostly branches.
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
        if constexpr (!TRAIN) {
            if (is_act) a.prob[(int64_t)b * A + lane] = pk;
            if (lane == 0) a.value[b] = v;
        } else {
            const float w = cur.valid * inv_n;                          // valids_mean (valid stays 1 where no Loss loads it)
            const float ret = cur.ret;
            const HeadTerms t = loss.row(a, cur, A, lane, pk, w);
            const float dv = 2.f * a.v_coeff * w * (v - ret);            // aac_base.py:60-61
            const float dlk = is_act ? t.dl : (lane == A ? dv : 0.f);   // policy | value
            if (lane < K) a.dout[(int64_t)b * K + lane] = dlk;
            if (lane == 0) {
                l0 += t.l0;
                l_v += a.v_coeff * w * (v - ret) * (v - ret);
                l_ent += t.l_ent;
            }
            // dh[b][c] = sum_{k < KH} dl_k W[k][c], k in order
            const int KH = Loss::dh_rows(A);
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
    }
    if constexpr (TRAIN) {
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
}

// ---------------------------------------------------------------- host

template <class Loss, int HVT>
int head_launch_hvt(const HeadArgs& a, int blocks, size_t lds, const arlw::DgradWtArgs& wt, hipStream_t s) {
    int rc = head_allow_lds(head_kernel<Loss, HVT>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL((head_kernel<Loss, HVT>), dim3(blocks), dim3(256), lds, s, a, wt);
    return arl::check_launch(Loss::NAME);
}

// `blocks` workgroups: a.head_blocks of the head, then wt's
template <class Loss>
int head_launch(const HeadArgs& a, int blocks, size_t lds, const arlw::DgradWtArgs& wt, hipStream_t s) {
    if (a.hid == 512) return head_launch_hvt<Loss, 8>(a, blocks, lds, wt, s);
    else if (a.hid == 256) return head_launch_hvt<Loss, 4>(a, blocks, lds, wt, s);
    else if (a.hid == 1024) return head_launch_hvt<Loss, 16>(a, blocks, lds, wt, s);
    else if (a.hid == 64) return head_launch_hvt<Loss, 1>(a, blocks, lds, wt, s);
    return head_launch_hvt<Loss, 0>(a, blocks, lds, wt, s);
}

// A training launch from checked arguments: `a` holds the inputs, dout, dh and the coefficients; the grid, the workspace
// (arl_pg_head_workspace_bytes: loss partials [256][4], weight partials, bias partials), the head's weight gradient and
// the three fold items are set here.  wt_items (Loss::WT only): the weight copies the launch carries, or null.
template <class Loss>
int head_loss_launch(HeadArgs a, float* dw_head, float* db_head, float* loss4, void* workspace, arl_fold_item* items3,
                     const arl_dgrad_wt* wt_items, int n_wt, hipStream_t s) {
    const int grid = (int)(((int64_t)a.batch + 3) / 4 < 256 ? ((int64_t)a.batch + 3) / 4 : 256);
    const int K = a.n_act + 1;
    const int Kp = (K + 3) & ~3;
    float* ws = (float*)workspace;
    float* part = ws + 256 * 4;
    const bool fused = K * a.hid <= FUSED_WGRAD_MAX;
    // one split's weight partials [K][hid], padded to a multiple of 4 floats (the fold reads float4s; the padding is
    // folded but not stored: items3[0].valid)
    const int64_t kh = (int64_t)K * a.hid, kh4 = (kh + 3) & ~(int64_t)3;
    float* part_b = part + (fused ? (int64_t)grid : (int64_t)WG_SPLITS) * kh4;
    a.loss_partials = ws;
    if (fused) { a.wpart = part; a.bpart = part_b; }
    a.wstride = kh4;
    a.head_blocks = grid;
    arlw::DgradWtArgs wt = {};
    int wt_blocks = 0, rc = 0;
    if (Loss::WT && wt_items && n_wt > 0) {
        rc = arlw::dgrad_wt_plan(wt_items, n_wt, &wt, &wt_blocks);
        if (rc) return rc;
    }
    rc = head_launch<Loss>(a, grid + wt_blocks, (size_t)(fused ? 5 : 1) * K * a.hid * 4, wt, s);
    if (rc) return rc;
    // head weight / bias gradient: row-split partials [WG_SPLITS][K][hid] and [WG_SPLITS][Kp]; their folds and the
    // fold of the per-workgroup loss partials [grid][4] are left to arl_fold_many (one launch per backward pass)
    if (!fused) {
        hipLaunchKernelGGL(head_wgrad_kernel, dim3((a.hid + 63) / 64, WG_SPLITS), dim3(256), 0, s, a.dout, a.h,
                           a.batch, a.hid, K, Kp, kh4, part, part_b);
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

}  // namespace
