// Categorical DQN ("C51") output stage for gfx950: everything after the network's last dense
// layer, which the reference expresses as Theano graph nodes.
//
//   arl_catdqn_act    per-action softmax over atoms, Q = sum_i p_i z_i, greedy action (first
//                     maximum, as T.argmax), epsilon-greedy override, served as a one-hot row so
//                     that the sampler's categorical kernel picks exactly that action
//                     (policies/dqn/atari_cat_dqn_policy.py:84-126, catdqn_cnn.py:94-99)
//   arl_catdqn_loss   distributional Bellman target projected on the fixed support, cross-entropy
//                     loss, KL priorities, and d loss / d logits in one pass
//                     (algos/dqn/cat_dqn.py:40-109)
//
//   arl_noisy_catdqn_loss_parts  arl_catdqn_loss reading a noisy output layer's two products' split partial sums,
//                     folding them and applying the noise as arl_noisy_dense_combine does (csrc/noisy.hip)
//
//   arl_dqn_act       plain Q-learning twin of arl_catdqn_act: greedy action = first maximum of the Q row
//                     (policies/dqn/atari_dqn_policy.py:61-63,118-130)
//   arl_dqn_loss      one-step / n-step Q-learning target (max or double-DQN selection), squared or
//                     Huber loss, clipped |TD error| priorities, d loss / d Q (algos/dqn/dqn.py:137-172)
//   arl_drq_loss      DrQ (Kostrikov et al. 2020; not in the reference): arl_dqn_loss with the target averaged over k and
//                     the loss over m shifted views of the sample, all inside the sample's lane
//   arl_mdqn_loss     Munchausen DQN (Vieillard et al. 2020; not in the reference): arl_dqn_loss with the soft-max
//                     bootstrap sum_a pi_a (q_a - tau_e log pi_a) of the target net on next_obs and the bonus
//                     alpha clip(tau_e log pi(action | obs), l0, 0) of the target net on obs added to the reward; max,
//                     then the exp sum with a ascending from 0, in the lane (formulas: include/accel_rl_hip.h)
//
//   arl_qrdqn_act     quantile-regression DQN twin of arl_catdqn_act: Q_a = (sum_i theta(a, i)) / N, greedy action = first
//                     maximum, override and one-hot row as there (Dabney et al. 2018; not in the reference)
//   arl_qrdqn_loss    greedy next action, target quantiles T_j = return + keep * (gamma_n * theta_tgt(a*, j)), the pairwise
//                     quantile-Huber loss over the N x N differences u_ij = T_j - theta_pred(action, i), priorities and
//                     d loss / d theta in one pass.  Summation order (per predicted quantile i = lane i): wave w adds its
//                     terms j = w, w + 4, w + 8, ... to 0 in ascending j; the four partial sums are combined as
//                     ((p0 + p1) + p2) + p3 -- at most N / 4 + 3 additions in a row; the loss then sums the lanes in
//                     wave_sum's butterfly order.  No atomics: two runs give the same bits.
//
// Layout: logits f32[batch][n_actions (+ 1 value row when dueling)][atom_stride], atom_stride = n_atoms rounded up to a
// multiple of 4 (the dense layer producing them is an MFMA kernel with 16-byte rows); the padding
// columns are ignored on input and receive zero gradient.  Lane i owns atom i; one wave per sample (action
// kernel) / one workgroup per sample (loss kernel); n_atoms <= 64.  fp32, compiled with -ffp-contract=off.
// The butterflies, first_max, the quantile-Huber term, the four-way combine and the serve tail are csrc/q_loss_dev.h's.

#include "arl_common.h"
#include "dgrad_wt_dev.h"
#include "q_loss_dev.h"
#include <type_traits>

namespace arlc {
int fold_wide_from();           // mfma_conv.hip: the split count from which a fold sums 64-way
}

namespace {

using namespace arlq;

// softmax over the atoms of one action; lane i holds logit x (lanes >= n_atoms: anything) and returns p_i (0 there)
__device__ __forceinline__ float atom_softmax(float x, int lane, int n_atoms) {
    x = lane < n_atoms ? x : -3.0e38f;
    const float m = wave_max(x);
    const float e = lane < n_atoms ? expf(x - m) : 0.f;
    return e / wave_sum(e);
}

// Where a sample's logit block [A (+ 1)][stride] is read from: the finished logits, or (Parts) the output layer's split
// partial sums as arl_conv2d_fwd's item has them -- logit = fold_splits_kernel's sum of the partials + bias, operation for
// operation (its 16 lanes-of-a-group partial sums s_g = 0 + p_g + p_{g+16} + ..., then s_0 + s_1 + ... + s_15, then the bias),
// so that the loss kernel can take the place of the fold launch without moving a bit.
struct Plain {
    const float* p;
    __device__ __forceinline__ float operator()(int off) const { return p[off]; }
};
template <int NS>                  // NS: compile-time number of splits (1, 2, 4, 8, 16), 0 = run-time (<= 127)
struct Parts {
    const float* p;             // this sample's block inside split 0
    const float* bias;          // [A (+ 1)][stride] (the output layer's bias), or null
    long long ss;               // floats between consecutive splits
    int splits;                 // 1 .. 127
    __device__ __forceinline__ float operator()(int off) const {
        if constexpr (NS > 0) {         // every partial requested before the first is used: ONE round trip
            float v[NS];
#pragma unroll
            for (int g = 0; g < NS; ++g) v[g] = p[(long long)g * ss + off];
            const float b = bias ? bias[off] : 0.f;
            float tot = 0.f + v[0];
#pragma unroll
            for (int g = 1; g < NS; ++g) tot += 0.f + v[g];
            return bias ? tot + b : tot;
        } else {
            float tot = 0.f;
            for (int g = 0; g < 16 && g < splits; ++g) {
                float sg = 0.f;
                for (int z = g; z < splits; z += 16) sg += p[(long long)z * ss + off];
                tot = g == 0 ? sg : tot + sg;
            }
            return bias ? tot + bias[off] : tot;
        }
    }
};

// NoisyParts: a noisy output layer's logits from its two products' split partial sums (AtariNoisyNetCatDqnPolicy) --
// logit = [x W + b] + f(e_out) * ([(x f(e_in)) W_sigma + b_sigma], each product folded as noisy.hip's combine_kernel folds
// it (zgn groups: 16, or 64 from arlc::fold_wide_from() splits; splits == 0: finished, bias already applied), operation
// for operation, so that the loss launch can take the place of the combine launch without moving a bit.
struct NoisySrc {
    const float* pw; const float* bias; const float* ps; const float* b_sigma; const float* feout;
    long long ssw, sss;         // floats between consecutive splits
    int nw, ns, zw, zs;         // splits (0: finished), fold groups
};
__device__ __forceinline__ float noisy_fold(const float* p, long long ss, int splits, int zgn, int off,
                                            const float* bias) {
    if (splits <= 0) return p[off];
    float s = 0.f;
    for (int k = 0; k < zgn; ++k) {
        float sk = 0.f;
        for (int z = k; z < splits; z += zgn) sk += p[(long long)z * ss + off];
        s = k == 0 ? sk : s + sk;
    }
    if (bias) s += bias[off];
    return s;
}
struct NoisyParts {
    NoisySrc q;                 // pointers at this sample's block
    __device__ __forceinline__ float operator()(int off) const {
        const float a = noisy_fold(q.pw, q.ssw, q.nw, q.zw, off, q.bias);
        const float s = noisy_fold(q.ps, q.sss, q.ns, q.zs, off, q.b_sigma);
        return a + q.feout[off] * s;
    }
};

// Dueling heads (policies/dqn/layers/dueling_merge_layer.py:32-35): the block holds n_actions advantage rows
// followed by ONE value row; logit(a, i) = val_i + (adv_ai - mean_a adv_ai).  Per lane (= atom): the mean and
// the value, read once per sample.
struct Duel { float mean, val; bool on; };
template <class L>
__device__ __forceinline__ Duel duel_terms(const L& logits, int lane, int n_actions, int n_atoms, int stride,
                                           bool dueling) {
    Duel d = {0.f, 0.f, dueling};
    if (dueling && lane < n_atoms) {
        float sum = 0.f;
        for (int a = 0; a < n_actions; ++a) sum += logits(a * stride + lane);
        d.mean = sum / (float)n_actions;
        d.val = logits(n_actions * stride + lane);
    }
    return d;
}
template <class L>
__device__ __forceinline__ float atom_logit(const L& logits, int a, int lane, int n_atoms, int stride,
                                            const Duel& d) {
    if (lane >= n_atoms) return 0.f;
    const float x = logits(a * stride + lane);
    return d.on ? d.val + (x - d.mean) : x;
}

// greedy action of one sample under `logits`: argmax_a sum_i softmax(logit(a, .))_i z_i, first maximum
__device__ __forceinline__ int greedy_action(const float* logits_p, int lane, int n_actions, int n_atoms,
                                             int stride, float z_lane, bool dueling) {
    const Plain logits = {logits_p};
    const Duel d = duel_terms(logits, lane, n_actions, n_atoms, stride, dueling);
    int best = 0;
    float best_q = -3.0e38f;
    for (int a = 0; a < n_actions; ++a) {
        const float q = wave_sum(atom_softmax(atom_logit(logits, a, lane, n_atoms, stride, d), lane, n_atoms) * z_lane);
        if (q > best_q) { best_q = q; best = a; }
    }
    return best;
}

__global__ __launch_bounds__(256) void catdqn_act_kernel(const float* __restrict__ logits,
                                                         const float* __restrict__ z,
                                                         const int32_t* __restrict__ override_or_null,
                                                         int64_t batch, int n_actions, int n_atoms, int stride,
                                                         int dueling, float* __restrict__ onehot,
                                                         uint8_t* __restrict__ greedy) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    const float z_lane = lane < n_atoms ? z[lane] : 0.f;
    const int g = greedy_action(logits + b * (n_actions + dueling) * stride, lane, n_actions, n_atoms, stride, z_lane,
                                dueling != 0);
    serve_wave(g, b, lane, n_actions, override_or_null, onehot, greedy);
}

struct LogitSrc { const float* p; const float* bias; long long ss; int splits; };     // splits == 0: finished logits
struct CatLossArgs {
    const float* pred_logits;       // policy net on obs              [B][A][S]
    const float* tgt_next_logits;   // target net on next_obs         [B][A][S]
    const float* pol_next_logits;   // policy net on next_obs (double DQN) or null
    LogitSrc src[3];                // PARTS: the same three (pred, tgt_next, pol_next), as split partial sums
    NoisySrc nsrc[3];               // NOISY: the same three, as a noisy layer's two products (block 0 of the batch)
    const float* z;                 // [n_atoms] support
    const uint8_t* actions;         // [B]
    const float* returns;           // [B] n-step discounted return
    const uint8_t* terminals;       // [B]
    const float* is_weights;        // [B] or null
    float* dlogits;                 // [B][A][S]
    float* loss_rows;               // [B] per-sample (weighted) loss / B
    float* kl;                      // [B] priorities
    int64_t batch;
    int n_actions, n_atoms, stride;
    int dueling;                    // 1: every [A][S] block above is [A + 1][S], the value row last
    float v_min, v_max, gamma_n;    // gamma_n = discount ** reward_horizon (rounded to f32 on the host)
};

// One workgroup per sample.  The greedy next action needs a softmax expectation per action -- a serial chain
// of wave reductions -- so the actions are dealt to the four waves; wave 0 then carries the sample through
// projection, loss and gradient (lane i = atom i).
// wt (PARTS): the workgroups behind the samples' own (blockIdx.x >= batch) write the data gradients' k-contiguous weight
// copies (dgrad_wt_dev.h) for the backward pass that follows -- as the policy-gradient head's launch does (learner.hip)
template <int NS>                  // -1: finished logits; >= 0: split partial sums (Parts<NS>); -2: NoisyParts
__global__ __launch_bounds__(256) void catdqn_loss_kernel(const CatLossArgs a, const arlw::DgradWtArgs wt) {
    constexpr bool PARTS = NS >= 0, NOISY = NS == -2;
    if ((PARTS || NOISY) && (int64_t)blockIdx.x >= a.batch) {
        arlw::dgrad_wt_block(wt, (int)(blockIdx.x - a.batch), (int)threadIdx.x);
        return;
    }
    __shared__ float s_next[64], s_znext[64], s_q[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    const int A = a.n_actions, n = a.n_atoms, S = a.stride;
    const bool duel = a.dueling != 0;
    const int64_t R = (int64_t)(A + a.dueling) * S;      // floats per sample
    const float z_lane = lane < n ? a.z[lane] : 0.f;
    using L = typename std::conditional<NOISY, NoisyParts,
                                        typename std::conditional<PARTS, Parts<(NS > 0 ? NS : 0)>, Plain>::type>::type;
    auto block_of = [&](int which, const float* plain) -> L {
        if constexpr (NOISY) {
            NoisySrc q = a.nsrc[which];
            q.pw += b * R; q.ps += b * R; q.feout += b * R;
            return L{q};
        } else if constexpr (PARTS) {
            const LogitSrc& q = a.src[which];
            return L{q.p + b * R, q.bias, q.ss, q.splits};
        } else {
            return Plain{plain + b * R};
        }
    };
    const L tgt = block_of(1, a.tgt_next_logits);
    // greedy next action: under the policy net (double DQN) or the target net (cat_dqn.py:77-81), first maximum
    {
        const bool dbl = NOISY ? a.nsrc[2].pw != nullptr : PARTS ? a.src[2].p != nullptr : a.pol_next_logits != nullptr;
        const L sel = dbl ? block_of(2, a.pol_next_logits) : tgt;
        const Duel d = duel_terms(sel, lane, A, n, S, duel);
        // this wave's actions (k = wave, wave + 4, ...; at most 16 of the <= 64): every logit requested before the first
        // softmax -- a lone global round trip instead of one per action
        float xs[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) xs[j] = wave + 4 * j < A ? atom_logit(sel, wave + 4 * j, lane, n, S, d) : 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = wave + 4 * j;
            if (k < A) {
                const float q = wave_sum(atom_softmax(xs[j], lane, n) * z_lane);
                if (lane == 0) s_q[k] = q;
            }
        }
    }
    // (wave 0's prediction logits do not depend on anything above: on their way across the barrier)
    const int act = a.actions[b];
    const L prd = block_of(0, a.pred_logits);
    float pred_x = 0.f;
    if (wave == 0) pred_x = atom_logit(prd, act, lane, n, S, duel_terms(prd, lane, A, n, S, duel));
    __syncthreads();
    if (wave != 0) return;
    const int a_next = first_max(s_q, A);
    const float next_p = atom_softmax(atom_logit(tgt, a_next, lane, n, S, duel_terms(tgt, lane, A, n, S, duel)), lane, n);
    // shifted support, clipped to [v_min, v_max] (:56-62)
    const float keep = a.terminals[b] ? 0.f : 1.f;
    float zn = a.returns[b] + keep * (a.gamma_n * z_lane);
    zn = fminf(fmaxf(zn, a.v_min), a.v_max);
    s_next[lane] = next_p;              // only wave 0 is left: in-order LDS access of one wave needs no barrier
    s_znext[lane] = zn;
    __builtin_amdgcn_wave_barrier();
    // projection on the base support (:63-70,88-90): proj_i = sum_j next_p_j clip(1 - |zn_j - z_i| / dz, 0, 1)
    const float dz = (a.v_max - a.v_min) / (float)(n - 1);
    float proj = 0.f;
    if (lane < n)
        for (int j = 0; j < n; ++j) {
            const float c = 1.f - fabsf(s_znext[j] - z_lane) / dz;
            proj += s_next[j] * fminf(fmaxf(c, 0.f), 1.f);
        }
    // prediction, cross-entropy with NaN guard (:92-94)
    const float pred = atom_softmax(pred_x, lane, n);
    const float pc = fminf(fmaxf(pred, 1e-6f), 1.f);
    const float w = (a.is_weights ? a.is_weights[b] : 1.f) / (float)a.batch;
    const float ce = lane < n ? -(proj * logf(pc)) : 0.f;
    const float loss_b = wave_sum(ce);
    // KL priority (:100-105)
    const float pj = fminf(fmaxf(proj, 1e-6f), 1.f);
    const float kl_b = wave_sum(lane < n ? pj * logf(pj / pc) : 0.f);
    // gradient: d loss / d pred_i = -w proj_i / pred_i inside the clip range, then softmax backward
    const float g = (lane < n && pred >= 1e-6f && pred <= 1.f) ? -w * proj / pred : 0.f;
    const float dot = wave_sum(g * pred);
    float* dl = a.dlogits + b * R;
    const float d_lane = lane < n ? pred * (g - dot) : 0.f;            // d loss / d logit(act, lane)
    if (!duel) {
        for (int q = lane; q < A * S; q += 64) {                       // every other action (and the padding) gets 0
            const int qa = q / S, qi = q - qa * S;
            if (qa != act || qi >= n) dl[q] = 0.f;
        }
        if (lane < n) dl[act * S + lane] = d_lane;
    } else {                                                           // through the merge: adv rows, then the value row
        const float share = d_lane / (float)A;
        for (int k = 0; k < A; ++k)
            for (int i = lane; i < S; i += 64) dl[k * S + i] = i < n ? (k == act ? d_lane - share : -share) : 0.f;
        for (int i = lane; i < S; i += 64) dl[A * S + i] = i < n ? d_lane : 0.f;
    }
    if (lane == 0) {
        a.loss_rows[b] = w * loss_b;
        a.kl[b] = fminf(fmaxf(kl_b, 1e-6f), 1e6f);
    }
}

// ---- plain DQN: Q rows f32[batch][q_stride], the first n_actions columns valid; one lane per sample ----
// (row_mean, q_at, first_argmax -- the dueling merge q_a = val + (adv_a - mean adv) -- are csrc/q_loss_dev.h's)
__global__ __launch_bounds__(256) void dqn_act_kernel(const float* __restrict__ q,
                                                      const int32_t* __restrict__ override_or_null, int64_t batch,
                                                      int n_actions, int stride, int dueling,
                                                      float* __restrict__ onehot, uint8_t* __restrict__ greedy) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int g = first_argmax(q + b * stride, n_actions, dueling != 0);
    int act = g;
    if (override_or_null && override_or_null[b] >= 0) act = override_or_null[b];
    for (int a = 0; a < n_actions; ++a) onehot[b * n_actions + a] = a == act ? 1.f : 0.f;
    if (greedy) greedy[b] = (uint8_t)g;
}

struct DqnLossArgs {
    const float* q;                 // policy net on obs              [B][S]
    const float* tgt_next_q;        // target net on next_obs         [B][S]
    const float* pol_next_q;        // policy net on next_obs (double DQN) or null
    const uint8_t* actions;         // [B]
    const float* returns;           // [B] n-step discounted return
    const uint8_t* terminals;       // [B]
    const float* is_weights;        // [B] or null
    float* dq;                      // [B][S]
    float* loss_rows;               // [B] per-sample (weighted) loss / B
    float* td_abs;                  // [B] priorities: |TD error| clipped to delta_clip
    int64_t batch;
    int n_actions, stride;
    int dueling;                    // 1: column n_actions of every row is the value stream
    float gamma_n, delta_clip;      // delta_clip <= 0: squared loss, unclipped priorities
};

// One TD row, shared by every loss kernel below: from the target y and the taken action to the (Huber) loss of Q row
// `row` of a.q under the weight w, and its gradient through the dueling merge into row `row` of a.dq.  Returns the
// weighted loss and the priority (|d|, clipped)
struct TdTerm { float wloss, p; };
__device__ __forceinline__ TdTerm dqn_td_row(const DqnLossArgs& a, int64_t row, float y, int act, float w) {
    const int A = a.n_actions, S = a.stride;
    const bool duel = a.dueling != 0;
    const float* qrow = a.q + row * S;
    const float d = y - q_at(qrow, act, A, duel, duel ? row_mean(qrow, A) : 0.f);
    const TdLoss t = td_loss(d, a.delta_clip);
    float* dq = a.dq + row * S;
    const float gq = -(w * t.slope);                                       // d = y - q, y carries no gradient
    for (int k = 0; k < S; ++k) dq[k] = 0.f;
    if (!duel) {
        dq[act] = gq;
    } else {                                                               // through the merge
        const float share = gq / (float)A;
        for (int k = 0; k < A; ++k) dq[k] = k == act ? gq - share : -share;
        dq[A] = gq;
    }
    return {w * t.loss, t.p};
}

// Second half of dqn_loss_kernel and mdqn_loss_kernel: sample b's row under the weight (is_weight or 1) / batch
__device__ __forceinline__ void dqn_loss_tail(const DqnLossArgs& a, int64_t b, float y, int act) {
    const float w = (a.is_weights ? a.is_weights[b] : 1.f) / (float)a.batch;
    const TdTerm t = dqn_td_row(a, b, y, act, w);
    a.loss_rows[b] = t.wloss;
    a.td_abs[b] = t.p;
}

// dqn.py:146-150 on row `row` of the next-observation blocks: double DQN picks the action with the policy net and values
// it with the target net
__device__ __forceinline__ float dqn_next_q(const DqnLossArgs& a, int64_t row) {
    const int A = a.n_actions, S = a.stride;
    const bool duel = a.dueling != 0;
    const float* tgt = a.tgt_next_q + row * S;
    const int a_next = first_argmax(a.pol_next_q ? a.pol_next_q + row * S : tgt, A, duel);
    return q_at(tgt, a_next, A, duel, duel ? row_mean(tgt, A) : 0.f);
}

__global__ __launch_bounds__(256) void dqn_loss_kernel(const DqnLossArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    const float next_q = dqn_next_q(a, b);
    const float keep = a.terminals[b] ? 0.f : 1.f;
    const float y = a.returns[b] + keep * (a.gamma_n * next_q);            // :152-153
    dqn_loss_tail(a, b, y, a.actions[b]);
}

// ---- DrQ: dqn_loss_kernel with the target averaged over k shifted views of next_obs and the loss over m shifted views
// of obs; rows view-major (view v of sample b: row v * batch + b); one lane per sample, every sum inside the lane ----
struct DrqLossArgs : DqnLossArgs {
    int k, m;
};

__global__ __launch_bounds__(256) void drq_loss_kernel(const DrqLossArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    float nbar = dqn_next_q(a, b);
    if (a.k > 1) {
        for (int i = 1; i < a.k; ++i) nbar += dqn_next_q(a, (int64_t)i * a.batch + b);
        nbar = nbar / (float)a.k;
    }
    const float keep = a.terminals[b] ? 0.f : 1.f;
    const float y = a.returns[b] + keep * (a.gamma_n * nbar);
    const int act = a.actions[b];
    const float w = ((a.is_weights ? a.is_weights[b] : 1.f) / (float)a.batch) / (float)a.m;
    TdTerm sum = dqn_td_row(a, b, y, act, w);
    for (int v = 1; v < a.m; ++v) {
        const TdTerm t = dqn_td_row(a, (int64_t)v * a.batch + b, y, act, w);
        sum.wloss += t.wloss;
        sum.p += t.p;
    }
    a.loss_rows[b] = sum.wloss;
    a.td_abs[b] = sum.p / (float)a.m;
}

// ---- regression on given targets (PQN: Q(lambda) returns computed once per batch): dqn_loss_kernel's TD row against
// y = returns[row], minibatch rows picked by idx; one lane per sample ----
struct QRegressArgs : DqnLossArgs {
    const int32_t* idx;             // [B] rows of actions / returns, or null: row b
};

__global__ __launch_bounds__(256) void q_regress_loss_kernel(const QRegressArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    const int64_t src = a.idx ? (int64_t)a.idx[b] : b;
    int act = a.actions[src];
    if (act >= a.n_actions) act = a.n_actions - 1;                         // (never outside the row)
    const TdTerm t = dqn_td_row(a, b, a.returns[src], act, 1.f / (float)a.batch);
    a.loss_rows[b] = t.wloss;
    a.td_abs[b] = t.p;
}

// ---- Munchausen DQN: dqn_loss_kernel with a soft-max bootstrap and the clipped log-policy bonus; one lane per sample ----
// (a Munchausen target selects no action: pol_next_q's slot carries the target net on obs, [B][S]; returns: the reward)
struct MdqnLossArgs : DqnLossArgs {
    float tau_e, alpha, l0;         // entropy temperature (> 0), bonus scale (>= 0), clip floor (<= 0)
};

// (SoftRow / soft_row -- v = max_a q_a, s, tl = tau_e logf(s) -- are csrc/q_loss_dev.h's)
__global__ __launch_bounds__(256) void mdqn_loss_kernel(const MdqnLossArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    const int A = a.n_actions, S = a.stride;
    const bool duel = a.dueling != 0;
    const float te = a.tau_e;
    const float* tgt = a.tgt_next_q + b * S;
    const float mean_n = duel ? row_mean(tgt, A) : 0.f;
    const SoftRow sn = soft_row(tgt, A, duel, mean_n, te);
    float soft = 0.f;                                                      // sum_a pi_a (q_a - tau_e log pi_a)
    for (int k = 0; k < A; ++k) {
        const float qk = q_at(tgt, k, A, duel, mean_n);
        const float ck = qk - sn.v;
        const float pi = expf(ck / te) / sn.s;
        soft += pi * (qk - (ck - sn.tl));
    }
    const int act = a.actions[b];
    const float* cur = a.pol_next_q + b * S;
    const float mean_c = duel ? row_mean(cur, A) : 0.f;
    const SoftRow sc = soft_row(cur, A, duel, mean_c, te);
    const float lp_act = (q_at(cur, act, A, duel, mean_c) - sc.v) - sc.tl;
    const float bonus = a.alpha * fminf(fmaxf(lp_act, a.l0), 0.f);         // on terminal rows too
    const float keep = a.terminals[b] ? 0.f : 1.f;
    const float y = (a.returns[b] + bonus) + keep * (a.gamma_n * soft);
    dqn_loss_tail(a, b, y, act);
}

// ---- quantile-regression DQN: theta f32[batch][n_actions (+ 1)][q_stride], lane i = quantile i (layout and dueling
// merge as the categorical head's) ----
// Q_a of every action under `theta`, first maximum; one wave.  Q_a = wave_sum(theta(a, .)) / N (lanes >= N add 0)
__device__ __forceinline__ int qr_greedy_action(const float* theta_p, int lane, int n_actions, int n, int stride,
                                                bool dueling) {
    const Plain theta = {theta_p};
    const Duel d = duel_terms(theta, lane, n_actions, n, stride, dueling);
    int best = 0;
    float best_q = -3.0e38f;
    for (int a = 0; a < n_actions; ++a) {
        const float q = wave_sum(atom_logit(theta, a, lane, n, stride, d)) / (float)n;
        if (a == 0 || q > best_q) { best_q = q; best = a; }
    }
    return best;
}

__global__ __launch_bounds__(256) void qrdqn_act_kernel(const float* __restrict__ theta,
                                                        const int32_t* __restrict__ override_or_null, int64_t batch,
                                                        int n_actions, int n, int stride, int dueling,
                                                        float* __restrict__ onehot, uint8_t* __restrict__ greedy) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    const int g = qr_greedy_action(theta + b * (n_actions + dueling) * stride, lane, n_actions, n, stride, dueling != 0);
    serve_wave(g, b, lane, n_actions, override_or_null, onehot, greedy);
}

struct QrLossArgs {
    const float* pred;              // policy net on obs              [B][A (+ 1)][S]
    const float* tgt_next;          // target net on next_obs         [B][A (+ 1)][S]
    const float* pol_next;          // policy net on next_obs (double DQN) or null
    const uint8_t* actions;         // [B]
    const float* returns;           // [B] n-step discounted return
    const uint8_t* terminals;       // [B]
    const float* is_weights;        // [B] or null
    float* dtheta;                  // [B][A (+ 1)][S]
    float* loss_rows;               // [B] per-sample (weighted) loss / B
    float* priorities;              // [B] clip(unweighted loss, 1e-6, 1e6)
    int64_t batch;
    int n_actions, n, stride;
    int dueling;
    float gamma_n, kappa;           // kappa == 0: plain quantile regression
};

// One workgroup per sample.  The actions of the greedy search are dealt to the four waves (a wave reduction each); wave 0
// stages the target quantiles T_j and the taken action's predicted quantiles in LDS; the N x N phase has lane i = predicted
// quantile i in every wave and the j loop dealt to the waves (j = wave, wave + 4, ...: all lanes read the same T_j, a
// broadcast); the four partial sums per lane are combined in the fixed order ((p0 + p1) + p2) + p3 by every wave alike,
// and the waves share the rows of dtheta between them.
__global__ __launch_bounds__(256) void qrdqn_loss_kernel(const QrLossArgs a) {
    __shared__ float s_q[64], s_t[64], s_pred[64], s_g[4][64], s_r[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    if (b >= a.batch) return;                                  // (whole workgroup: no barrier is left waiting)
    const int A = a.n_actions, n = a.n, S = a.stride;
    const bool duel = a.dueling != 0;
    const int64_t R = (int64_t)(A + a.dueling) * S;            // floats per sample
    const Plain tgt = {a.tgt_next + b * R};
    {
        const Plain sel = {(a.pol_next ? a.pol_next : a.tgt_next) + b * R};
        const Duel d = duel_terms(sel, lane, A, n, S, duel);
        float xs[16];                   // this wave's actions (k = wave, wave + 4, ...): every row requested before the first sum
#pragma unroll
        for (int j = 0; j < 16; ++j) xs[j] = wave + 4 * j < A ? atom_logit(sel, wave + 4 * j, lane, n, S, d) : 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = wave + 4 * j;
            if (k < A) {
                const float q = wave_sum(xs[j]) / (float)n;
                if (lane == 0) s_q[k] = q;
            }
        }
    }
    int act = a.actions[b];
    act = act < A ? act : A - 1;                               // an action the net does not have: never out of bounds
    if (wave == 0) {
        const Plain prd = {a.pred + b * R};
        s_pred[lane] = atom_logit(prd, act, lane, n, S, duel_terms(prd, lane, A, n, S, duel));
    }
    __syncthreads();
    if (wave == 0) {
        const int a_next = first_max(s_q, A);
        const float keep = a.terminals[b] ? 0.f : 1.f;
        s_t[lane] = a.returns[b] + keep * (a.gamma_n * atom_logit(tgt, a_next, lane, n, S, duel_terms(tgt, lane, A, n, S, duel)));
    }
    __syncthreads();
    // N x N phase: this wave's share of sum_j for predicted quantile `lane`
    const float kappa = a.kappa;
    float g = 0.f, r = 0.f;
    if (lane < n) {
        const float th = s_pred[lane];
        const float tau = ((float)lane + 0.5f) / (float)n;
        for (int j = wave; j < n; j += 4) {
            float gt, rt;
            quantile_huber_term(s_t[j] - th, tau, kappa, gt, rt);
            g += gt;
            r += rt;
        }
    }
    s_g[wave][lane] = g;
    s_r[wave][lane] = r;
    __syncthreads();
    // every wave combines the four partial sums in the same fixed order (a wave without terms left an exact 0)
    const float gs = combine4(s_g, lane), rs = combine4(s_r, lane);
    const float wgt = (a.is_weights ? a.is_weights[b] : 1.f) / (float)a.batch;
    const float d_lane = lane < n ? -(wgt / (float)n * gs) : 0.f;          // d loss / d theta(act, lane)
    float* dl = a.dtheta + b * R;
    const float share = d_lane / (float)A;
    for (int k = wave; k < A + a.dueling; k += 4) {            // the rows dealt to the waves; padding columns: exact zeros
        float v;
        if (!duel) v = k == act ? d_lane : 0.f;                // every other action gets 0
        else v = k == A ? d_lane : k == act ? d_lane - share : -share;     // through the merge: adv rows, then the value row
        for (int i = lane; i < S; i += 64) dl[(int64_t)k * S + i] = i < n ? v : 0.f;
    }
    if (wave == 0) {
        const float loss_b = wave_sum(lane < n ? rs : 0.f) / (float)n;
        if (lane == 0) {
            a.loss_rows[b] = wgt * loss_b;
            a.priorities[b] = fminf(fmaxf(loss_b, 1e-6f), 1e6f);
        }
    }
}

}  // namespace

static int check_q(int64_t batch, int n_actions, int stride, int dueling) {
    if (!arlq::q_sizes_ok(batch, n_actions, stride, dueling)) {
        arl::set_error("dqn: need batch > 0, 1 <= n_actions <= 255, q_stride >= n_actions (+ 1 if dueling) and %% 4 == 0");
        return ARL_E_RANGE;
    }
    return 0;
}

extern "C" int arl_dqn_act(const float* q, const int32_t* override_or_null, int64_t batch, int32_t n_actions,
                           int32_t q_stride, int32_t dueling, float* onehot, uint8_t* greedy_or_null, void* stream) {
    ARL_REQUIRE(q && onehot, ARL_E_ARG, "null pointer");
    int rc = check_q(batch, n_actions, q_stride, dueling);
    if (rc) return rc;
    hipLaunchKernelGGL(dqn_act_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       q, override_or_null, batch, n_actions, q_stride, dueling != 0, onehot, greedy_or_null);
    return arl::check_launch("dqn_act_kernel");
}

// The checks and fields that arl_dqn_loss and arl_mdqn_loss share, in the order both state them; `fn` names the entry
// point in the message.  ptrs_ok: every mandatory pointer of the caller is non-null.
static int fill_dqn_loss(DqnLossArgs& a, const char* fn, bool ptrs_ok, const float* q, const float* tgt_next_q,
                         const uint8_t* actions, const float* returns, const uint8_t* terminals,
                         const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t q_stride,
                         int32_t dueling, float gamma_n, float delta_clip, float* dq, float* loss_rows, float* td_abs) {
    if (!ptrs_ok) {
        arl::set_error("%s: %s", fn, "null pointer");
        return ARL_E_ARG;
    }
    int rc = check_q(batch, n_actions, q_stride, dueling);
    if (rc) return rc;
    a.q = q; a.tgt_next_q = tgt_next_q; a.actions = actions; a.returns = returns; a.terminals = terminals;
    a.is_weights = is_weights_or_null; a.dq = dq; a.loss_rows = loss_rows; a.td_abs = td_abs; a.batch = batch;
    a.n_actions = n_actions; a.stride = q_stride; a.dueling = dueling != 0; a.gamma_n = gamma_n; a.delta_clip = delta_clip;
    return 0;
}

extern "C" int arl_dqn_loss(const float* q, const float* tgt_next_q, const float* pol_next_q_or_null,
                            const uint8_t* actions, const float* returns, const uint8_t* terminals,
                            const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t q_stride,
                            int32_t dueling, float gamma_n, float delta_clip, float* dq, float* loss_rows,
                            float* td_abs, void* stream) {
    DqnLossArgs a = {};
    int rc = fill_dqn_loss(a, __func__, q && tgt_next_q && actions && returns && terminals && dq && loss_rows && td_abs, q,
                           tgt_next_q, actions, returns, terminals, is_weights_or_null, batch, n_actions, q_stride,
                           dueling, gamma_n, delta_clip, dq, loss_rows, td_abs);
    if (rc) return rc;
    a.pol_next_q = pol_next_q_or_null;
    hipLaunchKernelGGL(dqn_loss_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("dqn_loss_kernel");
}

extern "C" int arl_drq_loss(const float* q, const float* tgt_next_q, const float* pol_next_q_or_null,
                            const uint8_t* actions, const float* returns, const uint8_t* terminals,
                            const float* is_weights_or_null, int64_t batch, int32_t m, int32_t k, int32_t n_actions,
                            int32_t q_stride, int32_t dueling, float gamma_n, float delta_clip, float* dq,
                            float* loss_rows, float* td_abs, void* stream) {
    DrqLossArgs a = {};
    int rc = fill_dqn_loss(a, __func__, q && tgt_next_q && actions && returns && terminals && dq && loss_rows && td_abs, q,
                           tgt_next_q, actions, returns, terminals, is_weights_or_null, batch, n_actions, q_stride,
                           dueling, gamma_n, delta_clip, dq, loss_rows, td_abs);
    if (rc) return rc;
    ARL_REQUIRE(k >= 1 && k <= 8 && m >= 1 && m <= 8, ARL_E_RANGE, "need 1 <= k, m <= 8 views");
    ARL_REQUIRE(m * batch < ((int64_t)1 << 31) && k * batch < ((int64_t)1 << 31), ARL_E_RANGE,
                "m * batch and k * batch must stay below 2^31");
    a.pol_next_q = pol_next_q_or_null; a.k = k; a.m = m;
    hipLaunchKernelGGL(drq_loss_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("drq_loss_kernel");
}

extern "C" int arl_mdqn_loss(const float* q, const float* tgt_next_q, const float* tgt_cur_q, const uint8_t* actions,
                             const float* returns, const uint8_t* terminals, const float* is_weights_or_null,
                             int64_t batch, int32_t n_actions, int32_t q_stride, int32_t dueling, float gamma_n,
                             float delta_clip, float tau_e, float alpha, float l0, float* dq, float* loss_rows,
                             float* td_abs, void* stream) {
    MdqnLossArgs a = {};
    int rc = fill_dqn_loss(a, __func__, q && tgt_next_q && tgt_cur_q && actions && returns && terminals && dq && loss_rows &&
                           td_abs, q, tgt_next_q, actions, returns, terminals, is_weights_or_null, batch, n_actions,
                           q_stride, dueling, gamma_n, delta_clip, dq, loss_rows, td_abs);
    if (rc) return rc;
    ARL_REQUIRE(tau_e > 0.f && tau_e <= 3.0e38f, ARL_E_ARG, "tau_e must be finite and > 0");
    ARL_REQUIRE(alpha >= 0.f && alpha <= 3.0e38f, ARL_E_ARG, "alpha must be finite and >= 0");
    ARL_REQUIRE(l0 <= 0.f && l0 >= -3.0e38f, ARL_E_ARG, "l0 must be finite and <= 0");
    a.pol_next_q = tgt_cur_q; a.tau_e = tau_e; a.alpha = alpha; a.l0 = l0;
    hipLaunchKernelGGL(mdqn_loss_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("mdqn_loss_kernel");
}

extern "C" int arl_q_regress_loss(const float* q, const int32_t* idx_or_null, const uint8_t* actions,
                                  const float* returns, int64_t batch, int32_t n_actions, int32_t q_stride,
                                  float delta_clip, float* dq, float* loss_rows, float* td_abs, void* stream) {
    ARL_REQUIRE(q && actions && returns && dq && loss_rows && td_abs, ARL_E_ARG, "null pointer");
    int rc = check_q(batch, n_actions, q_stride, 0);
    if (rc) return rc;
    ARL_REQUIRE(batch <= INT32_MAX, ARL_E_RANGE, "batch must stay below 2^31");
    QRegressArgs a = {};
    a.q = q; a.actions = actions; a.returns = returns; a.dq = dq; a.loss_rows = loss_rows; a.td_abs = td_abs;
    a.batch = batch; a.n_actions = n_actions; a.stride = q_stride; a.dueling = 0; a.delta_clip = delta_clip;
    a.idx = idx_or_null;
    hipLaunchKernelGGL(q_regress_loss_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("q_regress_loss_kernel");
}

static int check_cat(int64_t batch, int n_actions, int n_atoms, int stride) {
    if (batch <= 0 || n_actions <= 0 || n_actions > 64 || n_atoms < 2 || n_atoms > 64 || stride < n_atoms || (stride & 3)) {
        arl::set_error("catdqn: need batch > 0, 1 <= n_actions <= 64, 2 <= n_atoms <= 64, atom_stride >= n_atoms and %% 4 == 0");
        return ARL_E_RANGE;
    }
    return 0;
}

extern "C" int arl_catdqn_act(const float* logits, const float* z, const int32_t* override_or_null, int64_t batch,
                              int32_t n_actions, int32_t n_atoms, int32_t atom_stride, int32_t dueling, float* onehot,
                              uint8_t* greedy_or_null, void* stream) {
    ARL_REQUIRE(logits && z && onehot, ARL_E_ARG, "null pointer");
    int rc = check_cat(batch, n_actions, n_atoms, atom_stride);
    if (rc) return rc;
    hipLaunchKernelGGL(catdqn_act_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       logits, z, override_or_null, batch, n_actions, n_atoms, atom_stride, dueling != 0, onehot,
                       greedy_or_null);
    return arl::check_launch("catdqn_act_kernel");
}

extern "C" int arl_catdqn_loss(const float* pred_logits, const float* tgt_next_logits, const float* pol_next_logits_or_null,
                               const float* z, const uint8_t* actions, const float* returns, const uint8_t* terminals,
                               const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t n_atoms,
                               int32_t atom_stride, int32_t dueling, float v_min, float v_max, float gamma_n,
                               float* dlogits, float* loss_rows, float* kl, void* stream) {
    ARL_REQUIRE(pred_logits && tgt_next_logits && z && actions && returns && terminals && dlogits && loss_rows && kl,
                ARL_E_ARG, "null pointer");
    int rc = check_cat(batch, n_actions, n_atoms, atom_stride);
    if (rc) return rc;
    ARL_REQUIRE(v_max > v_min, ARL_E_ARG, "v_max must exceed v_min");
    CatLossArgs a = {};
    a.pred_logits = pred_logits; a.tgt_next_logits = tgt_next_logits; a.pol_next_logits = pol_next_logits_or_null;
    a.z = z; a.actions = actions; a.returns = returns; a.terminals = terminals; a.is_weights = is_weights_or_null;
    a.dlogits = dlogits; a.loss_rows = loss_rows; a.kl = kl; a.batch = batch;
    a.n_actions = n_actions; a.n_atoms = n_atoms; a.stride = atom_stride; a.dueling = dueling != 0;
    a.v_min = v_min; a.v_max = v_max; a.gamma_n = gamma_n;
    hipLaunchKernelGGL(catdqn_loss_kernel<-1>, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a, arlw::DgradWtArgs{});
    return arl::check_launch("catdqn_loss_kernel");
}

static int check_qr(int64_t batch, int n_actions, int n_quantiles, int stride) {
    if (batch <= 0 || batch > 0x7fffffffLL || n_actions <= 0 || n_actions > 64 || n_quantiles < 2 || n_quantiles > 64 ||
        stride < n_quantiles || (stride & 3) || stride > (1 << 20)) {
        arl::set_error("qrdqn: need 1 <= batch < 2^31, 1 <= n_actions <= 64, 2 <= n_quantiles <= 64, "
                       "n_quantiles <= q_stride <= 2^20 and q_stride %% 4 == 0");
        return ARL_E_RANGE;
    }
    return 0;
}

extern "C" int arl_qrdqn_act(const float* theta, const int32_t* override_or_null, int64_t batch, int32_t n_actions,
                             int32_t n_quantiles, int32_t q_stride, int32_t dueling, float* onehot,
                             uint8_t* greedy_or_null, void* stream) {
    ARL_REQUIRE(theta && onehot, ARL_E_ARG, "null pointer");
    int rc = check_qr(batch, n_actions, n_quantiles, q_stride);
    if (rc) return rc;
    hipLaunchKernelGGL(qrdqn_act_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       theta, override_or_null, batch, n_actions, n_quantiles, q_stride, dueling != 0, onehot,
                       greedy_or_null);
    return arl::check_launch("qrdqn_act_kernel");
}

extern "C" int arl_qrdqn_loss(const float* pred, const float* tgt_next, const float* pol_next_or_null,
                              const uint8_t* actions, const float* returns, const uint8_t* terminals,
                              const float* is_weights_or_null, int64_t batch, int32_t n_actions, int32_t n_quantiles,
                              int32_t q_stride, int32_t dueling, float gamma_n, float kappa, float* dtheta,
                              float* loss_rows, float* priorities, void* stream) {
    ARL_REQUIRE(pred && tgt_next && actions && returns && terminals && dtheta && loss_rows && priorities, ARL_E_ARG,
                "null pointer");
    int rc = check_qr(batch, n_actions, n_quantiles, q_stride);
    if (rc) return rc;
    ARL_REQUIRE(kappa >= 0.f && kappa <= 3.0e38f, ARL_E_ARG, "kappa must be finite and >= 0");
    QrLossArgs a = {};
    a.pred = pred; a.tgt_next = tgt_next; a.pol_next = pol_next_or_null; a.actions = actions; a.returns = returns;
    a.terminals = terminals; a.is_weights = is_weights_or_null; a.dtheta = dtheta; a.loss_rows = loss_rows;
    a.priorities = priorities; a.batch = batch; a.n_actions = n_actions; a.n = n_quantiles; a.stride = q_stride;
    a.dueling = dueling != 0; a.gamma_n = gamma_n; a.kappa = kappa;
    hipLaunchKernelGGL(qrdqn_loss_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("qrdqn_loss_kernel");
}

extern "C" int arl_catdqn_loss_parts(const arl_logit_src* pred, const arl_logit_src* tgt_next,
                                     const arl_logit_src* pol_next_or_null, const float* z, const uint8_t* actions,
                                     const float* returns, const uint8_t* terminals, const float* is_weights_or_null,
                                     int64_t batch, int32_t n_actions, int32_t n_atoms, int32_t atom_stride,
                                     int32_t dueling, float v_min, float v_max, float gamma_n, float* dlogits,
                                     float* loss_rows, float* kl, const arl_dgrad_wt* wt_items_or_null, int32_t n_wt,
                                     void* stream) {
    ARL_REQUIRE(pred && tgt_next && pred->part && tgt_next->part && z && actions && returns && terminals && dlogits &&
                    loss_rows && kl && (!pol_next_or_null || pol_next_or_null->part), ARL_E_ARG, "null pointer");
    int rc = check_cat(batch, n_actions, n_atoms, atom_stride);
    if (rc) return rc;
    ARL_REQUIRE(v_max > v_min, ARL_E_ARG, "v_max must exceed v_min");
    const arl_logit_src* in[3] = {pred, tgt_next, pol_next_or_null};
    CatLossArgs a = {};
    for (int i = 0; i < 3; ++i) {
        if (!in[i]) continue;
        ARL_REQUIRE(in[i]->splits >= 1 && in[i]->splits < 128 && in[i]->split_stride > 0, ARL_E_RANGE,
                    "logit source: 1 <= splits < 128 partial sums, split_stride > 0 (finished logits: one split, no bias)");
        a.src[i].p = in[i]->part; a.src[i].bias = in[i]->bias_or_null; a.src[i].ss = in[i]->split_stride;
        a.src[i].splits = in[i]->splits;
    }
    a.z = z; a.actions = actions; a.returns = returns; a.terminals = terminals; a.is_weights = is_weights_or_null;
    a.dlogits = dlogits; a.loss_rows = loss_rows; a.kl = kl; a.batch = batch;
    a.n_actions = n_actions; a.n_atoms = n_atoms; a.stride = atom_stride; a.dueling = dueling != 0;
    a.v_min = v_min; a.v_max = v_max; a.gamma_n = gamma_n;
    // all sources on the same power-of-two split count (the usual case: the same layer at two batch sizes): unrolled loads
    int ns = a.src[0].splits;
    for (int i = 1; i < 3; ++i)
        if (in[i] && a.src[i].splits != ns) ns = 0;
    arlw::DgradWtArgs wt = {};
    int wt_blocks = 0;
    if (wt_items_or_null && n_wt > 0) {
        rc = arlw::dgrad_wt_plan(wt_items_or_null, n_wt, &wt, &wt_blocks);
        if (rc) return rc;
    }
    const dim3 grid((unsigned)(batch + wt_blocks));
    hipStream_t st = (hipStream_t)stream;
    switch (ns) {
    case 1: hipLaunchKernelGGL(catdqn_loss_kernel<1>, grid, dim3(256), 0, st, a, wt); break;
    case 2: hipLaunchKernelGGL(catdqn_loss_kernel<2>, grid, dim3(256), 0, st, a, wt); break;
    case 4: hipLaunchKernelGGL(catdqn_loss_kernel<4>, grid, dim3(256), 0, st, a, wt); break;
    case 8: hipLaunchKernelGGL(catdqn_loss_kernel<8>, grid, dim3(256), 0, st, a, wt); break;
    case 16: hipLaunchKernelGGL(catdqn_loss_kernel<16>, grid, dim3(256), 0, st, a, wt); break;
    default: hipLaunchKernelGGL(catdqn_loss_kernel<0>, grid, dim3(256), 0, st, a, wt);
    }
    return arl::check_launch("catdqn_loss_kernel (parts)");
}

extern "C" int arl_noisy_catdqn_loss_limits(int32_t* max_splits, int32_t* max_actions, int32_t* max_atoms) {
    ARL_REQUIRE(max_splits && max_actions && max_atoms, ARL_E_ARG, "null pointer");
    *max_splits = ARL_NOISY_CATDQN_MAX_SPLITS;
    *max_actions = 64;
    *max_atoms = 64;
    return 0;
}

extern "C" int arl_noisy_catdqn_loss_parts(const arl_noisy_logit_src* pred, const arl_noisy_logit_src* tgt_next,
                                           const arl_noisy_logit_src* pol_next_or_null, const float* z,
                                           const uint8_t* actions, const float* returns, const uint8_t* terminals,
                                           const float* is_weights_or_null, int64_t batch, int32_t n_actions,
                                           int32_t n_atoms, int32_t atom_stride, int32_t dueling, float v_min,
                                           float v_max, float gamma_n, float* dlogits, float* loss_rows, float* kl,
                                           const arl_dgrad_wt* wt_items_or_null, int32_t n_wt, void* stream) {
    ARL_REQUIRE(pred && tgt_next && z && actions && returns && terminals && dlogits && loss_rows && kl, ARL_E_ARG,
                "null pointer");
    int rc = check_cat(batch, n_actions, n_atoms, atom_stride);
    if (rc) return rc;
    ARL_REQUIRE(v_max > v_min, ARL_E_ARG, "v_max must exceed v_min");
    const arl_noisy_logit_src* in[3] = {pred, tgt_next, pol_next_or_null};
    const int wide = arlc::fold_wide_from();
    CatLossArgs a = {};
    for (int i = 0; i < 3; ++i) {
        if (!in[i]) continue;
        const arl_noisy_logit_src& q = *in[i];
        ARL_REQUIRE(q.w_part && q.s_part && q.feout, ARL_E_ARG, "null pointer in a logit source");
        ARL_REQUIRE(q.w_splits >= 0 && q.s_splits >= 0 && (q.w_splits == 0 || q.w_split_stride > 0) &&
                    (q.s_splits == 0 || q.s_split_stride > 0), ARL_E_ARG, "logit source: negative splits or stride");
        ARL_REQUIRE(q.w_splits <= ARL_NOISY_CATDQN_MAX_SPLITS && q.s_splits <= ARL_NOISY_CATDQN_MAX_SPLITS, ARL_E_RANGE,
                    "logit source: more than ARL_NOISY_CATDQN_MAX_SPLITS splits (fold them first: "
                    "arl_noisy_dense_combine + arl_catdqn_loss)");
        NoisySrc& d = a.nsrc[i];
        d.pw = q.w_part; d.bias = q.bias_or_null; d.ps = q.s_part; d.b_sigma = q.b_sigma_or_null; d.feout = q.feout;
        d.ssw = q.w_split_stride; d.sss = q.s_split_stride; d.nw = q.w_splits; d.ns = q.s_splits;
        d.zw = q.w_splits >= wide ? 64 : 16; d.zs = q.s_splits >= wide ? 64 : 16;
    }
    a.z = z; a.actions = actions; a.returns = returns; a.terminals = terminals; a.is_weights = is_weights_or_null;
    a.dlogits = dlogits; a.loss_rows = loss_rows; a.kl = kl; a.batch = batch;
    a.n_actions = n_actions; a.n_atoms = n_atoms; a.stride = atom_stride; a.dueling = dueling != 0;
    a.v_min = v_min; a.v_max = v_max; a.gamma_n = gamma_n;
    arlw::DgradWtArgs wt = {};
    int wt_blocks = 0;
    if (wt_items_or_null && n_wt > 0) {
        rc = arlw::dgrad_wt_plan(wt_items_or_null, n_wt, &wt, &wt_blocks);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(catdqn_loss_kernel<-2>, dim3((unsigned)(batch + wt_blocks)), dim3(256), 0, (hipStream_t)stream,
                       a, wt);
    return arl::check_launch("catdqn_loss_kernel (noisy parts)");
}
