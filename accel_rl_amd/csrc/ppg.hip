// Phasic policy gradient (single-network variant) for gfx950: the output stage of both phases.
//
//   arl_ppg_head_loss_parts   policy / value heads + softmax + the phase's losses and their gradients in one pass
//       ARL_PPG_POLICY  PPO's clipped surrogate, value and entropy losses; the value gradient stops at the last shared
//                       layer (dh leaves the value row out, dw_head / db_head keep it)
//       ARL_PPG_AUX     value regression + beta_clone * KL(old || new) on stored rollouts; dh takes every row
//
// The kernel and its launch are head_kernel_dev.h's, the ones learner.hip's A2C / PPO entry runs: this file adds the two
// phases' losses and the entry's own argument checks.  All fp32; compiled with -ffp-contract=off.

#include <cmath>

#include "head_kernel_dev.h"

namespace {

struct PpgPolicyLoss {       // PgLoss's kind 1 without valids; the value row's gradient stays in the head
    static constexpr bool TRAIN = true, WT = false;
    static constexpr const char* NAME = "ppg_head_kernel<policy>";
    float clip;
    __device__ explicit PpgPolicyLoss(const HeadArgs& a) : clip(a.clip_param * a.lr_mult[0]) {}
    __device__ void load(const HeadArgs& a, int64_t row, int A, int, HeadRow& m) const {
        m.ret = a.ret[row];
        m.act = a.actions[row];
        m.adv = a.adv[row];
        m.old = a.old_prob[row * A + m.act];
    }
    __device__ HeadTerms row(const HeadArgs& a, const HeadRow& r, int A, int lane, float pk, float w) const {
        return pg_row(a, r, true, clip, A, lane, pk, w);
    }
    static __device__ int dh_rows(int A) { return A; }
};

struct PpgAuxLoss {          // c * KL(old || p), c = beta_clone * w; lane k holds old_prob[row][k]
    static constexpr bool TRAIN = true, WT = false;
    static constexpr const char* NAME = "ppg_head_kernel<aux>";
    __device__ explicit PpgAuxLoss(const HeadArgs&) {}
    __device__ void load(const HeadArgs& a, int64_t row, int A, int lane, HeadRow& m) const {
        m.ret = a.ret[row];
        if (lane < A) m.old = a.old_prob[row * A + lane];
    }
    __device__ HeadTerms row(const HeadArgs& a, const HeadRow& r, int A, int lane, float pk, float w) const {
        const float TINY = HEAD_TINY;
        const bool is_act = lane < A;
        const float old = r.old;
        const float lg = is_act ? logf(pk + TINY) : 0.f;
        const float c = a.beta_clone * w;
        const float kl_k = is_act ? old * (logf(old + TINY) - lg) : 0.f;
        const float qk = is_act ? old * pk / (pk + TINY) : 0.f;
        float kl = 0.f, sq = 0.f;
        for (int k = 0; k < A; ++k) { kl += readlane_f(kl_k, k); sq += readlane_f(qk, k); }
        return {c * (pk * sq - qk), c * kl, 0.f};
    }
    static __device__ int dh_rows(int A) { return A + 1; }
};

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
    HeadArgs a = {};
    a.h = h; a.w_head = w_head; a.b_head = b_head; a.actions = actions; a.adv = advantages; a.ret = returns;
    a.old_prob = old_prob; a.idx = idx_or_null; a.lr_mult = lr_mult; a.inv_count = inv_count_or_null;
    a.dout = dout; a.dh = dh;
    a.batch = (int)batch; a.hid = hid; a.n_act = n_actions; a.tie_rule = tie_rule;
    a.clip_param = clip_param; a.v_coeff = v_loss_coeff; a.ent_coeff = ent_loss_coeff; a.beta_clone = beta_clone;
    a.mask_dh = relu_mask_dh;
    // (no weight copies in this launch: the backward pass launches arl_conv2d_dgrad_weights itself)
    return aux ? head_loss_launch<PpgAuxLoss>(a, dw_head, db_head, loss4, workspace, items3, nullptr, 0, s)
               : head_loss_launch<PpgPolicyLoss>(a, dw_head, db_head, loss4, workspace, items3, nullptr, 0, s);
}
