// Soft actor-critic for discrete actions (SAC-Discrete, Christodoulou 2019; not in the reference): everything after the
// last dense layers of the actor and of the two critics.
//
//   arl_sacd_act         the actor's soft-max row (the sampler's categorical kernel draws from it), or -- deterministic
//                        mode, or an override -- a one-hot row; greedy = first maximum of the logits
//   arl_sacd_loss        soft Bellman target from the two target critics and the actor on next_obs, the (Huber) TD loss of
//                        both online critics, the actor's loss and the policy's entropy on obs: three gradients and four
//                        statistics rows in one launch
//   arl_sacd_alpha_grad  d (alpha (H - H_target)) / d log_alpha from the entropy row, a fixed-order sum
//
// Rows f32[batch][stride] as arl_dqn_loss's; one lane per sample, every sum over the actions inside the lane with a
// ascending from 0 (formulas: include/accel_rl_hip.h).  The row soft-max sums, the first maximum and the TD loss of one
// error are csrc/q_loss_dev.h's -- the code arl_mdqn_loss and arl_dqn_loss run.  fp32, compiled with -ffp-contract=off:
// the operations and their order are part of the stated results.  No atomics: two runs give the same bits.

#include "arl_common.h"
#include "q_loss_dev.h"

namespace {

using namespace arlq;

__global__ __launch_bounds__(256) void sacd_act_kernel(const float* __restrict__ logits,
                                                       const int32_t* __restrict__ override_or_null, int64_t batch,
                                                       int n_actions, int stride, int deterministic,
                                                       float* __restrict__ prob, uint8_t* __restrict__ greedy) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const float* row = logits + b * stride;
    float* out = prob + b * n_actions;
    const int g = first_argmax(row, n_actions, false);
    const int ov = override_or_null ? override_or_null[b] : -1;
    if (ov >= 0 || deterministic) {
        const int act = ov >= 0 ? ov : g;
        for (int a = 0; a < n_actions; ++a) out[a] = a == act ? 1.f : 0.f;
    } else {
        const SoftRow r = soft_row(row, n_actions, false, 0.f, 1.f);
        for (int a = 0; a < n_actions; ++a) out[a] = expf(row[a] - r.v) / r.s;
    }
    if (greedy) greedy[b] = (uint8_t)g;
}

struct SacdLossArgs {
    const float* q1;                // online critics on obs                 [B][S]
    const float* q2;
    const float* q1t_next;          // target critics on next_obs            [B][S]
    const float* q2t_next;
    const float* logits;            // actor on obs                          [B][S]
    const float* logits_next;       // actor on next_obs                     [B][S]
    const uint8_t* actions;         // [B]
    const float* returns;           // [B]
    const uint8_t* terminals;       // [B]
    const float* is_weights;        // [B] or null
    const float* log_alpha;         // [1], read here: a captured graph sees every update of it
    float* dq1;                     // [B][S]
    float* dq2;
    float* dlogits;
    float* stats;                   // [4][B]: q_loss_rows | td_abs | pi_loss_rows | ent_rows
    int64_t batch;
    int n_actions, stride;
    float gamma_n, delta_clip;      // delta_clip <= 0: squared loss, unclipped priorities
};

// arl_dqn_loss's TD row without the dueling merge: row dq = exact zeros but for the taken action
__device__ __forceinline__ TdLoss sacd_td_row(const float* q, float* dq, int S, int act, float y, float w, float c) {
    const TdLoss t = td_loss(y - q[act], c);
    for (int k = 0; k < S; ++k) dq[k] = 0.f;
    dq[act] = -(w * t.slope);                                              // d = y - q, y carries no gradient
    return t;
}

__global__ __launch_bounds__(256) void sacd_loss_kernel(const SacdLossArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    const int A = a.n_actions, S = a.stride;
    const float alpha = expf(a.log_alpha[0]);
    const float fb = (float)a.batch;
    // soft value of next_obs under the actor and the smaller of the two target critics
    const float* ln = a.logits_next + b * S;
    const float* t1 = a.q1t_next + b * S;
    const float* t2 = a.q2t_next + b * S;
    const SoftRow sn = soft_row(ln, A, false, 0.f, 1.f);
    float soft = 0.f;
    for (int k = 0; k < A; ++k) {
        const float ck = ln[k] - sn.v;
        const float pi = expf(ck) / sn.s;
        soft += pi * (fminf(t1[k], t2[k]) - alpha * (ck - sn.tl));
    }
    const float keep = a.terminals[b] ? 0.f : 1.f;
    const float y = a.returns[b] + keep * (a.gamma_n * soft);
    int act = a.actions[b];
    if (act >= A) act = A - 1;                                             // (never outside the row)
    const float w = (a.is_weights ? a.is_weights[b] : 1.f) / fb;
    const float* c1 = a.q1 + b * S;
    const float* c2 = a.q2 + b * S;
    const TdLoss l1 = sacd_td_row(c1, a.dq1 + b * S, S, act, y, w, a.delta_clip);
    const TdLoss l2 = sacd_td_row(c2, a.dq2 + b * S, S, act, y, w, a.delta_clip);
    a.stats[b] = w * l1.loss + w * l2.loss;
    a.stats[a.batch + b] = (l1.p + l2.p) / 2.f;
    // the actor on obs against the smaller of the two online critics (which take no gradient from it)
    const float* lo = a.logits + b * S;
    const SoftRow sc = soft_row(lo, A, false, 0.f, 1.f);
    float J = 0.f, plp = 0.f;
    for (int k = 0; k < A; ++k) {
        const float ck = lo[k] - sc.v;
        const float pi = expf(ck) / sc.s;
        const float lp = ck - sc.tl;
        J += pi * (alpha * lp - fminf(c1[k], c2[k]));
        plp += pi * lp;
    }
    float* dl = a.dlogits + b * S;
    for (int k = 0; k < A; ++k) {
        const float ck = lo[k] - sc.v;
        const float pi = expf(ck) / sc.s;
        const float g = alpha * (ck - sc.tl) - fminf(c1[k], c2[k]);
        dl[k] = (pi * (g - J)) / fb;
    }
    for (int k = A; k < S; ++k) dl[k] = 0.f;
    a.stats[2 * a.batch + b] = J / fb;
    a.stats[3 * a.batch + b] = -plp;
}

// One 256-thread workgroup: thread t adds rows t, t + 256, ... to 0 in ascending order; the 256 partial sums are folded
// in LDS as s[t] += s[t + h], h = 128, 64, ... 1.
__global__ __launch_bounds__(256) void sacd_alpha_grad_kernel(const float* __restrict__ ent_rows, int64_t batch,
                                                              const float* __restrict__ log_alpha, float target_entropy,
                                                              float* __restrict__ grad_out) {
    __shared__ float s[256];
    const int t = threadIdx.x;
    float sum = 0.f;
    for (int64_t i = t; i < batch; i += 256) sum += ent_rows[i];
    s[t] = sum;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) s[t] += s[t + h];
        __syncthreads();
    }
    if (t == 0) grad_out[0] = expf(log_alpha[0]) * (s[0] / (float)batch - target_entropy);
    else if (t < 4) grad_out[t] = 0.f;
}

bool finite32(float x) { return x >= -3.0e38f && x <= 3.0e38f; }           // (a NaN fails)

int check_sacd(int64_t batch, int n_actions, int stride) {
    if (!q_sizes_ok(batch, n_actions, stride, 0) || batch > INT32_MAX) {
        arl::set_error("sacd: need 1 <= batch < 2^31, 1 <= n_actions <= 255, stride >= n_actions and %% 4 == 0");
        return ARL_E_RANGE;
    }
    return 0;
}

}  // namespace

extern "C" int arl_sacd_act(const float* logits, const int32_t* override_or_null, int64_t batch, int32_t n_actions,
                            int32_t stride, int32_t deterministic, float* prob, uint8_t* greedy_or_null, void* stream) {
    ARL_REQUIRE(logits && prob, ARL_E_ARG, "null pointer");
    int rc = check_sacd(batch, n_actions, stride);
    if (rc) return rc;
    hipLaunchKernelGGL(sacd_act_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits,
                       override_or_null, batch, n_actions, stride, deterministic != 0, prob, greedy_or_null);
    return arl::check_launch("sacd_act_kernel");
}

extern "C" int arl_sacd_loss(const float* q1, const float* q2, const float* q1t_next, const float* q2t_next,
                             const float* logits, const float* logits_next, const uint8_t* actions,
                             const float* returns, const uint8_t* terminals, const float* is_weights_or_null,
                             const float* log_alpha, int64_t batch, int32_t n_actions, int32_t stride, float gamma_n,
                             float delta_clip, float* dq1, float* dq2, float* dlogits, float* stats, void* stream) {
    ARL_REQUIRE(q1 && q2 && q1t_next && q2t_next && logits && logits_next && actions && returns && terminals &&
                    log_alpha && dq1 && dq2 && dlogits && stats, ARL_E_ARG, "null pointer");
    int rc = check_sacd(batch, n_actions, stride);
    if (rc) return rc;
    ARL_REQUIRE(finite32(gamma_n), ARL_E_ARG, "gamma_n must be finite");
    ARL_REQUIRE(finite32(delta_clip), ARL_E_ARG, "delta_clip must be finite");
    SacdLossArgs a = {};
    a.q1 = q1; a.q2 = q2; a.q1t_next = q1t_next; a.q2t_next = q2t_next; a.logits = logits; a.logits_next = logits_next;
    a.actions = actions; a.returns = returns; a.terminals = terminals; a.is_weights = is_weights_or_null;
    a.log_alpha = log_alpha; a.dq1 = dq1; a.dq2 = dq2; a.dlogits = dlogits; a.stats = stats; a.batch = batch;
    a.n_actions = n_actions; a.stride = stride; a.gamma_n = gamma_n; a.delta_clip = delta_clip;
    hipLaunchKernelGGL(sacd_loss_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("sacd_loss_kernel");
}

extern "C" int arl_sacd_alpha_grad(const float* ent_rows, int64_t batch, const float* log_alpha, float target_entropy,
                                   float* grad_out, void* stream) {
    ARL_REQUIRE(ent_rows && log_alpha && grad_out, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(batch >= 1 && batch <= INT32_MAX, ARL_E_RANGE, "1 <= batch < 2^31");
    ARL_REQUIRE(finite32(target_entropy), ARL_E_ARG, "target_entropy must be finite");
    hipLaunchKernelGGL(sacd_alpha_grad_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ent_rows, batch, log_alpha,
                       target_entropy, grad_out);
    return arl::check_launch("sacd_alpha_grad_kernel");
}
