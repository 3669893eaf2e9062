// V-MPO (single-GPU, feed-forward, synchronous variant) for gfx950: the three device stages the learner adds to the
// shared actor-critic machinery.
//
//   arl_vmpo_weights          top half of a minibatch's advantages (exact, ties to the lower position), psi = softmax(A /
//                             eta) over it, and the temperature's dual loss and gradient; one workgroup, no float atomics
//   arl_vmpo_head_loss_parts  policy / value heads + softmax + (-sum psi log pi(a)) + value loss + alpha * mean KL(old || pi)
//                             and their gradients in one pass: head_kernel_dev.h's kernel and launch with VmpoLoss
//   arl_vmpo_dual_step        one optimiser step on (eta, alpha) from the two stages' outputs, then max(x, 1e-8)
//
// include/accel_rl_hip.h states every expression and order.  fp32 where the head kernel is, float64 after the selection
// in the weights kernel; compiled with -ffp-contract=off.

#include <cmath>

#include "arl_optim_dev.h"
#include "head_kernel_dev.h"

namespace {

// ---------------------------------------------------------------- the head's loss

struct VmpoLoss {            // -psi log(p_a) + alpha * w * KL(old || p); lane k holds old_prob[row][k], HeadRow::adv is psi
    static constexpr bool TRAIN = true, WT = false;
    static constexpr const char* NAME = "vmpo_head_kernel";
    float alpha;
    __device__ explicit VmpoLoss(const HeadArgs& a) : alpha(a.duals[1]) {}
    __device__ void load(const HeadArgs& a, int64_t row, int A, int lane, HeadRow& m) const {
        m.ret = a.ret[row];
        m.act = a.actions[row];
        m.adv = a.adv[row];
        if (lane < A) m.old = a.old_prob[row * A + lane];
    }
    __device__ HeadTerms row(const HeadArgs&, const HeadRow& r, int A, int lane, float pk, float w) const {
        const float TINY = HEAD_TINY;
        const bool is_act = lane < A;
        const float old = r.old, psi = r.adv;
        const float pa = __shfl(pk, r.act, 64);
        const float lg = is_act ? logf(pk + TINY) : 0.f;
        const float kl_k = is_act ? old * (logf(old + TINY) - lg) : 0.f;
        const float qk = is_act ? old * pk / (pk + TINY) : 0.f;
        float kl = 0.f, sq = 0.f;
        for (int k = 0; k < A; ++k) { kl += readlane_f(kl_k, k); sq += readlane_f(qk, k); }
        // the weighted term through the softmax: g_k = -psi / (p_a + TINY) at k = a, else 0; sum_k g_k p_k = g_a p_a
        const float g_act = -psi / (pa + TINY);
        const float gk = (lane == r.act) ? g_act : 0.f;
        const float dot = g_act * pa;
        const float c = alpha * w;
        return {pk * (gk - dot) + c * (pk * sq - qk), -psi * logf(pa + TINY), w * kl};
    }
    static __device__ int dh_rows(int A) { return A + 1; }
};

// ---------------------------------------------------------------- top-half weights

constexpr int VW_THREADS = 1024;
constexpr float DUAL_FLOOR = 1e-8f;

// order-preserving uint32 of an fp32 value (+0 above -0)
__device__ __forceinline__ uint32_t vmpo_key(float a) {
    const uint32_t u = __float_as_uint(a);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float vmpo_unkey(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

// One workgroup.  Selection: a four-pass 8-bit radix select on the keys (LDS integer histogram) finds the n_top-th
// largest key T and how many keys equal to T belong to the top half; a block prefix count then hands those places to
// the ties in position order.  The keys are re-read from global memory in every pass.  Arithmetic: float64, thread t
// adds its positions t, t + 1024, ... in ascending order, the wave and the workgroup add in block_sum_d's fixed order.
__global__ __launch_bounds__(VW_THREADS) void vmpo_weights_kernel(const float* __restrict__ adv,
                                                                 const int32_t* __restrict__ idx, int n,
                                                                 const float* __restrict__ duals, double eps_eta,
                                                                 float* __restrict__ psi, float* __restrict__ temp4) {
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_sel[ARL_VMPO_MAX_ROWS / 32];      // bit b: position b is selected
    __shared__ unsigned s_pick[2];                           // the pass's bin | places left inside it
    __shared__ unsigned s_wave[VW_THREADS / 64];
    __shared__ unsigned s_max;
    __shared__ double s_red[VW_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_top = (n + 1) >> 1;
    auto row_of = [&](int b) { return idx ? (int64_t)idx[b] : (int64_t)b; };
    uint32_t prefix = 0, mask = 0;
    unsigned want = (unsigned)n_top;
    if (tid == 0) s_max = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) s_hist[tid] = 0u;
        __syncthreads();
        uint32_t mx = 0u;
        for (int b = tid; b < n; b += VW_THREADS) {
            const uint32_t k = vmpo_key(adv[row_of(b)]);
            if ((k & mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
            mx = k > mx ? k : mx;
        }
        if (pass == 0) atomicMax(&s_max, mx);
        __syncthreads();
        if (wave == 0) {        // lane l owns bins 255 - 4 l .. 252 - 4 l; exactly one lane holds the want-th largest key
            const int top = 255 - 4 * lane;
            const unsigned c0 = s_hist[top], c1 = s_hist[top - 1], c2 = s_hist[top - 2], c3 = s_hist[top - 3];
            const unsigned mine = (c0 + c1) + (c2 + c3);
            unsigned incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            unsigned above = incl - mine;
            if (above < want && want <= incl) {
                int bin = top;
                if (want > above + c0) { above += c0; bin = top - 1;
                    if (want > above + c1) { above += c1; bin = top - 2;
                        if (want > above + c2) { above += c2; bin = top - 3; } } }
                s_pick[0] = (unsigned)bin;
                s_pick[1] = want - above;
            }
        }
        __syncthreads();
        prefix |= s_pick[0] << shift;
        mask |= 0xFFu << shift;
        want = s_pick[1];
    }
    // prefix = the threshold key; want (>= 1) of the keys equal to it are selected, in position order
    unsigned base = 0u;
    for (int b0 = 0; b0 < n; b0 += VW_THREADS) {
        const int b = b0 + tid;
        const bool in = b < n;
        const uint32_t k = in ? vmpo_key(adv[row_of(b)]) : 0u;
        const bool tie = in && k == prefix;
        const unsigned long long tm = __ballot(tie);
        if (lane == 0) s_wave[wave] = (unsigned)__popcll(tm);
        __syncthreads();
        unsigned before = base, total = 0u;
        for (int w = 0; w < VW_THREADS / 64; ++w) {
            const unsigned c = s_wave[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        const unsigned rank = before + (unsigned)__popcll(tm & ((1ull << lane) - 1ull));
        const bool sel = in && (k > prefix || (tie && rank < want));
        const unsigned long long sm = __ballot(sel);
        if (lane == 0) {
            s_sel[(b0 >> 5) + 2 * wave] = (unsigned)sm;
            s_sel[(b0 >> 5) + 2 * wave + 1] = (unsigned)(sm >> 32);
        }
        base += total;
        __syncthreads();
    }
    const double eta = (double)duals[0];
    const double m = (double)vmpo_unkey(s_max);
    double s = 0.0;
    for (int b = tid; b < n; b += VW_THREADS)
        if ((s_sel[b >> 5] >> (b & 31)) & 1u) s += exp(((double)adv[row_of(b)] - m) / eta);
    const double S = arl::block_sum_d(s, s_red);
    double sa = 0.0;
    for (int b = tid; b < n; b += VW_THREADS) {
        const int64_t row = row_of(b);
        float out = 0.f;
        if ((s_sel[b >> 5] >> (b & 31)) & 1u) {
            const double a = (double)adv[row];
            const double p = exp((a - m) / eta) / S;
            sa += p * a;
            out = (float)p;
        }
        psi[row] = out;
    }
    const double SA = arl::block_sum_d(sa, s_red);
    if (tid == 0) {
        const double L = m / eta + log(S / (double)n_top);
        temp4[0] = (float)(eta * eps_eta + eta * L);
        temp4[1] = (float)((eps_eta + L) - SA / eta);
        temp4[2] = (float)L;
        temp4[3] = (float)n_top;
    }
}

// ---------------------------------------------------------------- the duals' step

// thread 0: eta on temp4[1]; thread 1: alpha on eps_alpha - loss4[2].  The step size is the flat-bucket update's
// (opt_update_block: t = step_count + 1, lr = lr_base * lr_mult[0], opt_step_size), the update update_one's.
template <int METHOD>
__global__ __launch_bounds__(64) void vmpo_dual_kernel(float* __restrict__ duals, float* __restrict__ slot0,
                                                       float* __restrict__ slot1, float* __restrict__ step_count,
                                                       const float* __restrict__ lr_mult,
                                                       const float* __restrict__ temp4, const float* __restrict__ loss4,
                                                       float eps_alpha, float lr_base, float b1, float b2, float eps) {
    const int i = threadIdx.x;
    const float t = step_count[0] + 1.0f;
    const float lr = lr_base * lr_mult[0];
    const float a_t = arl::opt_step_size<METHOD>(lr, b1, b2, t);
    if (i < 2) {
        const float g = i == 0 ? temp4[1] : eps_alpha - loss4[2];
        float p = duals[i], m = slot0[i], v = (METHOD == ARL_OPT_ADAM) ? slot1[i] : 0.f;
        arl::update_one<METHOD>(p, g, m, v, 1.f, 1.f, lr, a_t, b1, b2, eps);
        duals[i] = fmaxf(p, DUAL_FLOOR);
        slot0[i] = m;
        if (METHOD == ARL_OPT_ADAM) slot1[i] = v;
    }
    __syncthreads();                    // (every thread has read the old count)
    if (i == 0) step_count[0] = t;
}

}  // namespace

extern "C" int arl_vmpo_weights(const float* advantages, const int32_t* idx_or_null, int64_t n, const float* duals,
                                double eps_eta, float* psi, float* temp4, void* stream) {
    ARL_REQUIRE(advantages && duals && psi && temp4, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n >= 1 && n <= ARL_VMPO_MAX_ROWS, ARL_E_RANGE, "1 <= n <= ARL_VMPO_MAX_ROWS");
    ARL_REQUIRE(std::isfinite(eps_eta), ARL_E_ARG, "eps_eta must be finite");
    hipLaunchKernelGGL(vmpo_weights_kernel, dim3(1), dim3(VW_THREADS), 0, (hipStream_t)stream, advantages, idx_or_null,
                       (int)n, duals, eps_eta, psi, temp4);
    return arl::check_launch("vmpo_weights_kernel");
}

extern "C" int arl_vmpo_head_loss_parts(const float* h, const float* w_head, const float* b_head,
                                        const uint8_t* actions, const float* psi, const float* returns,
                                        const float* old_prob, const int32_t* idx_or_null, const float* duals,
                                        const float* inv_count_or_null, int64_t batch, int32_t hid, int32_t n_actions,
                                        float v_loss_coeff, int32_t relu_mask_dh, float* dout, float* dh,
                                        float* dw_head, float* db_head, float* loss4, void* workspace,
                                        arl_fold_item* items3, void* stream) {
    ARL_REQUIRE(h && w_head && b_head && actions && psi && returns && old_prob && duals && dout && dh && dw_head &&
                    db_head && loss4 && workspace && items3, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(std::isfinite(v_loss_coeff), ARL_E_ARG, "v_loss_coeff must be finite");
    int rc = check_head(batch, hid, n_actions);
    if (rc) return rc;
    HeadArgs a = {};
    a.h = h; a.w_head = w_head; a.b_head = b_head; a.actions = actions; a.adv = psi; a.ret = returns;
    a.old_prob = old_prob; a.idx = idx_or_null; a.inv_count = inv_count_or_null; a.duals = duals;
    a.dout = dout; a.dh = dh;
    a.batch = (int)batch; a.hid = hid; a.n_act = n_actions;
    a.v_coeff = v_loss_coeff;
    a.mask_dh = relu_mask_dh;
    // (no weight copies in this launch: the backward pass launches arl_conv2d_dgrad_weights itself)
    return head_loss_launch<VmpoLoss>(a, dw_head, db_head, loss4, workspace, items3, nullptr, 0, (hipStream_t)stream);
}

extern "C" int arl_vmpo_dual_step(float* duals, float* slot0, float* slot1_or_null, float* step_count,
                                  const float* lr_mult, const float* temp4, const float* loss4, float eps_alpha,
                                  int32_t method, float learning_rate, float beta1_or_rho, float beta2, float epsilon,
                                  void* stream) {
    ARL_REQUIRE(duals && slot0 && step_count && lr_mult && temp4 && loss4, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(method == ARL_OPT_ADAM || method == ARL_OPT_RMSPROP, ARL_E_ARG, "unknown method");
    ARL_REQUIRE(method != ARL_OPT_ADAM || slot1_or_null, ARL_E_ARG, "adam needs slot1");
    ARL_REQUIRE(std::isfinite(eps_alpha), ARL_E_ARG, "eps_alpha must be finite");
    // (arl_opt_step's own conditions, written so that a NaN fails)
    if (method == ARL_OPT_ADAM)
        ARL_REQUIRE(beta1_or_rho >= 0.f && beta1_or_rho < 1.f && beta2 >= 0.f && beta2 < 1.f, ARL_E_RANGE,
                    "adam: beta1 and beta2 in [0, 1)");
    else
        ARL_REQUIRE(beta1_or_rho >= 0.f && beta1_or_rho <= 1.f, ARL_E_RANGE, "rmsprop: rho in [0, 1]");
    ARL_REQUIRE(epsilon >= 0.f, ARL_E_RANGE, "epsilon negative or NaN");
    ARL_REQUIRE(learning_rate >= 0.f, ARL_E_RANGE, "learning_rate negative or NaN");
    hipStream_t s = (hipStream_t)stream;
    if (method == ARL_OPT_ADAM)
        hipLaunchKernelGGL((vmpo_dual_kernel<ARL_OPT_ADAM>), dim3(1), dim3(64), 0, s, duals, slot0, slot1_or_null,
                           step_count, lr_mult, temp4, loss4, eps_alpha, learning_rate, beta1_or_rho, beta2, epsilon);
    else
        hipLaunchKernelGGL((vmpo_dual_kernel<ARL_OPT_RMSPROP>), dim3(1), dim3(64), 0, s, duals, slot0, slot1_or_null,
                           step_count, lr_mult, temp4, loss4, eps_alpha, learning_rate, beta1_or_rho, beta2, epsilon);
    return arl::check_launch("vmpo_dual_kernel");
}
