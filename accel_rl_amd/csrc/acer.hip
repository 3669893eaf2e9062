// ACER (Wang et al. 2017, "Sample Efficient Actor-Critic with Experience Replay"; the reference has none) for gfx950:
// everything the learner adds around the network's forward and backward passes.
//
//   arl_acer_retrace_scan  Retrace(lambda) targets of Q, backwards over a rollout from the CURRENT network's soft-max rows
//                          and Q rows against the behaviour policy the sampler recorded
//   arl_acer_loss          the output stage of one minibatch: truncated importance weight, bias correction, entropy,
//                          trust-region projection against the average network, soft-max backward and the Q regression,
//                          in one launch
//   arl_acer_avg_step      avg = alpha avg + (1 - alpha) params over the flat bucket
//   arl_gather_segments    dst segment i = src segment index[i], the index on the device
//
// include/accel_rl_hip.h states every expression and its order.  The scan calls no device-library function and is float64
// throughout; the loss takes the fp32 soft-max of csrc/q_loss_dev.h (the device code arl_sacd_loss runs) and is float64 from
// there on.  Compiled with -ffp-contract=off; no atomics, no process-wide state: two launches give the same bits.
#include <cmath>

#include "arl_common.h"
#include "q_loss_dev.h"

namespace {

using namespace arlq;

constexpr int AC_CHUNK = 1024;
constexpr double AC_EPS = 1e-6;

// V = sum_a p_a q_a in float64, a ascending, the sum starts at 0.0
__device__ __forceinline__ double acer_value(const float* p, const float* q, int n) {
    double v = 0.0;
    for (int a = 0; a < n; ++a) v = v + (double)p[a] * (double)q[a];
    return v;
}

// ---------------------------------------------------------------- Retrace scan

// One wave (a 64-thread block) per env, the rollout walked in chunks of AC_CHUNK steps from its end (29 KiB of LDS
// whatever the horizon).  Parallel part: lane l takes the chunk's steps l, l + 64, ..: V_t, rho_t, Q_t(a_t), r_t, done_t
// into LDS.  Sequential part: lane 0 walks the chunk downwards, carrying qret in a register across steps and chunks.
__global__ __launch_bounds__(64) void acer_retrace_kernel(
    const float* __restrict__ prob, const float* __restrict__ prob_last, const float* __restrict__ q,
    const float* __restrict__ q_last, int64_t q_stride, const float* __restrict__ old_prob,
    const uint8_t* __restrict__ actions, const float* __restrict__ rewards, const uint8_t* __restrict__ dones,
    double discount, double lambda, int T, int A, float* __restrict__ qret_out, float* __restrict__ v_out,
    float* __restrict__ stats) {
    __shared__ double v_s[AC_CHUNK];         // V_t
    __shared__ double rho_s[AC_CHUNK];       // rho_t
    __shared__ double qa_s[AC_CHUNK];        // Q_t(a_t)
    __shared__ float rr[AC_CHUNK];           // r_t, then (float) qret_t
    __shared__ uint8_t dd[AC_CHUNK];         // done_t
    const int64_t e = blockIdx.x;
    const int64_t row0 = e * T;
    const int lane = threadIdx.x;
    double qret = acer_value(prob_last + e * A, q_last + e * q_stride, A), rho_sum = 0.0;
    int n_above = 0;
    for (int hi = T; hi > 0; hi -= AC_CHUNK) {
        const int lo = hi > AC_CHUNK ? hi - AC_CHUNK : 0;
        const int len = hi - lo;
        for (int i = lane; i < len; i += 64) {
            const int64_t row = row0 + lo + i;
            int a = actions[row];
            a = a < A - 1 ? a : A - 1;
            const float* p = prob + row * A;
            const float* qr = q + row * q_stride;
            v_s[i] = acer_value(p, qr, A);
            rho_s[i] = (double)p[a] / ((double)old_prob[row * A + a] + AC_EPS);
            qa_s[i] = (double)qr[a];
            rr[i] = rewards[row];
            dd[i] = dones[row];
        }
        __syncthreads();
        if (lane == 0) {
            for (int i = len - 1; i >= 0; --i) {
                const double rho = rho_s[i];
                qret = (double)rr[i] + (dd[i] ? 0.0 : discount * qret);
                rr[i] = (float)qret;
                const double cbar = lambda * (rho < 1.0 ? rho : 1.0);
                qret = cbar * (qret - qa_s[i]) + v_s[i];
                rho_sum = rho_sum + rho;
                n_above += rho > 1.0 ? 1 : 0;
            }
        }
        __syncthreads();
        for (int i = lane; i < len; i += 64) {
            qret_out[row0 + lo + i] = rr[i];
            if (v_out) v_out[row0 + lo + i] = (float)v_s[i];
        }
        __syncthreads();                     // the next chunk's loads overwrite what these stores read
    }
    if (stats && lane == 0) {
        stats[2 * e] = (float)rho_sum;
        stats[2 * e + 1] = (float)n_above;
    }
}

// ---------------------------------------------------------------- head loss

struct AcerLossArgs {
    const float* out;               // live network             [B][2S]: logits | Q
    const float* out_avg;           // average network          [B][2S]: logits (its Q half is not read)
    const float* old_prob;          // behaviour policy         [n][A], row src
    const uint8_t* actions;         // [n], row src
    const float* qret;              // [n], row src
    const int32_t* idx;             // [B] or null: src = idx[b]
    float* dout;                    // [B][2S]
    float* stats;                   // [5][B]: pi_loss_rows | q_loss_rows | ent_rows | trust scale s | rho(a_t)
    int64_t batch;
    int n_actions, half;            // half = S
    double c, delta, q_coeff, ent_coeff;
};

// what one sample's passes over the actions share: the two soft-max rows, V, the taken action and its terms
struct AcerRow {
    const float* z;                 // logits of the live network
    const float* qv;                // its Q values
    const float* zb;                // logits of the average network
    const float* mu;                // behaviour row
    SoftRow sz, sb;
    int act;
    double V, adv, f_t;             // f_t = min(c, rho(a_t)) * adv
    double c, ent_coeff;
};

__device__ __forceinline__ float acer_pi(const float* z, const SoftRow& r, int a) { return expf(z[a] - r.v) / r.s; }

// g_a and k_a of the header, term by term
__device__ __forceinline__ void acer_gk(const AcerRow& r, int a, double& g, double& k) {
    const float ca = r.z[a] - r.sz.v;
    const double P = (double)(expf(ca) / r.sz.s);
    const double lp = (double)(ca - r.sz.tl);
    const double Pb = (double)acer_pi(r.zb, r.sb, a);
    const double rho = P / ((double)r.mu[a] + AC_EPS);
    const double t1 = a == r.act ? r.f_t / (P + AC_EPS) : 0.0;
    const double w = 1.0 - r.c / (rho + AC_EPS);
    const double t2 = (w > 0.0 ? w : 0.0) * ((double)r.qv[a] - r.V);
    const double t3 = r.ent_coeff * (lp + 1.0);
    g = (t1 + t2) - t3;
    k = -(Pb / (P + AC_EPS));
}

__global__ __launch_bounds__(256) void acer_loss_kernel(const AcerLossArgs p) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.batch) return;
    const int A = p.n_actions, S = p.half;
    const int64_t src = p.idx ? (int64_t)p.idx[b] : b;
    const double fb = (double)p.batch;
    AcerRow r;
    r.z = p.out + b * 2 * S;
    r.qv = r.z + S;
    r.zb = p.out_avg + b * 2 * S;
    r.mu = p.old_prob + src * A;
    r.sz = soft_row(r.z, A, false, 0.f, 1.f);
    r.sb = soft_row(r.zb, A, false, 0.f, 1.f);
    r.c = p.c;
    r.ent_coeff = p.ent_coeff;
    int act = p.actions[src];
    if (act >= A) act = A - 1;                                             // (never outside the row)
    r.act = act;
    const double qret = (double)p.qret[src];
    double V = 0.0, ent = 0.0;
    for (int a = 0; a < A; ++a) {
        const float ca = r.z[a] - r.sz.v;
        const double P = (double)(expf(ca) / r.sz.s);
        V = V + P * (double)r.qv[a];
        ent = ent + P * (double)(ca - r.sz.tl);
    }
    r.V = V;
    r.adv = qret - V;
    const double P_t = (double)acer_pi(r.z, r.sz, act);
    const double lp_t = (double)((r.z[act] - r.sz.v) - r.sz.tl);
    const double rho_t = P_t / ((double)r.mu[act] + AC_EPS);
    r.f_t = (rho_t < p.c ? rho_t : p.c) * r.adv;
    // the projection's two sums (and the objective's diagnostic row)
    double kg = 0.0, kk = 0.0, obj = r.f_t * lp_t;
    for (int a = 0; a < A; ++a) {
        double g, k;
        acer_gk(r, a, g, k);
        kg = kg + k * g;
        kk = kk + k * k;
        const float ca = r.z[a] - r.sz.v;
        const double P = (double)(expf(ca) / r.sz.s);
        const double w = 1.0 - p.c / (P / ((double)r.mu[a] + AC_EPS) + AC_EPS);
        obj = obj + (((w > 0.0 ? w : 0.0) * ((double)r.qv[a] - V)) * P) * (double)(ca - r.sz.tl);
    }
    double s = 0.0;
    if (kk > 0.0) {                                                        // an all-zero pibar row: no projection, no NaN
        s = (kg - p.delta) / kk;
        s = s > 0.0 ? s : 0.0;
    }
    double pz = 0.0;
    for (int a = 0; a < A; ++a) {
        double g, k;
        acer_gk(r, a, g, k);
        pz = pz + (double)acer_pi(r.z, r.sz, a) * (g - s * k);
    }
    float* d = p.dout + b * 2 * S;
    for (int j = 0; j < A; ++j) {
        double g, k;
        acer_gk(r, j, g, k);
        d[j] = (float)(-((double)acer_pi(r.z, r.sz, j) * ((g - s * k) - pz)) / fb);
    }
    for (int j = A; j < 2 * S; ++j) d[j] = 0.f;
    const double dq = (double)r.qv[act] - qret;
    d[S + act] = (float)((p.q_coeff * dq) / fb);
    p.stats[b] = (float)(-(obj + p.ent_coeff * -ent) / fb);
    p.stats[p.batch + b] = (float)(((0.5 * p.q_coeff) * (dq * dq)) / fb);
    p.stats[2 * p.batch + b] = (float)(-ent);
    p.stats[3 * p.batch + b] = (float)s;
    p.stats[4 * p.batch + b] = (float)rho_t;
}

// ---------------------------------------------------------------- average network

__device__ __forceinline__ float avg_one(float alpha, float beta, float a, float p) { return alpha * a + beta * p; }

template <bool VEC>
__global__ __launch_bounds__(256) void acer_avg_kernel(float* __restrict__ avg, const float* __restrict__ params,
                                                       int64_t n, float alpha, float beta) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        const int64_t n4 = n >> 2;
        float4* a4 = reinterpret_cast<float4*>(avg);
        const float4* p4 = reinterpret_cast<const float4*>(params);
        for (int64_t i = t; i < n4; i += stride) {
            const float4 a = a4[i], p = p4[i];
            a4[i] = make_float4(avg_one(alpha, beta, a.x, p.x), avg_one(alpha, beta, a.y, p.y),
                                avg_one(alpha, beta, a.z, p.z), avg_one(alpha, beta, a.w, p.w));
        }
        for (int64_t i = (n4 << 2) + t; i < n; i += stride) avg[i] = avg_one(alpha, beta, avg[i], params[i]);
    } else {
        for (int64_t i = t; i < n; i += stride) avg[i] = avg_one(alpha, beta, avg[i], params[i]);
    }
}

// ---------------------------------------------------------------- segment gather

// grid (segment, part): the parts of one segment's blocks stride over its 16-byte words (VEC) or its bytes
template <bool VEC>
__global__ __launch_bounds__(256) void gather_segments_kernel(const uint8_t* __restrict__ src,
                                                              const int32_t* __restrict__ index, int64_t n_src_seg,
                                                              int64_t seg_bytes, uint8_t* __restrict__ dst) {
    const int64_t i = blockIdx.x;
    int64_t s = index[i];
    s = s < 0 ? 0 : s;
    s = s > n_src_seg - 1 ? n_src_seg - 1 : s;
    const uint8_t* from = src + s * seg_bytes;
    uint8_t* to = dst + i * seg_bytes;
    const int64_t t = (int64_t)blockIdx.y * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.y * blockDim.x;
    if (VEC) {
        const uint4* f4 = reinterpret_cast<const uint4*>(from);
        uint4* t4 = reinterpret_cast<uint4*>(to);
        for (int64_t w = t; w < (seg_bytes >> 4); w += stride) t4[w] = f4[w];
    } else {
        for (int64_t w = t; w < seg_bytes; w += stride) to[w] = from[w];
    }
}

}  // namespace

extern "C" int arl_acer_retrace_scan(const float* prob, const float* prob_last, const float* q, const float* q_last,
                                     int32_t q_stride, const float* old_prob, const uint8_t* actions,
                                     const float* rewards, const uint8_t* dones, double discount, double lambda,
                                     int64_t n_env, int32_t horizon, int32_t n_actions, float* qret_out,
                                     float* v_out_or_null, float* stats_or_null, void* stream) {
    ARL_REQUIRE(prob && prob_last && q && q_last && old_prob && actions && rewards && dones && qret_out, ARL_E_ARG,
                "null pointer");
    ARL_ENV_SCAN_SIZES(n_env, horizon);
    ARL_REQUIRE(n_actions >= 1 && n_actions <= ARL_MAX_ACTIONS, ARL_E_RANGE, "1 <= n_actions <= 18");
    ARL_ENV_SCAN_Q_STRIDE(q_stride, n_actions);
    ARL_REQUIRE(arl::unit_interval(discount) && arl::unit_interval(lambda), ARL_E_ARG,
                "discount and lambda must lie in [0, 1]");
    const int64_t steps = n_env * horizon;
    // (the Q rows: from the first row's first entry to the last row's last action)
    const arl::Span in[8] = {
        {prob, steps * n_actions * 4}, {prob_last, n_env * n_actions * 4},
        {q, ((steps - 1) * q_stride + n_actions) * 4}, {q_last, ((n_env - 1) * q_stride + n_actions) * 4},
        {old_prob, steps * n_actions * 4}, {actions, steps}, {rewards, steps * 4}, {dones, steps}};
    const arl::Span out[3] = {{qret_out, steps * 4}, {v_out_or_null, steps * 4}, {stats_or_null, n_env * 8}};
    if (!arl::check_disjoint(__func__, in, 8, out, 3)) return ARL_E_ARG;
    ARL_REQUIRE(arl::aligned4(prob) && arl::aligned4(prob_last) && arl::aligned4(q) && arl::aligned4(q_last) &&
                arl::aligned4(old_prob) && arl::aligned4(rewards) && arl::aligned4(qret_out) &&
                arl::aligned4(v_out_or_null) && arl::aligned4(stats_or_null), ARL_E_ALIGN,
                "every float pointer must be 4-byte aligned");
    hipLaunchKernelGGL(acer_retrace_kernel, dim3((unsigned)n_env), dim3(64), 0, (hipStream_t)stream, prob, prob_last, q,
                       q_last, (int64_t)q_stride, old_prob, actions, rewards, dones, discount, lambda, (int)horizon,
                       (int)n_actions, qret_out, v_out_or_null, stats_or_null);
    return arl::check_launch("acer_retrace_kernel");
}

extern "C" int arl_acer_loss(const float* out, const float* out_avg, const float* old_prob, const uint8_t* actions,
                             const float* qret, const int32_t* idx_or_null, int64_t batch, int32_t n_actions,
                             int32_t half_stride, double c, double delta, double q_coeff, double ent_coeff, float* dout,
                             float* stats, void* stream) {
    ARL_REQUIRE(out && out_avg && old_prob && actions && qret && dout && stats, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(batch >= 1 && batch <= INT32_MAX, ARL_E_RANGE, "1 <= batch < 2^31");
    ARL_REQUIRE(n_actions >= 1 && n_actions <= ARL_MAX_ACTIONS, ARL_E_RANGE, "1 <= n_actions <= 18");
    ARL_REQUIRE(half_stride >= n_actions && (half_stride & 3) == 0 && half_stride <= (1 << 19), ARL_E_RANGE,
                "n_actions <= half_stride <= 2^19, half_stride % 4 == 0");
    ARL_REQUIRE(c > 0.0 && delta >= 0.0, ARL_E_ARG, "c must be > 0 and delta >= 0 (+inf allowed, NaN not)");
    ARL_REQUIRE(std::isfinite(q_coeff) && std::isfinite(ent_coeff), ARL_E_ARG, "q_coeff and ent_coeff must be finite");
    const int64_t row_bytes = batch * 2 * half_stride * 4;
    ARL_REQUIRE(!arl::overlap(dout, row_bytes, out, row_bytes) && !arl::overlap(dout, row_bytes, out_avg, row_bytes) &&
                !arl::overlap(stats, batch * 20, out, row_bytes) && !arl::overlap(stats, batch * 20, out_avg, row_bytes) &&
                !arl::overlap(stats, batch * 20, dout, row_bytes), ARL_E_ARG, "dout and stats must not overlap out, "
                "out_avg or one another");
    ARL_REQUIRE(arl::aligned4(out) && arl::aligned4(out_avg) && arl::aligned4(old_prob) && arl::aligned4(qret) &&
                arl::aligned4(idx_or_null) && arl::aligned4(dout) && arl::aligned4(stats), ARL_E_ALIGN,
                "every float pointer and idx must be 4-byte aligned");
    AcerLossArgs a = {};
    a.out = out; a.out_avg = out_avg; a.old_prob = old_prob; a.actions = actions; a.qret = qret; a.idx = idx_or_null;
    a.dout = dout; a.stats = stats; a.batch = batch; a.n_actions = n_actions; a.half = half_stride; a.c = c;
    a.delta = delta; a.q_coeff = q_coeff; a.ent_coeff = ent_coeff;
    hipLaunchKernelGGL(acer_loss_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return arl::check_launch("acer_loss_kernel");
}

extern "C" int arl_acer_avg_step(float* avg, const float* params, int64_t n, float alpha, void* stream) {
    ARL_REQUIRE(avg && params, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(alpha >= 0.f && alpha <= 1.f, ARL_E_ARG, "alpha must lie in [0, 1]");          // (a NaN fails)
    ARL_REQUIRE(n >= 1 && n <= INT32_MAX, ARL_E_RANGE, "1 <= n < 2^31");
    ARL_REQUIRE(!arl::overlap(avg, n * 4, params, n * 4), ARL_E_ARG, "avg must not overlap params");
    ARL_REQUIRE(arl::aligned4(avg) && arl::aligned4(params), ARL_E_ALIGN, "avg and params must be 4-byte aligned");
    const float beta = 1.f - alpha;
    const bool vec = arl::aligned16(avg) && arl::aligned16(params);
    const unsigned grid = arl::stream_grid(vec ? (n + 3) / 4 : n, 256);
    if (vec)
        hipLaunchKernelGGL(acer_avg_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, avg, params, n, alpha, beta);
    else
        hipLaunchKernelGGL(acer_avg_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, avg, params, n, alpha,
                           beta);
    return arl::check_launch("acer_avg_kernel");
}

extern "C" int arl_gather_segments(const void* src, const int32_t* index, int64_t n_seg, int64_t n_src_seg,
                                   int64_t seg_bytes, void* dst, void* stream) {
    ARL_REQUIRE(src && index && dst, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n_seg >= 1 && n_seg <= INT32_MAX && n_src_seg >= 1 && n_src_seg <= INT32_MAX, ARL_E_RANGE,
                "1 <= n_seg, n_src_seg <= 2^31 - 1");
    ARL_REQUIRE(seg_bytes >= 1 && seg_bytes <= ((int64_t)1 << 31), ARL_E_RANGE, "1 <= seg_bytes <= 2^31");
    ARL_REQUIRE(!arl::overlap(dst, n_seg * seg_bytes, src, n_src_seg * seg_bytes) &&
                !arl::overlap(dst, n_seg * seg_bytes, index, n_seg * 4), ARL_E_ARG, "dst must not overlap src or index");
    ARL_REQUIRE(arl::aligned4(index), ARL_E_ALIGN, "index must be 4-byte aligned");
    const bool vec = (seg_bytes & 15) == 0 && arl::aligned16(src) && arl::aligned16(dst);
    const int64_t items = vec ? seg_bytes >> 4 : seg_bytes;
    int64_t parts = (items + 256 * 4 - 1) / (256 * 4);                     // about four copies per thread
    parts = parts < 1 ? 1 : (parts > 64 ? 64 : parts);
    const dim3 grid((unsigned)n_seg, (unsigned)parts);
    if (vec)
        hipLaunchKernelGGL(gather_segments_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream,
                           static_cast<const uint8_t*>(src), index, n_src_seg, seg_bytes, static_cast<uint8_t*>(dst));
    else
        hipLaunchKernelGGL(gather_segments_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream,
                           static_cast<const uint8_t*>(src), index, n_src_seg, seg_bytes, static_cast<uint8_t*>(dst));
    return arl::check_launch("gather_segments_kernel");
}
