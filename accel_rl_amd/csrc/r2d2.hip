// R2D2 (Kapturowski et al. 2019; the reference has none) on top of the replay memory of csrc/replay.hip (gfx950): the
// sequence layer -- stored recurrent states and reset flags next to the frame ring -- and the sequence loss.
//
//   arl_seq_store    append side: from one sampler batch, the recurrent state recorded BEFORE every step whose ring index
//                    is a multiple of the sequence stride goes into the state store, every step's reset flag into a ring
//   arl_seq_prepare  sample side: (env, slot) of a batch of sequences -> the expanded (env, step) lists that
//                    arl_replay_extract takes, the stored initial states and the reset flags of the sequences' rows
//   arl_r2d2_loss    n-step double-Q targets under the invertible value rescaling, the squared loss over the train window,
//                    its gradient through the dueling merge, |TD| and the mixed max / mean sequence priority
//
// The first two move values and compute none (bit for bit); both are latency-bound launches of one workgroup per
// environment / per sequence.  The loss is float64 from the float32 inputs in the order include/accel_rl_hip.h states,
// compiled with -ffp-contract=off and rounded to float32 once per output: one wave per sequence, lanes = train steps
// (argmax, target, TD error), then ONE lane walks the staged errors in time order for the two sums and the maximum, then
// the wave writes the sequence's whole dq block (zeros outside the train window included) in one pass of float4 stores.
// No atomics: two launches give the same bits.

#include "arl_common.h"
#include <cmath>

namespace {

struct SeqStates {
    const float4* in[2];
    float4* out[2];
};

// one workgroup per environment
__global__ __launch_bounds__(256) void seq_store_kernel(SeqStates st, int n_state, int h4, const uint8_t* __restrict__ resets,
                                                        int horizon, int size, int S, int idx,
                                                        uint8_t* __restrict__ reset_ring) {
    const int tid = threadIdx.x;
    const int64_t e = blockIdx.x;
    for (int t = tid; t < horizon; t += 256) reset_ring[e * size + (idx + t) % size] = resets[e * horizon + t];
    const int t0 = (S - idx % S) % S;                 // the first step of the batch whose ring index is a multiple of S
    const int n_slots = size / S;
    const int64_t per = (int64_t)(horizon / S) * h4;  // horizon % S == 0: exactly horizon / S such steps
    for (int s = 0; s < n_state; ++s)
        for (int64_t o = tid; o < per; o += 256) {
            const int k = (int)(o / h4), q = (int)(o - (int64_t)k * h4);
            const int t = t0 + k * S;
            const int slot = ((idx + t) % size) / S;
            st.out[s][(e * n_slots + slot) * h4 + q] = st.in[s][(e * horizon + t) * h4 + q];
        }
}

// one workgroup per sequence
__global__ __launch_bounds__(256) void seq_prepare_kernel(const int32_t* __restrict__ env, const int32_t* __restrict__ slot,
                                                          int U, int size, int S, SeqStates st, int n_state, int h4,
                                                          const uint8_t* __restrict__ reset_ring,
                                                          int32_t* __restrict__ env_rows, int32_t* __restrict__ step_rows,
                                                          uint8_t* __restrict__ resets_out) {
    const int tid = threadIdx.x;
    const int64_t j = blockIdx.x;
    const int64_t e = env[j], sl = slot[j];
    const int64_t first = sl * S;
    for (int t = tid; t < U; t += 256) {
        const int step = (int)((first + t) % size);
        env_rows[j * U + t] = (int32_t)e;
        step_rows[j * U + t] = step;
        resets_out[j * U + t] = reset_ring[e * size + step];
    }
    const int n_slots = size / S;
    for (int s = 0; s < n_state; ++s)
        for (int q = tid; q < h4; q += 256) st.out[s][j * h4 + q] = st.in[s][(e * n_slots + sl) * h4 + q];
}

struct R2d2Args {
    const float* q;                 // online net   [B * U][S]
    const float* q_tgt;             // target net   [B * U][S]
    const uint8_t* actions;         // [B * U]
    const float* returns;           // [B * U]
    const uint8_t* terminals;       // [B * U]
    const float* is_weights;        // [B] or null
    float* dq;                      // [B * U][S]
    float* td_abs;                  // [B][train_len]
    float* loss_rows;               // [B]
    float* priorities;              // [B]
    int batch, burn_in, train_len, n, n_actions, stride, dueling;
    double gamma_n, eps, eta;
};

// float64 twins of csrc/q_loss_dev.h's row helpers (the merge q_a = val + (adv_a - mean adv); the sum starts at 0.0, a ascending)
__device__ __forceinline__ double row_mean64(const float* row, int n) {
    double sum = 0.0;
    for (int a = 0; a < n; ++a) sum += (double)row[a];
    return sum / (double)n;
}
__device__ __forceinline__ double q_at64(const float* row, int a, int n, bool duel, double mean) {
    return duel ? (double)row[n] + ((double)row[a] - mean) : (double)row[a];
}
__device__ __forceinline__ double sign64(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

#define R2D2_MAX_TRAIN 1024

__global__ __launch_bounds__(64) void r2d2_loss_kernel(const R2d2Args a) {
    __shared__ double s_d[R2D2_MAX_TRAIN];          // the TD errors of the train window, unrounded
    __shared__ uint8_t s_act[R2D2_MAX_TRAIN];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int A = a.n_actions, S = a.stride, L = a.train_len;
    const int U = a.burn_in + L + a.n;
    const bool duel = a.dueling != 0;
    const int64_t row0 = b * U;
    const double eps = a.eps;

    for (int i = lane; i < L; i += 64) {
        const int64_t r = row0 + a.burn_in + i;
        const float* on_next = a.q + (r + a.n) * S;
        const float* tg_next = a.q_tgt + (r + a.n) * S;
        // a*: first maximum of the online row at t + n
        const double m_on = duel ? row_mean64(on_next, A) : 0.0;
        int best = 0;
        double best_q = q_at64(on_next, 0, A, duel, m_on);
        for (int k = 1; k < A; ++k) {
            const double v = q_at64(on_next, k, A, duel, m_on);
            if (v > best_q) { best_q = v; best = k; }
        }
        const double x = q_at64(tg_next, best, A, duel, duel ? row_mean64(tg_next, A) : 0.0);
        double hinv = x;
        if (eps > 0.0) {
            // the closed form ((s - 1) / (2 eps))^2 - 1 without its cancellation: with u = (s - 1) / (2 eps),
            // u - 1 = 2 |x| / (s + 1 + 2 eps) (from s^2 = (1 + 2 eps)^2 + 4 eps |x|) and u^2 - 1 = (u - 1) ((u - 1) + 2)
            const double s = sqrt(1.0 + (4.0 * eps) * ((fabs(x) + 1.0) + eps));
            const double dl = (2.0 * fabs(x)) / ((s + 1.0) + 2.0 * eps);
            hinv = sign64(x) * (dl * (dl + 2.0));
        }
        const double z = (double)a.returns[r] + (a.terminals[r] ? 0.0 : a.gamma_n * hinv);
        double y = z;
        if (eps > 0.0) y = sign64(z) * (sqrt(fabs(z) + 1.0) - 1.0) + eps * z;
        int act = a.actions[r];
        if (act >= A) act = A - 1;                                             // (never outside the row)
        const float* on = a.q + r * S;
        const double d = y - q_at64(on, act, A, duel, duel ? row_mean64(on, A) : 0.0);
        s_d[i] = d;
        s_act[i] = (uint8_t)act;
        a.td_abs[b * L + i] = (float)fabs(d);
    }
    __syncthreads();

    const double w = (a.is_weights ? (double)a.is_weights[b] : 1.0) / (double)((int64_t)a.batch * L);
    if (lane == 0) {                                                           // time order, from 0.0
        double sum_sq = 0.0, sum_abs = 0.0, mx = 0.0;
        for (int i = 0; i < L; ++i) {
            const double d = s_d[i], ad = fabs(d);
            sum_sq += 0.5 * (d * d);
            sum_abs += ad;
            if (ad > mx) mx = ad;
        }
        a.loss_rows[b] = (float)(w * sum_sq);
        a.priorities[b] = (float)(a.eta * mx + (1.0 - a.eta) * (sum_abs / (double)L));
    }

    // the sequence's dq block, every row: zeros outside the train window and outside the taken action (the merge's
    // shares when dueling); one float4 per lane and pass, each element written exactly once
    const int s4 = S >> 2;
    float4* dq4 = reinterpret_cast<float4*>(a.dq + row0 * S);
    const int64_t total4 = (int64_t)U * s4;
    for (int64_t o = lane; o < total4; o += 64) {
        const int t = (int)(o / s4), c0 = (int)(o - (int64_t)t * s4) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const int i = t - a.burn_in;
        if (i >= 0 && i < L) {
            const double gq = -(w * s_d[i]);                                   // d = y - q, y carries no gradient
            const int act = s_act[i];
            const double share = duel ? gq / (double)A : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + k;
                if (!duel) {
                    if (c == act) v[k] = (float)gq;
                } else if (c < A) {
                    v[k] = c == act ? (float)(gq - share) : (float)(-share);
                } else if (c == A) {
                    v[k] = (float)gq;
                }
            }
        }
        dq4[o] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

int fill_states(SeqStates& st, const float* const* in, float* const* out, int n_state) {
    for (int s = 0; s < n_state; ++s) {
        if (!arl::aligned16(in[s]) || !arl::aligned16(out[s])) return ARL_E_ALIGN;
        st.in[s] = reinterpret_cast<const float4*>(in[s]);
        st.out[s] = reinterpret_cast<float4*>(out[s]);
    }
    return 0;
}

}  // namespace

#define ARL_SEQ_STATES(in, out, n_state, hidden)                                                                   \
    do {                                                                                                           \
        ARL_REQUIRE((n_state) >= 0 && (n_state) <= 2, ARL_E_RANGE, "n_state outside 0 .. 2");                      \
        ARL_REQUIRE((n_state) == 0 || ((in) && (out)), ARL_E_ARG, "null pointer");                                 \
        for (int s_ = 0; s_ < (n_state); ++s_) ARL_REQUIRE((in)[s_] && (out)[s_], ARL_E_ARG, "null pointer");      \
        ARL_REQUIRE((hidden) >= 0 && (hidden) % 4 == 0 && (hidden) <= 1024 && ((n_state) == 0 || (hidden) >= 4),   \
                    ARL_E_RANGE, "hidden must be a multiple of 4 and <= 1024");                                    \
    } while (0)

extern "C" int arl_seq_store(const float* const* state_in, int32_t n_state, int32_t hidden, const uint8_t* resets,
                             int32_t n_env, int32_t horizon, int32_t size, int32_t seq_stride, int32_t idx,
                             float* const* state_store, uint8_t* reset_ring, void* stream) {
    ARL_REQUIRE(resets && reset_ring, ARL_E_ARG, "null pointer");
    ARL_SEQ_STATES(state_in, state_store, n_state, hidden);
    ARL_REQUIRE(n_env >= 1 && horizon >= 1 && size >= 1 && seq_stride >= 1, ARL_E_RANGE,
                "n_env, horizon, size and seq_stride must be >= 1");
    ARL_REQUIRE(horizon % seq_stride == 0 && size % seq_stride == 0 && horizon <= size, ARL_E_RANGE,
                "horizon and size must be multiples of seq_stride, horizon <= size");
    ARL_REQUIRE(idx >= 0 && idx < size, ARL_E_RANGE, "0 <= idx < size");
    SeqStates st = {};
    ARL_REQUIRE(fill_states(st, state_in, state_store, n_state) == 0, ARL_E_ALIGN, "states must be 16-byte aligned");
    hipLaunchKernelGGL(seq_store_kernel, dim3((unsigned)n_env), dim3(256), 0, (hipStream_t)stream, st, (int)n_state,
                       (int)(hidden / 4), resets, (int)horizon, (int)size, (int)seq_stride, (int)idx, reset_ring);
    return arl::check_launch("seq_store_kernel");
}

extern "C" int arl_seq_prepare(const int32_t* env, const int32_t* slot, int32_t batch, int32_t seq_len, int32_t size,
                               int32_t seq_stride, const float* const* state_store, int32_t n_state, int32_t hidden,
                               const uint8_t* reset_ring, int32_t* env_rows, int32_t* step_rows,
                               float* const* state_out, uint8_t* resets_out, void* stream) {
    ARL_REQUIRE(env && slot && reset_ring && env_rows && step_rows && resets_out, ARL_E_ARG, "null pointer");
    ARL_SEQ_STATES(state_store, state_out, n_state, hidden);
    ARL_REQUIRE(batch >= 1 && seq_len >= 1 && size >= 1 && seq_stride >= 1, ARL_E_RANGE,
                "batch, seq_len, size and seq_stride must be >= 1");
    ARL_REQUIRE(size % seq_stride == 0, ARL_E_RANGE, "size must be a multiple of seq_stride");
    ARL_REQUIRE((int64_t)batch * seq_len <= INT32_MAX, ARL_E_RANGE, "batch * seq_len <= 2^31 - 1");
    SeqStates st = {};
    ARL_REQUIRE(fill_states(st, state_store, state_out, n_state) == 0, ARL_E_ALIGN, "states must be 16-byte aligned");
    hipLaunchKernelGGL(seq_prepare_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, env, slot, (int)seq_len,
                       (int)size, (int)seq_stride, st, (int)n_state, (int)(hidden / 4), reset_ring, env_rows, step_rows,
                       resets_out);
    return arl::check_launch("seq_prepare_kernel");
}

extern "C" int arl_r2d2_loss(const float* q, const float* q_tgt, const uint8_t* actions, const float* returns,
                             const uint8_t* terminals, const float* is_weights_or_null, int32_t batch, int32_t burn_in,
                             int32_t train_len, int32_t n, int32_t n_actions, int32_t q_stride, int32_t dueling,
                             double gamma_n, double rescale_eps, double eta, float* dq, float* td_abs, float* loss_rows,
                             float* priorities, void* stream) {
    ARL_REQUIRE(q && q_tgt && actions && returns && terminals && dq && td_abs && loss_rows && priorities, ARL_E_ARG,
                "null pointer");
    ARL_REQUIRE(std::isfinite(gamma_n) && std::isfinite(rescale_eps) && std::isfinite(eta), ARL_E_ARG,
                "gamma_n, rescale_eps and eta must be finite");
    ARL_REQUIRE(batch >= 1 && train_len >= 1 && train_len <= R2D2_MAX_TRAIN && burn_in >= 0 && burn_in <= 1024 && n >= 1 &&
                    n <= ARL_REPLAY_MAX_HORIZON,
                ARL_E_RANGE, "need batch >= 1, 1 <= train_len <= 1024, 0 <= burn_in <= 1024, 1 <= n <= 16");
    ARL_REQUIRE(n_actions >= 1 && n_actions <= 255 && (q_stride & 3) == 0 && q_stride >= n_actions + (dueling != 0),
                ARL_E_RANGE, "need 1 <= n_actions <= 255, q_stride >= n_actions (+ 1 if dueling) and % 4 == 0");
    ARL_REQUIRE((int64_t)batch * (burn_in + train_len + n) <= INT32_MAX, ARL_E_RANGE,
                "batch * (burn_in + train_len + n) <= 2^31 - 1");
    ARL_REQUIRE(arl::aligned16(dq) && arl::aligned4(q) && arl::aligned4(q_tgt) && arl::aligned4(returns) &&
                    arl::aligned4(td_abs) && arl::aligned4(loss_rows) && arl::aligned4(priorities) &&
                    (!is_weights_or_null || arl::aligned4(is_weights_or_null)),
                ARL_E_ALIGN, "dq must be 16-byte, every other float pointer 4-byte aligned");
    R2d2Args a = {};
    a.q = q; a.q_tgt = q_tgt; a.actions = actions; a.returns = returns; a.terminals = terminals;
    a.is_weights = is_weights_or_null; a.dq = dq; a.td_abs = td_abs; a.loss_rows = loss_rows; a.priorities = priorities;
    a.batch = batch; a.burn_in = burn_in; a.train_len = train_len; a.n = n; a.n_actions = n_actions; a.stride = q_stride;
    a.dueling = dueling != 0; a.gamma_n = gamma_n; a.eps = rescale_eps; a.eta = eta;
    hipLaunchKernelGGL(r2d2_loss_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, a);
    return arl::check_launch("r2d2_loss_kernel");
}
