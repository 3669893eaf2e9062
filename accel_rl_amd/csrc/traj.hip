// Whole-trajectory minibatches for recurrent policies (gfx950): one launch turns the segment numbers of a minibatch
// into everything the recurrent backward pass needs besides the batch itself.
//
//   arl_traj_minibatch  <- accel_rl/optimizers/util.py:21-32 (iterate_traj_idxs: the rows of the chosen segments)
//                          + accel_rl/algos/pg/aac_base.py:157-161 (only s[::horizon] of a stored state is used)
//                          + accel_rl/algos/pg/util.py:49-53 (valids_mean's 1 / sum(valids))
//
// Latency-bound by construction: at the sizes the learner uses (<= 256 segments x 512 floats of state) the launch
// moves well under 1 MiB.  One workgroup per chosen segment writes that segment's T row numbers and copies its
// stored initial state rows (one float4 per lane: H <= 1024); one more workgroup counts the minibatch's valid rows.
// The count is an integer sum, so its value does not depend on the order of the additions: same bits every run.

#include "arl_common.h"

namespace {

struct TrajStates {
    const float4* in[2];     // [n_traj_total * T][H / 4]
    float4* out[2];          // [n_seg][H / 4]
};

__global__ __launch_bounds__(256) void traj_minibatch_kernel(const int32_t* __restrict__ seg, int n_seg, int T,
                                                             TrajStates st, int n_state, int h4,
                                                             const int8_t* __restrict__ valids,
                                                             int32_t* __restrict__ idx, float* __restrict__ inv_count) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < n_seg) {
        const int j = blockIdx.x;
        const int64_t row0 = (int64_t)seg[j] * T;                 // the segment's first row in the batch
        for (int t = tid; t < T; t += 256) idx[(int64_t)j * T + t] = (int32_t)(row0 + t);
        for (int s = 0; s < n_state; ++s)
            for (int q = tid; q < h4; q += 256) st.out[s][(int64_t)j * h4 + q] = st.in[s][row0 * h4 + q];
        return;
    }
    // the extra workgroup (launched only with inv_count): 1 / number of valid rows of the minibatch
    __shared__ int32_t lds[4];
    const int64_t total = (int64_t)n_seg * T;                     // <= 2^31 - 1: the count fits an int32
    int32_t c = 0;
    if (valids) {
        for (int64_t i = tid; i < total; i += 256) {
            const int64_t j = i / T;
            c += valids[(int64_t)seg[j] * T + (i - j * T)] != 0 ? 1 : 0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if ((tid & 63) == 0) lds[tid >> 6] = c;
        __syncthreads();
        c = lds[0] + lds[1] + lds[2] + lds[3];
    } else {
        c = (int32_t)total;
    }
    if (tid == 0) inv_count[0] = c > 0 ? 1.f / (float)c : 0.f;    // no valid row at all: 0, never inf
}

}  // namespace

extern "C" int arl_traj_minibatch(const int32_t* seg, int32_t n_seg, int32_t horizon, int64_t n_traj_total,
                                  const float* const* state_in, int32_t n_state, int32_t hidden,
                                  const int8_t* valids_or_null, int32_t* idx, float* const* state_out,
                                  float* inv_count_or_null, void* stream) {
    ARL_REQUIRE(seg && idx, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n_state >= 0 && n_state <= 2, ARL_E_RANGE, "n_state outside 0 .. 2");
    ARL_REQUIRE(n_state == 0 || (state_in && state_out), ARL_E_ARG, "null pointer");
    for (int s = 0; s < n_state; ++s) ARL_REQUIRE(state_in[s] && state_out[s], ARL_E_ARG, "null pointer");
    ARL_REQUIRE(n_seg >= 1 && horizon >= 1 && n_traj_total >= 1, ARL_E_RANGE, "n_seg, horizon and n_traj_total must be >= 1");
    ARL_REQUIRE(hidden >= 0 && hidden % 4 == 0 && hidden <= 1024 && (n_state == 0 || hidden >= 4), ARL_E_RANGE,
                "hidden must be a multiple of 4 and <= 1024");
    ARL_REQUIRE((int64_t)n_seg * horizon <= INT32_MAX && n_traj_total <= INT32_MAX / (int64_t)horizon, ARL_E_RANGE,
                "row numbers must fit an int32 (n_seg * horizon, n_traj_total * horizon <= 2^31 - 1)");
    TrajStates st = {};
    for (int s = 0; s < n_state; ++s) {
        ARL_REQUIRE(arl::aligned16(state_in[s]) && arl::aligned16(state_out[s]), ARL_E_ALIGN, "states must be 16-byte aligned");
        st.in[s] = reinterpret_cast<const float4*>(state_in[s]);
        st.out[s] = reinterpret_cast<float4*>(state_out[s]);
    }
    const unsigned grid = (unsigned)n_seg + (inv_count_or_null ? 1u : 0u);
    hipLaunchKernelGGL(traj_minibatch_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, seg, (int)n_seg, (int)horizon, st,
                       (int)n_state, (int)(hidden / 4), valids_or_null, idx, inv_count_or_null);
    return arl::check_launch("traj_minibatch_kernel");
}
