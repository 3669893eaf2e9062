// Reset-aware BPTT (gfx950): the hand-over of the recurrent state from step t-1 to step t of the learner's forward scan
// when an environment may have been reset inside the batch (mid_batch_reset with a recurrent policy).
//
//   arl_seq_handover  <- accel_rl/policies/base.py:50-93 (reset_one: the state of a reset environment is zero before
//                        its next step), applied where the learner re-runs the steps of a stored batch
//
// One launch per forward step replaces the two copies of the plain scan (h_prev into the contiguous operand of the
// h_prev W_h product and into hprev_all's slice of step t, which feeds dW_h) and masks on the way: where the flag of
// row (j, t-1) is set the previous state of (j, t) is +0, else the stored value, bit for bit.  The LSTM's c_prev goes
// through the same launch into a per-row buffer that the cell and its backward read (df = dc c_prev uses the masked
// value); the GRU's elementwise h_prev is hprev_all's slice itself.  No arithmetic: a select between a copy and zero.
//
// Latency-bound by construction: nb x H elements per step (64 segments x 256 floats = 64 KiB per array, at most two
// read and three written).  No roofline figure is claimed and none has been measured.  One float4 per lane
// (H % 4 == 0, H <= 1024, as csrc/traj.hip), rows strided as the cell kernels address time slices.

#include "arl_common.h"

namespace {

struct HandoverArgs {
    const float* h_prev;    // [B][H] strided: h of step t-1
    const float* c_prev;    // [B][H] strided: c of step t-1, or null
    float* hp;              // [B][H] contiguous: the operand of h_prev W_h
    float* hprev_out;       // [B][H] strided: hprev_all's slice of step t
    float* cprev_out;       // [B][H] strided: the masked c_prev of step t, or null
    int64_t batch;
    int h4;                 // H / 4
    int64_t h_stride, c_stride, hprev_stride, cprev_out_stride;     // elements between rows (multiples of 4)
};

__global__ __launch_bounds__(256) void seq_handover_kernel(const HandoverArgs a, const arl::CellFlags fl) {
    const int h4 = a.h4;
    const int64_t total = a.batch * h4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / h4;
        const int q = (int)(i - b * h4);
        const bool keep = !fl.at(b);
        float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
        if (keep) h = reinterpret_cast<const float4*>(a.h_prev + b * a.h_stride)[q];
        reinterpret_cast<float4*>(a.hp)[i] = h;
        reinterpret_cast<float4*>(a.hprev_out + b * a.hprev_stride)[q] = h;
        if (a.c_prev) {
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
            if (keep) c = reinterpret_cast<const float4*>(a.c_prev + b * a.c_stride)[q];
            reinterpret_cast<float4*>(a.cprev_out + b * a.cprev_out_stride)[q] = c;
        }
    }
}

}  // namespace

// a strided float4 array: 16-byte aligned base, and (more than one row) a row stride that keeps every row aligned
#define ARL_HANDOVER_VEC(p, stride, batch)                                                                     \
    ARL_REQUIRE(!(p) || (arl::aligned16(p) && ((batch) == 1 || (stride) % 4 == 0)), ARL_E_ALIGN,              \
                #p ": 16-byte aligned rows (base and stride)")

extern "C" int arl_seq_handover(const float* h_prev, int64_t h_stride, const float* c_prev_or_null, int64_t c_stride,
                                const uint8_t* reset, const int32_t* idx_or_null, int64_t flag_row0,
                                int64_t flag_row_step, int64_t batch, int32_t hidden, float* hp, float* hprev_out,
                                int64_t hprev_stride, float* cprev_out_or_null, int64_t cprev_out_stride, void* stream) {
    ARL_REQUIRE(h_prev && reset && hp && hprev_out, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(!c_prev_or_null == !cprev_out_or_null, ARL_E_ARG, "c_prev and cprev_out go together (null pointer)");
    ARL_CELL_SIZES(batch, hidden);
    ARL_REQUIRE(hidden % 4 == 0 && hidden <= 1024, ARL_E_RANGE, "hidden must be a multiple of 4 and <= 1024");
    ARL_CELL_STRIDE(h_prev, h_stride, hidden, batch);
    ARL_CELL_STRIDE(c_prev_or_null, c_stride, hidden, batch);
    ARL_CELL_STRIDE(hprev_out, hprev_stride, hidden, batch);
    ARL_CELL_STRIDE(cprev_out_or_null, cprev_out_stride, hidden, batch);
    ARL_CELL_FLAGS(reset, flag_row0, flag_row_step, batch);
    ARL_HANDOVER_VEC(h_prev, h_stride, batch);
    ARL_HANDOVER_VEC(c_prev_or_null, c_stride, batch);
    ARL_HANDOVER_VEC(hp, 0, batch);
    ARL_HANDOVER_VEC(hprev_out, hprev_stride, batch);
    ARL_HANDOVER_VEC(cprev_out_or_null, cprev_out_stride, batch);
    HandoverArgs a = {h_prev, c_prev_or_null, hp, hprev_out, cprev_out_or_null, batch, (int)(hidden / 4),
                      h_stride, c_stride, hprev_stride, cprev_out_stride};
    const arl::CellFlags fl = {reset, idx_or_null, flag_row0, flag_row_step};
    hipLaunchKernelGGL(seq_handover_kernel, dim3(arl::stream_grid(batch * (hidden / 4), 256)), dim3(256), 0,
                       (hipStream_t)stream, a, fl);
    return arl::check_launch("seq_handover_kernel");
}
