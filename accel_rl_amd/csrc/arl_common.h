// Shared helpers for the gfx950 kernels (internal; the public ABI is include/accel_rl_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <cmath>

#include "accel_rl_hip.h"
#include "accel_rl_hip_dev.h"

#define ARL_WAVE 64

namespace arl {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

inline bool overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}
inline bool unit_interval(double x) { return x >= 0.0 && x <= 1.0; }      // (a NaN fails both comparisons)
inline bool finite_positive(double x) { return std::isfinite(x) && x > 0.0; }

struct Span { const void* p; int64_t bytes; };

// every non-null output against every input and every later output; false with the error set as "<fn>: .."
inline bool check_disjoint(const char* fn, const Span* in, int n_in, const Span* out, int n_out) {
    const char* clash = nullptr;
    for (int o = 0; o < n_out && !clash; ++o) {
        if (!out[o].p) continue;
        for (int i = 0; i < n_in && !clash; ++i)
            if (overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) clash = "an output must not overlap an input";
        for (int k = o + 1; k < n_out && !clash; ++k)
            if (out[k].p && overlap(out[o].p, out[o].bytes, out[k].p, out[k].bytes))
                clash = "the outputs must not overlap one another";
    }
    if (clash) set_error("%s: %s", fn, clash);
    return !clash;
}

// grid for a streaming kernel: enough blocks to fill 256 CUs x 8, never more than needed
inline unsigned stream_grid(int64_t work_items, int per_block) {
    int64_t b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (unsigned)b;
}

// Reset flags of the rows of one time step (reset-aware BPTT: csrc/handover.hip and the *_cell_bwd_reset kernels).
// Row b of the launch is compact row row0 + b * row_step of a [trajectory][time] batch (row0 = the time step,
// row_step = the horizon); its flag is reset[idx ? idx[compact row] : compact row], so a trajectory minibatch's row
// map (arl_traj_minibatch's idx) addresses the full batch's flags in place.
struct CellFlags {
    const uint8_t* reset;
    const int32_t* idx;
    int64_t row0, row_step;
    __device__ __forceinline__ bool at(int64_t b) const {
        const int64_t r = row0 + b * row_step;
        return reset[idx ? (int64_t)idx[r] : r] != 0;
    }
};

}  // namespace arl

#define ARL_REQUIRE(cond, code, msg)            \
    do {                                        \
        if (!(cond)) {                          \
            arl::set_error("%s: %s", __func__, msg); \
            return (code);                      \
        }                                       \
    } while (0)

// Limits shared by the three per-env float64 scans (csrc/qlambda_scan.hip, csrc/vtrace_scan.hip, arl_acer_retrace_scan in
// csrc/acer.hip; stated in accel_rl_hip.h): host-side comparisons before the launch.
#define ARL_ENV_SCAN_SIZES(n_env, horizon)                                                                     \
    do {                                                                                                       \
        ARL_REQUIRE((n_env) >= 1 && (n_env) <= INT32_MAX, ARL_E_RANGE, "1 <= n_env <= 2^31 - 1");              \
        ARL_REQUIRE((horizon) >= 1 && (horizon) <= 4096, ARL_E_RANGE, "1 <= horizon <= 4096");                 \
    } while (0)
#define ARL_ENV_SCAN_Q_STRIDE(q_stride, n_actions)                                                             \
    ARL_REQUIRE((q_stride) >= (n_actions) && ((q_stride) & 3) == 0 && (q_stride) <= (1 << 20), ARL_E_RANGE,    \
                "n_actions <= q_stride <= 2^20, q_stride % 4 == 0")

// Limits shared by the six recurrent-cell entry points (csrc/lstm.hip, csrc/gru.hip; stated in accel_rl_hip.h):
// host-side comparisons before the launch, no device work.
#define ARL_CELL_SIZES(batch, hidden)                                                                          \
    do {                                                                                                       \
        ARL_REQUIRE((batch) >= 1 && (batch) <= ARL_CELL_MAX_BATCH, ARL_E_RANGE, "1 <= batch <= 2^24");         \
        ARL_REQUIRE((hidden) >= 1 && (hidden) <= ARL_CELL_MAX_HIDDEN, ARL_E_RANGE, "1 <= hidden <= 2^20");     \
    } while (0)
// the row stride of a non-null strided array of more than one row: width <= stride <= 2^28
#define ARL_CELL_STRIDE(p, stride, width, batch)                                                               \
    ARL_REQUIRE(!(p) || (batch) == 1 || ((stride) >= (int64_t)(width) && (stride) <= ARL_CELL_MAX_STRIDE),    \
                ARL_E_RANGE, #stride ": row width <= stride <= 2^28")
// the flag rows of a step (arl::CellFlags): 0 <= row0, 1 <= row_step, last compact row <= 2^31 - 1 (an int32 row map)
#define ARL_CELL_FLAGS(reset, row0, row_step, batch)                                                           \
    ARL_REQUIRE(!(reset) || ((row0) >= 0 && (row0) <= INT32_MAX && (row_step) >= 1 && (row_step) <= INT32_MAX &&   \
                             (row0) + ((int64_t)(batch) - 1) * (row_step) <= INT32_MAX),                            \
                ARL_E_RANGE, "flag rows: 0 <= row0, 1 <= row_step, row0 + (batch - 1) row_step <= 2^31 - 1")
