// Shared helpers for the gfx950 kernels (internal; the public ABI is include/accel_rl_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

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
