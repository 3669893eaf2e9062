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
