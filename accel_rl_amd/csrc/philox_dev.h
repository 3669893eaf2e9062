// Philox4x32-10 (Salmon et al. 2011), the counter-based generator of every device-side draw (csrc/noisy.hip: Gaussian
// layer noise; csrc/iqn.hip: uniform quantile fractions).  Internal; the streams' keys and counters are stated in
// include/accel_rl_hip.h.
#pragma once

#include <stdint.h>

namespace arlp {

constexpr uint32_t PH_M0 = 0xD2511F53u, PH_M1 = 0xCD9E8D57u, PH_W0 = 0x9E3779B9u, PH_W1 = 0xBB67AE85u;

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        if (i > 0) { k0 += PH_W0; k1 += PH_W1; }
        const uint64_t p0 = (uint64_t)PH_M0 * c[0], p1 = (uint64_t)PH_M1 * c[2];
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    }
}

}  // namespace arlp
