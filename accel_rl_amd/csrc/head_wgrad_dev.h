// What head_kernel_dev.h's output-layer kernel and launcher stand on besides head_dev.h's wave helpers: the limits, the
// separate head weight-gradient kernel with its row splits, and the two host-side checks in front of a launch.
#pragma once
#include "arl_common.h"

namespace {

constexpr int HID_MAX = 1024;      // hidden width supported by the head kernels
constexpr int K_MAX = ARL_MAX_ACTIONS + 1;

// Partial head weight gradient: part[rs][k][c] = sum_{b in row split rs} dout[b][k] h[b][c] (splits part_stride apart),
// k == K holds the bias gradient (h := 1).  grid = (hid/64 column tiles, row splits); the
// 4 waves of a block take rows b = wave, wave+4, ... of the split; dout rows pass through LDS
// WG_CHUNK at a time (a multiple of the 4 waves: every wave walks its rows in the same order
// whatever the chunking), so the kernel's LDS does not grow with the batch.
// Folded over row splits by arl_fold_many (fixed order) => deterministic.
constexpr int WG_SPLITS = 16;
constexpr int WG_CHUNK = 256;
// the head kernel sums the head's weight gradient itself while its four LDS slices [4][K][hid] (next to the staged
// weights [K][hid]) fit 64 KB: K * hid <= 3 072, e.g. 5 x 512, 19 x 128
constexpr int FUSED_WGRAD_MAX = 3072;

__global__ __launch_bounds__(256) void head_wgrad_kernel(const float* __restrict__ dout,
                                                         const float* __restrict__ h, int batch,
                                                         int hid, int K, int Kp, int64_t part_stride,
                                                         float* __restrict__ part, float* __restrict__ part_b) {
    __shared__ float lds[4][K_MAX][64];
    __shared__ __attribute__((aligned(16))) float s_dout[WG_CHUNK * K_MAX];     // [rows of this chunk][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int rows_per = (batch + WG_SPLITS - 1) / WG_SPLITS;
    const int b0 = blockIdx.y * rows_per;
    const int b1 = (b0 + rows_per < batch) ? b0 + rows_per : batch;
    const int n_rows = b1 > b0 ? b1 - b0 : 0;
    float acc[K_MAX];
#pragma unroll
    for (int k = 0; k < K_MAX; ++k) acc[k] = 0.f;
    float sb = 0.f;                                                    // bias column `lane` (block 0, wave 1)
    for (int r0 = 0; r0 < n_rows; r0 += WG_CHUNK) {
        const int nr = n_rows - r0 < WG_CHUNK ? n_rows - r0 : WG_CHUNK;
        if (r0) __syncthreads();                                       // the previous chunk is read
        for (int i = threadIdx.x; i < nr * K; i += blockDim.x) s_dout[i] = dout[(int64_t)(b0 + r0) * K + i];
        __syncthreads();
        if (c < hid) {
            for (int r = wave; r < nr; r += 4) {
                const float hv = h[(int64_t)(b0 + r0 + r) * hid + c];
#pragma unroll
                for (int k = 0; k < K_MAX; ++k)
                    if (k < K) acc[k] += s_dout[r * K + k] * hv;
            }
        }
        if (blockIdx.x == 0 && wave == 1 && lane < K)
            for (int r = 0; r < nr; ++r) sb += s_dout[r * K + lane];
    }
#pragma unroll
    for (int k = 0; k < K_MAX; ++k) lds[wave][k][lane] = acc[k];
    __syncthreads();
    if (wave == 0 && c < hid) {
        for (int k = 0; k < K; ++k)
            part[(int64_t)blockIdx.y * part_stride + (int64_t)k * hid + c] =
                ((lds[0][k][lane] + lds[1][k][lane]) + lds[2][k][lane]) + lds[3][k][lane];
    }
    // bias gradient: part_b[split][Kp], column c < K holds sum_b dout[b][c] (Kp = K rounded up to 4, padding zero)
    if (blockIdx.x == 0 && wave == 1 && lane < Kp) part_b[(int64_t)blockIdx.y * Kp + lane] = sb;
}

int check_head(int64_t batch, int32_t hid, int32_t n_act) {
    if (batch <= 0 || batch > INT32_MAX || hid <= 0 || hid > HID_MAX || n_act <= 0 || n_act > ARL_MAX_ACTIONS) {
        arl::set_error("head: need 1 <= batch <= 2^31 - 1, 1 <= hid <= %d, 1 <= n_actions <= %d (ARL_MAX_ACTIONS)",
                       HID_MAX, ARL_MAX_ACTIONS);
        return ARL_E_RANGE;
    }
    return 0;
}

// A head kernel's dynamic LDS ([K][hid] staged weights, + [4][K][hid] slices when fused) reaches (ARL_MAX_ACTIONS + 1) *
// HID_MAX * 4 = 77 824 B: past 64 KiB the launch opts in explicitly, per launch (the attribute belongs to the CURRENT
// device's copy of the kernel); sizes up to 64 KiB launch exactly as before
template <typename Kern>
int head_allow_lds(Kern kernel, size_t lds) {
    static_assert((size_t)K_MAX * HID_MAX * 4 + 2048 <= 160 * 1024, "head kernel LDS must fit a CU");
    if (lds <= 65536) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { arl::set_error("hipFuncSetAttribute(head kernel, LDS %zu): %s", lds, hipGetErrorString(e)); return (int)e; }
    return 0;
}

}  // namespace
