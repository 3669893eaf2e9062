// Learner glue for gfx950: everything around the policy's conv / GEMM calls that
// the reference expresses as Theano graph nodes (and PyTorch would run as ~150
// tiny elementwise / reduction launches per minibatch), as a handful of fused,
// HBM-bound streaming kernels over channels-last activations.
//
//   arl_gather_scale_obs_nhwc  minibatch gather + u8 -> f32 * (1/255), NCHW u8 -> NHWC f32
//                              (optimizers/util.py:86-89 `s[idxs]`, policies/layers.py:22-41)
//   arl_bias_relu              x[M][C] = relu(x + b[c])          (Lasagne Conv2D/Dense b + rectify)
//   arl_relu_bwd_bias_grad     dy *= (y > 0); db[c] = sum_m dy   (their backward), deterministic
//   arl_pg_head_loss           policy/value heads + softmax + A2C / PPO / value / entropy losses
//                              and their gradients in one pass
//                              (policies/pg/networks/pg_cnn.py:70-86; algos/pg/aac_base.py:60-70;
//                               a2c.py:43-46; ppo.py:42-51; distributions/categorical.py:35-88)
//   arl_pg_head_wgrad          dW_head = dout^T h, db_head = colsum(dout)
//   arl_pg_head_infer          heads + softmax for action serving (atari_cnn_policy.py:67,109)
// (the heads' kernel and launcher are head_kernel_dev.h's, shared with ppg.hip: this file holds their two losses)
//
// All fp32 (the reference's floatX); compiled with -ffp-contract=off.

#include "arl_common.h"
#include "head_kernel_dev.h"

namespace {

// ---------------------------------------------------------------- gather NCHW u8 -> NHWC f32 (C = 4)
// one lane: 4 consecutive pixels of all 4 planes -> 4 float4 (64 B) stores
__global__ __launch_bounds__(256) void gather_nhwc4_kernel(const uint8_t* __restrict__ obs,
                                                           const int32_t* __restrict__ idx,
                                                           int64_t batch, int plane, float scale,
                                                           float* __restrict__ out) {
    const int q_per_row = plane >> 2;                       // 4-pixel groups per plane
    const int64_t total = batch * q_per_row;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t b = i / q_per_row;
        const int q = (int)(i - b * q_per_row);
        const int64_t src = (idx ? (int64_t)idx[b] : b) * 4 * plane;
        uint32_t w[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            w[c] = *reinterpret_cast<const uint32_t*>(obs + src + (int64_t)c * plane + (q << 2));
        // The 4 lanes of a quad hold 16 consecutive pixels (same image: plane % 16 == 0 keeps quads inside
        // one row of groups).  Transposed inside the quad, store p of lane j writes pixel 4p + j, so every
        // store instruction covers whole 64-byte runs instead of 16-byte pieces of four different ones.
        const int j = threadIdx.x & 3;
        float4* o = reinterpret_cast<float4*>(out) + (b * plane + ((q & ~3) << 2)) + j;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            uint32_t v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                v[c] = (uint32_t)__shfl((int)w[c], (threadIdx.x & ~3) | p, 64) >> (8 * j);
            o[4 * p] = make_float4((float)(v[0] & 255u) * scale, (float)(v[1] & 255u) * scale,
                                   (float)(v[2] & 255u) * scale, (float)(v[3] & 255u) * scale);
        }
    }
}

// ---------------------------------------------------------------- bias + relu, in place
__global__ __launch_bounds__(256) void bias_relu_kernel(float4* __restrict__ x,
                                                        const float4* __restrict__ bias,
                                                        int64_t total4, int c4) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += stride) {
        const float4 b = bias[i % c4];
        float4 v = x[i];
        v.x = fmaxf(v.x + b.x, 0.f); v.y = fmaxf(v.y + b.y, 0.f);
        v.z = fmaxf(v.z + b.z, 0.f); v.w = fmaxf(v.w + b.w, 0.f);
        x[i] = v;
    }
}

// ---------------------------------------------------------------- relu backward + bias grad
// thread -> (row lane rl, float4 column cg); fixed-order reductions => deterministic.
__global__ __launch_bounds__(256) void relu_bwd_bias_kernel(float4* __restrict__ dy,
                                                            const float4* __restrict__ y, int64_t m,
                                                            int c4, float4* __restrict__ partials) {
    __shared__ float4 lds[256];
    const int rows_per_iter = 256 / c4;
    const int cg = threadIdx.x % c4, rl = threadIdx.x / c4;
    float4 acc = make_float4(0, 0, 0, 0);
    if (rl < rows_per_iter) {
        for (int64_t row = (int64_t)blockIdx.x * rows_per_iter + rl; row < m;
             row += (int64_t)gridDim.x * rows_per_iter) {
            const int64_t i = row * c4 + cg;
            float4 g = dy[i];
            const float4 a = y[i];
            g.x = a.x > 0.f ? g.x : 0.f; g.y = a.y > 0.f ? g.y : 0.f;
            g.z = a.z > 0.f ? g.z : 0.f; g.w = a.w > 0.f ? g.w : 0.f;
            dy[i] = g;
            acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
        }
    }
    lds[threadIdx.x] = acc;
    __syncthreads();
    if (rl == 0) {
        float4 s = make_float4(0, 0, 0, 0);
        for (int r = 0; r < rows_per_iter; ++r) {
            const float4 v = lds[r * c4 + cg];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        partials[(int64_t)blockIdx.x * c4 + cg] = s;
    }
}

// out[c] = sum_g partials[g][c].  Block = 64 columns x 16 waves: wave w sums the rows
// g = w, w+16, ... (coalesced 256-B loads, independent accumulators), then the 16 wave
// sums are folded in a fixed order => deterministic and ~16x shorter dependency chains
// than one thread walking all partials.
__global__ __launch_bounds__(1024) void fold_partials_kernel(const float* __restrict__ partials,
                                                             int n_partials, int width,
                                                             float* __restrict__ out) {
    __shared__ float lds[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float s0 = 0.f, s1 = 0.f;
    if (c < width) {
        int g = wave;
        for (; g + 16 < n_partials; g += 32) {
            s0 += partials[(int64_t)g * width + c];
            s1 += partials[(int64_t)(g + 16) * width + c];
        }
        if (g < n_partials) s0 += partials[(int64_t)g * width + c];
    }
    lds[wave][lane] = s0 + s1;
    __syncthreads();
    if (wave == 0 && c < width) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) s += lds[w][lane];
        out[c] = s;
    }
}

// ---------------------------------------------------------------- heads (head_kernel_dev.h: head_kernel<Loss, HVT>)

struct InferLoss {           // action serving: probabilities and values are the output
    static constexpr bool TRAIN = false, WT = false;
    static constexpr const char* NAME = "head_kernel<infer>";
    __device__ explicit InferLoss(const HeadArgs&) {}
};

struct PgLoss {              // A2C (kind 0) / PPO (kind 1): a runtime branch, one set of instantiations for both
    static constexpr bool TRAIN = true, WT = true;
    static constexpr const char* NAME = "head_kernel<train>";
    float clip;
    __device__ explicit PgLoss(const HeadArgs& a) : clip(a.clip_param * a.lr_mult[0]) {}
    __device__ void load(const HeadArgs& a, int64_t row, int A, int, HeadRow& m) const {
        m.act = a.actions[row];
        m.adv = a.adv[row]; m.ret = a.ret[row];
        m.valid = a.valids ? (a.valids[row] != 0 ? 1.f : 0.f) : 1.f;
        if (a.kind == 1) m.old = a.old_prob[row * A + m.act];
    }
    __device__ HeadTerms row(const HeadArgs& a, const HeadRow& r, int A, int lane, float pk, float w) const {
        return pg_row(a, r, a.kind == 1, clip, A, lane, pk, w);
    }
    static __device__ int dh_rows(int A) { return A + 1; }
};

}  // namespace

extern "C" int arl_gather_scale_obs_nhwc(const uint8_t* obs, const int32_t* idx_or_null,
                                         int64_t batch, int32_t channels, int32_t plane_bytes,
                                         float scale, float* out, void* stream) {
    ARL_REQUIRE(obs && out, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(batch >= 0 && plane_bytes > 0, ARL_E_ARG, "bad batch/plane");
    ARL_REQUIRE(channels == 4, ARL_E_RANGE, "NHWC gather is specialised for 4 stacked frames");
    ARL_REQUIRE((plane_bytes & 15) == 0, ARL_E_RANGE, "plane_bytes must be a multiple of 16");
    ARL_REQUIRE(arl::aligned4(obs) && arl::aligned16(out), ARL_E_ALIGN, "obs 4-byte, out 16-byte aligned");
    if (batch == 0) return 0;
    hipLaunchKernelGGL(gather_nhwc4_kernel, dim3(arl::stream_grid(batch * (plane_bytes >> 2), 256)),
                       dim3(256), 0, (hipStream_t)stream, obs, idx_or_null, batch, (int)plane_bytes,
                       scale, out);
    return arl::check_launch("gather_nhwc4_kernel");
}

extern "C" int arl_bias_relu(float* x, const float* bias, int64_t rows, int32_t channels, void* stream) {
    ARL_REQUIRE(x && bias, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(rows >= 0 && channels > 0 && (channels & 3) == 0, ARL_E_RANGE, "channels must be a multiple of 4");
    ARL_REQUIRE(arl::aligned16(x) && arl::aligned16(bias), ARL_E_ALIGN, "x/bias must be 16-byte aligned");
    if (rows == 0) return 0;
    const int64_t total4 = rows * (channels >> 2);
    hipLaunchKernelGGL(bias_relu_kernel, dim3(arl::stream_grid(total4, 256)), dim3(256), 0,
                       (hipStream_t)stream, (float4*)x, (const float4*)bias, total4, (int)(channels >> 2));
    return arl::check_launch("bias_relu_kernel");
}

extern "C" int64_t arl_relu_bwd_workspace_bytes(void) { return (int64_t)256 * HID_MAX * sizeof(float); }
extern "C" int64_t arl_pg_head_workspace_bytes(void) {
    // loss partials [256][4]; head-gradient partials: [WG_SPLITS][K][hid] (separate kernel) or [<= 256][K][hid] with
    // K * hid <= FUSED_WGRAD_MAX (summed inside the head kernel); bias partials [<= 256][Kp]
    return (int64_t)(256 * 4 + 256 * FUSED_WGRAD_MAX + WG_SPLITS * (K_MAX + 1) * HID_MAX + 256 * (K_MAX + 4)) * sizeof(float);
}

static int relu_bwd_bias_launch(float* dy, const float* y, int64_t rows, int32_t channels, float* dbias,
                                void* workspace, int* n_partials, void* stream) {
    ARL_REQUIRE(dy && y && dbias && workspace, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(rows > 0 && channels > 0 && (channels & 3) == 0 && channels <= HID_MAX, ARL_E_RANGE,
                "channels must be a multiple of 4 and <= 1024");
    ARL_REQUIRE(arl::aligned16(dy) && arl::aligned16(y) && arl::aligned16(workspace), ARL_E_ALIGN, "16-byte alignment");
    const int c4 = channels >> 2, rows_per_iter = 256 / c4;
    int64_t grid = (rows + rows_per_iter - 1) / rows_per_iter;
    if (grid > 256) grid = 256;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(relu_bwd_bias_kernel, dim3((unsigned)grid), dim3(256), 0, s, (float4*)dy,
                       (const float4*)y, rows, c4, (float4*)workspace);
    *n_partials = (int)grid;
    return arl::check_launch("relu_bwd_bias_kernel");
}

extern "C" int arl_relu_bwd_bias_grad(float* dy, const float* y, int64_t rows, int32_t channels,
                                      float* dbias, void* workspace, void* stream) {
    int grid = 0;
    int rc = relu_bwd_bias_launch(dy, y, rows, channels, dbias, workspace, &grid, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(fold_partials_kernel, dim3((channels + 63) / 64), dim3(1024), 0, (hipStream_t)stream,
                       (const float*)workspace, grid, (int)channels, dbias);
    return arl::check_launch("fold_partials_kernel");
}

extern "C" int arl_relu_bwd_bias_parts(float* dy, const float* y, int64_t rows, int32_t channels, float* dbias,
                                       void* workspace, arl_fold_item* item, void* stream) {
    ARL_REQUIRE(item, ARL_E_ARG, "null pointer");
    int grid = 0;
    int rc = relu_bwd_bias_launch(dy, y, rows, channels, dbias, workspace, &grid, stream);
    item->part = (const float*)workspace; item->out = dbias; item->total = channels; item->splits = grid; item->valid = 0;
    return rc;
}

extern "C" int arl_pg_head_infer(const float* h, const float* w_head, const float* b_head,
                                 int64_t batch, int32_t hid, int32_t n_actions, float* prob,
                                 float* value, void* stream) {
    ARL_REQUIRE(h && w_head && b_head && prob && value, ARL_E_ARG, "null pointer");
    int rc = check_head(batch, hid, n_actions);
    if (rc) return rc;
    HeadArgs a = {};
    a.h = h; a.w_head = w_head; a.b_head = b_head; a.batch = (int)batch; a.hid = hid; a.n_act = n_actions;
    a.prob = prob; a.value = value;
    a.head_blocks = (int)((batch + 3) / 4 < 1024 ? (batch + 3) / 4 : 1024);
    return head_launch<InferLoss>(a, a.head_blocks, (size_t)(n_actions + 1) * hid * 4, arlw::DgradWtArgs{},
                                  (hipStream_t)stream);
}

extern "C" int arl_pg_head_loss_parts(const float* h, const float* w_head, const float* b_head,
                                const uint8_t* actions, const float* advantages, const float* returns,
                                const float* old_prob, const int8_t* valids_or_null,
                                const int32_t* idx_or_null, const float* lr_mult,
                                const float* inv_count_or_null, int64_t batch, int32_t hid,
                                int32_t n_actions, int32_t kind, int32_t tie_rule, float clip_param, float v_loss_coeff,
                                float ent_loss_coeff, int32_t relu_mask_dh, float* dout, float* dh,
                                float* dw_head, float* db_head, float* loss4, void* workspace, arl_fold_item* items3,
                                      const arl_dgrad_wt* wt_items_or_null, int32_t n_wt, void* stream) {
    ARL_REQUIRE(h && w_head && b_head && actions && advantages && returns && lr_mult && dout && dh &&
                    dw_head && db_head && loss4 && workspace && items3, ARL_E_ARG, "null pointer");
    ARL_REQUIRE(kind == 0 || (kind == 1 && old_prob), ARL_E_ARG, "kind must be 0 (A2C) or 1 (PPO, needs old_prob)");
    ARL_REQUIRE(tie_rule == ARL_PPO_TIE_THEANO || tie_rule == ARL_PPO_TIE_MATH || tie_rule == ARL_PPO_TIE_BOTH, ARL_E_ARG,
                "tie_rule must be ARL_PPO_TIE_THEANO, ARL_PPO_TIE_MATH or ARL_PPO_TIE_BOTH");
    int rc = check_head(batch, hid, n_actions);
    if (rc) return rc;
    HeadArgs a = {};
    a.h = h; a.w_head = w_head; a.b_head = b_head; a.actions = actions; a.adv = advantages;
    a.ret = returns; a.old_prob = old_prob; a.valids = valids_or_null; a.idx = idx_or_null;
    a.lr_mult = lr_mult; a.inv_count = inv_count_or_null; a.dout = dout; a.dh = dh;
    a.batch = (int)batch; a.hid = hid; a.n_act = n_actions; a.kind = kind; a.tie_rule = tie_rule;
    a.clip_param = clip_param; a.v_coeff = v_loss_coeff; a.ent_coeff = ent_loss_coeff; a.mask_dh = relu_mask_dh;
    return head_loss_launch<PgLoss>(a, dw_head, db_head, loss4, workspace, items3, wt_items_or_null, n_wt,
                                    (hipStream_t)stream);
}

extern "C" int arl_pg_head_loss(const float* h, const float* w_head, const float* b_head,
                                const uint8_t* actions, const float* advantages, const float* returns,
                                const float* old_prob, const int8_t* valids_or_null,
                                const int32_t* idx_or_null, const float* lr_mult,
                                const float* inv_count_or_null, int64_t batch, int32_t hid,
                                int32_t n_actions, int32_t kind, int32_t tie_rule, float clip_param, float v_loss_coeff,
                                float ent_loss_coeff, int32_t relu_mask_dh, float* dout, float* dh,
                                float* dw_head, float* db_head, float* loss4, void* workspace, void* stream) {
    arl_fold_item items[3];
    int rc = arl_pg_head_loss_parts(h, w_head, b_head, actions, advantages, returns, old_prob, valids_or_null,
                                    idx_or_null, lr_mult, inv_count_or_null, batch, hid, n_actions, kind, tie_rule, clip_param,
                                    v_loss_coeff, ent_loss_coeff, relu_mask_dh, dout, dh, dw_head, db_head, loss4,
                                    workspace, items, nullptr, 0, stream);
    if (rc) return rc;
    return arl_fold_many(items, 3, stream);
}
