// Launchers, per-call context, split planning and the instantiation lists dealt out to mfma_conv_p1 .. p8.hip.
// Part of mfma_conv_impl.h.
#pragma once
#include "mfma_generic.h"
#include "mfma_igemm.h"
#include "mfma_wgrad.h"
#include "mfma_pair.h"

namespace arlc {

// arl_dev_conv_launch_log: what the calling thread's current (or last) entry-point call launched.  Host side only.
struct LaunchLog { int n; arl_dev_launch rec[ARL_DEV_LAUNCH_LOG_MAX]; };
extern thread_local LaunchLog t_launch_log;        // (mfma_conv.hip)
extern thread_local int t_launch_split;            // the open CallScope's split mode (= t_ctx.split)
inline void launch_log_clear() { t_launch_log.n = 0; }
struct Tile { int wgm, wgn, tm, tn, bk, minw; };
inline void log_launch(int family, Tile t, int flags, int splits, dim3 grid, size_t lds) {
    LaunchLog& l = t_launch_log;
    if (l.n < ARL_DEV_LAUNCH_LOG_MAX)
        l.rec[l.n] = arl_dev_launch{family, t.wgm, t.wgn, t.tm, t.tn, t.bk, t.minw, flags, t_launch_split, splits,
                                    grid.x, grid.y, grid.z, (uint32_t)lds};
    ++l.n;
}

template <int WGM, int WGN, int TM, int TN, int BK, bool B_KC, bool TAP_UNIFORM = false>
int launch_rowgather(const GemmArgs& a, int splits, hipStream_t s) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    constexpr int A_SZ = BM * (BK + 4), B_SZ = B_KC ? BN * (BK + 4) : BK * BN;
    const size_t lds = (size_t)2 * (A_SZ + B_SZ) * sizeof(float);
    ARL_REQUIRE(!a.o.out_bits, ARL_E_RANGE, "rectifier bits: not written by the generic kernels");
    dim3 grid((a.M + BM - 1) / BM, (a.N + BN - 1) / BN, splits);
    hipLaunchKernelGGL((rowgather_gemm_kernel<WGM, WGN, TM, TN, BK, B_KC, TAP_UNIFORM>), grid, dim3(256), lds, s, a);
    log_launch(ARL_DEV_K_ROWGATHER, {WGM, WGN, TM, TN, BK, 0},
               (B_KC ? ARL_DEV_F_B_KC : 0) | (TAP_UNIFORM ? ARL_DEV_F_TAP_UNIFORM : 0), splits, grid, lds);
    return arl::check_launch("rowgather_gemm_kernel");
}

template <int WGM, int WGN, int TM, int TN, int BK>
int launch_wgrad(const WgradArgs& a, int splits, hipStream_t s) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    const size_t lds = (size_t)2 * BK * (BM + BN) * sizeof(float);
    dim3 grid((a.N + BN - 1) / BN, (a.K_out + BM - 1) / BM, splits);
    hipLaunchKernelGGL((wgrad_kernel<WGM, WGN, TM, TN, BK>), grid, dim3(256), lds, s, a);
    log_launch(ARL_DEV_K_WGRAD, {WGM, WGN, TM, TN, BK, 0}, 0, splits, grid, lds);
    return arl::check_launch("wgrad_kernel");
}

inline int launch_flags(bool b_kc, bool n16, bool u8, bool multi_tap, bool has_pad, bool direct = false, bool corun = false) {
    return (b_kc ? ARL_DEV_F_B_KC : 0) | (n16 ? ARL_DEV_F_N16 : 0) | (u8 ? ARL_DEV_F_U8 : 0) |
           (multi_tap ? ARL_DEV_F_MULTI_TAP : 0) | (has_pad ? ARL_DEV_F_HAS_PAD : 0) | (direct ? ARL_DEV_F_DIRECT : 0) |
           (corun ? ARL_DEV_F_CORUN : 0);
}

constexpr bool lds_fits(int floats) { return floats * 4 <= 65536; }

template <typename K>
int allow_big_lds(K kernel, size_t lds) {           // > 64 KiB of dynamic LDS needs an explicit opt-in
    if (lds <= 65536) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { arl::set_error("hipFuncSetAttribute(LDS %zu): %s", lds, hipGetErrorString(e)); return (int)e; }
    return 0;
}

template <int WGM, int WGN, int TM, int TN, int BK, bool B_KC, bool N16 = false>
int launch_igemm(const GemmArgs& a, int splits, bool multi_tap, bool has_pad, hipStream_t s) {
    constexpr int BM = WGM * TM * (N16 ? 16 : 32), BN = N16 ? WGN * 16 : WGN * TN * 32;
    constexpr int A_SZ = BM * (BK + 4), B_SZ = B_KC ? BN * (BK + 4) : BK * (N16 ? BN + 4 : BN);
    const size_t lds = (size_t)2 * (A_SZ + B_SZ) * sizeof(float);
    ARL_REQUIRE(!a.o.out_bits, ARL_E_RANGE, "rectifier bits: not written by the fp32 chain's kernels");
    dim3 grid((a.M + BM - 1) / BM, (a.N + BN - 1) / BN, a.n_par ? a.n_par : splits);
    int rc = 0;
#define ARL_IGEMM(MT, HP)                                                                                  \
    do {                                                                                                   \
        auto k = igemm_kernel<WGM, WGN, TM, TN, BK, B_KC, MT, HP, N16>;                                    \
        rc = allow_big_lds(k, lds);                                                                        \
        if (!rc) hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);                                        \
    } while (0)
    if (multi_tap && has_pad) ARL_IGEMM(true, true);
    else if (multi_tap) ARL_IGEMM(true, false);
    else if (has_pad) ARL_IGEMM(false, true);
    else ARL_IGEMM(false, false);
#undef ARL_IGEMM
    if (!rc) log_launch(ARL_DEV_K_IGEMM, {WGM, WGN, TM, TN, BK, 0}, launch_flags(B_KC, N16, false, multi_tap, has_pad), splits, grid, lds);
    return rc ? rc : arl::check_launch("igemm_kernel");
}

// What one entry-point call carries down to its launches (set by the extern "C" function from its own arguments, for
// the duration of that call, on the calling thread: no state survives a call, none is shared between threads).
//   split   route of the fp32 contractions (arl_conv_geom::route): 0 = fp32 MFMA chain, 6 / 9 = bf16-split products
//   corun   an optimiser job (arl_corun_job) that the call's data-gradient launch may host in extra workgroups
struct CorunJob { arl::OptSeg seg; int blocks, host_blocks; };
static_assert(sizeof(CorunJob) <= sizeof(arl_corun_job), "arl_corun_job too small");
struct CallCtx { int split; const CorunJob* corun; bool corun_taken; };
extern thread_local CallCtx t_ctx;                 // (mfma_conv.hip)
#define g_split (t_ctx.split)
struct CallScope {
    // keep_log: a further scope of the same entry-point call (arl_conv2d_bwd_weight_group: one per plan)
    explicit CallScope(int split, const arl_corun_job* job = nullptr, bool keep_log = false) {
        t_ctx.split = split; t_ctx.corun = reinterpret_cast<const CorunJob*>(job); t_ctx.corun_taken = false;
        t_launch_split = split;
        if (!keep_log) launch_log_clear();
    }
    ~CallScope() { t_ctx.corun = nullptr; }
};
// arl_conv_geom::route -> split mode (-1: not a route)
inline int split_of(const arl_conv_geom* g) {
    if (!g) return 9;
    return g->route == ARL_CONV_ROUTE_SPLIT9 ? 9 : g->route == ARL_CONV_ROUTE_FP32 ? 0 : g->route == ARL_CONV_ROUTE_SPLIT6 ? 6
         : g->route == ARL_CONV_ROUTE_BF16 ? 1 : -1;
}
#define ARL_ROUTE_SCOPE(geom, job)                                                                         \
    ARL_REQUIRE(split_of(geom) >= 0, ARL_E_ARG, "conv route: ARL_CONV_ROUTE_SPLIT9, _FP32, _SPLIT6 or _BF16");    \
    const CallScope call_scope_(split_of(geom), job)
// a pending optimiser job for a data-gradient launch to host?  (taken at most once per call)
inline bool corun_take(arl::OptSeg* c, dim3* grid) {
    if (!t_ctx.corun || t_ctx.corun_taken) return false;
    *c = t_ctx.corun->seg;
    c->co_blocks = t_ctx.corun->blocks < t_ctx.corun->host_blocks ? t_ctx.corun->blocks : t_ctx.corun->host_blocks;
    grid->x += (unsigned)c->co_blocks;
    t_ctx.corun_taken = true;
    return true;
}

template <int WGM, int WGN, int TM, int TN, int BK, bool B_KC, bool N16, int MINW>
int launch_igemm_occ(const GemmArgs& a, bool multi_tap, bool has_pad, hipStream_t s, int splits = 1) {
    constexpr int BM = WGM * TM * (N16 ? 16 : 32), BN = N16 ? WGN * 16 : WGN * TN * 32;
    constexpr int A_SZ = BM * (BK + 4), B_SZ = B_KC ? BN * (BK + 4) : BK * (N16 ? BN + 4 : BN);
    const size_t lds = (size_t)2 * (A_SZ + B_SZ) * sizeof(float);
    static_assert(lds_fits(2 * (A_SZ + B_SZ)), "<= 64 KiB of LDS");
    ARL_REQUIRE(!a.o.out_bits, ARL_E_RANGE, "rectifier bits: not written by the fp32 chain's kernels");
    dim3 grid((a.M + BM - 1) / BM, (a.N + BN - 1) / BN, a.n_par ? a.n_par : splits);
    arl::OptSeg c = {};
    if constexpr (!B_KC) {                          // a data gradient hosts the call's optimiser job, if any
        if (!multi_tap && corun_take(&c, &grid)) {
            if (has_pad) hipLaunchKernelGGL((igemm_occ_kernel<WGM, WGN, TM, TN, BK, B_KC, false, true, N16, MINW, true>), grid, dim3(256), lds, s, a, c);
            else hipLaunchKernelGGL((igemm_occ_kernel<WGM, WGN, TM, TN, BK, B_KC, false, false, N16, MINW, true>), grid, dim3(256), lds, s, a, c);
            log_launch(ARL_DEV_K_IGEMM_OCC, {WGM, WGN, TM, TN, BK, MINW}, launch_flags(B_KC, N16, false, false, has_pad, false, true), splits, grid, lds);
            return arl::check_launch("igemm_occ_kernel (co-run)");
        }
    }
#define ARL_IGEMM_OCC(MT, HP) \
    hipLaunchKernelGGL((igemm_occ_kernel<WGM, WGN, TM, TN, BK, B_KC, MT, HP, N16, MINW>), grid, dim3(256), lds, s, a, c)
    if (multi_tap && has_pad) ARL_IGEMM_OCC(true, true);
    else if (multi_tap) ARL_IGEMM_OCC(true, false);
    else if (has_pad) ARL_IGEMM_OCC(false, true);
    else ARL_IGEMM_OCC(false, false);
#undef ARL_IGEMM_OCC
    log_launch(ARL_DEV_K_IGEMM_OCC, {WGM, WGN, TM, TN, BK, MINW}, launch_flags(B_KC, N16, false, multi_tap, has_pad), splits, grid, lds);
    return arl::check_launch("igemm_occ_kernel");
}

#ifdef ARL_NO_SPLIT6        // development builds: half the split kernels (mode 6 then runs the nine-product kernels)
#define ARL_BY_MODE(X1, X6, X9) do { X9; } while (0)
#else
#define ARL_BY_MODE(X1, X6, X9) do { if (g_split == 1) { X1; } else if (g_split == 6) { X6; } else { X9; } } while (0)
#endif

// the launch of igemm_split_kernel: two LDS stages of (1 or 3) + 3 bf16 planes; a data gradient hosts the pending
// optimiser job like launch_igemm_occ
// Rectifier masks as bits (OutDesc::mask_bits / out_bits): the one-wave-per-row-tile shapes on k-contiguous f32 operands with
// one tap per k-tile have a BITS twin -- the learner's conv 2 / conv 3 forward (which write them) and data gradients (which
// read them).  Any other launch compares the f32 mask as ever and refuses to write bits.
template <int WGM, int WGN, int TM, int TN, int BK, bool B_KC, bool U8, int MINW>
int launch_igemm_split(const GemmArgs& a_in, bool multi_tap, bool has_pad, hipStream_t s, int splits = 1) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    constexpr bool CAN_BITS = B_KC && WGM == 4 && WGN == 1 && (U8 || TM == 1);      // (u8: conv 1 off the image-stationary kernel)
    GemmArgs a = a_in;
    // (a forward has no mask and a data gradient writes no bits: the twin is the reading one or the writing one)
    const int bits = !(CAN_BITS && !multi_tap) ? 0 : a.o.out_bits ? 2 : a.o.mask_bits ? 1 : 0;
    if (!bits) {
        ARL_REQUIRE(!a.o.out_bits, ARL_E_RANGE, "rectifier bits: not written by this layer's kernel");
        a.o.mask_bits = nullptr;
    }
    const int npl = planes_of(g_split);
    const size_t lds = (size_t)2 * ((U8 ? 1 : npl) * BM + npl * BN) * BK * 2;
    const size_t lds_dir = (size_t)2 * npl * BN * BK * 2;       // direct gathered operand: only the weights live in LDS
    (void)lds_dir;
    dim3 grid((a.M + BM - 1) / BM, (a.N + BN - 1) / BN, a.n_par ? a.n_par : splits);
    arl::OptSeg c = {};
    int rc = 0;
    auto note = [&](bool mt, bool hp, bool co) {    // (ad: what ARL_SPLIT_PIN below selects)
        const bool ad = WGN == 1 && (U8 || !mt);
        if (!rc) log_launch(ARL_DEV_K_IGEMM_SPLIT, {WGM, WGN, TM, TN, BK, MINW}, launch_flags(B_KC, false, U8, mt, hp, ad, co), splits, grid, ad ? lds_dir : lds);
    };
#define ARL_SPLIT_K(MT, HP, SPL, CO, AD, BT)                                                               \
    do {                                                                                                   \
        auto k = igemm_split_kernel<WGM, WGN, TM, TN, BK, B_KC, MT, HP, U8, SPL, MINW, CO, AD, BT>;        \
        const size_t lds_k = (AD) ? lds_dir : lds;                                                         \
        rc = allow_big_lds(k, lds_k + (CO ? 64 : 0));                                                      \
        if (!rc) hipLaunchKernelGGL(k, grid, dim3(256), lds_k, s, a, c);                                   \
    } while (0)
// (one wave per row tile and one tap per k-tile: the gathered operand goes straight into the fragment registers)
#define ARL_SPLIT_PIN(MT, HP, SPL, CO)                                                                     \
    do {                                                                                                   \
        constexpr bool AD = WGN == 1 && (U8 || !(MT));                                                     \
        if constexpr (CAN_BITS && U8) {                     /* (a forward: the writing twin alone) */      \
            if (bits == 2) ARL_SPLIT_K(MT, HP, SPL, CO, AD, 2); else ARL_SPLIT_K(MT, HP, SPL, CO, AD, 0);  \
        } else if constexpr (CAN_BITS && !(MT) && (CO)) {   /* (only a data gradient carries a job) */     \
            if (bits == 1) ARL_SPLIT_K(MT, HP, SPL, CO, AD, 1); else ARL_SPLIT_K(MT, HP, SPL, CO, AD, 0);  \
        } else if constexpr (CAN_BITS && !(MT)) {                                                          \
            if (bits == 1) ARL_SPLIT_K(MT, HP, SPL, CO, AD, 1);                                            \
            else if (bits == 2) ARL_SPLIT_K(MT, HP, SPL, CO, AD, 2);                                       \
            else ARL_SPLIT_K(MT, HP, SPL, CO, AD, 0);                                                      \
        } else {                                                                                           \
            ARL_SPLIT_K(MT, HP, SPL, CO, AD, 0);                                                           \
        }                                                                                                  \
    } while (0)
#define ARL_SPLIT_MODE(MT, HP, CO)                                                                         \
    do {                                                                                                   \
        ARL_BY_MODE(ARL_SPLIT_PIN(MT, HP, 1, CO), ARL_SPLIT_PIN(MT, HP, 6, CO), ARL_SPLIT_PIN(MT, HP, 9, CO));                           \
    } while (0)
    if constexpr (U8) {
        ARL_SPLIT_MODE(false, false, false);
        note(false, false, false);
    } else {
        // (data gradients: k-major weights, or k-contiguous ones on the one-wave-per-row-tile shapes)
        if constexpr (!B_KC || (WGM == 4 && WGN == 1 && TM == 1)) {
            if (!multi_tap && bits != 2 && corun_take(&c, &grid)) {   // (a launch that writes bits is a forward: no job)
                if (has_pad) ARL_SPLIT_MODE(false, true, true); else ARL_SPLIT_MODE(false, false, true);
                note(false, has_pad, true);
                return rc ? rc : arl::check_launch("igemm_split_kernel (co-run)");
            }
        }
        if (multi_tap && has_pad) ARL_SPLIT_MODE(true, true, false);
        else if (multi_tap) ARL_SPLIT_MODE(true, false, false);
        else if (has_pad) ARL_SPLIT_MODE(false, true, false);
        else ARL_SPLIT_MODE(false, false, false);
        note(multi_tap, has_pad, false);
    }
#undef ARL_SPLIT_PIN
#undef ARL_SPLIT_MODE
#undef ARL_SPLIT_K
    return rc ? rc : arl::check_launch("igemm_split_kernel");
}

template <int WGM, int WGN, int TM, int TN, int BK, bool M16 = false>
int launch_wgrad_fast(const WgradArgs& a, int splits, bool has_pad, hipStream_t s) {
    constexpr int BM = M16 ? 16 : WGM * TM * 32, BN = WGN * TN * 32;
    const size_t lds = (size_t)2 * BK * (BM + BN) * sizeof(float);
    dim3 grid((a.N + BN - 1) / BN, (a.K_out + BM - 1) / BM, splits);
    int rc;
    if (has_pad) {
        auto k = wgrad_fast_kernel<WGM, WGN, TM, TN, BK, true, M16>;
        rc = allow_big_lds(k, lds + 4096);
        if (!rc) hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
    } else {
        auto k = wgrad_fast_kernel<WGM, WGN, TM, TN, BK, false, M16>;
        rc = allow_big_lds(k, lds + 4096);
        if (!rc) hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
    }
    if (!rc) log_launch(ARL_DEV_K_WGRAD_FAST, {WGM, WGN, TM, TN, BK, 0}, launch_flags(false, M16, false, false, has_pad), splits, grid, lds);
    return rc ? rc : arl::check_launch("wgrad_fast_kernel");
}

template <int WGM, int WGN, int TM, int TN, int BK, bool U8, int MINW>
int launch_wgrad_split(const WgradArgs& a, int splits, bool has_pad, hipStream_t s) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    const int npl = planes_of(g_split);
    const size_t lds = (size_t)2 * (npl * BM + (U8 ? 1 : npl) * BN) * BK * 2;
    dim3 grid((a.N + BN - 1) / BN, (a.K_out + BM - 1) / BM, splits);
    int rc = 0;
#define ARL_WSPLIT(HP, SPL)                                                                                \
    do {                                                                                                   \
        auto k = wgrad_split_kernel<WGM, WGN, TM, TN, BK, HP, U8, SPL, MINW>;                              \
        rc = allow_big_lds(k, lds + 4096);                                                                 \
        if (!rc) hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);                                        \
    } while (0)
    if constexpr (U8) {
        ARL_BY_MODE(ARL_WSPLIT(false, 1), ARL_WSPLIT(false, 6), ARL_WSPLIT(false, 9));
    } else if (has_pad) {
        ARL_BY_MODE(ARL_WSPLIT(true, 1), ARL_WSPLIT(true, 6), ARL_WSPLIT(true, 9));
    } else {
        ARL_BY_MODE(ARL_WSPLIT(false, 1), ARL_WSPLIT(false, 6), ARL_WSPLIT(false, 9));
    }
#undef ARL_WSPLIT
    if (!rc) log_launch(ARL_DEV_K_WGRAD_SPLIT, {WGM, WGN, TM, TN, BK, MINW}, launch_flags(false, false, U8, false, !U8 && has_pad), splits, grid, lds);
    return rc ? rc : arl::check_launch("wgrad_split_kernel");
}

constexpr int TARGET_WGS = 256;     // one workgroup per CU is already MFMA-bound (fp32 MFMA: 1 wave / SIMD)
constexpr int BKT = 32;             // k-tile of the skinny configurations (host-side split granularity)

extern unsigned long long* g_trace;   // arl_dev_conv_trace_buffer
extern bool g_force_generic;          // arl_dev_conv_force_generic: route every call to the generic kernels (tests)
extern int g_fwd_tile;                // arl_dev_fwd_tile: tile shape of the 33 .. 64-column forward kernels (-1: by size)

struct Geom {
    int64_t batch;
    int H, W, C, K, kh, kw, stride, pad_h, pad_w, Ho, Wo;
};

inline int check_geom(const arl_conv_geom* g, Geom* o) {
    if (!g || g->batch <= 0 || g->in_h <= 0 || g->in_w <= 0 || g->in_c <= 0 || g->out_c <= 0 || g->kh <= 0 ||
        g->kw <= 0 || g->stride <= 0 || g->pad_h < 0 || g->pad_w < 0) {
        arl::set_error("conv: bad geometry");
        return ARL_E_ARG;
    }
    if ((g->in_c & 3) || (g->out_c & 3)) {
        arl::set_error("conv: channel counts must be multiples of 4 (in %d, out %d)", g->in_c, g->out_c);
        return ARL_E_RANGE;
    }
    o->batch = g->batch; o->H = g->in_h; o->W = g->in_w; o->C = g->in_c; o->K = g->out_c;
    o->kh = g->kh; o->kw = g->kw; o->stride = g->stride; o->pad_h = g->pad_h; o->pad_w = g->pad_w;
    o->Ho = (g->in_h + 2 * g->pad_h - g->kh) / g->stride + 1;
    o->Wo = (g->in_w + 2 * g->pad_w - g->kw) / g->stride + 1;
    const int64_t lim = (int64_t)OOB / 4;       // elements: every tensor must stay below the OOB byte offset
    if (o->Ho <= 0 || o->Wo <= 0 || g->batch * (int64_t)o->Ho * o->Wo * g->out_c >= lim ||
        g->batch * (int64_t)g->in_h * g->in_w * g->in_c >= lim ||
        (int64_t)g->out_c * g->kh * g->kw * g->in_c >= lim) {
        arl::set_error("conv: tensor larger than the 2 GiB the 32-bit buffer offsets address");
        return ARL_E_RANGE;
    }
    return 0;
}

// A rectifier mask as bits (y_bits_or_null, mask_bits_or_null): u32[rows][channels / 32], bit c % 32 of word c / 32 =
// (y[row][c] > 0).  Null = not asked for; anything the kernels cannot serve is refused, never ignored.
inline int check_relu_bits(const void* bits, int channels) {
    if (!bits) return 0;
    ARL_REQUIRE(channels % 32 == 0, ARL_E_RANGE, "rectifier bits: the channel count must be a multiple of 32");
    ARL_REQUIRE(arl::aligned4(bits), ARL_E_ALIGN, "rectifier bits: 4-byte alignment");
    return 0;
}

inline int round_up(int x, int q) { return (x + q - 1) / q * q; }

// ceil(2^32 / d) if floor(n * that / 2^32) == n / d for every 0 <= n < rows (needs rows * d < 2^32), else 0
inline unsigned div_magic(int64_t rows, int d) {
    if (d <= 1 || rows * (int64_t)d >= ((int64_t)1 << 32)) return 0;
    return (unsigned)((((uint64_t)1 << 32) + (uint64_t)d - 1) / (uint64_t)d);
}

// 33 .. 64 output columns, the default: 32x64 tiles -- each wave two 16-row groups of one 16-column stripe
// (v_mfma_f32_16x16x4_f32), 32-deep k-tiles, two LDS stages (28 KB), compiled for five waves per SIMD.  Small tiles
// spread the rows evenly (1 728 tiles at the PPO minibatch: 7 on the busiest CU against 6.75 on average, where 864
// tiles of 64 rows leave it 4 against 3.375) and five or six resident workgroups per CU cover each other's barriers,
// prologues and epilogues.  Measured, 20 launches per hipGraph, conv 2 / conv 3 forward at 512 images: 36.6 / 40.1 us
// (64x64: 44.7 / 47.9, 112x64: 40.6 / 42.0); at 256: 22.4 / 24.1 (25.0 / 27.6, 25.4 / 26.7); at 128: 14.2 / 15.7
// (15.6 / 17.3, 22.9 / 25.2); 16-deep k-tiles at 6-8 waves per SIMD and 48-row tiles were slower everywhere
// (profiles/r02/tile_probe.txt).
template <bool B_KC>
int launch_n64(const GemmArgs& a, bool multi_tap, bool has_pad, hipStream_t s) {
    return launch_igemm_occ<1, 4, 2, 1, 32, B_KC, true, 5>(a, multi_tap, has_pad, s);
}

// split the reduction so that tiles * splits ~ TARGET_WGS, each split a multiple of BKT
inline void plan_split(int tiles, int red, int* splits, int* per, int want = TARGET_WGS) {
    int s = tiles >= want ? 1 : want / tiles;
    const int max_s = (red + 4 * BKT - 1) / (4 * BKT);          // at least 4 k-tiles per split
    if (s > max_s) s = max_s;
    if (s < 1) s = 1;
    *per = round_up((red + s - 1) / s, BKT);
    *splits = (red + *per - 1) / *per;
}

// Fast-path launch descriptions, so that a layer's data and weight gradient can share one launch
// (arl_conv2d_bwd_pair).  cfg: data gradient 0 = <4,1,1,1>, 1 = <2,2,1,1>, 2 = <2,2,2,2>;
// weight gradient 0 = <1,4,1,1>, 1 = <2,2,1,1>, 2 = <2,2,2,2>.
struct DgradPlan { GemmArgs a; bool fast, has_pad; int cfg; };
// kind / route: what arl_wgrad_plan keeps of a deferred weight gradient (arl_conv2d_bwd_weight_group): WPLAN_F32 = f32
// input (wgrad_impl; cfg as above), WPLAN_U8 = planar u8 input (cfg 0 = 16-row tiles, 1 / 2 = split kernel on 256 / 128
// columns, 3 = fp32 chain on 32-row tiles), 0 = nothing to launch; route = the planning call's split mode.
constexpr int WPLAN_F32 = 1, WPLAN_U8 = 2;
struct WgradPlan { WgradArgs a; bool fast, has_pad; int cfg, splits; int64_t total; int kind, route; };

template <int DWGM, int DWGN, int DTM, int DTN, int WWGM, int WWGN, int WTM, int WTN, int BK = 32>
int launch_pair(const DgradPlan& d, const WgradPlan& w, bool has_pad, hipStream_t s) {
    constexpr int DBM = DWGM * DTM * 32, DBN = DWGN * DTN * 32, WBM = WWGM * WTM * 32, WBN = WWGN * WTN * 32;
    const size_t lds_d = (size_t)2 * (DBM * (BK + 4) + BK * DBN) * sizeof(float);
    const size_t lds_w = (size_t)2 * BK * (WBM + WBN) * sizeof(float);
    const size_t lds = lds_d > lds_w ? lds_d : lds_w;
    const int dgx = (d.a.M + DBM - 1) / DBM, dgy = (d.a.N + DBN - 1) / DBN, dgz = d.a.n_par ? d.a.n_par : 1;
    const int wgx = (w.a.N + WBN - 1) / WBN, wgy = (w.a.K_out + WBM - 1) / WBM, wgz = w.splits;
    const int n_ig = dgx * dgy * dgz, n_wg = wgx * wgy * wgz;
    int rc;
    size_t lds_used = lds;
    if (g_split) {
        const size_t lds_s = (size_t)2 * planes_of(g_split) * ((DBM + DBN) > (WBM + WBN) ? (DBM + DBN) : (WBM + WBN)) * BK * 2;
#define ARL_PSPLIT_K(HP, SPL, BT)                                                                          \
    do {                                                                                                   \
        auto k = bwd_pair_kernel<DWGM, DWGN, DTM, DTN, WWGM, WWGN, WTM, WTN, BK, HP, SPL, BT>;             \
        rc = allow_big_lds(k, lds_s + 4096);                                                               \
        if (!rc) hipLaunchKernelGGL(k, dim3(n_ig + n_wg), dim3(256), lds_s, s, d.a, w.a, dgx, dgy, n_ig, wgx, wgy); \
    } while (0)
// (the data gradient's rectifier mask as bits: the 16-deep split kernels -- the learner's dense pair -- have a BITS twin)
#define ARL_PSPLIT(HP, SPL)                                                                                \
    do {                                                                                                   \
        if constexpr (BK == 16) {                                                                          \
            if (d.a.o.mask_bits) ARL_PSPLIT_K(HP, SPL, 1); else ARL_PSPLIT_K(HP, SPL, 0);                  \
        } else {                                                                                           \
            ARL_PSPLIT_K(HP, SPL, 0);                                                                      \
        }                                                                                                  \
    } while (0)
        if (has_pad) ARL_BY_MODE(ARL_PSPLIT(true, 1), ARL_PSPLIT(true, 6), ARL_PSPLIT(true, 9));
        else ARL_BY_MODE(ARL_PSPLIT(false, 1), ARL_PSPLIT(false, 6), ARL_PSPLIT(false, 9));
#undef ARL_PSPLIT
#undef ARL_PSPLIT_K
        lds_used = lds_s;
    } else if (has_pad) {
        auto k = bwd_pair_kernel<DWGM, DWGN, DTM, DTN, WWGM, WWGN, WTM, WTN, BK, true>;
        rc = allow_big_lds(k, lds + 4096);
        if (!rc) hipLaunchKernelGGL(k, dim3(n_ig + n_wg), dim3(256), lds, s, d.a, w.a, dgx, dgy, n_ig, wgx, wgy);
    } else {
        auto k = bwd_pair_kernel<DWGM, DWGN, DTM, DTN, WWGM, WWGN, WTM, WTN, BK, false>;
        rc = allow_big_lds(k, lds + 4096);
        if (!rc) hipLaunchKernelGGL(k, dim3(n_ig + n_wg), dim3(256), lds, s, d.a, w.a, dgx, dgy, n_ig, wgx, wgy);
    }
    // (tile = the data gradient's; both halves are 128 x 128 in every instantiation; splits = the weight gradient's)
    if (!rc) log_launch(ARL_DEV_K_BWD_PAIR, {DWGM, DWGN, DTM, DTN, BK, 0}, launch_flags(false, false, false, false, has_pad), wgz, dim3(n_ig + n_wg), lds_used);
    return rc ? rc : arl::check_launch("bwd_pair_kernel");
}


// img_conv.hip: the image-stationary kernels (>= 0: launched / error code; -1: not their geometry)
int launch_conv1_img(const unsigned char* obs, int64_t obs_rows, const int32_t* idx, float scale, const float* w, const float* bias, float* y,
                     int64_t batch, int C, int H, int W, int K, int kh, int kw, int stride, int Ho, int Wo, int relu,
                     hipStream_t s, unsigned char* copy_out = nullptr, long long copy_stride = 0, int* zero_word = nullptr,
                     unsigned* y_bits = nullptr);

// ---- the launcher instantiations, dealt out to translation units (mfma_conv_p<k>.hip define ARL_CONV_PART = k and hold the
// definitions of part k; every other unit sees them as extern templates) so that hipcc builds them side by side
#define ARL_GA const GemmArgs&, bool, bool, hipStream_t, int
#define ARL_P1(T) \
    T int launch_igemm_split<4, 1, 2, 1, 32, true, true, 2>(ARL_GA); \
    T int launch_igemm_split<4, 1, 1, 2, 32, true, false, 2>(ARL_GA); \
    T int launch_igemm_split<4, 1, 1, 1, 32, true, false, 2>(ARL_GA);
#define ARL_P2(T) \
    T int launch_igemm_split<2, 2, 2, 2, 32, true, false, 1>(ARL_GA); \
    T int launch_igemm_split<2, 2, 1, 1, 32, true, false, 3>(ARL_GA); \
    T int launch_igemm_split<2, 2, 1, 1, 32, false, false, 3>(ARL_GA);
#define ARL_P3(T) \
    T int launch_igemm_split<4, 1, 1, 2, 32, false, false, 2>(ARL_GA); \
    T int launch_igemm_split<4, 1, 1, 1, 32, false, false, 2>(ARL_GA); \
    T int launch_igemm_split<2, 2, 2, 2, 32, false, false, 1>(ARL_GA);
#define ARL_P4(T) \
    T int launch_wgrad_split<2, 2, 2, 2, 32, false, 1>(const WgradArgs&, int, bool, hipStream_t); \
    T int launch_wgrad_split<2, 2, 1, 1, 32, false, 2>(const WgradArgs&, int, bool, hipStream_t); \
    T int launch_wgrad_split<1, 4, 1, 1, 32, false, 2>(const WgradArgs&, int, bool, hipStream_t); \
    T int launch_wgrad_split<1, 4, 1, 1, 32, true, 2>(const WgradArgs&, int, bool, hipStream_t); \
    T int launch_wgrad_split<1, 4, 1, 2, 32, true, 2>(const WgradArgs&, int, bool, hipStream_t);
#define ARL_P5(T) \
    T int launch_pair<2, 2, 2, 2, 2, 2, 2, 2, 32>(const DgradPlan&, const WgradPlan&, bool, hipStream_t); \
    T int launch_pair<2, 2, 2, 2, 2, 2, 2, 2, 16>(const DgradPlan&, const WgradPlan&, bool, hipStream_t);
#define ARL_P6(T) \
    T int launch_igemm<2, 2, 1, 1, 32, true, false>(const GemmArgs&, int, bool, bool, hipStream_t); \
    T int launch_igemm<2, 2, 1, 1, 32, false, false>(const GemmArgs&, int, bool, bool, hipStream_t); \
    T int launch_igemm<2, 2, 2, 2, 32, true, false>(const GemmArgs&, int, bool, bool, hipStream_t); \
    T int launch_igemm<2, 2, 2, 2, 32, false, false>(const GemmArgs&, int, bool, bool, hipStream_t); \
    T int launch_igemm<4, 1, 2, 1, 16, true, true>(const GemmArgs&, int, bool, bool, hipStream_t); \
    T int launch_igemm<4, 1, 2, 1, 16, false, true>(const GemmArgs&, int, bool, bool, hipStream_t); \
    T int launch_igemm<4, 1, 1, 1, 32, true, false>(const GemmArgs&, int, bool, bool, hipStream_t); \
    T int launch_igemm<4, 1, 1, 1, 16, true, false>(const GemmArgs&, int, bool, bool, hipStream_t); \
    T int launch_igemm<4, 1, 1, 1, 16, false, false>(const GemmArgs&, int, bool, bool, hipStream_t);
#define ARL_P7(T) \
    T int launch_igemm_occ<2, 2, 2, 1, 32, false, true, 5>(ARL_GA); \
    T int launch_igemm_occ<1, 4, 2, 1, 32, true, true, 5>(ARL_GA); \
    T int launch_igemm_occ<1, 4, 2, 1, 32, false, true, 5>(ARL_GA); \
    T int launch_wgrad_fast<2, 2, 2, 2, 32, false>(const WgradArgs&, int, bool, hipStream_t); \
    T int launch_wgrad_fast<2, 2, 1, 1, 32, false>(const WgradArgs&, int, bool, hipStream_t); \
    T int launch_wgrad_fast<1, 4, 1, 1, 32, false>(const WgradArgs&, int, bool, hipStream_t); \
    T int launch_wgrad_fast<1, 4, 1, 1, 32, true>(const WgradArgs&, int, bool, hipStream_t);
#ifndef ARL_CONV_PART
#define ARL_CONV_PART 0
#endif
// (part 8: the grouped weight gradient, three routes of one kernel that holds four bodies)
int launch_wgrad_group(const WgradGroupArgs& g, int groups, size_t lds, hipStream_t s);
#if ARL_CONV_PART == 8
int launch_wgrad_group(const WgradGroupArgs& g, int groups, size_t lds, hipStream_t s) {
    int rc = 0;
#define ARL_WGROUP(SPL)                                                                                    \
    do {                                                                                                   \
        auto k = wgrad_group_kernel<SPL>;                                                                  \
        rc = allow_big_lds(k, lds + 4096);                                                                 \
        if (!rc) hipLaunchKernelGGL(k, dim3((unsigned)groups * 8), dim3(256), lds, s, g);                  \
    } while (0)
    ARL_BY_MODE(ARL_WGROUP(1), ARL_WGROUP(6), ARL_WGROUP(9));
#undef ARL_WGROUP
    if (!rc) log_launch(ARL_DEV_K_WGRAD_GROUP, {0, 0, 0, 0, 32, 0}, 0, g.n, dim3((unsigned)groups * 8), lds);
    return rc ? rc : arl::check_launch("wgrad_group_kernel");
}
#endif
#define ARL_T_DEF template
#define ARL_T_EXT extern template
#if ARL_CONV_PART == 1
ARL_P1(ARL_T_DEF)
#else
ARL_P1(ARL_T_EXT)
#endif
#if ARL_CONV_PART == 2
ARL_P2(ARL_T_DEF)
#else
ARL_P2(ARL_T_EXT)
#endif
#if ARL_CONV_PART == 3
ARL_P3(ARL_T_DEF)
#else
ARL_P3(ARL_T_EXT)
#endif
#if ARL_CONV_PART == 4
ARL_P4(ARL_T_DEF)
#else
ARL_P4(ARL_T_EXT)
#endif
#if ARL_CONV_PART == 5
ARL_P5(ARL_T_DEF)
#else
ARL_P5(ARL_T_EXT)
#endif
#if ARL_CONV_PART == 6
ARL_P6(ARL_T_DEF)
#else
ARL_P6(ARL_T_EXT)
#endif
#if ARL_CONV_PART == 7
ARL_P7(ARL_T_DEF)
#else
ARL_P7(ARL_T_EXT)
#endif

}  // namespace arlc
