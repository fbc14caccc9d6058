// Which kernel runs a convolution: ONE decision, conv_route(), read by everything that needs the answer - the launch, the kernel label
// of the accounting, and the plan-time queries that size what the launch must later agree with (GroupNorm partials, norms that are no
// launch of their own, residual segments).
#include <stdio.h>
#include <stdlib.h>

#include "conv_common.h"

namespace dmme {

// The dispatch table, by shape class.  conv_route() below decides it: the order in which the families are tried is written there and
// nowhere else, and each family's *_route function (in the family's .hip file) holds that family's shape rules and tile choice, so a row
// of this table is what those rules come to for the networks' layers.  Times are per launch at the
// benchmark configuration - default UNet, batch 128, bf16 - from profiles/r04_sample_b128_bf16_kernel_stats.csv and bench.py's
// event-bracketed forward; "B <= 32" rows from profiles/r04_bench_n1.json: small_batch:
//
//   shape class (16-bit plans)                               kernel                                   launches/step   us/launch
//   3x3 s1, 32x32 and 16x16 maps, Cin % 128 == 0, >= 256     conv3x3_ws2_kernel<11, T, 256>               18            66-72
//     256-pixel tiles of one image (the dominant kernel)       wave-specialised, persistent
//   ... the same where only 128-pixel tiles fill the chip    conv3x3_ws2_kernel<7, T, 128>                 4            41
//     (128-cout layers of the 16x16 level; 32x32 at B = 32)
//   3x3 s1 on 8x8 / 4x4 maps, DDPM blocks, <= 2 iterations   lvl_engine_kernel (plan_lvl.hip: a whole     3        131 / 181
//     per workgroup                                            level per launch; includes its 1x1 convs,
//                                                              norms and the 4x4 attention)
//   3x3 s1, few output pixels (small batches; IDDPM small    conv3x3_kw_kernel<NI, RING, DENSE, BM>       -           13-18
//     maps; 8x8 / 4x4 with DMME_NO_LVL)                        K split over the four waves
//   3x3 s2 (DownSample), 3x3 with fused 2x upsampling,       conv3x3_pipe_kernel<T, 64, 64, 3 | 9, UA>     4           36-45
//     everything the rows above decline                        four-wave software pipeline
//   1x1, K = 128 / 256, >= 128 tiles of 128 pixels           conv1x1_as_kernel<KCH, RES>                  15           14-25
//     (qkv, proj; the blocks' residual convs of the 32x32 /    activations stationary in registers
//      16x16 levels only with DMME_DEBUG_ROUTE=no_rseg: they
//      are a second K segment of conv2's launch, assign_rseg)
//   1x1 otherwise (K = 384 / 512, small maps, small batches) conv1x1_pipe_kernel<T, BM, BN>                2           20-30
//   output conv (<= 7 couts, NCHW fp32 out)                  conv_out_thin_kernel<NT, T>                   1            15
//   input conv (NCHW fp32 in, <= 4 channels)                 conv_in_mfma_kernel<T, CT> (generic file)     1            31
//   fp32 plans / precision="bf16x3" (fp32 tensors)           conv3x3_pipe / conv1x1_pipe <float[, ACC3]>;  -             -
//                                                              the 3-cout output conv: conv_mfma_kernel
//   precision="fp16r32", full-resolution level (ConvArgs::mix)  conv3x3_ws2_kernel<11, f16, 256, SPLIT>   11          120-240
//                                                              conv_out_thin_kernel<.., SPLIT>; its 1x1 residual
//                                                              convs and input conv on the fp32-tensor kernels
//   anything else (odd channel counts: the tiny test net)    conv_generic_kernel                           -             -
//
// A/B switches (they select among these kernels, never a CPU path): the product switches that bear on this table - DMME_NO_WS, DMME_NO_KW,
// DMME_NO_CONV1X1_AS, DMME_NO_CONV_THIN - are each read in their family's *_route function and nowhere else, the experiment / comparison
// routes are keys of DMME_DEBUG_ROUTE="key[=int],..." (debug_route()).  The route is a pure function of (dtype, ConvArgs, environment),
// evaluated when a plan is built and again at every dispatch: a plan must be built and run under one environment.
// The fusion requests in ConvArgs feed the route (gn_part, n_gno, has_gni, r_w: some kernels decline some of them), so a plan-time query
// that asks "what would run this conv if ..." says so with an explicit copy of the arguments.
ConvRoute conv_route(int dtype, const ConvArgs& a) {
    ConvRoute r{};
    if (conv_thin_route(dtype, a, r)) return r;
    if (conv1x1_split_route(dtype, a, r)) return r;
    if (conv1x1_domain(dtype, a) && (conv1x1_as_route(dtype, a, r) || conv1x1_tiled_route(dtype, a, r))) return r;
    if (conv3x3_split_route(dtype, a, r)) return r;
    if (conv3x3_pipe_route(dtype, a, r)) {  // (the two kernels that take over from the four-wave one need its tile to exist)
        if (!conv3x3_ws_route(dtype, a, r)) conv3x3_kw_route(dtype, a, r);
        return r;
    }
    if (conv_mfma_route(dtype, a, r)) return r;
    conv_generic_route(a, r);
    return r;
}

int launch_conv(const ConvRoute& r, int dtype, const ConvArgs& a, hipStream_t s) {
    DMME_REQUIRE(!a.r_w || r.rseg, DMME_ERR_UNSUPPORTED,
                 "conv with a residual segment: only the wave-specialised 3x3 kernel takes it, with raw channel counts inside its domain");
    switch (r.family) {
        case CONV_THIN: return launch_conv_out_thin(a, s);
        case CONV1X1_AS: return launch_conv1x1_as(a, s);
        case CONV1X1_SPLIT:
        case CONV1X1_TILED: return launch_conv1x1(r, dtype, a, s);
        case CONV3X3_SPLIT:
        case CONV3X3_WS:
        case CONV3X3_KW:
        case CONV3X3_PIPE: return launch_conv3x3(r, dtype, a, s);
        case CONV_MFMA: return launch_conv_mfma(r, dtype, a, s);
        default: return launch_conv_generic(dtype, a, s);
    }
}

int launch_conv(int dtype, const ConvArgs& a, hipStream_t s, int force) {
    ConvRoute r{};  // (CONV_GENERIC)
    if (force == 0)
        r = conv_route(dtype, a);
    else if (force == 2)
        conv_mfma_route(dtype, a, r);
    return launch_conv(r, dtype, a, s);
}

void conv_label(const ConvRoute& r, int dtype, const ConvArgs& a, char* buf, int cap) {
    const char* tn = dtype == DMME_BF16 ? "bf16" : dtype == DMME_F16 ? "f16" : a.x3 ? "float:bf16x3" : "float";
    switch (r.family) {
        case CONV_THIN: snprintf(buf, (size_t)cap, a.mix == 3 ? "conv_out_thin_kernel<%d,f16x3>" : "conv_out_thin_kernel<%d>", a.Cout * 9 <= 32 ? 1 : 2); break;
        case CONV1X1_SPLIT: snprintf(buf, (size_t)cap, "conv1x1_split_kernel<128,128>"); break;
        case CONV1X1_AS: snprintf(buf, (size_t)cap, "conv1x1_as_kernel<%d>", (a.C1 + a.C2) / 64); break;
        case CONV1X1_TILED: snprintf(buf, (size_t)cap, "conv1x1_pipe_kernel<%s,%d,%d>", tn, r.BM, r.BN); break;
        case CONV3X3_SPLIT: snprintf(buf, (size_t)cap, a.mix == 2 ? "conv3x3_ws2_kernel<11,f16x3,src16>" : "conv3x3_ws2_kernel<11,f16x3>"); break;
        case CONV3X3_WS: snprintf(buf, (size_t)cap, r.BM == 128 ? (a.r_w ? "conv3x3_ws2_kernel<7,128,res>" : "conv3x3_ws2_kernel<7,128>") : a.r_w ? "conv3x3_ws2_kernel<11,res>" : "conv3x3_ws2_kernel<11>"); break;
        case CONV3X3_KW: snprintf(buf, (size_t)cap, "conv3x3_kw_kernel<%d,%d,%d>", r.NI, r.ring, r.BM); break;
        case CONV3X3_PIPE: snprintf(buf, (size_t)cap, "conv3x3_pipe_kernel<%s,%d,%d,%d,%d>", tn, r.BM, r.BN, r.GT, r.UA); break;
        case CONV_MFMA: snprintf(buf, (size_t)cap, "conv_mfma_kernel<%s,%d,%d,%d>", tn, a.taps, r.BM, r.BN); break;
        default: snprintf(buf, (size_t)cap, "%s<%s>", conv_generic_kernel_name(a), dtype == DMME_BF16 ? "bf16" : dtype == DMME_F16 ? "f16" : "float"); break;
    }
}

// Fused statistics need the staged fast epilogue, one image per tile (stat_tiles), whole cout blocks of whole groups, 16-byte group slices.
// The kernel is the one that runs the conv WITHOUT the request: a kernel that takes the conv either way keeps it (the activation-stationary
// 1x1 kernel declines a request it cannot serve, and the conv would move to the tiled kernel for its statistics' sake).
bool conv_stats_query(int dtype, const ConvArgs& a, int cg, int* tiles, int* px) {
    ConvArgs b = a;
    b.gn_part = nullptr;
    const ConvRoute r = conv_route(dtype, b);
    if (!r.stat_tiles || !stats_cols_ok(a, r.stat_bn, cg, r.vec)) return false;
    *tiles = r.stat_tiles;
    *px = r.stat_px;
    return true;
}

bool conv_gn_in_query(int dtype, const ConvArgs& a) {
    if (getenv("DMME_NO_GN_IN") || !is16(dtype)) return false;  // (read per plan build: the tests toggle it)
    const ConvRoute r = conv_route(dtype, a);
    switch (r.family) {
        case CONV_THIN: return true;      // keeps its image's rows in LDS anyway
        case CONV3X3_SPLIT:               // fills its rows like the wave-specialised kernel it is
        case CONV3X3_WS: return true;     // its parameter fill (ws_fill_par_gni)
        case CONV1X1_AS: return true;     // the store team
        case CONV1X1_TILED: return conv1x1_tiled_gn_in_ok(a, r);  // the tiled kernel's preamble
        case CONV3X3_KW: return !debug_route("no_gn_in_kw") && r.tile.TN == 1;  // one image per tile, the wave's own chunk rows in its LDS
        case CONV3X3_PIPE: return conv3x3_pipe_gn_in_ok(dtype, a, r);
        default: return false;
    }
}

// Whole images per tile: the conv's epilogue sees every value of an (image, group) and finishes the norms itself.
//  - the 64- / 128-pixel tiles of the K-split and four-wave kernels on 8x8 / 4x4 maps (conv_epilogue_store_direct): 1;
//  - the wave-specialised kernel whose 256-pixel tile is a whole 16x16 image, stored in two passes whose statistics it merges itself
//    (scale / shift / {mean, rstd} only - the first pass is in memory before the statistics exist, so no pre-activated output): 2.
int conv_gn_direct_query(int dtype, const ConvArgs& a, const int* cg, int n) {
    if (a.mix || n < 1 || n > 2) return 0;
    const ConvRoute r = conv_route(dtype, a);
    const ConvTile& g = r.tile;
    if (r.family == CONV3X3_WS) {
        if (debug_route("no_gn_direct_ws") || g.TH != a.Hout || g.TW != a.Wout || r.BM != 256) return 0;
        const int cgs = a.gn_cg;  // this tensor's own group size
        if (cgs < 8 || cgs % 8 || 128 % cgs || !stats_cols_ok(a, 128, cgs, 8)) return 0;
        for (int k = 0; k < n; ++k) {
            const int f = cg[k] / cgs;
            if (cg[k] % cgs || (f != 1 && f != 2 && f != 4) || 128 % cg[k]) return 0;
        }
        return 2;
    }
    if (r.family != CONV3X3_KW && r.family != CONV3X3_PIPE) return 0;
    const int HW = a.Hout * a.Wout;
    if (a.out_silu || a.out_nchw || a.res2 || a.Cout % r.vec || HW > 64 || (HW & (HW - 1))) return 0;
    if (r.family == CONV3X3_KW) {
        if (a.up) return 0;
    } else {
        // a conv that the split-K heuristic (few workgroups) would take keeps that path: the route of the same conv with no fusion
        // requested and scratch to split into
        ConvArgs b = a;
        b.n_gno = 0;
        b.gn_part = nullptr;
        b.splitk = (float*)4096;
        b.splitk_cap = (int64_t)1 << 40;
        if (r.BM != 64 || conv_route(dtype, b).ksplit != 1) return 0;
    }
    if (g.TH != a.Hout || g.TW != a.Wout || g.TN * g.TH * g.TW != r.BM || a.Cout % r.BN) return 0;  // whole images, whole cout tiles
    if (HW < 64 / (r.BN / r.vec)) return 0;  // a wave's pixels per channel vector must not straddle images
    for (int k = 0; k < n; ++k)
        if (cg[k] % r.vec || r.BN % cg[k]) return 0;
    return 1;
}

}  // namespace dmme
