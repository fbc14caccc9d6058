// x0 thresholding in front of every sampler update: the static clip (clip_denoised of the published DDPM / IDDPM / ADM samplers) and the
// dynamic percentile clip (Saharia et al. 2022, section 2.3).  The stage rewrites the eps prediction in place so that the x0 it implies,
// x0 = A_t x - B_t e, lies in [-1, 1]; the update kinds, their tables and their kernels are untouched.  All HBM-bound, fp32, NCHW.  Like
// prediction.hip the translation unit is compiled with -ffp-contract=off (csrc/Makefile) and every product, sum, difference and quotient is
// rounded on its own: a numpy float32 restatement reproduces every bit (tests/threshold_ref.py).  The percentile is an exact order
// statistic, found by a radix select over the bit patterns of |x0| (non-negative floats order like their unsigned bits) with integer
// atomics only: the result does not depend on the order in which threads arrive.
#include "plan.h"

namespace dmme {

constexpr int kThrLdsCapacity = 36864;  // elements of one image the one-workgroup form keeps in LDS (144 KiB of the CU's 160)
constexpr int kThrLdsThreads = 1024;
constexpr int kThrParts = 64;           // streaming form: workgroups per image at the most
constexpr int kThrPartElems = 4096;     // ... and the elements one of them takes where the image has enough
// streaming form, per image: four digit histograms, then {non-finite flag, smallest value above a_k, two spare words}
constexpr int kThrHistWords = 4 * 256;
constexpr int kThrImageWords = kThrHistWords + 4;

struct ThrArgs {
    float* out;               // the network output: [B][planes][chw], or two halves [2][B][chw] (conditional, unconditional)
    const float* x;           // x_t, [B][chw] (of the first half)
    const float* table;       // [T+1][4] = {A, B, C, D}
    const int64_t* t;         // device timesteps, t_len of them
    const float* sg_coef;     // two halves, chain form: the guidance scale is sg_coef[sg_row * sg_state[0] + sg_col] ...
    const int64_t* sg_state;  // ... at the loop state's index
    float sg;                 // two halves, eager form
    int sg_row, sg_col;
    int T, t_len, B, planes, halves;
    int64_t chw;
    int k;                    // dynamic: the order statistic below the quantile ...
    float frac;               // ... and the weight of the one above
    unsigned* scratch;        // streaming form: kThrImageWords per image
};

struct ThrRow {
    float A, B, C, D;
};
// A timestep outside 0..T is never used as an index: its row comes out NaN, and so does the image
__device__ __forceinline__ ThrRow thr_row(const ThrArgs& a, int64_t b) {
    const int64_t tn = a.t[a.t_len == 1 ? 0 : b];
    const float n = __builtin_nanf("");
    if (tn < 0 || tn > a.T) return {n, n, n, n};
    const float* r = a.table + 4 * tn;
    return {r[0], r[1], r[2], r[3]};
}
__device__ __forceinline__ float thr_scale(const ThrArgs& a) {
    if (a.halves != 2) return 1.0f;
    return a.sg_coef ? a.sg_coef[(int64_t)a.sg_row * a.sg_state[0] + a.sg_col] : a.sg;
}
// where element j of image b's eps plane sits in `out` (first half), and how far on its unconditional twin
__device__ __forceinline__ int64_t thr_eps_index(const ThrArgs& a, int64_t b, int64_t j) { return b * a.planes * a.chw + j; }
__device__ __forceinline__ int64_t thr_half_stride(const ThrArgs& a) { return (int64_t)a.B * a.chw; }
// the eps the update will use: the plane itself, or the update's own mix of the two halves
__device__ __forceinline__ float thr_eps(const ThrArgs& a, int64_t eo, float sg) {
    const float e = a.out[eo];
    return a.halves == 2 ? cfg_mix(e, a.out[eo + thr_half_stride(a)], sg) : e;
}
__device__ __forceinline__ float thr_x0(const ThrRow& r, float x, float e) { return __fsub_rn(__fmul_rn(r.A, x), __fmul_rn(r.B, e)); }
__device__ __forceinline__ unsigned thr_abs_bits(float x0) { return __float_as_uint(x0) & 0x7fffffffu; }
__device__ __forceinline__ bool thr_finite(unsigned abs_bits) { return abs_bits < 0x7f800000u; }
// an element with s == 1 and |x0| <= 1 is left alone (false); every other one gets e' from the clamped x0
__device__ __forceinline__ bool thr_clip(const ThrRow& r, float s, float x, float x0, float& e) {
    if (s == 1.0f && fabsf(x0) <= 1.0f) return false;
    const float c = fminf(fmaxf(x0, -s), s);
    e = __fsub_rn(__fmul_rn(r.C, x), __fmul_rn(r.D, __fdiv_rn(c, s)));
    return true;
}
__device__ __forceinline__ void thr_store(const ThrArgs& a, int64_t eo, float e) {
    a.out[eo] = e;
    if (a.halves == 2) a.out[eo + thr_half_stride(a)] = e;
}
// s = max(1, a_k + frac (a_k1 - a_k)); a_k1 is not looked at where frac == 0
__device__ __forceinline__ float thr_s(unsigned ak, unsigned ak1, float frac) {
    const float lo = __uint_as_float(ak);
    const float q = frac == 0.0f ? lo : __fadd_rn(lo, __fmul_rn(frac, __fsub_rn(__uint_as_float(ak1), lo)));
    return q > 1.0f ? q : 1.0f;
}

// ------------------------------------------------------------------ static mode: elementwise, no reduction
// chw % 4 == 0 and 16-byte aligned pointers: a quad never straddles two images or planes
__global__ void __launch_bounds__(256) thr_static_quad_kernel(ThrArgs a, int64_t chw4, int64_t total4) {
    const float sg = thr_scale(a);
    const float nan = __builtin_nanf("");
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total4; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = q / chw4, j = (q - b * chw4) * 4, eo = thr_eps_index(a, b, j);
        const ThrRow r = thr_row(a, b);
        const float4 xv = *reinterpret_cast<const float4*>(a.x + q * 4);
        float4 ev = *reinterpret_cast<const float4*>(a.out + eo);
        const float* xs = reinterpret_cast<const float*>(&xv);
        float* es = reinterpret_cast<float*>(&ev);
        if (a.halves == 2) {
            const float4 uv = *reinterpret_cast<const float4*>(a.out + eo + thr_half_stride(a));
            const float* us = reinterpret_cast<const float*>(&uv);
#pragma unroll
            for (int i = 0; i < 4; ++i) es[i] = cfg_mix(es[i], us[i], sg);
        }
        bool touched[4];
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x0 = thr_x0(r, xs[i], es[i]);
            if (!thr_finite(thr_abs_bits(x0))) {
                es[i] = nan;
                touched[i] = true;
            } else {
                touched[i] = thr_clip(r, 1.0f, xs[i], x0, es[i]);
            }
            any |= touched[i];
        }
        if (!any) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (touched[i]) thr_store(a, eo + i, es[i]);
    }
}
// ragged sizes: element by element
__global__ void __launch_bounds__(256) thr_static_elem_kernel(ThrArgs a, int64_t total) {
    const float sg = thr_scale(a);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / a.chw, eo = thr_eps_index(a, b, i - b * a.chw);
        const ThrRow r = thr_row(a, b);
        const float x = a.x[i];
        float e = thr_eps(a, eo, sg);
        const float x0 = thr_x0(r, x, e);
        if (!thr_finite(thr_abs_bits(x0)))
            thr_store(a, eo, __builtin_nanf(""));
        else if (thr_clip(r, 1.0f, x, x0, e))
            thr_store(a, eo, e);
    }
}

// ------------------------------------------------------------------ dynamic mode: the radix select
// One digit of the select, by the block's first wave: hist[256] (LDS) counts the candidates by their digit; the bin that holds rank k
// becomes the digit, k the rank inside it, eq the bin's count.  sel = {prefix, k, eq}.  The caller synchronises around it.
__device__ __forceinline__ void thr_pick_digit(const unsigned* hist, int shift, unsigned* sel) {
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const unsigned k = sel[1];
    unsigned h[4], local = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = hist[4 * lane + i];
        local += h[i];
    }
    unsigned incl = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned n = __shfl_up(incl, off);
        if (lane >= off) incl += n;
    }
    unsigned cum = incl - local;
    if (cum <= k && k < incl) {  // one lane: the candidates number more than k
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (k < cum + h[i]) {
                sel[0] |= (unsigned)(4 * lane + i) << shift;
                sel[1] = k - cum;
                sel[2] = h[i];
                break;
            }
            cum += h[i];
        }
    }
}
__device__ __forceinline__ unsigned thr_digit_mask(int pass) { return pass == 0 ? 0u : 0xffffffffu << (32 - 8 * pass); }

__device__ __forceinline__ void thr_fill_nan(const ThrArgs& a, int64_t b, int64_t first, int64_t stride) {
    const float nan = __builtin_nanf("");
    for (int64_t j = first; j < a.chw; j += stride) thr_store(a, thr_eps_index(a, b, j), nan);
}
__device__ __forceinline__ void thr_apply(const ThrArgs& a, const ThrRow& r, float sg, float s, int64_t b, int64_t first, int64_t stride) {
    for (int64_t j = first; j < a.chw; j += stride) {
        const int64_t eo = thr_eps_index(a, b, j);
        const float x = a.x[b * a.chw + j];
        float e = thr_eps(a, eo, sg);
        if (thr_clip(r, s, x, thr_x0(r, x, e), e)) thr_store(a, eo, e);
    }
}

// One workgroup per image, the image's |x0| bits resident in LDS: four digit passes over LDS, one for the neighbour above a_k where the
// quantile needs it, then the rewrite.
__global__ void __launch_bounds__(kThrLdsThreads) thr_lds_kernel(ThrArgs a) {
    extern __shared__ unsigned vals[];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[3];
    __shared__ unsigned bad, above;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int n = (int)a.chw;
    const ThrRow r = thr_row(a, b);
    const float sg = thr_scale(a);
    if (tid < 256) hist[tid] = 0u;
    if (tid == 0) {
        sel[0] = 0u;
        sel[1] = (unsigned)a.k;
        sel[2] = 0u;
        bad = 0u;
        above = 0xffffffffu;
    }
    __syncthreads();
    bool mine_bad = false;
    for (int j = tid; j < n; j += kThrLdsThreads) {
        const unsigned v = thr_abs_bits(thr_x0(r, a.x[b * a.chw + j], thr_eps(a, thr_eps_index(a, b, j), sg)));
        vals[j] = v;
        mine_bad |= !thr_finite(v);
    }
    if (mine_bad) atomicOr(&bad, 1u);
    __syncthreads();
    if (bad) {  // (the whole block takes this branch)
        thr_fill_nan(a, b, tid, kThrLdsThreads);
        return;
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned mask = thr_digit_mask(pass), prefix = sel[0];
        for (int j = tid; j < n; j += kThrLdsThreads) {
            const unsigned v = vals[j];
            if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        thr_pick_digit(hist, shift, sel);
        __syncthreads();
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
    }
    const unsigned ak = sel[0];
    unsigned ak1 = ak;
    if (a.frac != 0.0f && sel[1] + 1u >= sel[2]) {  // the next order statistic is the smallest value above a_k
        for (int j = tid; j < n; j += kThrLdsThreads) {
            const unsigned v = vals[j];
            if (v > ak) atomicMin(&above, v);
        }
        __syncthreads();
        ak1 = above;
    }
    thr_apply(a, r, sg, thr_s(ak, ak1, a.frac), b, tid, kThrLdsThreads);
}

// The streaming form: grid (parts, B), one launch per stage on the same grid, the image's histograms in `scratch`.
//   stage 0..3  the digit's histogram of this block's share, added to the image's (stage 0 also raises the non-finite flag)
//   stage 4     the smallest value above a_k, where the quantile needs it
//   stage 5     the rewrite
// Every block re-derives the digits chosen so far from the finished histograms of the earlier stages, so nothing but the counts
// passes from one launch to the next.  thr_clear_kernel comes first: the scratch need not be zero on entry.
__global__ void __launch_bounds__(256) thr_clear_kernel(unsigned* scratch, int64_t words) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x)
        scratch[i] = i % kThrImageWords == kThrHistWords + 1 ? 0xffffffffu : 0u;
}
__global__ void __launch_bounds__(256) thr_stream_kernel(ThrArgs a, int stage) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel[3];
    __shared__ unsigned above;
    const int64_t b = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t first = blockIdx.x * (int64_t)blockDim.x + tid, stride = (int64_t)gridDim.x * blockDim.x;
    unsigned* img = a.scratch + b * kThrImageWords;
    const ThrRow r = thr_row(a, b);
    const float sg = thr_scale(a);
    if (stage > 0 && img[kThrHistWords]) {  // a non-finite x0 somewhere in the image: nothing to select, NaN everywhere
        if (stage == 5) thr_fill_nan(a, b, first, stride);
        return;
    }
    if (tid == 0) {
        sel[0] = 0u;
        sel[1] = (unsigned)a.k;
        sel[2] = 0u;
        above = 0xffffffffu;
    }
    const int done = stage < 4 ? stage : 4;
    for (int pass = 0; pass < done; ++pass) {
        hist[tid] = img[256 * pass + tid];
        __syncthreads();
        thr_pick_digit(hist, 24 - 8 * pass, sel);
        __syncthreads();
    }
    if (stage < 4) {
        const int shift = 24 - 8 * stage;
        const unsigned mask = thr_digit_mask(stage);
        hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = sel[0];
        bool mine_bad = false;
        for (int64_t j = first; j < a.chw; j += stride) {
            const unsigned v = thr_abs_bits(thr_x0(r, a.x[b * a.chw + j], thr_eps(a, thr_eps_index(a, b, j), sg)));
            mine_bad |= !thr_finite(v);
            if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
        }
        if (stage == 0 && mine_bad) atomicOr(&img[kThrHistWords], 1u);
        __syncthreads();
        if (hist[tid]) atomicAdd(&img[256 * stage + tid], hist[tid]);
        return;
    }
    __syncthreads();
    const unsigned ak = sel[0];
    const bool needs_above = a.frac != 0.0f && sel[1] + 1u >= sel[2];
    if (stage == 4) {
        if (!needs_above) return;
        for (int64_t j = first; j < a.chw; j += stride) {
            const unsigned v = thr_abs_bits(thr_x0(r, a.x[b * a.chw + j], thr_eps(a, thr_eps_index(a, b, j), sg)));
            if (v > ak) atomicMin(&above, v);
        }
        __syncthreads();
        if (tid == 0 && above != 0xffffffffu) atomicMin(&img[kThrHistWords + 1], above);
        return;
    }
    thr_apply(a, r, sg, thr_s(ak, needs_above ? img[kThrHistWords + 1] : ak, a.frac), b, first, stride);
}

static inline unsigned thr_grid_for(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}
static inline int thr_parts(int64_t chw) {
    const int64_t p = (chw + kThrPartElems - 1) / kThrPartElems;
    return (int)(p > kThrParts ? kThrParts : (p < 1 ? 1 : p));
}
int64_t x0_threshold_scratch_bytes(int B, int64_t chw) { return B > 0 && chw > 0 ? (int64_t)B * kThrImageWords * (int64_t)sizeof(unsigned) : 0; }

// sg_coef / sg_state: the chain form's guidance scale (two halves), else sg
int launch_x0_threshold(int mode, float* out, const float* x, const float* table, int T, const int64_t* t, int t_len, int B, int64_t chw, int planes,
                        int halves, float sg, const float* sg_coef, int sg_row, int sg_col, const int64_t* sg_state, int k, float frac, void* scratch,
                        hipStream_t s) {
    DMME_REQUIRE(mode == DMME_THRESHOLD_STATIC || mode == DMME_THRESHOLD_DYNAMIC, DMME_ERR_INVALID,
                 "x0_threshold: mode %d (1: static, 2: dynamic; 0 means no thresholding: do not launch)", mode);
    DMME_REQUIRE(out && x && t && T > 0 && B > 0 && B <= 65535 && chw > 0 && chw < (1ll << 31), DMME_ERR_INVALID, "x0_threshold: bad argument (B = %d, chw = %lld)", B,
                 (long long)chw);
    DMME_REQUIRE(table, DMME_ERR_INVALID, "x0_threshold: null table (needs the [T+1][4] rows A, B, C, D)");
    DMME_REQUIRE(t_len == 1 || t_len == B, DMME_ERR_INVALID, "x0_threshold: timestep tensor of length %d does not broadcast against batch %d", t_len, B);
    DMME_REQUIRE((planes == 1 || planes == 2) && (halves == 1 || halves == 2) && (halves == 1 || planes == 1), DMME_ERR_INVALID,
                 "x0_threshold: %d planes per image in %d halves (one or two planes; two halves hold one plane each)", planes, halves);
    DMME_REQUIRE(!sg_coef || sg_state, DMME_ERR_INVALID, "x0_threshold: a guidance scale read from the chain's table needs the loop state");
    ThrArgs a{};
    a.out = out, a.x = x, a.table = table, a.t = t, a.sg_coef = halves == 2 ? sg_coef : nullptr, a.sg_state = sg_state, a.sg = sg, a.sg_row = sg_row, a.sg_col = sg_col;
    a.T = T, a.t_len = t_len, a.B = B, a.planes = planes, a.halves = halves, a.chw = chw, a.k = k, a.frac = frac, a.scratch = (unsigned*)scratch;
    const int64_t total = (int64_t)B * chw;
    if (mode == DMME_THRESHOLD_STATIC) {
        if (chw % 4 == 0 && (((uintptr_t)out | (uintptr_t)x) & 15) == 0)
            hipLaunchKernelGGL(thr_static_quad_kernel, dim3(thr_grid_for(total / 4)), dim3(256), 0, s, a, chw / 4, total / 4);
        else
            hipLaunchKernelGGL(thr_static_elem_kernel, dim3(thr_grid_for(total)), dim3(256), 0, s, a, total);
        DMME_CHECK_LAUNCH();
        return DMME_OK;
    }
    // p outside [0, 1] has no (k, frac): k = floor(p (n - 1)) lies in 0..n-1, frac in [0, 1], and the last order statistic has none above it
    DMME_REQUIRE(k >= 0 && (int64_t)k < chw && frac >= 0.0f && frac <= 1.0f && ((int64_t)k + 1 < chw || frac == 0.0f), DMME_ERR_INVALID,
                 "x0_threshold: order statistic k = %d with weight %g on the next one, of %lld values (a percentile outside [0, 1]?)", k, (double)frac,
                 (long long)chw);
    if (chw <= kThrLdsCapacity && !debug_route("thr_stream")) {
        static bool lds_allowed = false;  // (the first launch of a shape is never inside a capture: the chain's trial step, or an eager call)
        if (!lds_allowed) {
            DMME_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(thr_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               kThrLdsCapacity * (int)sizeof(unsigned)));
            lds_allowed = true;
        }
        hipLaunchKernelGGL(thr_lds_kernel, dim3(B), dim3(kThrLdsThreads), (size_t)chw * sizeof(unsigned), s, a);
        DMME_CHECK_LAUNCH();
        return DMME_OK;
    }
    DMME_REQUIRE(scratch, DMME_ERR_INVALID, "x0_threshold: images of %lld values (more than %d) are selected through a scratch buffer of dmme_x0_threshold_scratch_bytes",
                 (long long)chw, kThrLdsCapacity);
    const int64_t words = (int64_t)B * kThrImageWords;
    hipLaunchKernelGGL(thr_clear_kernel, dim3(thr_grid_for(words)), dim3(256), 0, s, a.scratch, words);
    DMME_CHECK_LAUNCH();
    for (int stage = 0; stage < 6; ++stage) {
        hipLaunchKernelGGL(thr_stream_kernel, dim3(thr_parts(chw), B), dim3(256), 0, s, a, stage);
        DMME_CHECK_LAUNCH();
    }
    return DMME_OK;
}

}  // namespace dmme

// ------------------------------------------------------------------ entry points
DMME_API int dmme_x0_threshold(int mode, float* model_out, const float* x, const float* table, int T, const int64_t* t, int t_len, int B, int64_t chw,
                               int planes, int halves, float guidance_scale, int k, float frac, void* scratch, void* stream) {
    return launch_x0_threshold(mode, model_out, x, table, T, t, t_len, B, chw, planes, halves, guidance_scale, nullptr, 0, 0, nullptr, k, frac, scratch,
                               (hipStream_t)stream);
}

DMME_API int64_t dmme_x0_threshold_scratch_bytes(int B, int64_t chw) { return x0_threshold_scratch_bytes(B, chw); }

DMME_API int dmme_x0_threshold_lds_capacity(void) { return kThrLdsCapacity; }

DMME_API int dmme_unet_plan_set_threshold(dmme_plan* plan, int mode, const float* table, int T, int k, float frac, void* scratch) {
    DMME_REQUIRE(plan, DMME_ERR_INVALID, "plan_set_threshold: null plan");
    DMME_REQUIRE(mode == DMME_THRESHOLD_NONE || mode == DMME_THRESHOLD_STATIC || mode == DMME_THRESHOLD_DYNAMIC, DMME_ERR_INVALID,
                 "plan_set_threshold: mode %d (0: none, 1: static, 2: dynamic)", mode);
    if (mode == DMME_THRESHOLD_NONE) {
        plan->thr_mode = DMME_THRESHOLD_NONE;
        plan->thr_table = nullptr;
        plan->thr_scratch = nullptr;
        plan->thr_T = plan->thr_k = 0;
        plan->thr_frac = 0.f;
        return DMME_OK;
    }
    DMME_REQUIRE(plan->cfg.arch != DMME_ARCH_CLASSIFIER, DMME_ERR_INVALID, "plan_set_threshold: a classifier predicts no noise: nothing to threshold");
    DMME_REQUIRE(table && T > 0, DMME_ERR_INVALID, "plan_set_threshold: thresholding needs its [T+1][4] table");
    const int64_t chw = (int64_t)plan->cfg.in_channels * plan->H * plan->W;
    if (mode == DMME_THRESHOLD_DYNAMIC) {
        DMME_REQUIRE(k >= 0 && (int64_t)k < chw && frac >= 0.0f && frac <= 1.0f && ((int64_t)k + 1 < chw || frac == 0.0f), DMME_ERR_INVALID,
                     "plan_set_threshold: order statistic k = %d with weight %g on the next one, of %lld values (a percentile outside [0, 1]?)", k, (double)frac,
                     (long long)chw);
        DMME_REQUIRE(scratch || (chw <= kThrLdsCapacity && !debug_route("thr_stream")), DMME_ERR_INVALID,
                     "plan_set_threshold: images of %lld values need a scratch buffer of dmme_x0_threshold_scratch_bytes", (long long)chw);
    }
    plan->thr_mode = mode;
    plan->thr_table = table;
    plan->thr_T = T;
    plan->thr_k = k;
    plan->thr_frac = frac;
    plan->thr_scratch = scratch;
    return DMME_OK;
}
