// Consistency distillation (Song, Dhariwal, Chen & Sutskever 2023, Algorithm 2) on the discrete grid of GeneralizedDDIM(..., "linear"),
// with the boundary scalings of Latent Consistency Models (Luo et al. 2023): the launches that dmme_distill_noise and dmme_distill_mid do
// not already cover - the target network's consistency function at (zh_m, m), the per-image pseudo-Huber / L2 metric with its gradient
// with respect to the student's raw output, and the moving average of the target network's flat parameter buffer.  All HBM-bound, fp32,
// NCHW.  Like distill.hip the translation unit is compiled with -ffp-contract=off (csrc/Makefile) and every fp32 product and sum is
// rounded on its own (never an fma), so a numpy float32 restatement reproduces the elementwise results bit for bit; the per-image scalars
// (the metric's value and the gradient's row scalar) are formed once per image in double and rounded once.
#include "distill_dev.h"

namespace dmme {

static inline unsigned grid_for(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

static inline bool quads(int64_t chw, std::initializer_list<const void*> ptrs) {
    uintptr_t all = 0;
    for (const void* p : ptrs) all |= (uintptr_t)p;
    return chw % 4 == 0 && (all & 15) == 0;
}

// THE consistency function f(z, .; o) = (c.x z) + (c.y x0), x0 = (p.x o) + (p.y z) clamped iff clip: c = (cs, co), p = (p0, p1) of one
// side of a table row.  The target launch and both loss launches call this one function, so f is one function and not two.
__device__ __forceinline__ float cm_f(float2 c, float2 p, float o, float z, int clip) { return distill_axpby(c, z, distill_x0(p, o, z, clip)); }

struct CmRow {
    float2 p, c;
};
// the row's side at the true m (slots 2, 3 and 8, 9) or at t (slots 0, 1 and 6, 7); NaN for an index outside 1..N
__device__ __forceinline__ CmRow cm_row(const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t b, bool at_m) {
    const int64_t i = distill_index(idx, N, b);
    CmRow r;
    r.p = distill_pair(rows, i, at_m ? 2 : 0);
    r.c = distill_pair(rows, i, at_m ? 8 : 6);
    return r;
}

// ------------------------------------------------------------------ f_target = (cs' z_m) + (co' x0')
__global__ void __launch_bounds__(256) cm_target_quad_kernel(int clip, const float* __restrict__ z_m, const float* __restrict__ out_m,
                                                             const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t chw4,
                                                             int64_t total4, float* __restrict__ f_target) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total4; q += (int64_t)gridDim.x * blockDim.x) {
        const CmRow r = cm_row(rows, idx, N, q / chw4, true);
        const float4 o = reinterpret_cast<const float4*>(out_m)[q], z = reinterpret_cast<const float4*>(z_m)[q];
        reinterpret_cast<float4*>(f_target)[q] =
            make_float4(cm_f(r.c, r.p, o.x, z.x, clip), cm_f(r.c, r.p, o.y, z.y, clip), cm_f(r.c, r.p, o.z, z.z, clip), cm_f(r.c, r.p, o.w, z.w, clip));
    }
}
__global__ void __launch_bounds__(256) cm_target_elem_kernel(int clip, const float* __restrict__ z_m, const float* __restrict__ out_m,
                                                             const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t chw,
                                                             int64_t total, float* __restrict__ f_target) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const CmRow r = cm_row(rows, idx, N, i / chw, true);
        f_target[i] = cm_f(r.c, r.p, out_m[i], z_m[i], clip);
    }
}

// ------------------------------------------------------------------ the metric: three plain launches, no workgroup waits for another
// 1. block (p, b) sums its share of image b's squared differences into scratch[b * parts + p]
// 2. one block finishes every image: S_b = the partials in index order, the metric's value and the gradient's row scalar g_b (both in
//    double, rounded once), sumsq[b], scratch[B * parts + b] = g_b, and loss = (sum_b d_b) / B
// 3. (only with d_out) d_out = g_b (f - f_target), f recomputed by the same device function: the same bits as in launch 1
constexpr int kCmParts = 64;  // blocks per image at the most: scratch holds B * (kCmParts + 1) floats
static inline int cm_parts(int64_t chw) {
    const int64_t p = (chw + 1023) / 1024;
    return (int)(p > kCmParts ? kCmParts : p);
}

__device__ __forceinline__ float cm_diff(const CmRow& r, float o, float z, float ft) { return __fsub_rn(cm_f(r.c, r.p, o, z, 0), ft); }
__device__ __forceinline__ float cm_sq_add(float acc, float d) { return __fadd_rn(acc, __fmul_rn(d, d)); }

template <bool QUAD>
__global__ void __launch_bounds__(256) cm_partial_kernel(const float* __restrict__ z_t, const float* __restrict__ out, const float* __restrict__ f_target,
                                                         const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t chw,
                                                         float* __restrict__ partial) {
    __shared__ float red[16];
    const int b = blockIdx.y;
    const CmRow r = cm_row(rows, idx, N, b, false);
    const int64_t base = (int64_t)b * chw;
    float acc = 0.f;
    if (QUAD) {
        const float4* z4 = reinterpret_cast<const float4*>(z_t + base);
        const float4* o4 = reinterpret_cast<const float4*>(out + base);
        const float4* f4 = reinterpret_cast<const float4*>(f_target + base);
        for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < chw / 4; q += (int64_t)gridDim.x * blockDim.x) {
            const float4 z = z4[q], o = o4[q], f = f4[q];
            acc = cm_sq_add(acc, cm_diff(r, o.x, z.x, f.x));
            acc = cm_sq_add(acc, cm_diff(r, o.y, z.y, f.y));
            acc = cm_sq_add(acc, cm_diff(r, o.z, z.z, f.z));
            acc = cm_sq_add(acc, cm_diff(r, o.w, z.w, f.w));
        }
    } else {
        for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < chw; j += (int64_t)gridDim.x * blockDim.x)
            acc = cm_sq_add(acc, cm_diff(r, out[base + j], z_t[base + j], f_target[base + j]));
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = tot;
}

// one block; thread b (strided) finishes image b.  metric 0: pseudo-Huber d = sqrt(S + c^2) - c, g = gs co p0 / (B sqrt(S + c^2));
// metric 1: L2 d = S / chw, g = 2 gs co p0 / (B chw).  A bad index has NaN partials (its row is NaN), so S, d, g and the loss are NaN.
__global__ void __launch_bounds__(256) cm_finish_kernel(int metric, const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int B,
                                                        int parts, double chw, double c, double gscale, float* __restrict__ scratch,
                                                        float* __restrict__ sumsq, float* __restrict__ loss) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float S = 0.f;
        for (int p = 0; p < parts; ++p) S = __fadd_rn(S, scratch[(int64_t)b * parts + p]);
        const CmRow r = cm_row(rows, idx, N, b, false);
        const double num = (gscale * (double)r.c.y) * (double)r.p.x;
        double d, g;
        if (metric == 0) {
            const double root = sqrt((double)S + c * c);
            d = root - c;
            g = num / ((double)B * root);
        } else {
            d = (double)S / chw;
            g = (2.0 * num) / ((double)B * chw);
        }
        if (sumsq) sumsq[b] = S;
        scratch[(int64_t)B * parts + b] = (float)g;
        acc = __fadd_rn(acc, (float)d);
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = __fmul_rn(tot, (float)(1.0 / (double)B));
}

template <bool QUAD>
__global__ void __launch_bounds__(256) cm_grad_kernel(const float* __restrict__ z_t, const float* __restrict__ out, const float* __restrict__ f_target,
                                                      const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t chw,
                                                      const float* __restrict__ g_rows, float* __restrict__ d_out) {
    const int b = blockIdx.y;
    const CmRow r = cm_row(rows, idx, N, b, false);
    const float g = g_rows[b];
    const int64_t base = (int64_t)b * chw;
    if (QUAD) {
        const float4* z4 = reinterpret_cast<const float4*>(z_t + base);
        const float4* o4 = reinterpret_cast<const float4*>(out + base);
        const float4* f4 = reinterpret_cast<const float4*>(f_target + base);
        float4* d4 = reinterpret_cast<float4*>(d_out + base);
        for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < chw / 4; q += (int64_t)gridDim.x * blockDim.x) {
            const float4 z = z4[q], o = o4[q], f = f4[q];
            d4[q] = make_float4(__fmul_rn(g, cm_diff(r, o.x, z.x, f.x)), __fmul_rn(g, cm_diff(r, o.y, z.y, f.y)), __fmul_rn(g, cm_diff(r, o.z, z.z, f.z)),
                                __fmul_rn(g, cm_diff(r, o.w, z.w, f.w)));
        }
    } else {
        for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < chw; j += (int64_t)gridDim.x * blockDim.x)
            d_out[base + j] = __fmul_rn(g, cm_diff(r, out[base + j], z_t[base + j], f_target[base + j]));
    }
}

// ------------------------------------------------------------------ dst = (dst decay) + (src one_minus)
__device__ __forceinline__ float ema_elem(float d, float s, float decay, float one_minus) { return __fadd_rn(__fmul_rn(d, decay), __fmul_rn(s, one_minus)); }

// quads over the first 4 * n4 elements, the last numel % 4 element by element (16-byte aligned pointers)
__global__ void __launch_bounds__(256) ema_lerp_quad_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n4, int64_t numel, float decay,
                                                            float one_minus) {
    const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    for (int64_t q = first; q < n4; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 d = reinterpret_cast<float4*>(dst)[q], s = reinterpret_cast<const float4*>(src)[q];
        reinterpret_cast<float4*>(dst)[q] = make_float4(ema_elem(d.x, s.x, decay, one_minus), ema_elem(d.y, s.y, decay, one_minus),
                                                        ema_elem(d.z, s.z, decay, one_minus), ema_elem(d.w, s.w, decay, one_minus));
    }
    const int64_t j = 4 * n4 + first;
    if (j < numel) dst[j] = ema_elem(dst[j], src[j], decay, one_minus);
}
__global__ void __launch_bounds__(256) ema_lerp_elem_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t numel, float decay, float one_minus) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < numel; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = ema_elem(dst[i], src[i], decay, one_minus);
}

}  // namespace dmme

// ------------------------------------------------------------------ entry points
DMME_API int dmme_cm_target(int clip, const float* z_m, const float* out_m, const float* rows, const int64_t* idx, int N, int B, int64_t chw, float* f_target,
                            void* stream) {
    using namespace dmme;
    DMME_REQUIRE(z_m && out_m && rows && idx && f_target, DMME_ERR_INVALID, "cm_target: null argument");
    DMME_REQUIRE(N >= 1 && B > 0 && chw > 0, DMME_ERR_INVALID, "cm_target: N = %d, B = %d, chw = %lld", N, B, (long long)chw);
    const int64_t total = (int64_t)B * chw;
    hipStream_t s = (hipStream_t)stream;
    if (quads(chw, {z_m, out_m, f_target}))
        hipLaunchKernelGGL(cm_target_quad_kernel, dim3(grid_for(total / 4)), dim3(256), 0, s, clip != 0, z_m, out_m, rows, idx, N, chw / 4, total / 4, f_target);
    else
        hipLaunchKernelGGL(cm_target_elem_kernel, dim3(grid_for(total)), dim3(256), 0, s, clip != 0, z_m, out_m, rows, idx, N, chw, total, f_target);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

DMME_API int dmme_cm_loss(int metric, const float* z_t, const float* out, const float* f_target, const float* rows, const int64_t* idx, int N, int B,
                          int64_t chw, float c, float* loss, float* sumsq, float* d_out, float grad_scale, float* scratch, void* stream) {
    using namespace dmme;
    DMME_REQUIRE(metric == DMME_CM_PSEUDO_HUBER || metric == DMME_CM_L2, DMME_ERR_INVALID, "cm_loss: metric %d (0: pseudo-huber, 1: l2)", metric);
    DMME_REQUIRE(z_t && out && f_target && rows && idx && loss && scratch, DMME_ERR_INVALID, "cm_loss: null argument");
    DMME_REQUIRE(N >= 1 && B > 0 && B <= 65535 && chw > 0, DMME_ERR_INVALID, "cm_loss: N = %d, B = %d (1..65535), chw = %lld", N, B, (long long)chw);
    DMME_REQUIRE(metric != DMME_CM_PSEUDO_HUBER || c > 0.f, DMME_ERR_INVALID, "cm_loss: the pseudo-Huber metric needs c > 0, got %g", (double)c);
    const int parts = cm_parts(chw);
    hipStream_t s = (hipStream_t)stream;
    const bool quad = quads(chw, {z_t, out, f_target, d_out});  // (a null d_out is aligned)
    if (quad)
        hipLaunchKernelGGL(cm_partial_kernel<true>, dim3(parts, B), dim3(256), 0, s, z_t, out, f_target, rows, idx, N, chw, scratch);
    else
        hipLaunchKernelGGL(cm_partial_kernel<false>, dim3(parts, B), dim3(256), 0, s, z_t, out, f_target, rows, idx, N, chw, scratch);
    DMME_CHECK_LAUNCH();
    hipLaunchKernelGGL(cm_finish_kernel, dim3(1), dim3(256), 0, s, metric, rows, idx, N, B, parts, (double)chw, (double)c, (double)grad_scale, scratch, sumsq, loss);
    DMME_CHECK_LAUNCH();
    if (d_out) {
        const float* g_rows = scratch + (int64_t)B * parts;
        if (quad)
            hipLaunchKernelGGL(cm_grad_kernel<true>, dim3(parts, B), dim3(256), 0, s, z_t, out, f_target, rows, idx, N, chw, g_rows, d_out);
        else
            hipLaunchKernelGGL(cm_grad_kernel<false>, dim3(parts, B), dim3(256), 0, s, z_t, out, f_target, rows, idx, N, chw, g_rows, d_out);
        DMME_CHECK_LAUNCH();
    }
    return DMME_OK;
}

DMME_API int dmme_ema_lerp(float* dst, const float* src, int64_t numel, float decay, void* stream) {
    using namespace dmme;
    DMME_REQUIRE(dst && src && numel > 0, DMME_ERR_INVALID, "ema_lerp: null argument or numel = %lld", (long long)numel);
    DMME_REQUIRE(decay >= 0.f && decay <= 1.f, DMME_ERR_INVALID, "ema_lerp: decay %g outside [0, 1]", (double)decay);
    const float one_minus = (float)(1.0 - (double)decay);
    hipStream_t s = (hipStream_t)stream;
    if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0 && numel >= 4) {
        const int64_t n4 = numel / 4;
        hipLaunchKernelGGL(ema_lerp_quad_kernel, dim3(grid_for(n4)), dim3(256), 0, s, dst, src, n4, numel, decay, one_minus);
    } else {
        hipLaunchKernelGGL(ema_lerp_elem_kernel, dim3(grid_for(numel)), dim3(256), 0, s, dst, src, numel, decay, one_minus);
    }
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}
