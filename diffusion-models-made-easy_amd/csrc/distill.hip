// Progressive distillation (Salimans & Ho, ICLR 2022, Algorithm 2) on the discrete grid of GeneralizedDDIM(..., "linear"): the three
// elementwise launches around the teacher's two forwards - forward noising at the timestep a student index stands for, the teacher's
// first DDIM step, and the student's regression target.  The target is the convex combination x~ = w1 x1 + w2 x2 of the teacher's two x0
// estimates (the paper's quotient (z_e - r z_t) / (alpha_e - r alpha_t) subtracts nearly equal numbers and is never formed; neither is
// z_e).  All HBM-bound, fp32, NCHW.  Like prediction.hip the translation unit is compiled with -ffp-contract=off (csrc/Makefile) and every
// product and sum below is explicitly rounded on its own (never an fma): z_t carries dmme_q_sample's bits, and a numpy float32
// restatement reproduces the rest bit for bit.
#include "distill_dev.h"  // distill_index, distill_pair, distill_axpby, distill_x0: shared with consistency.hip

namespace dmme {

static inline unsigned grid_for(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// ------------------------------------------------------------------ z_t at t = tt[idx][0], and the timestep vectors of the two forwards
__device__ __forceinline__ float distill_noise_elem(float sa, float sd, float x, float n) { return __fadd_rn(__fmul_rn(sa, x), __fmul_rn(sd, n)); }

struct NoiseRow {
    float sa, sd;
};
// the first thread of an image also writes its two timesteps (0, 0 and the status word where the index is bad)
__device__ __forceinline__ NoiseRow distill_noise_row(const int64_t* __restrict__ idx, const int64_t* __restrict__ tt, const float* __restrict__ sqrt_abar,
                                                      const float* __restrict__ sqrt_1m_abar, int N, int64_t b, bool first, int64_t* __restrict__ t_out,
                                                      int64_t* __restrict__ m_out, int* __restrict__ status) {
    const int64_t i = distill_index(idx, N, b);
    NoiseRow r;
    if (i == 0) {
        r.sa = r.sd = __builtin_nanf("");
        if (first) {
            t_out[b] = 0;
            m_out[b] = 0;
            status[0] = 1;
        }
        return r;
    }
    const int64_t t = tt[2 * i];
    r.sa = sqrt_abar[t];
    r.sd = sqrt_1m_abar[t];
    if (first) {
        t_out[b] = t;
        m_out[b] = tt[2 * i + 1];
    }
    return r;
}

// chw % 4 == 0 and 16-byte aligned pointers: a quad never straddles two images
__global__ void __launch_bounds__(256) distill_noise_quad_kernel(const float* __restrict__ x0, const float* __restrict__ z, const int64_t* __restrict__ idx,
                                                                 const int64_t* __restrict__ tt, const float* __restrict__ sqrt_abar,
                                                                 const float* __restrict__ sqrt_1m_abar, int N, int64_t chw4, int64_t total4,
                                                                 float* __restrict__ z_t, int64_t* __restrict__ t_out, int64_t* __restrict__ m_out,
                                                                 int* __restrict__ status) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total4; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = q / chw4;
        const NoiseRow r = distill_noise_row(idx, tt, sqrt_abar, sqrt_1m_abar, N, b, q == b * chw4, t_out, m_out, status);
        const float4 x = reinterpret_cast<const float4*>(x0)[q], n = reinterpret_cast<const float4*>(z)[q];
        reinterpret_cast<float4*>(z_t)[q] = make_float4(distill_noise_elem(r.sa, r.sd, x.x, n.x), distill_noise_elem(r.sa, r.sd, x.y, n.y),
                                                        distill_noise_elem(r.sa, r.sd, x.z, n.z), distill_noise_elem(r.sa, r.sd, x.w, n.w));
    }
}
// ragged sizes: element by element
__global__ void __launch_bounds__(256) distill_noise_elem_kernel(const float* __restrict__ x0, const float* __restrict__ z, const int64_t* __restrict__ idx,
                                                                 const int64_t* __restrict__ tt, const float* __restrict__ sqrt_abar,
                                                                 const float* __restrict__ sqrt_1m_abar, int N, int64_t chw, int64_t total,
                                                                 float* __restrict__ z_t, int64_t* __restrict__ t_out, int64_t* __restrict__ m_out,
                                                                 int* __restrict__ status) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / chw;
        const NoiseRow r = distill_noise_row(idx, tt, sqrt_abar, sqrt_1m_abar, N, b, i == b * chw, t_out, m_out, status);
        z_t[i] = distill_noise_elem(r.sa, r.sd, x0[i], z[i]);
    }
}

// ------------------------------------------------------------------ the teacher's first DDIM step: z_m = m0 x1 + m1 z_t
struct MidRow {
    float2 p, m;
};
__device__ __forceinline__ MidRow distill_mid_row(const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t b) {
    const int64_t i = distill_index(idx, N, b);
    MidRow r;
    r.p = distill_pair(rows, i, 0);
    r.m = distill_pair(rows, i, 4);
    return r;
}
__device__ __forceinline__ float distill_mid_elem(const MidRow& r, float o1, float zt, int clip) {
    return distill_axpby(r.m, distill_x0(r.p, o1, zt, clip), zt);
}

__global__ void __launch_bounds__(256) distill_mid_quad_kernel(int clip, const float* __restrict__ z_t, const float* __restrict__ out1,
                                                               const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t chw4,
                                                               int64_t total4, float* __restrict__ z_m) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total4; q += (int64_t)gridDim.x * blockDim.x) {
        const MidRow r = distill_mid_row(rows, idx, N, q / chw4);
        const float4 o = reinterpret_cast<const float4*>(out1)[q], z = reinterpret_cast<const float4*>(z_t)[q];
        reinterpret_cast<float4*>(z_m)[q] =
            make_float4(distill_mid_elem(r, o.x, z.x, clip), distill_mid_elem(r, o.y, z.y, clip), distill_mid_elem(r, o.z, z.z, clip), distill_mid_elem(r, o.w, z.w, clip));
    }
}
__global__ void __launch_bounds__(256) distill_mid_elem_kernel(int clip, const float* __restrict__ z_t, const float* __restrict__ out1,
                                                               const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t chw,
                                                               int64_t total, float* __restrict__ z_m) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        z_m[i] = distill_mid_elem(distill_mid_row(rows, idx, N, i / chw), out1[i], z_t[i], clip);
}

// ------------------------------------------------------------------ the student's target: q0 (w1 x1 + w2 x2) + q1 z_t
struct TargetRow {
    float2 p, p2, w, q;
};
__device__ __forceinline__ TargetRow distill_target_row(const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t b) {
    const int64_t i = distill_index(idx, N, b);
    TargetRow r;
    r.p = distill_pair(rows, i, 0);
    r.p2 = distill_pair(rows, i, 2);
    r.w = distill_pair(rows, i, 6);
    r.q = distill_pair(rows, i, 8);
    return r;
}
__device__ __forceinline__ float distill_target_elem(const TargetRow& r, float zt, float o1, float zm, float o2, int clip) {
    const float x1 = distill_x0(r.p, o1, zt, clip);
    const float x2 = distill_x0(r.p2, o2, zm, clip);
    return distill_axpby(r.q, distill_axpby(r.w, x1, x2), zt);
}

__global__ void __launch_bounds__(256) distill_target_quad_kernel(int clip, const float* __restrict__ z_t, const float* __restrict__ out1,
                                                                  const float* __restrict__ z_m, const float* __restrict__ out2,
                                                                  const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t chw4,
                                                                  int64_t total4, float* __restrict__ target) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total4; q += (int64_t)gridDim.x * blockDim.x) {
        const TargetRow r = distill_target_row(rows, idx, N, q / chw4);
        const float4 zt = reinterpret_cast<const float4*>(z_t)[q], o1 = reinterpret_cast<const float4*>(out1)[q];
        const float4 zm = reinterpret_cast<const float4*>(z_m)[q], o2 = reinterpret_cast<const float4*>(out2)[q];
        reinterpret_cast<float4*>(target)[q] = make_float4(distill_target_elem(r, zt.x, o1.x, zm.x, o2.x, clip), distill_target_elem(r, zt.y, o1.y, zm.y, o2.y, clip),
                                                           distill_target_elem(r, zt.z, o1.z, zm.z, o2.z, clip), distill_target_elem(r, zt.w, o1.w, zm.w, o2.w, clip));
    }
}
__global__ void __launch_bounds__(256) distill_target_elem_kernel(int clip, const float* __restrict__ z_t, const float* __restrict__ out1,
                                                                  const float* __restrict__ z_m, const float* __restrict__ out2,
                                                                  const float* __restrict__ rows, const int64_t* __restrict__ idx, int N, int64_t chw,
                                                                  int64_t total, float* __restrict__ target) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        target[i] = distill_target_elem(distill_target_row(rows, idx, N, i / chw), z_t[i], out1[i], z_m[i], out2[i], clip);
}

static inline bool quads(int64_t chw, std::initializer_list<const void*> ptrs) {
    uintptr_t all = 0;
    for (const void* p : ptrs) all |= (uintptr_t)p;
    return chw % 4 == 0 && (all & 15) == 0;
}

}  // namespace dmme

// ------------------------------------------------------------------ entry points
DMME_API int dmme_distill_noise(const float* x0, const float* z, const int64_t* idx, const int64_t* tt, const float* sqrt_abar, const float* sqrt_1m_abar,
                                int N, int B, int64_t chw, float* z_t, int64_t* t_out, int64_t* m_out, int* status, void* stream) {
    using namespace dmme;
    DMME_REQUIRE(x0 && z && idx && tt && sqrt_abar && sqrt_1m_abar && z_t && t_out && m_out && status, DMME_ERR_INVALID, "distill_noise: null argument");
    DMME_REQUIRE(N >= 1 && B > 0 && chw > 0, DMME_ERR_INVALID, "distill_noise: N = %d, B = %d, chw = %lld", N, B, (long long)chw);
    const int64_t total = (int64_t)B * chw;
    hipStream_t s = (hipStream_t)stream;
    if (quads(chw, {x0, z, z_t}))
        hipLaunchKernelGGL(distill_noise_quad_kernel, dim3(grid_for(total / 4)), dim3(256), 0, s, x0, z, idx, tt, sqrt_abar, sqrt_1m_abar, N, chw / 4, total / 4, z_t,
                           t_out, m_out, status);
    else
        hipLaunchKernelGGL(distill_noise_elem_kernel, dim3(grid_for(total)), dim3(256), 0, s, x0, z, idx, tt, sqrt_abar, sqrt_1m_abar, N, chw, total, z_t, t_out, m_out,
                           status);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

DMME_API int dmme_distill_mid(int pred, int clip, const float* z_t, const float* out1, const float* rows, const int64_t* idx, int N, int B, int64_t chw,
                              float* z_m, void* stream) {
    using namespace dmme;
    DMME_REQUIRE(pred == DMME_PRED_EPS || pred == DMME_PRED_X0 || pred == DMME_PRED_V, DMME_ERR_INVALID, "distill_mid: prediction %d (0: eps, 1: x0, 2: v)", pred);
    DMME_REQUIRE(z_t && out1 && rows && idx && z_m, DMME_ERR_INVALID, "distill_mid: null argument");
    DMME_REQUIRE(N >= 1 && B > 0 && chw > 0, DMME_ERR_INVALID, "distill_mid: N = %d, B = %d, chw = %lld", N, B, (long long)chw);
    const int64_t total = (int64_t)B * chw;
    hipStream_t s = (hipStream_t)stream;
    if (quads(chw, {z_t, out1, z_m}))
        hipLaunchKernelGGL(distill_mid_quad_kernel, dim3(grid_for(total / 4)), dim3(256), 0, s, clip != 0, z_t, out1, rows, idx, N, chw / 4, total / 4, z_m);
    else
        hipLaunchKernelGGL(distill_mid_elem_kernel, dim3(grid_for(total)), dim3(256), 0, s, clip != 0, z_t, out1, rows, idx, N, chw, total, z_m);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

DMME_API int dmme_distill_target(int pred, int clip, const float* z_t, const float* out1, const float* z_m, const float* out2, const float* rows,
                                 const int64_t* idx, int N, int B, int64_t chw, float* target, void* stream) {
    using namespace dmme;
    DMME_REQUIRE(pred == DMME_PRED_EPS || pred == DMME_PRED_X0 || pred == DMME_PRED_V, DMME_ERR_INVALID, "distill_target: prediction %d (0: eps, 1: x0, 2: v)", pred);
    DMME_REQUIRE(z_t && out1 && z_m && out2 && rows && idx && target, DMME_ERR_INVALID, "distill_target: null argument");
    DMME_REQUIRE(N >= 1 && B > 0 && chw > 0, DMME_ERR_INVALID, "distill_target: N = %d, B = %d, chw = %lld", N, B, (long long)chw);
    const int64_t total = (int64_t)B * chw;
    hipStream_t s = (hipStream_t)stream;
    if (quads(chw, {z_t, out1, z_m, out2, target}))
        hipLaunchKernelGGL(distill_target_quad_kernel, dim3(grid_for(total / 4)), dim3(256), 0, s, clip != 0, z_t, out1, z_m, out2, rows, idx, N, chw / 4, total / 4,
                           target);
    else
        hipLaunchKernelGGL(distill_target_elem_kernel, dim3(grid_for(total)), dim3(256), 0, s, clip != 0, z_t, out1, z_m, out2, rows, idx, N, chw, total, target);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}
