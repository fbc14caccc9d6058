// Analytic-DPM (Bao et al., ICLR 2022; dmme_hip.h: dmme_analytic_*): what the optimal reverse variance of a fixed-variance network needs
// beside the network.  The statistics pass  m_b = mean_j eps_theta[b][j]^2  accumulated per timestep into double tables, and the rows of the
// K-step variational bound of such a network: the Gaussian KL above index 1, the discretised-Gaussian NLL of x_0 at index 1.  Both follow
// iddpm_loss_rows_kernel (kernels_sampler.hip) and the probe dot (pfode.hip): up to 32 workgroups per image leave partial sums in caller
// scratch, one workgroup finishes them in index order in double; no atomics, no workgroup waits for another, equal inputs give equal bits.
// Elements go one by one (any chw).  A value read from device memory is checked before it indexes anything.  The translation unit is
// compiled with -ffp-contract=off (csrc/Makefile): the only fused operations are the explicit fmaf below.
#include "common.h"

namespace dmme {

constexpr int kAnThreads = 256;
constexpr int kAnParts = 32;  // workgroups per image at the most: `scratch` holds B * kAnParts floats at the most

static inline int an_parts(int64_t chw) {
    const int64_t p = (chw + 1023) / 1024;
    return (int)(p > kAnParts ? kAnParts : (p < 1 ? 1 : p));
}

__device__ __forceinline__ double an_partials(const float* __restrict__ partial, int parts, int64_t b) {
    double S = 0.0;
    for (int p = 0; p < parts; ++p) S += (double)partial[b * parts + p];
    return S;
}

// ------------------------------------------------------------------ the moment
// workgroup (b, part): sum of eps^2 over its share of image b, each thread its elements in ascending order by fma from 0
__global__ void __launch_bounds__(kAnThreads) an_moment_partial_kernel(const float* __restrict__ out, int64_t stride, int parts, int64_t chw,
                                                                       float* __restrict__ partial) {
    __shared__ float red[16];
    const int64_t b = blockIdx.x / parts;
    const int part = (int)(blockIdx.x - b * parts);
    const float* ob = out + b * stride;
    float acc = 0.f;
    for (int64_t r = (int64_t)part * kAnThreads + threadIdx.x; r < chw; r += (int64_t)parts * kAnThreads) acc = fmaf(ob[r], ob[r], acc);
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// one workgroup.  256 images at a time: thread k finishes image base + k (the partials in index order, in double, over chw), then thread 0
// walks those images in order and adds each to the tables, so a timestep that occurs twice in a batch has one well-defined result
__global__ void __launch_bounds__(kAnThreads) an_moment_finish_kernel(const float* __restrict__ partial, int parts, const int64_t* __restrict__ t, int T, int B,
                                                                      double chw, double* __restrict__ sum, int64_t* __restrict__ count,
                                                                      float* __restrict__ rows, int* __restrict__ status) {
    __shared__ double m[kAnThreads];
    __shared__ int64_t tt[kAnThreads];
    bool bad = false;
    for (int base = 0; base < B; base += kAnThreads) {
        const int b = base + (int)threadIdx.x;
        if (b < B) {
            const int64_t tb = t[b];
            const bool valid = tb >= 1 && tb <= (int64_t)T;
            const double mb = an_partials(partial, parts, b) / chw;
            m[threadIdx.x] = mb;
            tt[threadIdx.x] = valid ? tb : 0;  // 0: adds nothing
            if (rows) rows[b] = valid ? (float)mb : __int_as_float(0x7fc00000);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = B - base < kAnThreads ? B - base : kAnThreads;
            for (int k = 0; k < n; ++k) {
                const int64_t tb = tt[k];
                if (tb == 0) {
                    bad = true;
                    continue;
                }
                sum[tb] = sum[tb] + m[k];
                count[tb] = count[tb] + 1;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && bad && status) *status = 1;
}

int launch_analytic_moment(const float* out, int64_t stride, const int64_t* t, int T, int B, int64_t chw, double* sum, int64_t* count, float* rows, int* status,
                           float* scratch, hipStream_t s) {
    DMME_REQUIRE(out && t && sum && count && scratch, DMME_ERR_INVALID, "analytic_moment: null argument");
    DMME_REQUIRE(B > 0 && chw > 0 && T >= 1, DMME_ERR_INVALID, "analytic_moment: B = %d images of %lld values, T = %d", B, (long long)chw, T);
    DMME_REQUIRE(stride >= chw, DMME_ERR_INVALID, "analytic_moment: image_stride = %lld below the image's %lld values", (long long)stride, (long long)chw);
    const int parts = an_parts(chw);
    DMME_REQUIRE((int64_t)B * parts <= 0x7fffffff, DMME_ERR_INVALID, "analytic_moment: B = %d is too large", B);
    hipLaunchKernelGGL(an_moment_partial_kernel, dim3((unsigned)(B * parts)), dim3(kAnThreads), 0, s, out, stride, parts, chw, scratch);
    DMME_CHECK_LAUNCH();
    hipLaunchKernelGGL(an_moment_finish_kernel, dim3(1), dim3(kAnThreads), 0, s, (const float*)scratch, parts, t, T, B, (double)chw, sum, count, rows, status);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ the rows of the bound
// coef row i, 8 floats: {k0, k1, log sigma_i^2, log lambda_i^2, sqrt(abar_tau_i), sqrt(1 - abar_tau_i), -, -}
// the discretised-Gaussian NLL of x_0 in bins of +-1/255, open at +-1: the expressions of iddpm_loss_elem's t == 1 branch (kernels_sampler.hip),
// in its order, on this process's mean and standard deviation
__device__ __forceinline__ float an_discrete_nll(float x0, float mean, float sd) {
    const float ap = (x0 + 1.0f / 255.0f - mean) / sd, am = (x0 - 1.0f / 255.0f - mean) / sd;
    const bool up = x0 < 1.0f, lo = x0 > -1.0f;
    const float Fp = up ? 0.5f * (1.0f + erff(ap * 0.70710678118654752f)) : 1.0f;
    const float Fm = lo ? 0.5f * (1.0f + erff(am * 0.70710678118654752f)) : 0.0f;
    return -logf(fmaxf(Fp - Fm, 1e-12f));
}

// workgroup (b, part): idx_b == 1: sum of the NLL terms; idx_b >= 2: sum of (mu~ - mu_theta)^2 = (k1 (eps - eps_theta))^2, eps re-derived from
// x_t and x_0 by dmme_q_sample's own expression (x_t - sqrt(abar) x_0) / sqrt(1 - abar); an index outside [1, S] reads no row and sums nothing
__global__ void __launch_bounds__(kAnThreads) an_vlb_partial_kernel(const float* __restrict__ out, int64_t stride, const float* __restrict__ x_t,
                                                                    const float* __restrict__ x_0, const int64_t* __restrict__ idx,
                                                                    const float* __restrict__ coef, int S, int parts, int64_t chw,
                                                                    float* __restrict__ partial) {
    __shared__ float red[16];
    const int64_t b = blockIdx.x / parts;
    const int part = (int)(blockIdx.x - b * parts);
    const int64_t i = idx[b];
    float acc = 0.f;
    if (i >= 1 && i <= (int64_t)S) {
        const float* c = coef + i * 8;
        const float k0 = c[0], k1 = c[1], sa = c[4], s1 = c[5];
        const float* ob = out + b * stride;
        const float* xt = x_t + b * chw;
        const float* x0 = x_0 + b * chw;
        if (i == 1) {
            const float sd = sqrtf(expf(c[2]));
            for (int64_t r = (int64_t)part * kAnThreads + threadIdx.x; r < chw; r += (int64_t)parts * kAnThreads)
                acc += an_discrete_nll(x0[r], __fadd_rn(__fmul_rn(k0, xt[r]), __fmul_rn(k1, ob[r])), sd);
        } else {
            for (int64_t r = (int64_t)part * kAnThreads + threadIdx.x; r < chw; r += (int64_t)parts * kAnThreads) {
                const float eps = (xt[r] - sa * x0[r]) / s1;
                const float d = k1 * (eps - ob[r]);
                acc = fmaf(d, d, acc);
            }
        }
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// one workgroup; thread b (strided) finishes image b in double: the NLL's mean, or 0.5 (log s2 - log l2 + (l2 + mean d^2) / s2 - 1)
__global__ void __launch_bounds__(kAnThreads) an_vlb_finish_kernel(const float* __restrict__ partial, int parts, const int64_t* __restrict__ idx,
                                                                   const float* __restrict__ coef, int S, int B, double chw, float* __restrict__ rows,
                                                                   int* __restrict__ status) {
    bool bad = false;
    for (int b = threadIdx.x; b < B; b += kAnThreads) {
        const int64_t i = idx[b];
        if (i < 1 || i > (int64_t)S) {
            rows[b] = __int_as_float(0x7fc00000);
            bad = true;
            continue;
        }
        const double mean = an_partials(partial, parts, b) / chw;
        if (i == 1) {
            rows[b] = (float)mean;
        } else {
            const double ls = (double)coef[i * 8 + 2], ll = (double)coef[i * 8 + 3];
            rows[b] = (float)(0.5 * (ls - ll + (exp(ll) + mean) / exp(ls) - 1.0));
        }
    }
    if (bad && status) *status = 1;
}

int launch_analytic_vlb_rows(const float* out, int64_t stride, const float* x_t, const float* x_0, const int64_t* idx, const float* coef, int S, int B, int64_t chw,
                             float* rows, int* status, float* scratch, hipStream_t s) {
    DMME_REQUIRE(out && x_t && x_0 && idx && coef && rows && scratch, DMME_ERR_INVALID, "analytic_vlb_rows: null argument");
    DMME_REQUIRE(B > 0 && chw > 0 && S >= 1, DMME_ERR_INVALID, "analytic_vlb_rows: B = %d images of %lld values, S = %d", B, (long long)chw, S);
    DMME_REQUIRE(stride >= chw, DMME_ERR_INVALID, "analytic_vlb_rows: image_stride = %lld below the image's %lld values", (long long)stride, (long long)chw);
    const int parts = an_parts(chw);
    DMME_REQUIRE((int64_t)B * parts <= 0x7fffffff, DMME_ERR_INVALID, "analytic_vlb_rows: B = %d is too large", B);
    hipLaunchKernelGGL(an_vlb_partial_kernel, dim3((unsigned)(B * parts)), dim3(kAnThreads), 0, s, out, stride, x_t, x_0, idx, coef, S, parts, chw, scratch);
    DMME_CHECK_LAUNCH();
    hipLaunchKernelGGL(an_vlb_finish_kernel, dim3(1), dim3(kAnThreads), 0, s, (const float*)scratch, parts, idx, coef, S, B, (double)chw, rows, status);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

}  // namespace dmme

using namespace dmme;

// ------------------------------------------------------------------ entry points
DMME_API int dmme_analytic_moment(const float* model_out, int64_t image_stride, const int64_t* t, int T, int B, int64_t chw, double* sum, int64_t* count,
                                  float* rows, int* status, float* scratch, void* stream) {
    return launch_analytic_moment(model_out, image_stride, t, T, B, chw, sum, count, rows, status, scratch, (hipStream_t)stream);
}

DMME_API int dmme_analytic_vlb_rows(const float* model_out, int64_t image_stride, const float* x_t, const float* x_0, const int64_t* idx, const float* coef, int S,
                                    int B, int64_t chw, float* rows, int* status, float* scratch, void* stream) {
    return launch_analytic_vlb_rows(model_out, image_stride, x_t, x_0, idx, coef, S, B, chw, rows, status, scratch, (hipStream_t)stream);
}
