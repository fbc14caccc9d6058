// Classifier guidance (Dhariwal & Nichol 2021, "Diffusion Models Beat GANs", Algorithms 1 and 2): the head of the noise-aware
// classifier (DMME_ARCH_CLASSIFIER: GroupNorm -> SiLU -> mean over H x W -> Linear) forward and backward, and the row-wise
// log-softmax that turns its logits into the training loss or the guidance gradient d sum_i log p(y_i | x_i, t) / d logits.
//
// The head reads the top activation of the plan (middle_layers' output, NHWC in the compute dtype).  That map is small (4 x 4 at
// 32 x 32 inputs): one workgroup per image holds every channel of it, so statistics, activation, pooling and the C_top x K GEMV are
// one launch; the backward recomputes the statistics the same way (bit-identical to the forward's) instead of keeping them.
#include "common.h"

namespace dmme {

constexpr int kHeadMaxC = 1024;  // channels of the top map one workgroup holds in LDS (plan_create refuses wider heads)

// wave-wide sum / max: DPP inside each 16-lane row, then the gfx950 row and half-wave swaps (common.h); every lane gets the result
__device__ __forceinline__ float wave_sum_x(float v) {
    v = half_sum(v);
    float a = v, b = v;
    permlane32_swap(a, b);
    return a + b;
}
__device__ __forceinline__ float wave_max_x(float v) {
    v = fmaxf(v, DMME_DPP_F(v, 0xB1));
    v = fmaxf(v, DMME_DPP_F(v, 0x4E));
    v = fmaxf(v, DMME_DPP_F(v, 0x141));
    v = fmaxf(v, DMME_DPP_F(v, 0x140));
    float a = v, b = v;
    permlane16_swap(a, b);
    v = fmaxf(a, b);
    a = v;
    b = v;
    permlane32_swap(a, b);
    return fmaxf(a, b);
}

__device__ __forceinline__ float sigmoid_acc(float y) { return 1.0f / (1.0f + expf(-y)); }

// GroupNorm statistics of one image of the top map (two passes: mean, then the mean squared deviation), eps 1e-5 as nn.GroupNorm.
// s_tmp: C floats of scratch; s_mean / s_rstd: G floats.
template <typename T>
__device__ void head_stats(const T* __restrict__ x, int HW, int C, int G, float* s_tmp, float* s_mean, float* s_rstd) {
    const int cg = C / G;
    const float inv = 1.0f / (float)(cg * HW);
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float s = 0.f;
        for (int p = 0; p < HW; ++p) s += to_f(x[(int64_t)p * C + c]);
        s_tmp[c] = s;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        float s = 0.f;
        for (int j = 0; j < cg; ++j) s += s_tmp[g * cg + j];
        s_mean[g] = s * inv;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float m = s_mean[c / cg];
        float s = 0.f;
        for (int p = 0; p < HW; ++p) {
            const float d = to_f(x[(int64_t)p * C + c]) - m;
            s += d * d;
        }
        s_tmp[c] = s;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        float s = 0.f;
        for (int j = 0; j < cg; ++j) s += s_tmp[g * cg + j];
        s_rstd[g] = 1.0f / sqrtf(s * inv + 1e-5f);
    }
    __syncthreads();
}

// logits[b][k] = bias[k] + sum_c W[k][c] * mean_p silu(GN(x)[p][c]);  grid B, block 256
template <typename T>
__global__ void __launch_bounds__(256) cls_head_fwd_kernel(const T* __restrict__ top, int HW, int C, int G, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ W, const float* __restrict__ bias,
                                                           int K, float* __restrict__ logits) {
    __shared__ float s_tmp[kHeadMaxC], s_pool[kHeadMaxC], s_mean[kHeadMaxC], s_rstd[kHeadMaxC];
    const int b = blockIdx.x;
    const T* x = top + (int64_t)b * HW * C;
    head_stats(x, HW, C, G, s_tmp, s_mean, s_rstd);
    const int cg = C / G;
    const float inv_hw = 1.0f / (float)HW;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float m = s_mean[c / cg], r = s_rstd[c / cg], ga = gamma[c], be = beta[c];
        float s = 0.f;
        for (int p = 0; p < HW; ++p) {
            const float y = (to_f(x[(int64_t)p * C + c]) - m) * r * ga + be;
            s += y * sigmoid_acc(y);
        }
        s_pool[c] = s * inv_hw;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int k = wv; k < K; k += nw) {  // (wave-uniform loop: every lane reaches the reduction)
        const float* wr = W + (int64_t)k * C;
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc += wr[c] * s_pool[c];
        acc = wave_sum_x(acc);
        if (lane == 0) logits[(int64_t)b * K + k] = acc + bias[k];
    }
}

// From d logits: d pooled = dlog W / HW (spatially constant), through SiLU and GroupNorm into d top (written, not accumulated).
// pooled (nullable): the forward's pooled activations [B][C]; rows (nullable): per-image d beta / d gamma [B][2][C].  grid B, block 256
template <typename T>
__global__ void __launch_bounds__(256) cls_head_bwd_kernel(const T* __restrict__ top, int HW, int C, int G, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ W, int K,
                                                           const float* __restrict__ dlog, T* __restrict__ dtop, float* __restrict__ pooled,
                                                           float* __restrict__ rows) {
    __shared__ float s_tmp[kHeadMaxC], s_mean[kHeadMaxC], s_rstd[kHeadMaxC], s_dp[kHeadMaxC], s_g2[kHeadMaxC], s_m1[kHeadMaxC], s_m2[kHeadMaxC];
    __shared__ float s_dl[256];
    const int b = blockIdx.x;
    const T* x = top + (int64_t)b * HW * C;
    head_stats(x, HW, C, G, s_tmp, s_mean, s_rstd);
    const int cg = C / G;
    const float inv_hw = 1.0f / (float)HW;
    for (int c = threadIdx.x; c < C; c += blockDim.x) s_dp[c] = 0.f;
    __syncthreads();
    // d pooled[c] = sum_k dlog[b][k] W[k][c], K in chunks of 256 staged in LDS
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int kn = K - k0 < 256 ? K - k0 : 256;
        if ((int)threadIdx.x < kn) s_dl[threadIdx.x] = dlog[(int64_t)b * K + k0 + threadIdx.x];
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            float s = s_dp[c];
            for (int k = 0; k < kn; ++k) s += s_dl[k] * W[(int64_t)(k0 + k) * C + c];
            s_dp[c] = s;
        }
        __syncthreads();
    }
    // per channel: d silu, d beta = sum_p ds, d gamma = sum_p ds xhat; the GroupNorm backward's two sums (s_tmp, s_g2) of dxhat = ds gamma
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float m = s_mean[c / cg], r = s_rstd[c / cg], ga = gamma[c], be = beta[c];
        const float gy = s_dp[c] * inv_hw;
        float sd = 0.f, sdx = 0.f, sp = 0.f;
        for (int p = 0; p < HW; ++p) {
            const float xh = (to_f(x[(int64_t)p * C + c]) - m) * r;
            const float y = xh * ga + be;
            const float sg = sigmoid_acc(y);
            sp += y * sg;
            const float ds = gy * sg * (1.0f + y * (1.0f - sg));  // d silu(y) / dy
            sd += ds;
            sdx += ds * xh;
        }
        if (pooled) pooled[(int64_t)b * C + c] = sp * inv_hw;
        if (rows) {
            rows[(int64_t)b * 2 * C + c] = sd;       // d beta
            rows[(int64_t)b * 2 * C + C + c] = sdx;  // d gamma
        }
        s_tmp[c] = sd * ga;
        s_g2[c] = sdx * ga;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        float a = 0.f, q = 0.f;
        for (int j = 0; j < cg; ++j) {
            a += s_tmp[g * cg + j];
            q += s_g2[g * cg + j];
        }
        s_m1[g] = a / (float)(cg * HW);
        s_m2[g] = q / (float)(cg * HW);
    }
    __syncthreads();
    // dx = rstd (dxhat - mean_group(dxhat) - xhat mean_group(dxhat xhat))
    T* dx = dtop + (int64_t)b * HW * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const int g = c / cg;
        const float m = s_mean[g], r = s_rstd[g], ga = gamma[c], be = beta[c], m1 = s_m1[g], m2 = s_m2[g];
        const float gy = s_dp[c] * inv_hw;
        for (int p = 0; p < HW; ++p) {
            const float xh = (to_f(x[(int64_t)p * C + c]) - m) * r;
            const float y = xh * ga + be;
            const float sg = sigmoid_acc(y);
            const float dxh = gy * sg * (1.0f + y * (1.0f - sg)) * ga;
            dx[(int64_t)p * C + c] = from_f<T>(r * (dxh - m1 - xh * m2));
        }
    }
}

// dW[k][c] += sum_b dlog[b][k] pooled[b][c];  db[k] += sum_b dlog[b][k];  dbeta / dgamma[c] += sum_b rows (fixed order: deterministic)
__global__ void __launch_bounds__(256) cls_head_wgrad_kernel(const float* __restrict__ dlog, const float* __restrict__ pooled,
                                                             const float* __restrict__ rows, int B, int K, int C, float* __restrict__ dW,
                                                             float* __restrict__ db, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int64_t n = (int64_t)K * C + K + 2 * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        if (i < (int64_t)K * C) {
            const int k = (int)(i / C), c = (int)(i - (int64_t)k * C);
            for (int b = 0; b < B; ++b) s += dlog[(int64_t)b * K + k] * pooled[(int64_t)b * C + c];
            dW[i] += s;
        } else if (i < (int64_t)K * C + K) {
            const int k = (int)(i - (int64_t)K * C);
            for (int b = 0; b < B; ++b) s += dlog[(int64_t)b * K + k];
            db[k] += s;
        } else {
            const int j = (int)(i - (int64_t)K * C - K);  // [0, C): beta, [C, 2C): gamma
            const int c = j < C ? j : j - C;
            for (int b = 0; b < B; ++b) s += rows[(int64_t)b * 2 * C + j];
            if (j < C)
                dbeta[c] += s;
            else
                dgamma[c] += s;
        }
    }
}

// one workgroup of four waves; wave w takes rows w, w + 4, ...  (mode 0: training, 1: guidance; include/dmme_hip.h)
__global__ void __launch_bounds__(256) log_softmax_grad_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y, int B, int K, int mode,
                                                               float scale, float* __restrict__ loss, float* __restrict__ dlog, int* status) {
    __shared__ float s_part[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc = 0.f;  // this wave's rows, in row order
    for (int r = wv; r < B; r += 4) {
        const float* l = logits + (int64_t)r * K;
        const int64_t lab = y[r];
        const bool ok = lab >= 0 && lab < K;
        float mx = -INFINITY;
        for (int k = lane; k < K; k += 64) mx = fmaxf(mx, l[k]);
        mx = wave_max_x(mx);
        float se = 0.f;
        for (int k = lane; k < K; k += 64) se += expf(l[k] - mx);
        se = wave_sum_x(se);
        const float lse = mx + logf(se);
        if (!ok) {
            if (lane == 0 && status) atomicExch(status, 1);
            if (dlog)
                for (int k = lane; k < K; k += 64) dlog[(int64_t)r * K + k] = NAN;
            acc += NAN;
            continue;
        }
        const float lp = l[lab] - lse;
        acc += mode == 0 ? -lp : lp;
        if (dlog)
            for (int k = lane; k < K; k += 64) {
                const float p = expf(l[k] - lse), oh = k == lab ? 1.f : 0.f;
                dlog[(int64_t)r * K + k] = mode == 0 ? scale * (p - oh) / (float)B : scale * (oh - p);
            }
    }
    if (lane == 0) s_part[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && loss) {
        const float tot = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
        loss[0] = mode == 0 ? tot / (float)B : tot;
    }
}

int launch_cls_head_fwd(int dtype, const void* top, int B, int HW, int C, int G, const float* gamma, const float* beta, const float* W,
                        const float* bias, int K, float* logits, hipStream_t s) {
    DMME_REQUIRE(C > 0 && C <= kHeadMaxC && G > 0 && C % G == 0 && K > 0 && HW > 0, DMME_ERR_UNSUPPORTED, "classifier head: C=%d G=%d K=%d", C, G, K);
    if (dtype == DMME_BF16)
        hipLaunchKernelGGL(cls_head_fwd_kernel<bf16>, dim3(B), dim3(256), 0, s, (const bf16*)top, HW, C, G, gamma, beta, W, bias, K, logits);
    else if (dtype == DMME_F16)
        hipLaunchKernelGGL(cls_head_fwd_kernel<f16>, dim3(B), dim3(256), 0, s, (const f16*)top, HW, C, G, gamma, beta, W, bias, K, logits);
    else
        hipLaunchKernelGGL(cls_head_fwd_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)top, HW, C, G, gamma, beta, W, bias, K, logits);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

int launch_cls_head_bwd(int dtype, const void* top, int B, int HW, int C, int G, const float* gamma, const float* beta, const float* W, int K,
                        const float* dlog, void* dtop, float* pooled, float* rows, hipStream_t s) {
    DMME_REQUIRE(C > 0 && C <= kHeadMaxC && G > 0 && C % G == 0 && K > 0 && HW > 0, DMME_ERR_UNSUPPORTED, "classifier head: C=%d G=%d K=%d", C, G, K);
    if (dtype == DMME_BF16)
        hipLaunchKernelGGL(cls_head_bwd_kernel<bf16>, dim3(B), dim3(256), 0, s, (const bf16*)top, HW, C, G, gamma, beta, W, K, dlog, (bf16*)dtop, pooled, rows);
    else if (dtype == DMME_F16)
        hipLaunchKernelGGL(cls_head_bwd_kernel<f16>, dim3(B), dim3(256), 0, s, (const f16*)top, HW, C, G, gamma, beta, W, K, dlog, (f16*)dtop, pooled, rows);
    else
        hipLaunchKernelGGL(cls_head_bwd_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)top, HW, C, G, gamma, beta, W, K, dlog, (float*)dtop, pooled,
                           rows);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

int launch_cls_head_wgrad(const float* dlog, const float* pooled, const float* rows, int B, int K, int C, float* dW, float* db, float* dgamma,
                          float* dbeta, hipStream_t s) {
    const int64_t n = (int64_t)K * C + K + 2 * C;
    hipLaunchKernelGGL(cls_head_wgrad_kernel, dim3((unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, s, dlog, pooled, rows, B, K, C, dW, db, dgamma, dbeta);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

int launch_log_softmax_grad(const float* logits, const int64_t* y, int B, int K, int mode, float scale, float* loss, float* dlog, int* status,
                            hipStream_t s) {
    DMME_REQUIRE(logits && y && B > 0 && K > 0 && (mode == 0 || mode == 1), DMME_ERR_INVALID, "log_softmax_grad: bad argument (B=%d K=%d mode=%d)", B, K, mode);
    hipLaunchKernelGGL(log_softmax_grad_kernel, dim3(1), dim3(256), 0, s, logits, y, B, K, mode, scale, loss, dlog, status);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

}  // namespace dmme
