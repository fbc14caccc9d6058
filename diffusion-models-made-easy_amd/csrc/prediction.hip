// Networks that predict x0 or v (Salimans & Ho 2022) instead of the noise: the adapter that turns their output into an eps prediction in
// front of today's sampler updates, the training targets of the three parameterisations, and the per-timestep weighted MSE loss
// (min-SNR-gamma, Hang et al. 2023).  All HBM-bound, fp32, NCHW.  Like kernels_sampler.hip the translation unit is compiled with
// -ffp-contract=off (csrc/Makefile) and every product, sum and difference below is explicitly rounded on its own (never an fma): the
// x_t / eps target of q_sample_pred_kernel carry dmme_q_sample's bits, and a numpy float32 restatement reproduces the rest bit for bit.
#include "plan.h"

namespace dmme {

static inline unsigned grid_for(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// ------------------------------------------------------------------ network output -> eps
// e = (a[t_b] * out) + (b[t_b] * x), in place on out; ab: [T+1][2].  A timestep outside 0..T is never used as an index: its rows come
// out NaN.  t_len == 1: every image reads t[0] (a chain's loop state), else image b reads t[b].
__device__ __forceinline__ float2 pred_row(const float* __restrict__ ab, int T, const int64_t* __restrict__ t, int t_len, int64_t b) {
    const int64_t tn = t[t_len == 1 ? 0 : b];
    if (tn < 0 || tn > T) return make_float2(__builtin_nanf(""), __builtin_nanf(""));
    return make_float2(ab[2 * tn], ab[2 * tn + 1]);
}
__device__ __forceinline__ float pred_eps(float2 r, float o, float x) { return __fadd_rn(__fmul_rn(r.x, o), __fmul_rn(r.y, x)); }

// chw % 4 == 0 and 16-byte aligned pointers: a quad never straddles two images
__global__ void __launch_bounds__(256) pred_to_eps_quad_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ ab, int T,
                                                               const int64_t* __restrict__ t, int t_len, int64_t chw4, int64_t total4) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total4; q += (int64_t)gridDim.x * blockDim.x) {
        const float2 r = pred_row(ab, T, t, t_len, q / chw4);
        const float4 o = reinterpret_cast<const float4*>(out)[q], v = reinterpret_cast<const float4*>(x)[q];
        reinterpret_cast<float4*>(out)[q] = make_float4(pred_eps(r, o.x, v.x), pred_eps(r, o.y, v.y), pred_eps(r, o.z, v.z), pred_eps(r, o.w, v.w));
    }
}
// ragged sizes (the eager sampler kinds accept them): element by element
__global__ void __launch_bounds__(256) pred_to_eps_elem_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ ab, int T,
                                                               const int64_t* __restrict__ t, int t_len, int64_t chw, int64_t total) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = pred_eps(pred_row(ab, T, t, t_len, i / chw), out[i], x[i]);
}

int launch_pred_to_eps(int pred, float* model_out, const float* x, const float* ab, int T, const int64_t* t, int t_len, int B, int64_t chw,
                       hipStream_t s) {
    DMME_REQUIRE(pred == DMME_PRED_X0 || pred == DMME_PRED_V, DMME_ERR_INVALID,
                 "pred_to_eps: prediction %d (1: x0, 2: v; an eps network's output needs no conversion: do not launch)", pred);
    DMME_REQUIRE(model_out && x && ab && t && T > 0 && B > 0 && chw > 0, DMME_ERR_INVALID, "pred_to_eps: bad argument");
    DMME_REQUIRE(t_len == 1 || t_len == B, DMME_ERR_INVALID, "pred_to_eps: timestep tensor of length %d does not broadcast against batch %d", t_len, B);
    const int64_t total = (int64_t)B * chw;
    if (chw % 4 == 0 && (((uintptr_t)model_out | (uintptr_t)x) & 15) == 0)
        hipLaunchKernelGGL(pred_to_eps_quad_kernel, dim3(grid_for(total / 4)), dim3(256), 0, s, model_out, x, ab, T, t, t_len, chw / 4, total / 4);
    else
        hipLaunchKernelGGL(pred_to_eps_elem_kernel, dim3(grid_for(total)), dim3(256), 0, s, model_out, x, ab, T, t, t_len, chw, total);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ forward noising with the target of a parameterisation
// x_t and the eps target: q_sample_kernel's expressions (kernels_sampler.hip), the same bits
__global__ void __launch_bounds__(256) q_sample_pred_kernel(int pred, const float* __restrict__ x0, const float* __restrict__ z,
                                                            const float* __restrict__ sqrt_abar, const float* __restrict__ sqrt_1m_abar,
                                                            const int64_t* __restrict__ t, int64_t chw, int64_t total, float* __restrict__ x_t,
                                                            float* __restrict__ target) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t tn = t[i / chw];
        const float sa = sqrt_abar[tn], sd = sqrt_1m_abar[tn];
        const float x = x0[i], n = z[i];
        const float mean = __fmul_rn(sa, x);
        const float xt = __fadd_rn(mean, __fmul_rn(sd, n));
        x_t[i] = xt;
        if (target) {
            if (pred == DMME_PRED_X0)
                target[i] = x;
            else if (pred == DMME_PRED_V)
                target[i] = __fsub_rn(__fmul_rn(sa, n), __fmul_rn(sd, x));  // (the injected noise, not the re-derived one)
            else
                target[i] = __fdiv_rn(__fsub_rn(xt, mean), sd);
        }
    }
}

int launch_q_sample_pred(int pred, const float* x0, const float* z, const float* sqrt_abar, const float* sqrt_1m_abar, const int64_t* t, int B,
                         int64_t chw, float* x_t, float* target, hipStream_t s) {
    const int64_t total = (int64_t)B * chw;
    hipLaunchKernelGGL(q_sample_pred_kernel, dim3(grid_for(total)), dim3(256), 0, s, pred, x0, z, sqrt_abar, sqrt_1m_abar, t, chw, total, x_t, target);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ MSE loss with a weight per timestep (+ gradient)
// Reduced like mse_partial_kernel / mse_final_kernel, with the blocks laid out per image: block (p, b) sums its share of image b's squared
// differences and weighs the sum once with w[t_b]; the gradient's row scalar 2 w[t_b] grad_scale / numel is formed once per thread, in
// double, and rounded once.
constexpr int kMseRowParts = 64;  // blocks per image at the most: scratch holds B * kMseRowParts floats
static inline int mse_row_parts(int64_t chw) {
    const int64_t p = (chw + 1023) / 1024;
    return (int)(p > kMseRowParts ? kMseRowParts : p);
}

__global__ void __launch_bounds__(256) mse_rows_partial_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                               const float* __restrict__ w_table, const int64_t* __restrict__ t, int64_t chw,
                                                               float* __restrict__ d_out, double gscale_over_numel, float* __restrict__ partial) {
    __shared__ float red[16];
    const int b = blockIdx.y;
    const float w = w_table[t[b]];
    const float g = (float)(2.0 * (double)w * gscale_over_numel);
    const float* o = out + (int64_t)b * chw;
    const float* tg = target + (int64_t)b * chw;
    float* d = d_out ? d_out + (int64_t)b * chw : nullptr;
    float acc = 0.f;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < chw; j += (int64_t)gridDim.x * blockDim.x) {
        const float diff = __fsub_rn(o[j], tg[j]);
        acc += diff * diff;
        if (d) d[j] = __fmul_rn(diff, g);
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = tot * w;
}
__global__ void __launch_bounds__(256) mse_rows_final_kernel(const float* partial, int n, float inv_numel, float* loss) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partial[i];
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = tot * inv_numel;
}

int launch_mse_rows(const float* out, const float* target, const float* w_table, const int64_t* t, int B, int64_t chw, float* loss, float* d_out,
                    float gscale, float* scratch, hipStream_t s) {
    DMME_REQUIRE(B > 0 && B <= 65535 && chw > 0, DMME_ERR_INVALID, "mse_loss_rows: B = %d (1..65535), chw = %lld", B, (long long)chw);
    const int parts = mse_row_parts(chw);
    const double numel = (double)B * (double)chw;
    hipLaunchKernelGGL(mse_rows_partial_kernel, dim3(parts, B), dim3(256), 0, s, out, target, w_table, t, chw, d_out, (double)gscale / numel, scratch);
    DMME_CHECK_LAUNCH();
    hipLaunchKernelGGL(mse_rows_final_kernel, dim3(1), dim3(256), 0, s, scratch, parts * B, (float)(1.0 / numel), loss);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

}  // namespace dmme

// ------------------------------------------------------------------ entry points
DMME_API int dmme_pred_to_eps(int pred, float* model_out, const float* x, const float* ab, int T, const int64_t* t, int t_len, int B, int64_t chw,
                              void* stream) {
    return launch_pred_to_eps(pred, model_out, x, ab, T, t, t_len, B, chw, (hipStream_t)stream);
}

DMME_API int dmme_unet_plan_set_prediction(dmme_plan* plan, int pred, const float* ab, int T) {
    DMME_REQUIRE(plan, DMME_ERR_INVALID, "plan_set_prediction: null plan");
    DMME_REQUIRE(pred == DMME_PRED_EPS || pred == DMME_PRED_X0 || pred == DMME_PRED_V, DMME_ERR_INVALID, "plan_set_prediction: prediction %d (0: eps, 1: x0, 2: v)",
                 pred);
    if (pred == DMME_PRED_EPS) {
        plan->pred = DMME_PRED_EPS;
        plan->pred_ab = nullptr;
        plan->pred_T = 0;
        return DMME_OK;
    }
    DMME_REQUIRE(ab && T > 0, DMME_ERR_INVALID, "plan_set_prediction: an x0 / v network needs its [T+1][2] table");
    DMME_REQUIRE(plan->cfg.arch != DMME_ARCH_CLASSIFIER && plan->out_channels == plan->cfg.in_channels, DMME_ERR_UNSUPPORTED,
                 "plan_set_prediction: an x0 / v network has one output plane (%d output channels for %d input channels)", plan->out_channels,
                 plan->cfg.in_channels);
    DMME_REQUIRE(((int64_t)plan->cfg.in_channels * plan->H * plan->W) % 4 == 0, DMME_ERR_INVALID, "plan_set_prediction: C*H*W must be a multiple of 4");
    plan->pred = pred;
    plan->pred_ab = ab;
    plan->pred_T = T;
    return DMME_OK;
}

DMME_API int dmme_q_sample_pred(int pred, const float* x0, const float* z, const float* sqrt_abar, const float* sqrt_1m_abar, const int64_t* t, int B,
                                int64_t chw, float* x_t, float* target, void* stream) {
    DMME_REQUIRE(pred == DMME_PRED_EPS || pred == DMME_PRED_X0 || pred == DMME_PRED_V, DMME_ERR_INVALID, "q_sample_pred: prediction %d (0: eps, 1: x0, 2: v)", pred);
    DMME_REQUIRE(x0 && z && sqrt_abar && sqrt_1m_abar && t && x_t && B > 0 && chw > 0, DMME_ERR_INVALID, "q_sample_pred: bad argument");
    return launch_q_sample_pred(pred, x0, z, sqrt_abar, sqrt_1m_abar, t, B, chw, x_t, target, (hipStream_t)stream);
}

DMME_API int dmme_mse_loss_rows(const float* out, const float* target, const float* w_table, const int64_t* t, int B, int64_t chw, float* loss,
                                float* d_out, float grad_scale, float* scratch, void* stream) {
    DMME_REQUIRE(out && target && w_table && t && loss && scratch, DMME_ERR_INVALID, "mse_loss_rows: null argument");
    return launch_mse_rows(out, target, w_table, t, B, chw, loss, d_out, grad_scale, scratch, (hipStream_t)stream);
}
