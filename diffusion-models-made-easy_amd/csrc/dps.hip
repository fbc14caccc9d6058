// DPS (Chung et al., ICLR 2023, Algorithm 1): DDPM's reverse step followed by a gradient step on ||y - A(x0^(x_t))|| taken through the
// network (dmme_hip.h: dmme_dps_step).  The operator acts on each channel plane, A x = M o (Kh x_c Kw^T) with dense Kh [h][H], Kw [w][W].
// This file holds what is not the network: the measurement, the adjoint kernel that turns (x, eps) into the residual's pull-back
//   x0 = A_t x - B_t e;  T = x0 Kw^T;  Y = Kh T;  r = m ? y - Y : 0;  U = r Kw;  g = Kh^T U;  d_out = B_t g;  sumsq = sum r^2
// and the update  x' = u + (zeta / n_b)(A_t g - dx)  behind dmme_unet_backward_input, which turns d_out into dx = J_eps^T (B_t g).
// The elementwise parts round operation by operation (the translation unit is compiled with -ffp-contract=off, csrc/Makefile, and the
// reverse step carries DDPM's bits); the four products are chains of explicit fmaf in ONE function, dps_dot, that every form calls:
// eager = chain and measure = the adjoint's forward half, bit for bit.
//
// One form: one workgroup per (image, channel) plane, the plane, its intermediates and both tables in LDS.  The last block of the chain
// update advances the chain's loop state (chain_advance); the adjoint kernel only reads it.
#include "common.h"
#include "sampler_dev.h"

namespace dmme {

constexpr int kDpsThreads = 256;
constexpr int kDpsCapacity = 4096;      // H * W of a plane: 64 x 64
constexpr int kDpsLdsMax = 96 * 1024;   // bytes of LDS a workgroup may ask for

struct DpsArgs {
    const float* x;     // the iterate (dmme_dps_measure: the images)
    const float* out;   // network output, out_planes * chw values per image, the eps plane first; null: dmme_dps_measure
    const float* y;     // (B, C, h, w)
    const float* mask;  // (B, C, h, w), 0 or 1; null: everything is measured
    const float* Kh;    // [h][H]
    const float* Kw;    // [w][W]
    float* g;           // (B, C, H, W)
    float* d_out;       // (B, out_planes * C, H, W)
    float* sumsq;       // [B][C]
    float* y_out;       // dmme_dps_measure: (B, C, h, w)
    const float* coef;  // chain form: the table, 8 floats per loop index
    const ChainState* st;  // chain form; null: the eager form, whose row is `row`
    float row[8];
    int C, H, W, h, w, out_planes;
};

// THE dot product of every matrix product here: acc = fma(a[k sa], b[k sb], acc) for k = 0 .. n - 1 in this order from acc = 0.  The
// summation order and the fma are fixed here, once.
__device__ __forceinline__ float dps_dot(const float* __restrict__ a, int sa, const float* __restrict__ b, int sb, int n) {
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc = fmaf(a[k * sa], b[k * sb], acc);
    return acc;
}

// LDS, in floats: P [H][W] (x0, later U [h][W]), T [H][w], R [h][w], Kh [h][H + 1], Kw [w][W + 1] (the odd strides keep lanes that walk
// a table's rows on different banks), 256 partial sums
__host__ __device__ inline int64_t dps_lds_floats(int H, int W, int h, int w) {
    return (int64_t)H * W + (int64_t)H * w + (int64_t)h * w + (int64_t)h * (H + 1) + (int64_t)w * (W + 1) + kDpsThreads;
}

struct DpsLds {
    float *P, *T, *R, *Kh, *Kw, *red;
    int SH, SW;
};
__device__ __forceinline__ DpsLds dps_carve(float* base, int H, int W, int h, int w) {
    DpsLds l;
    l.SH = H + 1, l.SW = W + 1;
    l.P = base;
    l.T = l.P + H * W;
    l.R = l.T + H * w;
    l.Kh = l.R + h * w;
    l.Kw = l.Kh + h * l.SH;
    l.red = l.Kw + w * l.SW;
    return l;
}
__device__ __forceinline__ void dps_load_tables(const DpsArgs& a, const DpsLds& l) {
    const int tid = threadIdx.x, H = a.H, W = a.W;
    for (int idx = tid; idx < a.h * H; idx += kDpsThreads) l.Kh[(idx / H) * l.SH + idx % H] = a.Kh[idx];
    for (int idx = tid; idx < a.w * W; idx += kDpsThreads) l.Kw[(idx / W) * l.SW + idx % W] = a.Kw[idx];
}
// T = P Kw^T, then Y = Kh T for the cell idx (the caller loops and places the barrier between the two)
__device__ __forceinline__ void dps_rows(const DpsArgs& a, const DpsLds& l) {
    const int W = a.W, w = a.w;
    for (int idx = threadIdx.x; idx < a.H * w; idx += kDpsThreads) {
        const int i = idx / w, q = idx - i * w;
        l.T[idx] = dps_dot(l.P + i * W, 1, l.Kw + q * l.SW, 1, W);
    }
}
__device__ __forceinline__ float dps_cell(const DpsArgs& a, const DpsLds& l, int idx) {
    const int w = a.w, p = idx / w, q = idx - p * w;
    return dps_dot(l.Kh + p * l.SH, 1, l.T + q, w, a.H);
}

// ---- the measurement: y_out = M o (Kh x Kw^T), one workgroup per plane
__global__ void __launch_bounds__(kDpsThreads) dps_measure_kernel(DpsArgs a) {
    extern __shared__ float4 dps_lds4[];
    const DpsLds l = dps_carve(reinterpret_cast<float*>(dps_lds4), a.H, a.W, a.h, a.w);
    const int tid = threadIdx.x, hw = a.H * a.W, cells = a.h * a.w;
    const int64_t base = (int64_t)blockIdx.x * hw, cbase = (int64_t)blockIdx.x * cells;
    dps_load_tables(a, l);
    for (int q = tid; q < hw / 4; q += kDpsThreads) *reinterpret_cast<float4*>(l.P + 4 * q) = load4(a.x + base + 4 * q);
    __syncthreads();
    dps_rows(a, l);
    __syncthreads();
    for (int idx = tid; idx < cells; idx += kDpsThreads) {
        const float v = dps_cell(a, l, idx);
        const bool m = a.mask ? a.mask[cbase + idx] != 0.0f : true;
        a.y_out[cbase + idx] = m ? v : 0.0f;
    }
}

// ---- the adjoint kernel: one workgroup per plane; reads the loop state (chain form), never advances it
__global__ void __launch_bounds__(kDpsThreads) dps_adjoint_kernel(DpsArgs a) {
    extern __shared__ float4 dps_lds4[];
    const int H = a.H, W = a.W, h = a.h, w = a.w;
    const DpsLds l = dps_carve(reinterpret_cast<float*>(dps_lds4), H, W, h, w);
    const int tid = threadIdx.x, hw = H * W, cells = h * w, plane = blockIdx.x;
    const int b = plane / a.C, c = plane - b * a.C;
    const float* row = chain_cursor(a.st, a.coef, a.row).row;
    const float At = row[3], Bt = row[4];
    const int64_t base = (int64_t)plane * hw, cbase = (int64_t)plane * cells;
    const int64_t obase = ((int64_t)b * a.out_planes * a.C + c) * hw;  // this plane of the eps half of the network output / of d_out
    dps_load_tables(a, l);
    for (int q = tid; q < hw / 4; q += kDpsThreads) {
        const float4 xv = load4(a.x + base + 4 * q), ev = load4(a.out + obase + 4 * q);
        *reinterpret_cast<float4*>(l.P + 4 * q) = make_float4(__fsub_rn(__fmul_rn(At, xv.x), __fmul_rn(Bt, ev.x)), __fsub_rn(__fmul_rn(At, xv.y), __fmul_rn(Bt, ev.y)),
                                                              __fsub_rn(__fmul_rn(At, xv.z), __fmul_rn(Bt, ev.z)), __fsub_rn(__fmul_rn(At, xv.w), __fmul_rn(Bt, ev.w)));
    }
    __syncthreads();
    dps_rows(a, l);
    __syncthreads();
    float part = 0.f;  // this thread's cells in ascending order, then the fixed tree below: the same bits on every run
    for (int idx = tid; idx < cells; idx += kDpsThreads) {
        const float Y = dps_cell(a, l, idx);
        const bool m = a.mask ? a.mask[cbase + idx] != 0.0f : true;
        const float r = m ? __fsub_rn(a.y[cbase + idx], Y) : 0.0f;  // a select: y is not looked at where the cell is not measured
        l.R[idx] = r;
        part = __fadd_rn(part, __fmul_rn(r, r));
    }
    l.red[tid] = part;
    __syncthreads();
    for (int s = kDpsThreads / 2; s > 0; s >>= 1) {
        if (tid < s) l.red[tid] = __fadd_rn(l.red[tid], l.red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) a.sumsq[plane] = l.red[0];
    // U = R Kw into P's place (x0 is no longer read: every T is behind the barriers above)
    for (int idx = tid; idx < h * W; idx += kDpsThreads) {
        const int p = idx / W, j = idx - p * W;
        l.P[idx] = dps_dot(l.R + p * w, 1, l.Kw + j, l.SW, w);
    }
    __syncthreads();
    // g = Kh^T U, four columns per thread, stored 16 bytes at a time with d_out = B_t g beside it
    for (int q = tid; q < hw / 4; q += kDpsThreads) {
        const int i = (4 * q) / W, j = (4 * q) - i * W;
        float gv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[e] = dps_dot(l.Kh + i, l.SH, l.P + j + e, W, h);
        *reinterpret_cast<float4*>(a.g + base + 4 * q) = make_float4(gv[0], gv[1], gv[2], gv[3]);
        *reinterpret_cast<float4*>(a.d_out + obase + 4 * q) = make_float4(__fmul_rn(Bt, gv[0]), __fmul_rn(Bt, gv[1]), __fmul_rn(Bt, gv[2]), __fmul_rn(Bt, gv[3]));
        if (a.out_planes == 2) *reinterpret_cast<float4*>(a.d_out + obase + (int64_t)a.C * hw + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// ---- the update, elementwise in quads
struct DpsUpdArgs {
    float* x;
    const float* out;
    const float* g;
    const float* dx;
    const float* sumsq;  // [B][C]
    const float* zin;    // [numel] normals: the eager form's z, the chain form's override
    const float* coef;
    const long long* t_table;
    ChainState* st;
    float row[8];
    int C, out_planes;
    int64_t chw, numel, n4;
};

__global__ void __launch_bounds__(kDpsThreads) dps_update_kernel(DpsUpdArgs a) {
    const ChainCursor k = chain_cursor(a.st, a.coef, a.row);
    const float* row = k.row;
    const float c0 = row[0], c1 = row[1], c2 = row[2], At = row[3], zeta = row[5];
    const int64_t q = (int64_t)blockIdx.x * kDpsThreads + threadIdx.x;
    if (q < a.n4) {
        const int64_t e0 = 4 * q, b = e0 / a.chw;
        const float4 xv = load4(a.x + e0), ev = load4(a.out + eps_index(e0, a.chw, a.out_planes));
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, es[4] = {ev.x, ev.y, ev.z, ev.w};
        float u[4], z[4];
        if (c2 != 0.0f) chain_noise4(a.zin, a.numel, a.n4, k.seed, k.off, 0, e0, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u[j] = ddpm_mean(xs[j], es[j], c0, c1);
            if (c2 != 0.0f) u[j] = __fadd_rn(u[j], __fmul_rn(c2, z[j]));
        }
        if (zeta != 0.0f) {  // (zeta == 0: g, dx and sumsq are not read)
            float ss = 0.f;
            for (int c = 0; c < a.C; ++c) ss = __fadd_rn(ss, a.sumsq[b * a.C + c]);  // the image's ||r||^2, in channel order
            const float nb = __fsqrt_rn(ss);
            if (nb != 0.0f) {
                const float sc = __fdiv_rn(zeta, nb);
                const float4 gq = load4(a.g + e0), dq = load4(a.dx + e0);
                const float gs[4] = {gq.x, gq.y, gq.z, gq.w}, ds[4] = {dq.x, dq.y, dq.z, dq.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) u[j] = __fadd_rn(u[j], __fmul_rn(sc, __fsub_rn(__fmul_rn(At, gs[j]), ds[j])));
            }
        }
        *reinterpret_cast<float4*>(a.x + e0) = make_float4(u[0], u[1], u[2], u[3]);
    }
    if (a.st) {
        __syncthreads();
        chain_advance(a.st, a.t_table, k.i, (unsigned long long)a.n4, false);
    }
}

int dps_capacity() { return kDpsCapacity; }

// the checks of the operator's shape every plane-wise entry point makes, and the LDS the launch asks for
static int dps_shape(const char* what, int B, int C, int H, int W, int h, int w, size_t* lds) {
    DMME_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0, DMME_ERR_INVALID, "%s: bad argument (%d images of %d x %d x %d measured at %d x %d)", what, B, C,
                 H, W, h, w);
    DMME_REQUIRE(h <= H && w <= W, DMME_ERR_INVALID, "%s: a measurement of %d x %d is larger than the image's %d x %d (Kh: [h][H], Kw: [w][W], h <= H, w <= W)", what,
                 h, w, H, W);
    DMME_REQUIRE(W % 4 == 0 && ((int64_t)C * H * W) % 4 == 0, DMME_ERR_UNSUPPORTED, "%s: image width %d and image size %lld must be multiples of 4", what, W,
                 (long long)C * H * W);
    const int64_t bytes = dps_lds_floats(H, W, h, w) * (int64_t)sizeof(float);
    DMME_REQUIRE((int64_t)H * W <= kDpsCapacity && bytes <= kDpsLdsMax, DMME_ERR_UNSUPPORTED,
                 "%s: a plane of %d x %d = %lld values measured at %d x %d is beyond the one-workgroup form (dmme_dps_capacity: %d values, %d bytes of LDS with its "
                 "tables; this one needs %lld); a streaming form is not built",
                 what, H, W, (long long)H * W, h, w, kDpsCapacity, kDpsLdsMax, (long long)bytes);
    DMME_REQUIRE((int64_t)B * C < (1ll << 31) && (int64_t)B * C * H * W < (1ll << 40), DMME_ERR_UNSUPPORTED, "%s: %d planes of %d x %d", what, B * C, H, W);
    static bool lds_allowed = false;  // (the first launch is never inside a capture: the chain's trial step, or an eager call)
    if (!lds_allowed) {
        for (const void* k : {reinterpret_cast<const void*>(dps_measure_kernel), reinterpret_cast<const void*>(dps_adjoint_kernel)})
            DMME_CHECK_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kDpsLdsMax));
        lds_allowed = true;
    }
    *lds = (size_t)bytes;
    return DMME_OK;
}

int launch_dps_measure(const float* x, const float* Kh, const float* Kw, const float* mask, float* y_out, int B, int C, int H, int W, int h, int w, hipStream_t s) {
    DMME_REQUIRE(x && Kh && Kw && y_out, DMME_ERR_INVALID, "dps_measure: null argument");
    size_t lds = 0;
    if (int rc = dps_shape("dps_measure", B, C, H, W, h, w, &lds)) return rc;
    DpsArgs a{};
    a.x = x, a.Kh = Kh, a.Kw = Kw, a.mask = mask, a.y_out = y_out, a.C = C, a.H = H, a.W = W, a.h = h, a.w = w, a.out_planes = 1;
    hipLaunchKernelGGL(dps_measure_kernel, dim3((unsigned)(B * C)), dim3(kDpsThreads), lds, s, a);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// row: the eager form's 8 host floats; coef / state: the chain form's (exactly one of the two is given)
int launch_dps_adjoint(const char* what, const float* x, const float* model_out, const float* y, const float* mask, const float* Kh, const float* Kw,
                       const float* row, const float* coef, const void* state, float* g, float* d_out, float* sumsq, int B, int C, int H, int W, int h, int w,
                       int out_planes, hipStream_t s) {
    DMME_REQUIRE(x && model_out && y && Kh && Kw && g && d_out && sumsq, DMME_ERR_INVALID, "%s: null argument", what);
    DMME_REQUIRE(row ? !state : (coef && state), DMME_ERR_INVALID, "%s: null argument", what);
    DMME_REQUIRE(out_planes == 1 || out_planes == 2, DMME_ERR_INVALID, "%s: a network output of %d planes per image (1: eps, 2: eps and v)", what, out_planes);
    size_t lds = 0;
    if (int rc = dps_shape(what, B, C, H, W, h, w, &lds)) return rc;
    DpsArgs a{};
    a.x = x, a.out = model_out, a.y = y, a.mask = mask, a.Kh = Kh, a.Kw = Kw, a.g = g, a.d_out = d_out, a.sumsq = sumsq, a.coef = coef;
    a.st = (const ChainState*)state, a.C = C, a.H = H, a.W = W, a.h = h, a.w = w, a.out_planes = out_planes;
    if (row)
        for (int j = 0; j < 8; ++j) a.row[j] = row[j];
    hipLaunchKernelGGL(dps_adjoint_kernel, dim3((unsigned)(B * C)), dim3(kDpsThreads), lds, s, a);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

int launch_dps_update(const char* what, float* x, const float* model_out, const float* g, const float* dx, const float* sumsq, const float* z, const float* row,
                      const float* coef, const int64_t* t_table, void* state, int B, int C, int H, int W, int out_planes, hipStream_t s) {
    DMME_REQUIRE(x && model_out && B > 0 && C > 0 && H > 0 && W > 0, DMME_ERR_INVALID, "%s: bad argument", what);
    DMME_REQUIRE(row ? !state : (coef && t_table && state), DMME_ERR_INVALID, "%s: null argument", what);
    DMME_REQUIRE(out_planes == 1 || out_planes == 2, DMME_ERR_INVALID, "%s: a network output of %d planes per image (1: eps, 2: eps and v)", what, out_planes);
    DpsUpdArgs a{};
    a.chw = (int64_t)C * H * W, a.numel = a.chw * B, a.n4 = a.numel / 4;
    DMME_REQUIRE(a.chw % 4 == 0, DMME_ERR_UNSUPPORTED, "%s: image size %lld is not a multiple of 4", what, (long long)a.chw);
    const int64_t blocks = (a.n4 + kDpsThreads - 1) / kDpsThreads;
    DMME_REQUIRE(blocks < (1ll << 31), DMME_ERR_UNSUPPORTED, "%s: %lld values", what, (long long)a.numel);
    a.x = x, a.out = model_out, a.g = g, a.dx = dx, a.sumsq = sumsq, a.zin = z, a.coef = coef, a.t_table = (const long long*)t_table, a.st = (ChainState*)state;
    a.C = C, a.out_planes = out_planes;
    if (row) {
        for (int j = 0; j < 8; ++j) a.row[j] = row[j];
        DMME_REQUIRE(z || row[2] == 0.0f, DMME_ERR_INVALID, "%s: a step that adds noise needs z", what);
        DMME_REQUIRE((g && dx && sumsq) || row[5] == 0.0f, DMME_ERR_INVALID, "%s: a step with zeta != 0 needs g, dx and sumsq", what);
    } else {
        DMME_REQUIRE(g && dx && sumsq, DMME_ERR_INVALID, "%s: null argument", what);
    }
    hipLaunchKernelGGL(dps_update_kernel, dim3((unsigned)blocks), dim3(kDpsThreads), 0, s, a);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

}  // namespace dmme

using namespace dmme;

// ------------------------------------------------------------------ entry points
DMME_API int dmme_dps_capacity(void) { return dps_capacity(); }

DMME_API int dmme_dps_measure(const float* x, const float* Kh, const float* Kw, const float* mask, float* y_out, int B, int C, int H, int W, int h, int w,
                              void* stream) {
    return launch_dps_measure(x, Kh, Kw, mask, y_out, B, C, H, W, h, w, (hipStream_t)stream);
}

DMME_API int dmme_dps_adjoint(const float* x, const float* model_out, int out_planes, const float* row, const float* y, const float* mask, const float* Kh,
                              const float* Kw, float* g, float* d_out, float* sumsq, int B, int C, int H, int W, int h, int w, void* stream) {
    DMME_REQUIRE(row, DMME_ERR_INVALID, "dps_adjoint: null argument");
    return launch_dps_adjoint("dps_adjoint", x, model_out, y, mask, Kh, Kw, row, nullptr, nullptr, g, d_out, sumsq, B, C, H, W, h, w, out_planes,
                              (hipStream_t)stream);
}

DMME_API int dmme_chain_adjoint_dps(const float* x, const float* model_out, int out_planes, const float* step_coef, const void* state, const float* y,
                                    const float* mask, const float* Kh, const float* Kw, float* g, float* d_out, float* sumsq, int B, int C, int H, int W, int h,
                                    int w, void* stream) {
    DMME_REQUIRE(step_coef && state, DMME_ERR_INVALID, "chain_adjoint_dps: null argument");
    return launch_dps_adjoint("chain_adjoint_dps", x, model_out, y, mask, Kh, Kw, nullptr, step_coef, state, g, d_out, sumsq, B, C, H, W, h, w, out_planes,
                              (hipStream_t)stream);
}

DMME_API int dmme_dps_step(float* x, const float* model_out, const float* g, const float* dx, const float* sumsq, const float* z, const float* row, int B, int C,
                           int H, int W, int out_planes, void* stream) {
    DMME_REQUIRE(row, DMME_ERR_INVALID, "dps_step: null argument");
    return launch_dps_update("dps_step", x, model_out, g, dx, sumsq, z, row, nullptr, nullptr, nullptr, B, C, H, W, out_planes, (hipStream_t)stream);
}

DMME_API int dmme_chain_update_dps(float* x, const float* model_out, const float* g, const float* dx, const float* sumsq, const float* noise,
                                   const float* step_coef, const int64_t* t_table, void* state, int B, int C, int H, int W, int out_planes, void* stream) {
    DMME_REQUIRE(step_coef && t_table && state, DMME_ERR_INVALID, "chain_update_dps: null argument");
    return launch_dps_update("chain_update_dps", x, model_out, g, dx, sumsq, noise, nullptr, step_coef, t_table, state, B, C, H, W, out_planes,
                             (hipStream_t)stream);
}
