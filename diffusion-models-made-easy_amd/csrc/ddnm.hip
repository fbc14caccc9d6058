// DDNM (Wang, Yu, Zhang 2023): every x0 prediction has its range-space part rectified against a measurement y = A x (dmme_hip.h:
// dmme_ddnm_step), for the operator family A = M o Pool_s o Gray_g whose pseudo-inverse replicates a cell's value over the cell:
//   x0 = (A_t x) - (B_t e);   r = m (mean_cell(x0) - y);   xh = x0 - lambda r;   u = ca xh [+ cb x] [+ cz z0];   x' = u, or r0 u + r1 z1.
// A cell is the n = (C if gray else 1) s s image elements one measurement value averages, so the update is neither elementwise nor
// plane-wise: it reduces over cells that span channels and s x s pixel blocks.  Every operation is rounded on its own (the translation
// unit is compiled with -ffp-contract=off, csrc/Makefile); a cell's mean is formed by ONE function, ddnm_cell_mean, that the measurement
// entry point and both update forms call: eager = chain = dmme_ddnm_measure bit for bit, whatever the batch and the image's place in it.
//
// Two forms.  Quad (n == 1: plain inpainting): elementwise, a thread per aligned quad, no LDS, no barrier.  Band (every other case): a
// workgroup owns one image's band of s rows across all C channels, stages x0 in LDS cell-minor ([element of the cell][cell], so that the
// threads that sum neighbouring cells read neighbouring banks), reduces one cell per thread, and after the barrier reads x again and
// writes x'.  The block that takes the last ticket advances the chain's loop state (chain_advance).
#include "common.h"
#include "sampler_dev.h"

namespace dmme {

constexpr int kDdnmThreads = 256;
constexpr int kDdnmBandCapacity = 36864;            // values C * s * W of one band the band form stages (144 KiB of the CU's 160, as threshold.hip)
constexpr int kDdnmLdsBytes = 160 * 1024 - 1024;    // ... and what a workgroup may ask for in all: the staged band, its padding, one residual per cell

struct DdnmArgs {
    float* x;           // updated in place (dmme_ddnm_measure: null)
    const float* src;   // dmme_ddnm_measure only: the images to measure
    const float* out;   // network output, out_planes * chw values per image, the eps plane first
    const float* y;     // the measurement, (B, Cm, h, w)
    const float* mask;  // (B, Cm, h, w), 1 = measured; dmme_ddnm_measure: nullable (everything is measured)
    float* y_out;       // dmme_ddnm_measure only
    const float* zin;   // [2][numel] normals: the eager form's, or the chain form's override
    const float* coef;  // chain form: the table, 8 floats per loop index
    const long long* t_table;
    ChainState* st;     // chain form; null: the eager form, whose row is `row`
    float row[8];
    int C, H, W, s, gray, out_planes;
    int cells, n, stride;   // band form: cells of a band, elements of a cell, the LDS stride between two elements of a cell (cells, padded to odd)
    int64_t hw, chw, numel, n4;
};

struct DdnmRow {
    float ca, cb, cz, A, B, lam, r0, r1;
    long long i;
    unsigned long long seed, off;
};

// the step's row (chain_cursor: called at the top of each kernel)
__device__ __forceinline__ DdnmRow ddnm_row(const DdnmArgs& a) {
    const ChainCursor k = chain_cursor(a.st, a.coef, a.row);
    const float* c = k.row;
    DdnmRow r;
    r.i = k.i, r.seed = k.seed, r.off = k.off;
    r.ca = c[0], r.cb = c[1], r.cz = c[2], r.A = c[3], r.B = c[4], r.lam = c[5], r.r0 = c[6], r.r1 = c[7];
    return r;
}

// THE mean of a cell: its n elements at p[0], p[stride], ... summed in this order from the first one, every sum rounded, one correctly
// rounded division.  The order of a cell's elements is (channel,) row, column.
__device__ __forceinline__ float ddnm_cell_mean(const float* p, int n, int stride) {
    float acc = p[0];
    for (int k = 1; k < n; ++k) acc = __fadd_rn(acc, p[(int64_t)k * stride]);
    return __fdiv_rn(acc, (float)n);
}

// x0 as threshold.hip's thr_x0 rounds it
__device__ __forceinline__ float ddnm_x0(const DdnmRow& r, float x, float e) { return __fsub_rn(__fmul_rn(r.A, x), __fmul_rn(r.B, e)); }

// the residual of a cell: zero where it is not measured, and y is not looked at there
__device__ __forceinline__ float ddnm_residual(float mean, float m, const float* y) { return m != 0.0f ? __fsub_rn(mean, *y) : 0.0f; }

// the elementwise tail for the quad at element g, from x, x0 and the residual of each element's cell; a stream whose coefficient is
// zero is neither drawn nor read
__device__ __forceinline__ void ddnm_finish(const DdnmArgs& a, const DdnmRow& r, int64_t g, const float (&xs)[4], const float (&x0)[4], const float (&res)[4]) {
    float u[4], z[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xh = __fsub_rn(x0[j], __fmul_rn(r.lam, res[j]));
        u[j] = __fmul_rn(r.ca, xh);
        if (r.cb != 0.0f) u[j] = __fadd_rn(u[j], __fmul_rn(r.cb, xs[j]));
    }
    if (r.cz != 0.0f) {
        chain_noise4(a.zin, a.numel, a.n4, r.seed, r.off, 0, g, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = __fadd_rn(u[j], __fmul_rn(r.cz, z[j]));
    }
    if (r.r1 != 0.0f) {
        chain_noise4(a.zin, a.numel, a.n4, r.seed, r.off, 1, g, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = __fadd_rn(__fmul_rn(r.r0, u[j]), __fmul_rn(r.r1, z[j]));
    }
    *reinterpret_cast<float4*>(a.x + g) = make_float4(u[0], u[1], u[2], u[3]);
}

// ---- quad form: n == 1, the measurement has x's layout
__global__ void __launch_bounds__(kDdnmThreads) ddnm_quad_kernel(DdnmArgs a) {
    const DdnmRow r = ddnm_row(a);
    const int64_t q = (int64_t)blockIdx.x * kDdnmThreads + threadIdx.x;
    if (q < a.n4) {
        const int64_t g = 4 * q;
        const float4 xv = load4((a.src ? a.src : a.x) + g);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
        float ms[4] = {1.f, 1.f, 1.f, 1.f};
        if (a.mask) {
            const float4 mv = load4(a.mask + g);
            ms[0] = mv.x, ms[1] = mv.y, ms[2] = mv.z, ms[3] = mv.w;
        }
        if (a.src) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = ms[j] != 0.0f ? ddnm_cell_mean(&xs[j], 1, 0) : 0.0f;
            *reinterpret_cast<float4*>(a.y_out + g) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            const float4 ev = load4(a.out + eps_index(g, a.chw, a.out_planes));
            const float es[4] = {ev.x, ev.y, ev.z, ev.w};
            float x0[4], res[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x0[j] = ddnm_x0(r, xs[j], es[j]);
                res[j] = ddnm_residual(ddnm_cell_mean(&x0[j], 1, 0), ms[j], a.y + g + j);
            }
            ddnm_finish(a, r, g, xs, x0, res);
        }
    }
    if (a.st) {
        __syncthreads();
        chain_advance(a.st, a.t_table, r.i, 2ull * (unsigned long long)a.n4, false);
    }
}

// where the band's element (c, i, col) sits: its cell within the band, and its place within the cell
__device__ __forceinline__ void ddnm_place(const DdnmArgs& a, int c, int i, int col, int& cell, int& k) {
    const int w = a.W / a.s, cw = col / a.s, jj = col - cw * a.s;
    cell = a.gray ? cw : c * w + cw;
    k = ((a.gray ? c * a.s : 0) + i) * a.s + jj;
}

// ---- band form: workgroup = (image, band of s rows); LDS: x0 [n][stride], then one residual per cell
__global__ void __launch_bounds__(kDdnmThreads) ddnm_band_kernel(DdnmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ddnm_lds[];
    float* X0 = ddnm_lds;
    float* R = X0 + (int64_t)a.n * a.stride;
    const DdnmRow r = ddnm_row(a);
    const int tid = threadIdx.x, s = a.s, W = a.W, bands = a.H / s, w = W / s;
    const int b = blockIdx.x / bands, band = blockIdx.x - b * bands;
    const int sW = s * W, Q = (a.C * sW) >> 2;
    const int64_t base = (int64_t)b * a.chw + (int64_t)band * sW;  // + c * hw + i * W + col
    const float* xin = a.src ? a.src : a.x;
    for (int q = tid; q < Q; q += kDdnmThreads) {
        const int idx = 4 * q, c = idx / sW, rem = idx - c * sW, i = rem / W, col = rem - i * W;
        const int64_t g = base + (int64_t)c * a.hw + rem;
        const float4 xv = load4(xin + g);
        float v[4] = {xv.x, xv.y, xv.z, xv.w};
        if (!a.src) {
            const float4 ev = load4(a.out + eps_index(g, a.chw, a.out_planes));
            v[0] = ddnm_x0(r, v[0], ev.x), v[1] = ddnm_x0(r, v[1], ev.y), v[2] = ddnm_x0(r, v[2], ev.z), v[3] = ddnm_x0(r, v[3], ev.w);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int cell, k;
            ddnm_place(a, c, i, col + j, cell, k);
            X0[k * a.stride + cell] = v[j];
        }
    }
    __syncthreads();
    const int Cm = a.gray ? 1 : a.C;
    for (int cell = tid; cell < a.cells; cell += kDdnmThreads) {
        const float mean = ddnm_cell_mean(X0 + cell, a.n, a.stride);
        const int cm = a.gray ? 0 : cell / w, cw = cell - cm * w;
        const int64_t yo = (((int64_t)b * Cm + cm) * bands + band) * w + cw;
        const float m = a.mask ? a.mask[yo] : 1.0f;
        if (a.src)
            a.y_out[yo] = m != 0.0f ? mean : 0.0f;
        else
            R[cell] = ddnm_residual(mean, m, a.y + yo);
    }
    if (a.src) return;
    __syncthreads();
    for (int q = tid; q < Q; q += kDdnmThreads) {
        const int idx = 4 * q, c = idx / sW, rem = idx - c * sW, i = rem / W, col = rem - i * W;
        const int64_t g = base + (int64_t)c * a.hw + rem;
        const float4 xv = load4(a.x + g);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
        float x0[4], res[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int cell, k;
            ddnm_place(a, c, i, col + j, cell, k);
            x0[j] = X0[k * a.stride + cell];
            res[j] = R[cell];
        }
        ddnm_finish(a, r, g, xs, x0, res);
    }
    if (a.st) {
        __syncthreads();
        chain_advance(a.st, a.t_table, r.i, 2ull * (unsigned long long)a.n4, false);
    }
}

int ddnm_band_capacity() { return kDdnmBandCapacity; }

// the checks of the shape every entry point makes, then the launch of the form the shape takes
static int ddnm_launch(const char* what, DdnmArgs& a, int B, hipStream_t s) {
    const int C = a.C, H = a.H, W = a.W, sc = a.s;
    DMME_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && sc > 0, DMME_ERR_INVALID, "%s: bad argument (%d images of %d x %d x %d, scale %d)", what, B, C, H, W, sc);
    DMME_REQUIRE(a.gray == 0 || a.gray == 1, DMME_ERR_INVALID, "%s: gray = %d (0: every channel is measured, 1: their mean)", what, a.gray);
    DMME_REQUIRE(H % sc == 0 && W % sc == 0, DMME_ERR_INVALID, "%s: scale %d does not divide the image size %d x %d", what, sc, H, W);
    a.hw = (int64_t)H * W, a.chw = a.hw * C, a.numel = a.chw * B, a.n4 = a.numel / 4;
    DMME_REQUIRE(W % 4 == 0 && a.chw % 4 == 0, DMME_ERR_UNSUPPORTED, "%s: image width %d and image size %lld must be multiples of 4", what, W, (long long)a.chw);
    DMME_REQUIRE(a.numel < (1ll << 40), DMME_ERR_UNSUPPORTED, "%s: %lld values", what, (long long)a.numel);
    a.n = (a.gray ? C : 1) * sc * sc;
    if (a.n == 1) {
        const int64_t blocks = (a.n4 + kDdnmThreads - 1) / kDdnmThreads;
        DMME_REQUIRE(blocks < (1ll << 31), DMME_ERR_UNSUPPORTED, "%s: %lld values", what, (long long)a.numel);
        hipLaunchKernelGGL(ddnm_quad_kernel, dim3((unsigned)blocks), dim3(kDdnmThreads), 0, s, a);
        DMME_CHECK_LAUNCH();
        return DMME_OK;
    }
    const int64_t band = (int64_t)C * sc * W;
    DMME_REQUIRE(band <= kDdnmBandCapacity, DMME_ERR_UNSUPPORTED,
                 "%s: a band of %d x %d x %d = %lld values is beyond the band form's %d (dmme_ddnm_band_capacity); a streaming form is not built", what, C, sc, W,
                 (long long)band, kDdnmBandCapacity);
    a.cells = (int)(band / a.n);
    // an odd stride keeps the quads' scattered stores on different banks; dropped where the padding would not fit
    a.stride = a.cells % 2 == 0 && ((int64_t)a.n * (a.cells + 1) + a.cells) * 4 <= kDdnmLdsBytes ? a.cells + 1 : a.cells;
    const int64_t lds = ((int64_t)a.n * a.stride + a.cells) * 4;
    DMME_REQUIRE(lds <= kDdnmLdsBytes, DMME_ERR_UNSUPPORTED, "%s: a band of %lld values in %d cells needs %lld bytes of LDS, above %d", what, (long long)band,
                 a.cells, (long long)lds, kDdnmLdsBytes);
    const int64_t blocks = (int64_t)B * (H / sc);
    DMME_REQUIRE(blocks < (1ll << 31), DMME_ERR_UNSUPPORTED, "%s: %lld bands", what, (long long)blocks);
    static bool lds_allowed = false;  // (the first launch is never inside a capture: the chain's trial step, or an eager call)
    if (!lds_allowed) {
        DMME_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ddnm_band_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kDdnmLdsBytes));
        lds_allowed = true;
    }
    hipLaunchKernelGGL(ddnm_band_kernel, dim3((unsigned)blocks), dim3(kDdnmThreads), (size_t)lds, s, a);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

int launch_ddnm_measure(const float* x, const float* mask, float* y_out, int B, int C, int H, int W, int sc, int gray, hipStream_t s) {
    DMME_REQUIRE(x && y_out, DMME_ERR_INVALID, "ddnm_measure: null argument");
    DdnmArgs a{};
    a.src = x, a.mask = mask, a.y_out = y_out, a.C = C, a.H = H, a.W = W, a.s = sc, a.gray = gray, a.out_planes = 1;
    return ddnm_launch("ddnm_measure", a, B, s);
}

// row: the eager form's 8 host floats; coef / t_table / state: the chain form's (exactly one of the two is given)
int launch_ddnm(const char* what, float* x, const float* model_out, const float* y, const float* mask, const float* z2, const float* row, const float* coef,
                const int64_t* t_table, void* state, int B, int C, int H, int W, int sc, int gray, int out_planes, hipStream_t s) {
    DMME_REQUIRE(x && model_out && y && mask, DMME_ERR_INVALID, "%s: null argument", what);
    DMME_REQUIRE(row ? !state : (coef && t_table && state), DMME_ERR_INVALID, "%s: null argument", what);
    DMME_REQUIRE(out_planes == 1 || out_planes == 2, DMME_ERR_INVALID, "%s: a network output of %d planes per image (1: eps, 2: eps and v)", what, out_planes);
    DdnmArgs a{};
    a.x = x, a.out = model_out, a.y = y, a.mask = mask, a.zin = z2, a.coef = coef, a.t_table = (const long long*)t_table, a.st = (ChainState*)state;
    a.C = C, a.H = H, a.W = W, a.s = sc, a.gray = gray, a.out_planes = out_planes;
    if (row) {
        for (int j = 0; j < 8; ++j) a.row[j] = row[j];
        DMME_REQUIRE(z2 || (row[2] == 0.0f && row[7] == 0.0f), DMME_ERR_INVALID, "%s: a step that adds noise needs z", what);
    }
    return ddnm_launch(what, a, B, s);
}

}  // namespace dmme

using namespace dmme;

// ------------------------------------------------------------------ entry points
DMME_API int dmme_ddnm_band_capacity(void) { return ddnm_band_capacity(); }

DMME_API int dmme_ddnm_measure(const float* x, const float* mask, float* y_out, int B, int C, int H, int W, int s, int gray, void* stream) {
    return launch_ddnm_measure(x, mask, y_out, B, C, H, W, s, gray, (hipStream_t)stream);
}

DMME_API int dmme_ddnm_step(float* x, const float* model_out, const float* y, const float* mask, const float* z2, const float* row, int B, int C, int H, int W,
                            int s, int gray, int out_planes, void* stream) {
    DMME_REQUIRE(row, DMME_ERR_INVALID, "ddnm_step: null argument");
    return launch_ddnm("ddnm_step", x, model_out, y, mask, z2, row, nullptr, nullptr, nullptr, B, C, H, W, s, gray, out_planes, (hipStream_t)stream);
}

DMME_API int dmme_chain_update_ddnm(float* x, const float* model_out, const float* y, const float* mask, const float* noise, const float* step_coef,
                                    const int64_t* t_table, void* state, int B, int C, int H, int W, int s, int gray, int out_planes, void* stream) {
    DMME_REQUIRE(step_coef && t_table && state, DMME_ERR_INVALID, "chain_update_ddnm: null argument");
    return launch_ddnm("chain_update_ddnm", x, model_out, y, mask, noise, nullptr, step_coef, t_table, state, B, C, H, W, s, gray, out_planes,
                       (hipStream_t)stream);
}
