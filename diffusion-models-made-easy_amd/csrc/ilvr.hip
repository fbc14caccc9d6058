// ILVR (Choi et al. 2021): DDPM's reverse step followed by a low-pass refinement against a reference image (dmme_hip.h: dmme_ilvr_step),
//   u = c0 (x - c1 e) [+ c2 z0];   k = ka y [+ ks z1];   x' = u + phi(k - u),   phi(d) = Ph d Pw^T per channel plane,
// the one sampler update that is not elementwise: phi is a bicubic down-then-up resize, two dense matrix products per H x W plane.
// The elementwise half is rounded operation by operation like every other update (the translation unit is compiled with
// -ffp-contract=off, csrc/Makefile, and the reverse step carries DDPM's bits); the two products are chains of explicit fmaf in ONE
// function, lp_dot4, that every form calls: eager = chain and fused = streaming, bit for bit.
//
// Two forms.  Fused (planes of at most kLpCapacity values whose tables fit): one workgroup per plane, d, T = d Pw^T and both tables in
// LDS, u in registers, one launch.  Streaming (larger planes): a row pass that stages kLpRowTile rows of d in LDS and writes T to a
// scratch buffer, then a column pass that stages kLpColTile columns of T, recomputes u from the same operands and Philox counters and
// writes x'.  The last block of the last launch advances the chain's loop state (chain_advance).
#include "common.h"
#include "sampler_dev.h"

namespace dmme {

constexpr int kLpThreads = 256;
constexpr int kLpCapacity = 4096;       // H * W of the fused form: 64 x 64, four quads per thread held in registers
constexpr int kLpQuads = kLpCapacity / 4 / kLpThreads;
constexpr int kLpLdsMax = 96 * 1024;    // bytes of LDS a workgroup of either form may ask for
constexpr int kLpRowTile = 32;          // streaming row pass: rows of d per workgroup, one per lane of a half wave
constexpr int kLpColTile = 64;          // streaming column pass: columns of T per workgroup, 16 quads

struct LpArgs {
    float* x;           // updated in place (dmme_lowpass: the destination)
    const float* src;   // dmme_lowpass only: the planes to filter; the update forms leave it null
    const float* out;   // network output, out_planes * chw values per image, the eps plane first
    const float* ref;   // y, in x's layout
    const float* zin;   // [2][numel] normals: the eager form's, or the chain form's override
    const float* Ph;    // [H][H]
    const float* Pw;    // [W][W]
    float* scratch;     // streaming form: T, planes * H * W values
    const float* coef;  // chain form: the table, 8 floats per loop index
    const long long* t_table;
    ChainState* st;     // chain form; null: the eager form, whose row is `row`
    float row[8];
    int H, W, out_planes;
    int64_t hw, chw, numel, n4;
};

struct LpRow {
    float c0, c1, c2, ka, ks;
    int used;   // bit 0: z0 is added, bit 1: z1 is added, bit 2: the step is conditioned
    long long i;
    unsigned long long seed, off;
};

// the step's row (chain_cursor: called at the top of each kernel)
__device__ __forceinline__ LpRow lp_row(const LpArgs& a) {
    const ChainCursor k = chain_cursor(a.st, a.coef, a.row);
    const float* c = k.row;
    LpRow r;
    r.i = k.i, r.seed = k.seed, r.off = k.off;
    r.c0 = c[0], r.c1 = c[1], r.c2 = c[2], r.ka = c[3], r.ks = c[4];
    const bool cond = c[5] != 0.0f;
    r.used = (r.c2 != 0.0f ? 1 : 0) | (cond && r.ks != 0.0f ? 2 : 0) | (cond ? 4 : 0);
    return r;
}

// the elementwise half for the quad at element b: u, and d = k - u where want_d (dmme_lowpass: u = 0, d = src)
__device__ __forceinline__ void lp_quad(const LpArgs& a, const LpRow& r, int64_t b, bool want_d, float (&u)[4], float (&d)[4]) {
    if (a.src) {
        const float4 v = load4(a.src + b);
        u[0] = u[1] = u[2] = u[3] = 0.f;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        return;
    }
    float z[4];
    if (r.used & 1) chain_noise4(a.zin, a.numel, a.n4, r.seed, r.off, 0, b, z);
    const float4 xv = load4(a.x + b), ev = load4(a.out + eps_index(b, a.chw, a.out_planes));
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, es[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        u[j] = ddpm_mean(xs[j], es[j], r.c0, r.c1);
        if (r.used & 1) u[j] = __fadd_rn(u[j], __fmul_rn(r.c2, z[j]));
    }
    if (!want_d) return;
    if (r.used & 2) chain_noise4(a.zin, a.numel, a.n4, r.seed, r.off, 1, b, z);
    const float4 yv = load4(a.ref + b);
    const float ys[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float k = __fmul_rn(r.ka, ys[j]);
        if (r.used & 2) k = __fadd_rn(k, __fmul_rn(r.ks, z[j]));
        d[j] = __fsub_rn(k, u[j]);
    }
}

// THE dot product of both passes, four outputs at a time: acc_j = fma(a[k], b[k sb + j jb], acc_j) for k = 0 .. n - 1 in this order from
// acc_j = 0.  VEC: the four b values of a k are one aligned 16-byte read (jb = 1).  The summation order and the fma are fixed here, once.
template <bool VEC>
__device__ __forceinline__ void lp_dot4(const float* __restrict__ a, const float* __restrict__ b, int sb, int jb, int n, float (&acc)[4]) {
    acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
    for (int k = 0; k < n; ++k) {
        const float av = a[k];
        const float* bk = b + (int64_t)k * sb;
        float bv[4];
        if (VEC) {
            const float4 v = load4(bk);
            bv[0] = v.x, bv[1] = v.y, bv[2] = v.z, bv[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = bk[j * jb];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(av, bv[j], acc[j]);
    }
}

__device__ __forceinline__ void lp_store(float* p, const float (&u)[4], const float (&f)[4], bool plain) {
    *reinterpret_cast<float4*>(p) = plain ? make_float4(f[0], f[1], f[2], f[3])
                                          : make_float4(__fadd_rn(u[0], f[0]), __fadd_rn(u[1], f[1]), __fadd_rn(u[2], f[2]), __fadd_rn(u[3], f[3]));
}

// LDS of the fused form, in floats: T [H][W], Pw transposed [W][W + 4] (16-byte reads along c, no two lanes of a read on one bank),
// d [H][W + 1] and Ph [H][H + 1] (rows read by a few lanes each: the odd stride keeps rows on different banks)
__host__ __device__ inline int lp_fused_floats(int H, int W) { return H * W + W * (W + 4) + H * (W + 1) + H * (H + 1); }
static bool lp_fits_fused(int H, int W) {
    return (int64_t)H * W <= kLpCapacity && (int64_t)H <= kLpCapacity && (int64_t)W <= kLpCapacity && (int64_t)lp_fused_floats(H, W) * 4 <= kLpLdsMax;
}

// ---- fused: one workgroup per plane
__global__ void __launch_bounds__(kLpThreads) ilvr_fused_kernel(LpArgs a) {
    extern __shared__ float4 lp_lds4[];
    float* T = reinterpret_cast<float*>(lp_lds4);
    const int H = a.H, W = a.W, SW = W + 4, SD = W + 1, SH = H + 1;
    float* PwT = T + H * W;
    float* D = PwT + W * SW;
    float* PhL = D + H * SD;
    const int tid = threadIdx.x;
    const LpRow r = lp_row(a);
    const bool cond = a.src || (r.used & 4);
    const int Q = (int)(a.hw >> 2);
    const int64_t base = (int64_t)blockIdx.x * a.hw;
    float u[kLpQuads][4];
    if (cond) {
        for (int idx = tid; idx < W * W; idx += kLpThreads) PwT[(idx % W) * SW + idx / W] = a.Pw[idx];
        for (int idx = tid; idx < H * H; idx += kLpThreads) PhL[(idx / H) * SH + idx % H] = a.Ph[idx];
    }
#pragma unroll
    for (int j = 0; j < kLpQuads; ++j) {
        const int q = tid + kLpThreads * j;
        if (q < Q) {
            float d[4];
            lp_quad(a, r, base + 4 * (int64_t)q, cond, u[j], d);
            if (cond) {
                const int row = (4 * q) / W, c = (4 * q) % W;
#pragma unroll
                for (int e = 0; e < 4; ++e) D[row * SD + c + e] = d[e];
            } else {
                lp_store(a.x + base + 4 * (int64_t)q, u[j], u[j], true);
            }
        }
    }
    if (cond) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kLpQuads; ++j) {  // the row pass: T = d Pw^T
            const int q = tid + kLpThreads * j;
            if (q < Q) {
                const int row = (4 * q) / W, c = (4 * q) % W;
                float t[4];
                lp_dot4<true>(D + row * SD, PwT + c, SW, 1, W, t);
                *reinterpret_cast<float4*>(T + 4 * q) = make_float4(t[0], t[1], t[2], t[3]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kLpQuads; ++j) {  // the column pass: F = Ph T, and x' = u + F
            const int q = tid + kLpThreads * j;
            if (q < Q) {
                const int row = (4 * q) / W, c = (4 * q) % W;
                float f[4];
                lp_dot4<true>(PhL + row * SH, T + c, W, 1, H, f);
                lp_store(a.x + base + 4 * (int64_t)q, u[j], f, a.src != nullptr);
            }
        }
    }
    if (a.st) {
        __syncthreads();
        chain_advance(a.st, a.t_table, r.i, 2ull * (unsigned long long)a.n4, false);
    }
}

// ---- streaming, first launch: workgroup (plane, tile of kLpRowTile rows) stages its rows of d in LDS ([rows][W + 1]: lane = row, the
// odd stride keeps the lanes on different banks) and writes T = d Pw^T for them; Pw's rows are read from memory, uniform across a half wave
__global__ void __launch_bounds__(kLpThreads) ilvr_rows_kernel(LpArgs a, int tiles) {
    extern __shared__ float4 lp_lds4[];
    float* D = reinterpret_cast<float*>(lp_lds4);
    const int H = a.H, W = a.W, SD = W + 1, tid = threadIdx.x;
    const LpRow r = lp_row(a);
    if (!a.src && !(r.used & 4)) return;
    const int plane = blockIdx.x / tiles, r0 = (blockIdx.x % tiles) * kLpRowTile;
    const int rows = min(kLpRowTile, H - r0), WQ = W >> 2;
    const int64_t base = (int64_t)plane * a.hw + (int64_t)r0 * W;
    for (int q = tid; q < rows * WQ; q += kLpThreads) {
        float u[4], d[4];
        lp_quad(a, r, base + 4 * (int64_t)q, true, u, d);
        const int row = q / WQ, c = 4 * (q % WQ);
#pragma unroll
        for (int e = 0; e < 4; ++e) D[row * SD + c + e] = d[e];
    }
    __syncthreads();
    for (int o = tid; o < kLpRowTile * WQ; o += kLpThreads) {
        const int row = o % kLpRowTile, c = 4 * (o / kLpRowTile);
        if (row < rows) {
            float t[4];
            lp_dot4<false>(D + row * SD, a.Pw + (int64_t)c * W, 1, W, W, t);
            *reinterpret_cast<float4*>(a.scratch + base + (int64_t)row * W + c) = make_float4(t[0], t[1], t[2], t[3]);
        }
    }
}

// ---- streaming, second launch: workgroup (plane, tile of kLpColTile columns) stages its columns of T in LDS ([H][kLpColTile]),
// recomputes u for its quads from the same operands and counters, and writes x' = u + Ph T
__global__ void __launch_bounds__(kLpThreads) ilvr_cols_kernel(LpArgs a, int tiles) {
    extern __shared__ float4 lp_lds4[];
    float* T = reinterpret_cast<float*>(lp_lds4);
    const int H = a.H, W = a.W, tid = threadIdx.x;
    const LpRow r = lp_row(a);
    const bool cond = a.src || (r.used & 4);
    const int plane = blockIdx.x / tiles, c0 = (blockIdx.x % tiles) * kLpColTile;
    const int cols = min(kLpColTile, W - c0), CQ = cols >> 2;
    const int64_t base = (int64_t)plane * a.hw;
    if (cond) {
        for (int q = tid; q < H * CQ; q += kLpThreads) {
            const int row = q / CQ, c = 4 * (q % CQ);
            *reinterpret_cast<float4*>(T + row * kLpColTile + c) = load4(a.scratch + base + (int64_t)row * W + c0 + c);
        }
        __syncthreads();
    }
    for (int q = tid; q < H * CQ; q += kLpThreads) {
        const int row = q / CQ, c = 4 * (q % CQ);
        const int64_t b = base + (int64_t)row * W + c0 + c;
        float u[4], d[4], f[4];
        lp_quad(a, r, b, false, u, d);
        if (cond) lp_dot4<true>(a.Ph + (int64_t)row * H, T + c, kLpColTile, 1, H, f);
        lp_store(a.x + b, u, cond ? f : u, a.src != nullptr || !cond);
    }
    if (a.st) {
        __syncthreads();
        chain_advance(a.st, a.t_table, r.i, 2ull * (unsigned long long)a.n4, false);
    }
}

int lowpass_lds_capacity() { return kLpCapacity; }
int64_t lowpass_scratch_bytes(int planes, int H, int W) { return planes > 0 && H > 0 && W > 0 ? (int64_t)planes * H * W * (int64_t)sizeof(float) : 0; }

static int lp_launch(const char* what, LpArgs& a, int planes, int force_streaming, hipStream_t s) {
    const int H = a.H, W = a.W;
    DMME_REQUIRE(a.Ph && a.Pw, DMME_ERR_INVALID, "%s: null table (Ph: [H][H], Pw: [W][W])", what);
    DMME_REQUIRE(W % 4 == 0, DMME_ERR_UNSUPPORTED, "%s: plane width %d is not a multiple of 4", what, W);
    DMME_REQUIRE((int64_t)planes * H * W < (1ll << 31) && planes <= (1 << 20), DMME_ERR_UNSUPPORTED, "%s: %d planes of %d x %d", what, planes, H, W);
    static bool lds_allowed = false;  // (the first launch is never inside a capture: the chain's trial step, or an eager call)
    if (!lds_allowed) {
        for (const void* k : {reinterpret_cast<const void*>(ilvr_fused_kernel), reinterpret_cast<const void*>(ilvr_rows_kernel),
                              reinterpret_cast<const void*>(ilvr_cols_kernel)})
            DMME_CHECK_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLpLdsMax));
        lds_allowed = true;
    }
    if (lp_fits_fused(H, W) && !force_streaming) {
        hipLaunchKernelGGL(ilvr_fused_kernel, dim3(planes), dim3(kLpThreads), (size_t)lp_fused_floats(H, W) * sizeof(float), s, a);
        DMME_CHECK_LAUNCH();
        return DMME_OK;
    }
    const size_t row_lds = (size_t)kLpRowTile * (W + 1) * sizeof(float), col_lds = (size_t)H * kLpColTile * sizeof(float);
    DMME_REQUIRE(row_lds <= (size_t)kLpLdsMax && col_lds <= (size_t)kLpLdsMax, DMME_ERR_UNSUPPORTED,
                 "%s: a plane of %d x %d is beyond the streaming form (H <= %d, W <= %d)", what, H, W, kLpLdsMax / 4 / kLpColTile, kLpLdsMax / 4 / kLpRowTile - 1);
    DMME_REQUIRE(a.scratch, DMME_ERR_INVALID, "%s: planes of %d x %d go through the streaming form, which needs a scratch buffer of dmme_lowpass_scratch_bytes", what,
                 H, W);
    const int row_tiles = (H + kLpRowTile - 1) / kLpRowTile, col_tiles = (W + kLpColTile - 1) / kLpColTile;
    hipLaunchKernelGGL(ilvr_rows_kernel, dim3(planes * row_tiles), dim3(kLpThreads), row_lds, s, a, row_tiles);
    DMME_CHECK_LAUNCH();
    hipLaunchKernelGGL(ilvr_cols_kernel, dim3(planes * col_tiles), dim3(kLpThreads), col_lds, s, a, col_tiles);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

int launch_lowpass(const float* src, float* dst, int planes, int H, int W, const float* Ph, const float* Pw, float* scratch, int force_streaming,
                   hipStream_t s) {
    DMME_REQUIRE(src && dst && planes > 0 && H > 0 && W > 0, DMME_ERR_INVALID, "lowpass: bad argument (%d planes of %d x %d)", planes, H, W);
    LpArgs a{};
    a.x = dst, a.src = src, a.Ph = Ph, a.Pw = Pw, a.scratch = scratch, a.H = H, a.W = W, a.out_planes = 1;
    a.hw = (int64_t)H * W, a.chw = a.hw, a.numel = a.hw * planes, a.n4 = a.numel / 4;
    return lp_launch("lowpass", a, planes, force_streaming, s);
}

// row: the eager form's 8 host floats; coef / t_table / state: the chain form's (exactly one of the two is given)
int launch_ilvr(const char* what, float* x, const float* model_out, const float* ref, const float* z2, const float* row, const float* Ph, const float* Pw,
                float* scratch, const float* coef, const int64_t* t_table, void* state, int B, int C, int H, int W, int out_planes, int force_streaming,
                hipStream_t s) {
    DMME_REQUIRE(x && model_out && ref && B > 0 && C > 0 && H > 0 && W > 0, DMME_ERR_INVALID, "%s: bad argument", what);
    DMME_REQUIRE(row ? !state : (coef && t_table && state), DMME_ERR_INVALID, "%s: null argument", what);
    DMME_REQUIRE(out_planes == 1 || out_planes == 2, DMME_ERR_INVALID, "%s: a network output of %d planes per image (1: eps, 2: eps and v)", what, out_planes);
    const int64_t chw = (int64_t)C * H * W;
    DMME_REQUIRE(chw % 4 == 0, DMME_ERR_UNSUPPORTED, "%s: image size %lld is not a multiple of 4", what, (long long)chw);
    LpArgs a{};
    a.x = x, a.out = model_out, a.ref = ref, a.zin = z2, a.Ph = Ph, a.Pw = Pw, a.scratch = scratch, a.coef = coef, a.t_table = (const long long*)t_table;
    a.st = (ChainState*)state, a.H = H, a.W = W, a.out_planes = out_planes;
    a.hw = (int64_t)H * W, a.chw = chw, a.numel = chw * B, a.n4 = a.numel / 4;
    if (row) {
        for (int j = 0; j < 8; ++j) a.row[j] = row[j];
        const bool cond = row[5] != 0.0f;
        DMME_REQUIRE(z2 || (row[2] == 0.0f && !(cond && row[4] != 0.0f)), DMME_ERR_INVALID, "%s: a step that adds noise needs z", what);
    }
    return lp_launch(what, a, B * C, force_streaming, s);
}

}  // namespace dmme

using namespace dmme;

// ------------------------------------------------------------------ entry points
DMME_API int dmme_lowpass(const float* src, float* dst, int planes, int H, int W, const float* Ph, const float* Pw, float* scratch, int force_streaming,
                          void* stream) {
    return launch_lowpass(src, dst, planes, H, W, Ph, Pw, scratch, force_streaming, (hipStream_t)stream);
}

DMME_API int dmme_lowpass_lds_capacity(void) { return lowpass_lds_capacity(); }

DMME_API int64_t dmme_lowpass_scratch_bytes(int planes, int H, int W) { return lowpass_scratch_bytes(planes, H, W); }

DMME_API int dmme_ilvr_step(float* x, const float* model_out, const float* ref, const float* z2, const float* row, const float* Ph, const float* Pw,
                            float* scratch, int B, int C, int H, int W, int out_planes, int force_streaming, void* stream) {
    DMME_REQUIRE(row, DMME_ERR_INVALID, "ilvr_step: null argument");
    return launch_ilvr("ilvr_step", x, model_out, ref, z2, row, Ph, Pw, scratch, nullptr, nullptr, nullptr, B, C, H, W, out_planes, force_streaming,
                       (hipStream_t)stream);
}

DMME_API int dmme_chain_update_ilvr(float* x, const float* model_out, const float* ref, const float* noise, const float* Ph, const float* Pw, float* scratch,
                                    const float* step_coef, const int64_t* t_table, void* state, int B, int C, int H, int W, int out_planes,
                                    int force_streaming, void* stream) {
    DMME_REQUIRE(step_coef && t_table && state, DMME_ERR_INVALID, "chain_update_ilvr: null argument");
    return launch_ilvr("chain_update_ilvr", x, model_out, ref, noise, nullptr, Ph, Pw, scratch, step_coef, t_table, state, B, C, H, W, out_planes,
                       force_streaming, (hipStream_t)stream);
}
