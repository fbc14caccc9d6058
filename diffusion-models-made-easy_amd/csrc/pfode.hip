// Probability-flow ODE (Song et al., ICLR 2021, section 4.3 and appendix D.2; dmme_hip.h: dmme_pf_*): what a Heun stage needs beside the
// network.  The Rademacher probe written straight into a buffer of the network output's layout, the per-image dot  s = sum z dx  with
// its double accumulator, the standard-normal log-density of the latent, the uniform dequantisation, and the four-term stage update
//   x_new = c0 x + c1 xs + c2 e + c3 es     (xs <- x, es <- e where the row says save)
// in ONE device function, pf_update, that the eager and the chain form both call.  All of it is HBM-bound: quads where an image is a
// whole number of them, elements otherwise.  The reductions are a grid (parts, B) of partial sums and one finishing launch: no atomics,
// no workgroup waits for another, the same bits on every run and at every place of a batch.  The translation unit is compiled with
// -ffp-contract=off (csrc/Makefile): the only fused operations are the explicit fmaf below.
#include "common.h"
#include "sampler_dev.h"

namespace dmme {

constexpr int kPfThreads = 256;
constexpr int kPfParts = 64;  // blocks per image at the most

static inline int pf_parts(int64_t chw) {
    const int64_t p = (chw + 1023) / 1024;
    return (int)(p > kPfParts ? kPfParts : (p < 1 ? 1 : p));
}
int64_t pf_scratch_floats(int B, int64_t chw) { return (int64_t)B * pf_parts(chw); }

static inline bool pf_aligned(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((uintptr_t)p % 16 != 0) return false;
    return true;
}
// may a quad of the flat index be handled as one float4?  Every image starts on a quad, or there is one image of one plane
static inline bool pf_quads(int B, int64_t chw, int planes, std::initializer_list<const void*> ptrs) {
    return (chw % 4 == 0 || (B == 1 && planes == 1)) && pf_aligned(ptrs);
}

// ------------------------------------------------------------------ the probe and the dequantisation: one thread per Philox quad
struct PfDrawArgs {
    float* dst;             // the probe: (B, planes * chw); the dequantisation: x, numel values
    const ChainState* st;   // chain form: seed and offset are read here
    unsigned long long seed, offset;
    int64_t chw, numel, quads;
    int planes, vec;
};

__global__ void __launch_bounds__(kPfThreads) pf_probe_kernel(PfDrawArgs a) {
    unsigned long long seed = a.seed, off = a.offset;
    if (a.st) seed = a.st->seed, off = a.st->offset;
    const int64_t q = (int64_t)blockIdx.x * kPfThreads + threadIdx.x;
    if (q >= a.quads) return;
    uint32_t r[4];
    philox4x32_10(seed, off + (uint64_t)q, r);
    float z[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = (r[j] >> 31) ? -1.0f : 1.0f;
    const int64_t e0 = 4 * q;
    if (a.vec && e0 + 3 < a.numel) {
        const int64_t o = eps_index(e0, a.chw, a.planes);
        *reinterpret_cast<float4*>(a.dst + o) = make_float4(z[0], z[1], z[2], z[3]);
        if (a.planes == 2) *reinterpret_cast<float4*>(a.dst + o + a.chw) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (int j = 0; j < 4 && e0 + j < a.numel; ++j) {
            const int64_t o = eps_index(e0 + j, a.chw, a.planes);
            a.dst[o] = z[j];
            if (a.planes == 2) a.dst[o + a.chw] = 0.0f;
        }
    }
}

// x += (u - 0.5) * (2 / 255): the difference is exact (u is a multiple of 2^-24 in (0, 1]), the product and the sum round once each
__device__ __forceinline__ float pf_dequant(float x, uint32_t word) { return __fadd_rn(x, __fmul_rn(__fsub_rn(u01(word), 0.5f), (float)(2.0 / 255.0))); }

__global__ void __launch_bounds__(kPfThreads) pf_dequantize_kernel(PfDrawArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kPfThreads + threadIdx.x;
    if (q >= a.quads) return;
    uint32_t r[4];
    philox4x32_10(a.seed, a.offset + (uint64_t)q, r);
    const int64_t e0 = 4 * q;
    if (a.vec && e0 + 3 < a.numel) {
        const float4 v = load4(a.dst + e0);
        *reinterpret_cast<float4*>(a.dst + e0) = make_float4(pf_dequant(v.x, r[0]), pf_dequant(v.y, r[1]), pf_dequant(v.z, r[2]), pf_dequant(v.w, r[3]));
    } else {
        for (int j = 0; j < 4 && e0 + j < a.numel; ++j) a.dst[e0 + j] = pf_dequant(a.dst[e0 + j], r[j]);
    }
}

// ------------------------------------------------------------------ the reductions: partial sums per (part, image), one finishing launch
// block (p, b) sums a[b][j] * c[b][j] over its share of image b: each thread its elements in ascending order by fma from 0, the wave by a
// butterfly, the waves in index order (block_sum).  a has `planes` chw-sized planes per image and its first is read; c has one.
template <bool QUAD>
__global__ void __launch_bounds__(kPfThreads) pf_dot_partial_kernel(const float* __restrict__ a, int planes, const float* __restrict__ c, int64_t chw,
                                                                    float* __restrict__ partial) {
    __shared__ float red[16];
    const int b = blockIdx.y;
    const float* ab = a + (int64_t)b * planes * chw;
    const float* cb = c + (int64_t)b * chw;
    float acc = 0.f;
    if (QUAD) {
        for (int64_t q = blockIdx.x * (int64_t)kPfThreads + threadIdx.x; q < chw / 4; q += (int64_t)gridDim.x * kPfThreads) {
            const float4 u = load4(ab + 4 * q), v = load4(cb + 4 * q);
            acc = fmaf(u.x, v.x, acc);
            acc = fmaf(u.y, v.y, acc);
            acc = fmaf(u.z, v.z, acc);
            acc = fmaf(u.w, v.w, acc);
        }
    } else {
        for (int64_t j = blockIdx.x * (int64_t)kPfThreads + threadIdx.x; j < chw; j += (int64_t)gridDim.x * kPfThreads) acc = fmaf(ab[j], cb[j], acc);
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = tot;
}

// one block; thread b (strided) finishes image b: the partials in index order in double
__device__ __forceinline__ double pf_partials(const float* __restrict__ partial, int parts, int b) {
    double S = 0.0;
    for (int p = 0; p < parts; ++p) S += (double)partial[(int64_t)b * parts + p];
    return S;
}
__global__ void __launch_bounds__(kPfThreads) pf_dot_finish_kernel(const float* __restrict__ partial, int parts, int B, const float* __restrict__ coef,
                                                                   const ChainState* __restrict__ st, float w_host, float* __restrict__ s_out,
                                                                   double* __restrict__ acc) {
    const float w = st ? coef[8 * st->i + 4] : w_host;
    for (int b = threadIdx.x; b < B; b += kPfThreads) {
        const float sf = (float)pf_partials(partial, parts, b);
        s_out[b] = sf;
        acc[b] = acc[b] + (double)w * (double)sf;
    }
}
__global__ void __launch_bounds__(kPfThreads) pf_prior_finish_kernel(const float* __restrict__ partial, int parts, int B, double chw, double* __restrict__ out) {
    for (int b = threadIdx.x; b < B; b += kPfThreads) out[b] = -0.5 * pf_partials(partial, parts, b) - (0.5 * chw) * 1.8378770664093453;  // ln(2 pi)
}

// ------------------------------------------------------------------ the stage update
// THE update of a stage (dmme_hip.h: dmme_pf_stage): the order of the operations is fixed here, once; a term whose coefficient is zero is
// skipped, so its operand may hold anything
__device__ __forceinline__ float pf_update(float x, float xs, float e, float es, float c0, float c1, float c2, float c3) {
    float r = 0.0f;
    if (c0 != 0.0f) r = __fmul_rn(c0, x);
    if (c1 != 0.0f) r = fmaf(c1, xs, r);
    if (c2 != 0.0f) r = fmaf(c2, e, r);
    if (c3 != 0.0f) r = fmaf(c3, es, r);
    return r;
}

struct PfStageArgs {
    float* x;
    const float* out;  // network output, planes * chw values per image, the eps plane first
    float* xs;         // (B, chw): the state at the step's first node
    float* es;         // (B, chw): the prediction at the step's first node
    const float* coef;
    const long long* t_table;
    ChainState* st;    // chain form; null: the eager form, whose row is `row`
    float row[8];
    int64_t chw, numel, n4;  // n4: quads handled as float4; the elements from 4 n4 on go one by one
    int planes;
    unsigned long long offset_inc;
};

__global__ void __launch_bounds__(kPfThreads) pf_stage_kernel(PfStageArgs a) {
    const ChainCursor k = chain_cursor(a.st, a.coef, a.row);
    const float* row = k.row;
    const float c0 = row[0], c1 = row[1], c2 = row[2], c3 = row[3];
    const bool save = row[5] != 0.0f;
    const int64_t first = (int64_t)blockIdx.x * kPfThreads + threadIdx.x;
    if (first < a.n4) {
        const int64_t e0 = 4 * first, eo = eps_index(e0, a.chw, a.planes);
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 xv = load4(a.x + e0), ev = load4(a.out + eo);
        const float4 sv = c1 != 0.0f ? load4(a.xs + e0) : zero, tv = c3 != 0.0f ? load4(a.es + e0) : zero;
        if (save) {
            *reinterpret_cast<float4*>(a.xs + e0) = xv;
            *reinterpret_cast<float4*>(a.es + e0) = ev;
        }
        *reinterpret_cast<float4*>(a.x + e0) = make_float4(pf_update(xv.x, sv.x, ev.x, tv.x, c0, c1, c2, c3), pf_update(xv.y, sv.y, ev.y, tv.y, c0, c1, c2, c3),
                                                           pf_update(xv.z, sv.z, ev.z, tv.z, c0, c1, c2, c3), pf_update(xv.w, sv.w, ev.w, tv.w, c0, c1, c2, c3));
    }
    const int64_t j = 4 * a.n4 + first;
    if (j < a.numel) {
        const float xv = a.x[j], ev = a.out[eps_index(j, a.chw, a.planes)];
        const float sv = c1 != 0.0f ? a.xs[j] : 0.0f, tv = c3 != 0.0f ? a.es[j] : 0.0f;
        if (save) a.xs[j] = xv, a.es[j] = ev;
        a.x[j] = pf_update(xv, sv, ev, tv, c0, c1, c2, c3);
    }
    if (a.st) {
        __syncthreads();
        chain_advance(a.st, a.t_table, k.i, a.offset_inc, false);
    }
}

// ------------------------------------------------------------------ launchers
static int pf_shape(const char* what, int B, int64_t chw, int planes) {
    DMME_REQUIRE(B > 0 && B <= 65535 && chw > 0 && (int64_t)B * chw < (1ll << 40), DMME_ERR_INVALID, "%s: B = %d (1..65535), chw = %lld", what, B, (long long)chw);
    DMME_REQUIRE(planes == 1 || planes == 2, DMME_ERR_INVALID, "%s: a network output of %d planes per image (1: eps, 2: eps and v)", what, planes);
    return DMME_OK;
}

int launch_pf_probe(const char* what, float* d_out, const void* state, uint64_t seed, uint64_t offset, int B, int64_t chw, int out_planes, hipStream_t s) {
    DMME_REQUIRE(d_out, DMME_ERR_INVALID, "%s: null argument", what);
    if (int rc = pf_shape(what, B, chw, out_planes)) return rc;
    PfDrawArgs a{};
    a.dst = d_out, a.st = (const ChainState*)state, a.seed = seed, a.offset = offset, a.chw = chw, a.numel = (int64_t)B * chw, a.quads = (a.numel + 3) / 4;
    a.planes = out_planes, a.vec = pf_quads(B, chw, out_planes, {d_out}) ? 1 : 0;
    hipLaunchKernelGGL(pf_probe_kernel, dim3((unsigned)((a.quads + kPfThreads - 1) / kPfThreads)), dim3(kPfThreads), 0, s, a);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

static int launch_pf_dequantize(float* x, int64_t numel, uint64_t seed, uint64_t offset, hipStream_t s) {
    DMME_REQUIRE(x && numel >= 0 && numel < (1ll << 40), DMME_ERR_INVALID, "pf_dequantize: bad argument");
    if (numel == 0) return DMME_OK;
    PfDrawArgs a{};
    a.dst = x, a.seed = seed, a.offset = offset, a.chw = numel, a.numel = numel, a.quads = (numel + 3) / 4, a.planes = 1, a.vec = pf_aligned({x}) ? 1 : 0;
    hipLaunchKernelGGL(pf_dequantize_kernel, dim3((unsigned)((a.quads + kPfThreads - 1) / kPfThreads)), dim3(kPfThreads), 0, s, a);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// the partial sums of  sum a c  per image into scratch
static int launch_pf_partials(const float* a, int planes, const float* c, int B, int64_t chw, float* scratch, hipStream_t s) {
    const int parts = pf_parts(chw);
    if (chw % 4 == 0 && pf_aligned({a, c}))
        hipLaunchKernelGGL(pf_dot_partial_kernel<true>, dim3(parts, B), dim3(kPfThreads), 0, s, a, planes, c, chw, scratch);
    else
        hipLaunchKernelGGL(pf_dot_partial_kernel<false>, dim3(parts, B), dim3(kPfThreads), 0, s, a, planes, c, chw, scratch);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

int launch_pf_dot(const char* what, const float* d_out, int out_planes, const float* dx, const float* row, const float* coef, const void* state, int B, int64_t chw,
                  float* scratch, float* s_out, double* acc, hipStream_t s) {
    DMME_REQUIRE(d_out && dx && scratch && s_out && acc, DMME_ERR_INVALID, "%s: null argument", what);
    DMME_REQUIRE(row ? !state : (coef && state), DMME_ERR_INVALID, "%s: null argument", what);
    if (int rc = pf_shape(what, B, chw, out_planes)) return rc;
    if (int rc = launch_pf_partials(d_out, out_planes, dx, B, chw, scratch, s)) return rc;
    hipLaunchKernelGGL(pf_dot_finish_kernel, dim3(1), dim3(kPfThreads), 0, s, scratch, pf_parts(chw), B, coef, (const ChainState*)state, row ? row[4] : 0.0f, s_out,
                       acc);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

static int launch_pf_prior(const float* x, int B, int64_t chw, float* scratch, double* out, hipStream_t s) {
    DMME_REQUIRE(x && scratch && out, DMME_ERR_INVALID, "pf_prior: null argument");
    if (int rc = pf_shape("pf_prior", B, chw, 1)) return rc;
    if (int rc = launch_pf_partials(x, 1, x, B, chw, scratch, s)) return rc;
    hipLaunchKernelGGL(pf_prior_finish_kernel, dim3(1), dim3(kPfThreads), 0, s, scratch, pf_parts(chw), B, (double)chw, out);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

int launch_pf_stage(const char* what, float* x, const float* model_out, int out_planes, float* xs, float* es, const float* row, const float* coef,
                    const int64_t* t_table, void* state, int advance_offset, int B, int64_t chw, hipStream_t s) {
    DMME_REQUIRE(x && model_out && xs && es, DMME_ERR_INVALID, "%s: null argument", what);
    DMME_REQUIRE(row ? !state : (coef && t_table && state), DMME_ERR_INVALID, "%s: null argument", what);
    if (int rc = pf_shape(what, B, chw, out_planes)) return rc;
    PfStageArgs a{};
    a.x = x, a.out = model_out, a.xs = xs, a.es = es, a.coef = coef, a.t_table = (const long long*)t_table, a.st = (ChainState*)state;
    a.chw = chw, a.numel = (int64_t)B * chw, a.planes = out_planes;
    a.n4 = pf_quads(B, chw, out_planes, {x, model_out, xs, es}) ? a.numel / 4 : 0;
    a.offset_inc = advance_offset ? (unsigned long long)(a.numel / 4) : 0ull;
    DMME_REQUIRE(!advance_offset || chw % 4 == 0, DMME_ERR_UNSUPPORTED, "%s: image size %lld is not a multiple of 4", what, (long long)chw);
    if (row)
        for (int j = 0; j < 8; ++j) a.row[j] = row[j];
    const int64_t tail = a.numel - 4 * a.n4, work = a.n4 > tail ? a.n4 : tail;
    hipLaunchKernelGGL(pf_stage_kernel, dim3((unsigned)((work + kPfThreads - 1) / kPfThreads)), dim3(kPfThreads), 0, s, a);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

}  // namespace dmme

using namespace dmme;

// ------------------------------------------------------------------ entry points
DMME_API int dmme_rademacher(float* out, int64_t numel, uint64_t seed, uint64_t offset, void* stream) {
    DMME_REQUIRE(out && numel >= 0 && numel < (1ll << 40), DMME_ERR_INVALID, "rademacher: bad argument");
    if (numel == 0) return DMME_OK;
    // one image of one plane: the span's values in element order
    PfDrawArgs a{};
    a.dst = out, a.seed = seed, a.offset = offset, a.chw = numel, a.numel = numel, a.quads = (numel + 3) / 4, a.planes = 1, a.vec = pf_aligned({out}) ? 1 : 0;
    hipLaunchKernelGGL(pf_probe_kernel, dim3((unsigned)((a.quads + kPfThreads - 1) / kPfThreads)), dim3(kPfThreads), 0, (hipStream_t)stream, a);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

DMME_API int dmme_pf_probe(float* d_out, int B, int64_t chw, int out_planes, uint64_t seed, uint64_t offset, void* stream) {
    return launch_pf_probe("pf_probe", d_out, nullptr, seed, offset, B, chw, out_planes, (hipStream_t)stream);
}

DMME_API int dmme_chain_probe_pf(float* d_out, const void* state, int B, int64_t chw, int out_planes, void* stream) {
    DMME_REQUIRE(state, DMME_ERR_INVALID, "chain_probe_pf: null argument");
    return launch_pf_probe("chain_probe_pf", d_out, state, 0, 0, B, chw, out_planes, (hipStream_t)stream);
}

DMME_API int dmme_pf_dequantize(float* x, int64_t numel, uint64_t seed, uint64_t offset, void* stream) {
    return launch_pf_dequantize(x, numel, seed, offset, (hipStream_t)stream);
}

DMME_API int64_t dmme_pf_scratch_floats(int B, int64_t chw) { return B > 0 && chw > 0 ? pf_scratch_floats(B, chw) : 0; }

DMME_API int dmme_pf_dot(const float* d_out, int out_planes, const float* dx, const float* row, int B, int64_t chw, float* scratch, float* s_out, double* acc,
                         void* stream) {
    DMME_REQUIRE(row, DMME_ERR_INVALID, "pf_dot: null argument");
    return launch_pf_dot("pf_dot", d_out, out_planes, dx, row, nullptr, nullptr, B, chw, scratch, s_out, acc, (hipStream_t)stream);
}

DMME_API int dmme_chain_dot_pf(const float* d_out, int out_planes, const float* dx, const float* step_coef, const void* state, int B, int64_t chw,
                               float* scratch, float* s_out, double* acc, void* stream) {
    DMME_REQUIRE(step_coef && state, DMME_ERR_INVALID, "chain_dot_pf: null argument");
    return launch_pf_dot("chain_dot_pf", d_out, out_planes, dx, nullptr, step_coef, state, B, chw, scratch, s_out, acc, (hipStream_t)stream);
}

DMME_API int dmme_pf_prior(const float* x, int B, int64_t chw, float* scratch, double* out, void* stream) {
    return launch_pf_prior(x, B, chw, scratch, out, (hipStream_t)stream);
}

DMME_API int dmme_pf_stage(float* x, const float* model_out, int out_planes, float* xs, float* es, const float* row, int B, int64_t chw, void* stream) {
    DMME_REQUIRE(row, DMME_ERR_INVALID, "pf_stage: null argument");
    return launch_pf_stage("pf_stage", x, model_out, out_planes, xs, es, row, nullptr, nullptr, nullptr, 0, B, chw, (hipStream_t)stream);
}

DMME_API int dmme_chain_stage_pf(float* x, const float* model_out, int out_planes, float* xs, float* es, const float* step_coef, const int64_t* t_table,
                                 void* state, int advance_offset, int B, int64_t chw, void* stream) {
    DMME_REQUIRE(step_coef && t_table && state, DMME_ERR_INVALID, "chain_stage_pf: null argument");
    return launch_pf_stage("chain_stage_pf", x, model_out, out_planes, xs, es, nullptr, step_coef, t_table, state, advance_offset, B, chw, (hipStream_t)stream);
}
