// Elementwise kernels of the diffusion process: forward noising, DDPM / DDIM updates,
// MSE loss, Philox normals / Dropout2d multipliers.  All HBM-bound, fp32, NCHW.
// The translation unit is compiled with -ffp-contract=off (csrc/Makefile) so each
// expression rounds exactly like the reference's sequence of separate torch ops
// (mul then add, never fma); square roots come from host tables.
#include "common.h"
#include "sampler_dev.h"

#include <type_traits>

namespace dmme {

__global__ void __launch_bounds__(256) randn_kernel(float* out, int64_t numel, uint64_t seed, uint64_t offset) {
    const int64_t quads = (numel + 3) / 4;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
        float z[4];
        normal4(seed, offset + (uint64_t)q, z);
        const int64_t b = q * 4;
        if (b + 3 < numel) {
            *reinterpret_cast<float4*>(out + b) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
            for (int j = 0; j < 4 && b + j < numel; ++j) out[b + j] = z[j];
        }
    }
}

static inline unsigned grid_for(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

int launch_randn(float* out, int64_t numel, uint64_t seed, uint64_t offset, hipStream_t s) {
    if (numel <= 0) return DMME_OK;
    hipLaunchKernelGGL(randn_kernel, dim3(grid_for((numel + 3) / 4)), dim3(256), 0, s, out, numel, seed, offset);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// Dropout2d multipliers: 0 with probability p, else 1/(1-p)  (nn.Dropout2d, models/ddpm.py:29)
__global__ void __launch_bounds__(256) dropmask_kernel(float* out, int64_t numel, float p, uint64_t seed, uint64_t offset) {
    const int64_t quads = (numel + 3) / 4;
    const float keep = 1.0f / (1.0f - p);
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
        uint32_t r[4];
        philox4x32_10(seed, offset + (uint64_t)q, r);
        for (int j = 0; j < 4 && q * 4 + j < numel; ++j) out[q * 4 + j] = (u01(r[j]) <= p) ? 0.0f : keep;
    }
}
int launch_dropmask(float* out, int64_t numel, float p, uint64_t seed, uint64_t offset, hipStream_t s) {
    if (numel <= 0) return DMME_OK;
    hipLaunchKernelGGL(dropmask_kernel, dim3(grid_for((numel + 3) / 4)), dim3(256), 0, s, out, numel, p, seed, offset);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ forward noising
// forward_process + Normal.sample + target re-derivation (see dmme_hip.h)
__global__ void __launch_bounds__(256) q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ z,
                                                       const float* __restrict__ sqrt_abar,
                                                       const float* __restrict__ sqrt_1m_abar,
                                                       const int64_t* __restrict__ t, int64_t chw, int64_t total,
                                                       float* __restrict__ x_t, float* __restrict__ target) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t tn = t[i / chw];
        const float sa = sqrt_abar[tn], sd = sqrt_1m_abar[tn];
        const float mean = sa * x0[i];
        const float xt = mean + sd * z[i];
        x_t[i] = xt;
        if (target) target[i] = (xt - mean) / sd;
    }
}
int launch_q_sample(const float* x0, const float* z, const float* sqrt_abar, const float* sqrt_1m_abar,
                    const int64_t* t, int B, int64_t chw, float* x_t, float* target, hipStream_t s) {
    const int64_t total = (int64_t)B * chw;
    if (total <= 0) return DMME_OK;
    hipLaunchKernelGGL(q_sample_kernel, dim3(grid_for(total)), dim3(256), 0, s, x0, z, sqrt_abar, sqrt_1m_abar, t, chw, total,
                       x_t, target);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ reverse updates
// One element function per sampler kind (DMME_CHAIN_*, dmme_hip.h), used by the eager kernel (host scalars, z from memory) and by the
// chain kernel (scalars from device tables, z drawn in the kernel): the two agree bit for bit because they run the same code.  Every
// operation is explicitly rounded (never contracted into fma): the rounding sequence of the reference's separate torch ops.
//   c0..c3: DDPM  1/sqrt(alpha_t), beta_t/sqrt(1-abar_t), sqrt(beta_t), -      IDDPM  as DDPM, then log beta_t, log max(beta~_t, 1e-12)
//           DDIM  sqrt(1-abar_tau_i), sqrt(abar_tau_{i-1}), -, -               GDDIM  k0, k1, k2, - (dmme_hip.h: dmme_gddim_step)
//           DDPM_GUIDED  as DDPM, then s beta_t                                DDIM_GUIDED  as DDIM, then s sqrt(1-abar_tau_i)
// the DDIM update as the reference ships it: sqrt(abar_prev) * x0_hat, x0_hat = (x - sqrt(1-abar) eps) / sqrt(abar_prev)
__device__ __forceinline__ float ddim_collapse(float x, float e, float c0, float c1) {
    return __fmul_rn(c1, __fdiv_rn(__fsub_rn(x, __fmul_rn(c0, e)), c1));
}
// Sigma = exp(v log beta_t + (1 - v) log max(beta~_t, 1e-12)) (equations/iddpm/losses.py:34-37)
__device__ __forceinline__ float iddpm_std(float v, float log_beta, float log_beta_tilde) {
    return sqrtf(expf(__fadd_rn(__fmul_rn(v, log_beta), __fmul_rn(__fsub_rn(1.0f, v), log_beta_tilde))));
}
// e: predicted noise, v: learned-variance output (IDDPM), g: d log p(y | x_t, t) / d x_t (guided kinds), z: a normal, read where add_noise
template <int KIND>
__device__ __forceinline__ float sampler_update(float x, float e, float v, float g, float z, float c0, float c1, float c2, float c3, int add_noise) {
    if (KIND == DMME_CHAIN_DDIM) return ddim_collapse(x, e, c0, c1);
    if (KIND == DMME_CHAIN_DDIM_GUIDED) return ddim_collapse(x, __fsub_rn(e, __fmul_rn(c2, g)), c0, c1);
    float m;
    if (KIND == DMME_CHAIN_GDDIM) {  // paper form (Song et al. 2021, eq. 12), any eta, either direction: (k0 x + k1 eps) + k2 z
        m = __fadd_rn(__fmul_rn(c0, x), __fmul_rn(c1, e));
    } else {
        m = ddpm_mean(x, e, c0, c1);
        if (KIND == DMME_CHAIN_DDPM_GUIDED) m = __fadd_rn(m, __fmul_rn(c3, g));  // (the shift stays at t == 1)
    }
    return add_noise ? __fadd_rn(m, __fmul_rn(KIND == DMME_CHAIN_IDDPM ? iddpm_std(v, c2, c3) : c2, z)) : m;
}
// DPM-Solver++(2M) (Lu et al. 2022), data-prediction form: the kinds whose update carries state of its own from one step to the next, the
// previous step's x0 prediction, in a buffer of x's layout that the thread owning a quad reads (only where the history is valid: it may hold
// anything before, NaN included) and overwrites.  Per loop index, 8 floats:
//   {q0 = 1/alpha_a, q1 = -sigma_a/alpha_a, k0 = sigma_p/sigma_a, k1 = -alpha_p expm1(-h), w = h / (2 h_prev), clip, s, -}
//   x0 = q0 x + q1 e (clamped to [-1, 1] iff clip);  D = valid ? x0 + w (x0 - x0_prev) : x0;  x' = k0 x + k1 D;  history <- x0
struct DpmppRow {
    float q0, q1, k0, k1, w, clip, s;
};
__device__ __forceinline__ float dpmpp_update(float x, float e, float prev, const DpmppRow& r, bool valid, float& x0) {
    x0 = __fadd_rn(__fmul_rn(r.q0, x), __fmul_rn(r.q1, e));
    if (r.clip != 0.0f) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    const float d = valid ? __fadd_rn(x0, __fmul_rn(r.w, __fsub_rn(x0, prev))) : x0;
    return __fadd_rn(__fmul_rn(r.k0, x), __fmul_rn(r.k1, d));
}
// RePaint (Lugmayr et al. 2022) / SDEdit: one row is a reverse step a -> b, the known image noised to level b, the two blended by the mask,
// and the forward jump b -> c that the walk takes next, folded into one Gaussian.  Per loop index, 8 floats:
//   {c0 = 1/sqrt(alpha), c1 = beta/sqrt(1-abar_a), c2 = sqrt(beta), ka = sqrt(abar_b), ks = sqrt(1-abar_b), r0 = sqrt(abar_c/abar_b), r1 = sqrt(1-abar_c/abar_b), -}
//   u = c0 (x - c1 e) [+ c2 z0];  k = ka x0 [+ ks z1];  y = m k + (1 - m) u;  x' = y, or r0 y + r1 z2: each bracket only where its bit of `used` is set
struct PaintRow {
    float c0, c1, c2, ka, ks, r0, r1;
};
__device__ __forceinline__ float paint_update(float x, float e, float x0, float m, float z0, float z1, float z2, const PaintRow& r, int used) {
    float u = ddpm_mean(x, e, r.c0, r.c1);
    if (used & 1) u = __fadd_rn(u, __fmul_rn(r.c2, z0));
    float k = __fmul_rn(r.ka, x0);
    if (used & 2) k = __fadd_rn(k, __fmul_rn(r.ks, z1));
    const float y = __fadd_rn(__fmul_rn(m, k), __fmul_rn(__fsub_rn(1.0f, m), u));
    return used & 4 ? __fadd_rn(__fmul_rn(r.r0, y), __fmul_rn(r.r1, z2)) : y;
}

// ---- the layer around the arithmetic.  A kind is described once (kind_*, common.h); update_quad<KIND> is the one place that loads a quad's
// operands, mixes the two halves of a classifier-free kind, runs the arithmetic above and stores; eager_kernel<KIND> feeds it a table row and
// a flag from its arguments and normals from memory, chain_kernel<KIND> a row from the device table at the loop index, the flag from the loop
// state and normals drawn in place, and ends in chain_advance, the only writer of the loop state besides chain_set_kernel.
// The loop state and chain_advance: sampler_dev.h.

__global__ void chain_set_kernel(ChainState* st, long long i, const long long* __restrict__ t_table, unsigned long long seed, unsigned long long offset) {
    st->i = i;
    st->t = t_table[i];
    st->offset = offset;
    st->seed = seed;
    st->ticket = 0u;
    st->pad = 0u;
    st->history_valid = 0ull;  // a chain's first step is first order wherever it starts (no other kind reads the word)
}
int launch_chain_set(void* state, int64_t i, const int64_t* t_table, uint64_t seed, uint64_t offset, hipStream_t s) {
    hipLaunchKernelGGL(chain_set_kernel, dim3(1), dim3(1), 0, s, (ChainState*)state, (long long)i, (const long long*)t_table, (unsigned long long)seed,
                       (unsigned long long)offset);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

struct Row {  // one table row: c0..c3 of sampler_update (a classifier-free kind's s in c3), or the DpmppRow / PaintRow and a spare
    float c[8];
};

// the normals of the quad at element b: zeros where the step adds none, else those in `zin` (always given where the kernel does not draw) or,
// without them, the draw at Philox counter `ctr`
template <bool DRAWS>
__device__ __forceinline__ void noise4(bool add_noise, const float* zin, int64_t b, uint64_t seed, uint64_t ctr, float (&z)[4]) {
    z[0] = z[1] = z[2] = z[3] = 0.f;
    if (!add_noise) return;
    if (!DRAWS || zin) {
        const float4 zv = load4(zin + b);
        z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
    } else {
        normal4(seed, ctr, z);
    }
}

// the normals of quad q for every stream of the kind, z[4 s ..] from stream s: memory holds the streams one after another, numel values each
// (the block one dmme_randn of kind_streams * numel values at `off` writes), and the draw of stream s sits at counter off + s n4 + q.
// A single-stream kind calls noise4 the way it always did: through the loop at one trip the same values cost chain_kernel<2> and <7> one more
// scalar spill each (-Rpass-analysis=kernel-resource-usage).
template <int KIND, bool DRAWS>
__device__ __forceinline__ void step_noise(const SamplerOperands& o, int flag, const float* zin, int64_t q, uint64_t seed, uint64_t off,
                                           float (&z)[4 * kind_streams(KIND)]) {
    if constexpr (kind_streams(KIND) == 1) {
        noise4<DRAWS>(kind_draws(KIND, flag, 0), zin, q * 4, seed, off + (uint64_t)q, z);
    } else {
#pragma unroll
        for (int s = 0; s < kind_streams(KIND); ++s)
            noise4<DRAWS>(kind_draws(KIND, flag, s), zin ? zin + s * o.numel : nullptr, q * 4, seed, off + (uint64_t)s * (uint64_t)o.n4 + (uint64_t)q,
                          *reinterpret_cast<float(*)[4]>(z + 4 * s));
    }
}

// quad q of x (a classifier-free kind: of its first half, the result into both; noise and history are indexed by the first half, so such a
// chain at batch B draws exactly what an unguided chain at batch B does).  Every access is 16 bytes, aligned and inside one image: chw % 4 == 0.
// flag: add_noise, (kind_hist) the history is valid, or (kind_paint) the streams the row uses.  The mixed prediction e^ = e_u + s (e_c - e_u) is three separately rounded operations;
// s = 1 is plain conditional sampling (Ho & Salimans' w = s - 1).  The caller has z ready, so nothing loaded here is live across a draw.
template <int KIND>
__device__ __forceinline__ void update_quad(const SamplerOperands& o, int64_t q, const Row& r, int flag, const float (&z)[4 * kind_streams(KIND)]) {
    const int64_t b = q * 4;
    const int planes = kind_planes(KIND) ? kind_planes(KIND) : o.planes;
    const int64_t eo = planes == 2 ? b + (b / o.chw) * o.chw : b;  // [B][2][chw]: the eps plane, then (IDDPM's v) the plane chw further on
    float4 xv = load4(o.x + b), ev = load4(o.out + eo), av = make_float4(0.f, 0.f, 0.f, 0.f);  // av: v, g or the previous x0, by kind
    float *xs = reinterpret_cast<float*>(&xv), *es = reinterpret_cast<float*>(&ev), *as = reinterpret_cast<float*>(&av);
    if constexpr (kind_cfg(KIND)) {
        const float4 uv = load4(o.out + o.n4 * 4 + b);
        const float* us = reinterpret_cast<const float*>(&uv);
#pragma unroll
        for (int j = 0; j < 4; ++j) es[j] = cfg_mix(es[j], us[j], r.c[kind_scol(KIND)]);
    }
    if constexpr (kind_hist(KIND)) {
        const DpmppRow d = {r.c[0], r.c[1], r.c[2], r.c[3], r.c[4], r.c[5], r.c[6]};
        if (flag) av = load4(o.hist + b);
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[j] = dpmpp_update(xs[j], es[j], as[j], d, flag != 0, as[j]);
        *reinterpret_cast<float4*>(o.hist + b) = av;
    } else if constexpr (kind_paint(KIND)) {
        const PaintRow p = {r.c[0], r.c[1], r.c[2], r.c[3], r.c[4], r.c[5], r.c[6]};
        const float4 mv = load4(o.mask + b);
        av = load4(o.known + b);
        const float* ms = reinterpret_cast<const float*>(&mv);
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[j] = paint_update(xs[j], es[j], as[j], ms[j], z[j], z[4 + j], z[8 + j], p, flag);
    } else {
        constexpr bool LEARNED = KIND == DMME_CHAIN_IDDPM;
        if (LEARNED && flag) av = load4(o.out + eo + o.chw);
        if (kind_grad(KIND)) av = load4(o.grad + b);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            xs[j] = sampler_update<kind_base(KIND)>(xs[j], es[j], LEARNED ? as[j] : 0.f, kind_grad(KIND) ? as[j] : 0.f, z[j], r.c[0], r.c[1], r.c[2],
                                                    kind_cfg(KIND) ? 0.f : r.c[3], flag);
    }
    *reinterpret_cast<float4*>(o.x + b) = xv;
    if (kind_cfg(KIND)) *reinterpret_cast<float4*>(o.x + o.n4 * 4 + b) = xv;
}

// The eager update, in place on x: one thread per quad.  The kinds of kind_ragged go element by element where the quad is not whole or
// (IDDPM) does not lie inside one image, aligned in both planes, which it does exactly when chw % 4 == 0.  z is read only where add_noise.
template <int KIND>
__global__ void __launch_bounds__(256) eager_kernel(SamplerOperands o, Row r, int flag) {
    const bool quads_fit = KIND != DMME_CHAIN_IDDPM || o.chw % 4 == 0;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < o.n4; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = q * 4;
        if (!kind_ragged(KIND) || (b + 3 < o.numel && quads_fit)) {
            float z[4 * kind_streams(KIND)];
            step_noise<KIND, false>(o, flag, o.zin, q, 0, 0, z);
            update_quad<KIND>(o, q, r, flag, z);
        } else if constexpr (kind_ragged(KIND)) {
            for (int64_t i = b; i < b + 4 && i < o.numel; ++i) {
                const int64_t eo = KIND == DMME_CHAIN_IDDPM ? i + (i / o.chw) * o.chw : i;
                o.x[i] = sampler_update<KIND>(o.x[i], o.out[eo], KIND == DMME_CHAIN_IDDPM && flag ? o.out[eo + o.chw] : 0.f, 0.f, flag ? o.zin[i] : 0.f,
                                              r.c[0], r.c[1], r.c[2], r.c[3], flag);
            }
        }
    }
}

// The chain form: the row at coef[kind_row * i], the flag from the loop state (t != 1 / c2 != 0 / the row's streams by the kind's noise rule,
// or the history flag), normals drawn at Philox(seed, offset + stream * n4 + quad) unless o.zin is given (the kinds of kind_zin; tests).  The
// offset advances by the quads of the update times the kind's streams at every step, whether or not the step used its normals (the reference
// draws and discards at t == 1).  Every draw of a quad comes before its first load: nothing loaded is live across the sin / cos / log.
// amdgpu_waves_per_eu(8): the draw's sin / cos / log keep the kinds that also branch on zin within a few scalar registers of the 8-wave budget;
// told the target, the scheduler stays inside it (no spill) instead of settling for 7 waves.
template <int KIND>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) chain_kernel(SamplerOperands o, const float* __restrict__ coef, const long long* __restrict__ t_table, ChainState* st) {
    const long long i = st->i, t = st->t;
    const unsigned long long off = st->offset, seed = st->seed;
    Row r;
#pragma unroll
    for (int j = 0; j < kind_row(KIND); ++j) r.c[j] = coef[kind_row(KIND) * i + j];
    const int flag = kind_hist(KIND) ? st->history_valid != 0ull : kind_paint(KIND) ? paint_streams_used(r.c[2], r.c[4], r.c[6]) : kind_adds_noise(KIND, r.c[2], t != 1);
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < o.n4; q += (int64_t)gridDim.x * blockDim.x) {
        float z[4 * kind_streams(KIND)];
        step_noise<KIND, true>(o, flag, kind_zin(KIND) ? o.zin : nullptr, q, seed, off, z);
        update_quad<KIND>(o, q, r, flag, z);
    }
    __syncthreads();
    chain_advance(st, t_table, i, kind_hist(KIND) ? 0ull : (unsigned long long)o.n4 * kind_streams(KIND), kind_hist(KIND));
}

// the run-time kind as a compile-time one: f(std::integral_constant<int, kind>)
template <int K = 0, class F>
static int dispatch_kind(int kind, F&& f) {
    if constexpr (K > DMME_CHAIN_REPAINT) {
        set_error("unknown sampler kind %d", kind);
        return DMME_ERR_INVALID;
    } else {
        return kind == K ? f(std::integral_constant<int, K>{}) : dispatch_kind<K + 1>(kind, f);
    }
}
static int check_operands(const char* what, int kind, const SamplerOperands& o, bool eager) {
    DMME_REQUIRE(kind_known(kind), DMME_ERR_INVALID, "%s: unknown sampler kind %d", what, kind);
    DMME_REQUIRE(o.x && o.out && (o.hist || !kind_hist(kind)) && ((o.known && o.mask) || !kind_paint(kind)) && o.numel > 0 && o.chw > 0, DMME_ERR_INVALID,
                 "%s: bad argument", what);
    DMME_REQUIRE(kind_grad(kind) == (o.grad != nullptr), DMME_ERR_INVALID, "%s: the guided kinds (3, 4) and only they take a gradient", what);
    DMME_REQUIRE(kind_planes(kind) || o.planes == 1 || o.planes == 2, DMME_ERR_INVALID, "%s: a network output of %d planes per image (1: eps, 2: eps and v)",
                 what, o.planes);
    DMME_REQUIRE((eager && kind_ragged(kind)) || o.chw % 4 == 0, DMME_ERR_UNSUPPORTED, "%s: image size %lld is not a multiple of 4", what, (long long)o.chw);
    return DMME_OK;
}
int launch_sampler_eager(const char* what, int kind, const SamplerOperands& o, const float* row, int flag, hipStream_t s) {
    if (kind_ragged(kind) && o.numel <= 0) return DMME_OK;
    if (int rc = check_operands(what, kind, o, true)) return rc;
    DMME_REQUIRE(row, DMME_ERR_INVALID, "%s: null argument", what);
    Row r = {};
    for (int j = 0; j < kind_row(kind); ++j) r.c[j] = row[j];
    if (!kind_hist(kind)) flag = kind_paint(kind) ? paint_streams_used(r.c[2], r.c[4], r.c[6]) : kind_adds_noise(kind, r.c[2], flag);
    DMME_REQUIRE(o.zin || kind_hist(kind) || !flag, DMME_ERR_INVALID, "%s: a step that adds noise needs z", what);
    return dispatch_kind(kind, [&](auto k) -> int {
        constexpr int K = decltype(k)::value;
        if constexpr (kind_grad(K)) {
            set_error("%s: the guided kinds have no eager form", what);
            return DMME_ERR_INVALID;
        } else {
            hipLaunchKernelGGL(eager_kernel<K>, dim3(grid_for(o.n4)), dim3(256), 0, s, o, r, flag);
            DMME_CHECK_LAUNCH();
            return DMME_OK;
        }
    });
}
int launch_sampler_chain(const char* what, int kind, const SamplerOperands& o, const float* coef, const int64_t* t_table, void* state, hipStream_t s) {
    if (int rc = check_operands(what, kind, o, false)) return rc;
    DMME_REQUIRE(coef && t_table && state, DMME_ERR_INVALID, "%s: null argument", what);
    return dispatch_kind(kind, [&](auto k) -> int {
        hipLaunchKernelGGL(chain_kernel<decltype(k)::value>, dim3(grid_for(o.n4)), dim3(256), 0, s, o, coef, (const long long*)t_table, (ChainState*)state);
        DMME_CHECK_LAUNCH();
        return DMME_OK;
    });
}

// ------------------------------------------------------------------ MSE loss (+ gradient)
__global__ void __launch_bounds__(256) mse_partial_kernel(const float* __restrict__ eps, const float* __restrict__ target,
                                                          int64_t numel, float* __restrict__ d_eps, float gscale,
                                                          float* __restrict__ partial) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < numel; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = target[i] - eps[i];
        acc += d * d;
        if (d_eps) d_eps[i] = (-2.0f * d) * gscale;
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(256) mse_final_kernel(const float* partial, int n, float inv_numel, float* loss) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partial[i];
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = tot * inv_numel;
}
int launch_mse(const float* eps, const float* target, int64_t numel, float* loss, float* d_eps, float gscale,
               float* scratch, hipStream_t s) {
    DMME_REQUIRE(numel > 0, DMME_ERR_INVALID, "mse: numel must be positive");
    unsigned g = grid_for(numel);
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(mse_partial_kernel, dim3(g), dim3(256), 0, s, eps, target, numel, d_eps,
                       gscale / (float)numel, scratch);
    DMME_CHECK_LAUNCH();
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, s, scratch, (int)g, 1.0f / (float)numel, loss);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ Improved DDPM (learned variance)
// Hybrid / VLB loss and its gradient w.r.t. the raw network output, one pass (diffusion_models/iddpm.py:62-116,
// equations/iddpm/losses.py:9-98).  coef: per-timestep fp32 table, 8 floats per t:
//   [0] 1/sqrt(alpha_t)  [1] beta_t/sqrt(1-abar_t)  [2] log beta_t  [3] log max(beta~_t, 1e-12)
//   [4] sqrt(abar_{t-1}) beta_t/(1-abar_t)  [5] sqrt(alpha_t)(1-abar_{t-1})/(1-abar_t)  [6] sqrt(beta~_t)  [7] unused
// L_vlb uses the predicted noise with a stop-gradient, so d/d(eps) comes from L_simple only and d/d(v) from L_vlb only.
// one element of the loss: d = target - eps (L_simple's residual), the VLB term and d(VLB term)/dv.  Shared by iddpm_loss_kernel and
// iddpm_loss_rows_kernel, so the two evaluate the same expressions in the same order.
__device__ __forceinline__ void iddpm_loss_elem(const float* __restrict__ c, bool t_is_one, float e, float v, float xt, float x0, float tgt,
                                                float& d, float& vlb, float& dv) {
    d = tgt - e;
    const float mean = c[0] * (xt - c[1] * e);
    const float sd = iddpm_std(v, c[2], c[3]);
    const float hl = 0.5f * (c[2] - c[3]);  // d(sd)/dv = sd * hl
    if (t_is_one) {  // discrete NLL of x_0 in bins of +-1/255 (losses.py:9-20)
        const float ap = (x0 + 1.0f / 255.0f - mean) / sd, am = (x0 - 1.0f / 255.0f - mean) / sd;
        const bool up = x0 < 1.0f, lo = x0 > -1.0f;
        const float Fp = up ? 0.5f * (1.0f + erff(ap * 0.70710678118654752f)) : 1.0f;
        const float Fm = lo ? 0.5f * (1.0f + erff(am * 0.70710678118654752f)) : 0.0f;
        const float prob = Fp - Fm;
        vlb = -logf(fmaxf(prob, 1e-12f));
        const float pp = up ? 0.3989422804014327f * expf(-0.5f * ap * ap) * ap : 0.f;
        const float pm = lo ? 0.3989422804014327f * expf(-0.5f * am * am) * am : 0.f;
        dv = prob >= 1e-12f ? hl * (pp - pm) / prob : 0.f;  // -(1/prob) d(prob)/d(sd) * sd * hl, d Phi(a)/d sd = -phi(a) a / sd
    } else {  // KL(q(x_{t-1} | x_t, x_0) || p_theta) (losses.py:23-31, torch kl_normal_normal)
        const float qm = c[4] * x0 + c[5] * xt;
        const float q = c[6] / sd, ratio = q * q;
        const float u = (qm - mean) / sd, t1 = u * u;
        vlb = 0.5f * (ratio + t1 - 1.0f - logf(ratio));
        dv = hl * (1.0f - ratio - t1);
    }
}
__global__ void __launch_bounds__(256) iddpm_loss_kernel(const float* __restrict__ out, const float* __restrict__ x_t, const float* __restrict__ x_0,
                                                         const float* __restrict__ target, const int64_t* __restrict__ t,
                                                         const float* __restrict__ coef, int64_t chw, int64_t total, float w_simple, float w_vlb,
                                                         float gscale, float* __restrict__ d_out, float* __restrict__ partial) {
    __shared__ float red[16];
    float acc_s = 0.f, acc_v = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / chw, r = i - b * chw;
        const int64_t tt = t[b];
        float d, vlb, dv;
        iddpm_loss_elem(coef + tt * 8, tt == 1, out[b * 2 * chw + r], out[b * 2 * chw + chw + r], x_t[i], x_0[i], target[i], d, vlb, dv);
        acc_s += d * d;
        acc_v += vlb;
        if (d_out) {
            d_out[b * 2 * chw + r] = (-2.0f * d) * (w_simple * gscale);
            d_out[b * 2 * chw + chw + r] = dv * (w_vlb * gscale);
        }
    }
    const float ts = block_sum(acc_s, red);
    __syncthreads();
    const float tv = block_sum(acc_v, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = ts;
        partial[2 * blockIdx.x + 1] = tv;
    }
}
__global__ void __launch_bounds__(256) iddpm_loss_final_kernel(const float* partial, int n, float inv_numel, float w_simple, float w_vlb,
                                                               float* loss) {
    __shared__ float red[16];
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        a += partial[2 * i];
        b += partial[2 * i + 1];
    }
    const float ta = block_sum(a, red);
    __syncthreads();
    const float tb = block_sum(b, red);
    if (threadIdx.x == 0) {
        loss[1] = ta * inv_numel;  // L_simple
        loss[2] = tb * inv_numel;  // L_vlb
        loss[0] = w_simple * loss[1] + w_vlb * loss[2];
    }
}
int launch_iddpm_loss(const float* out, const float* x_t, const float* x_0, const float* target, const int64_t* t, const float* coef, int B,
                      int64_t chw, float w_simple, float w_vlb, float* loss, float* d_out, float gscale, float* scratch, hipStream_t s) {
    const int64_t total = (int64_t)B * chw;
    DMME_REQUIRE(total > 0, DMME_ERR_INVALID, "iddpm_loss: empty batch");
    unsigned g = grid_for(total);
    if (g > 512) g = 512;
    hipLaunchKernelGGL(iddpm_loss_kernel, dim3(g), dim3(256), 0, s, out, x_t, x_0, target, t, coef, chw, total, w_simple, w_vlb,
                       gscale / (float)total, d_out, scratch);
    DMME_CHECK_LAUNCH();
    hipLaunchKernelGGL(iddpm_loss_final_kernel, dim3(1), dim3(256), 0, s, scratch, (int)g, 1.0f / (float)total, w_simple, w_vlb, loss);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ Improved DDPM as published: per-image loss rows, prior, timestep resampler
// (dmme_hip.h: dmme_iddpm_loss_rows, dmme_iddpm_prior_rows, dmme_tsampler_draw, dmme_tsampler_update).  No kernel here uses a value read
// from device memory as an index before it has checked it against the table it indexes.

constexpr int ROWS_MAX_PARTS = 32;  // workgroups per image of iddpm_loss_rows_kernel: `scratch` holds 2 * B * ROWS_MAX_PARTS floats at most
static inline int rows_parts(int64_t chw) {
    const int64_t p = (chw + 1023) / 1024;
    return (int)(p > ROWS_MAX_PARTS ? ROWS_MAX_PARTS : (p < 1 ? 1 : p));
}

// workgroup (b, part) sums its share of image b: partial[(b * parts + part) * 2 + {0, 1}] = sum (target - eps)^2, sum VLB term (plain stores,
// one owner each).  An image whose t is outside [1, T] reads no table row: its gradient rows become NaN and the final pass flags it.
__global__ void __launch_bounds__(256) iddpm_loss_rows_kernel(const float* __restrict__ out, const float* __restrict__ x_t, const float* __restrict__ x_0,
                                                              const float* __restrict__ target, const int64_t* __restrict__ t,
                                                              const float* __restrict__ coef, int T, const float* __restrict__ weight, int parts,
                                                              int64_t chw, float w_simple, float w_vlb, float gscale, float* __restrict__ d_out,
                                                              float* __restrict__ partial) {
    __shared__ float red[16];
    const int64_t b = blockIdx.x / parts;
    const int part = (int)(blockIdx.x - b * parts);
    const int64_t tt = t[b];
    const bool valid = tt >= 1 && tt <= (int64_t)T;
    const float* ob = out + b * 2 * chw;
    float* db = d_out ? d_out + b * 2 * chw : nullptr;
    float acc_s = 0.f, acc_v = 0.f;
    if (valid) {
        const float* c = coef + tt * 8;
        const bool weighted = weight != nullptr;
        const float wb = weighted ? weight[b] : 1.0f;
        for (int64_t r = (int64_t)part * blockDim.x + threadIdx.x; r < chw; r += (int64_t)parts * blockDim.x) {
            const int64_t i = b * chw + r;
            float d, vlb, dv;
            iddpm_loss_elem(c, tt == 1, ob[r], ob[chw + r], x_t[i], x_0[i], target[i], d, vlb, dv);
            acc_s += d * d;
            acc_v += vlb;
            if (db) {
                const float ge = (-2.0f * d) * (w_simple * gscale), gv = dv * (w_vlb * gscale);
                db[r] = weighted ? ge * wb : ge;
                db[chw + r] = weighted ? gv * wb : gv;
            }
        }
    } else if (db) {
        const float nan = __int_as_float(0x7fc00000);
        for (int64_t r = (int64_t)part * blockDim.x + threadIdx.x; r < chw; r += (int64_t)parts * blockDim.x) {
            db[r] = nan;
            db[chw + r] = nan;
        }
    }
    const float ts = block_sum(acc_s, red);
    __syncthreads();
    const float tv = block_sum(acc_v, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = ts;
        partial[2 * blockIdx.x + 1] = tv;
    }
}
// one workgroup: thread b adds image b's partials in index order, then fixed-order block sums over the images
__global__ void __launch_bounds__(256) iddpm_loss_rows_final_kernel(const float* __restrict__ partial, int parts, const int64_t* __restrict__ t, int T,
                                                                    const float* __restrict__ weight, int B, float inv_chw, float w_simple,
                                                                    float w_vlb, float* __restrict__ loss, float* __restrict__ rows,
                                                                    int* __restrict__ status) {
    __shared__ float red[16];
    const float nan = __int_as_float(0x7fc00000);
    float a_s = 0.f, a_v = 0.f, a_w = 0.f;
    bool bad = false;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const int64_t tt = t[b];
        float S = 0.f, V = 0.f;
        for (int p = 0; p < parts; ++p) {
            S += partial[2 * ((int64_t)b * parts + p)];
            V += partial[2 * ((int64_t)b * parts + p) + 1];
        }
        S *= inv_chw;
        V *= inv_chw;
        if (tt < 1 || tt > (int64_t)T) {
            S = nan;
            V = nan;
            bad = true;
        }
        const float row = w_simple * S + w_vlb * V;
        rows[b] = S;
        rows[B + b] = V;
        rows[2 * B + b] = row;
        a_s += S;
        a_v += V;
        a_w += weight ? weight[b] * row : row;
    }
    if (bad && status) *status = 1;
    const float ts = block_sum(a_s, red);
    const float tv = block_sum(a_v, red);
    const float tw = block_sum(a_w, red);
    if (threadIdx.x == 0) {
        const float inv_b = 1.0f / (float)B;
        loss[0] = tw * inv_b;
        loss[1] = ts * inv_b;
        loss[2] = tv * inv_b;
    }
}
int launch_iddpm_loss_rows(const float* out, const float* x_t, const float* x_0, const float* target, const int64_t* t, const float* coef, int T,
                           const float* weight, int B, int64_t chw, float w_simple, float w_vlb, float* loss, float* rows, float* d_out,
                           float gscale, int* status, float* scratch, hipStream_t s) {
    DMME_REQUIRE(out && x_t && x_0 && target && t && coef && loss && rows && scratch, DMME_ERR_INVALID, "iddpm_loss_rows: null argument");
    DMME_REQUIRE(B > 0 && chw > 0 && T >= 1, DMME_ERR_INVALID, "iddpm_loss_rows: B = %d images of %lld values, T = %d", B, (long long)chw, T);
    const int parts = rows_parts(chw);
    DMME_REQUIRE((int64_t)B * parts <= 0x7fffffff, DMME_ERR_INVALID, "iddpm_loss_rows: B = %d is too large", B);
    const int64_t total = (int64_t)B * chw;
    hipLaunchKernelGGL(iddpm_loss_rows_kernel, dim3((unsigned)(B * parts)), dim3(256), 0, s, out, x_t, x_0, target, t, coef, T, weight, parts, chw,
                       w_simple, w_vlb, gscale / (float)total, d_out, scratch);
    DMME_CHECK_LAUNCH();
    hipLaunchKernelGGL(iddpm_loss_rows_final_kernel, dim3(1), dim3(256), 0, s, (const float*)scratch, parts, t, T, weight, B, 1.0f / (float)chw,
                       w_simple, w_vlb, loss, rows, status);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// prior[b] = 0.5 (k + abar_T mean(x_0^2)), k = -log(1 - abar_T) - abar_T: one workgroup per image.  k is evaluated on the host in double
// (log1p: the three constant terms of the KL cancel to ~abar_T^2 / 2, far below fp32 next to 1).
__global__ void __launch_bounds__(256) iddpm_prior_rows_kernel(const float* __restrict__ x_0, int64_t chw, double k, double abar,
                                                               float* __restrict__ prior) {
    __shared__ float red[16];
    const float* xb = x_0 + (int64_t)blockIdx.x * chw;
    float acc = 0.f;
    for (int64_t r = threadIdx.x; r < chw; r += blockDim.x) acc += xb[r] * xb[r];
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) prior[blockIdx.x] = (float)(0.5 * (k + abar * ((double)tot / (double)chw)));
}
int launch_iddpm_prior_rows(const float* x_0, int B, int64_t chw, float alpha_bar_T, float* prior, hipStream_t s) {
    DMME_REQUIRE(x_0 && prior, DMME_ERR_INVALID, "iddpm_prior_rows: null argument");
    DMME_REQUIRE(B > 0 && chw > 0, DMME_ERR_INVALID, "iddpm_prior_rows: B = %d images of %lld values", B, (long long)chw);
    DMME_REQUIRE(alpha_bar_T >= 0.0f && alpha_bar_T < 1.0f, DMME_ERR_INVALID, "iddpm_prior_rows: alpha_bar_T = %g is outside [0, 1)", (double)alpha_bar_T);
    const double ab = (double)alpha_bar_T;
    hipLaunchKernelGGL(iddpm_prior_rows_kernel, dim3((unsigned)B), dim3(256), 0, s, x_0, chw, -log1p(-ab) - ab, ab, prior);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// Loss-second-moment timestep resampler (Nichol & Dhariwal 2021, section 3.3).  One workgroup: (1) warm iff every count[1..T] == H;
// (2) s_t = sqrt(mean_k hist[t][k]^2), p_t = (1 - u0) s_t / sum(s) + u0 / T, or 1 / T while not warm (or where sum(s) is not a positive
// finite number); (3) inclusive fp32 prefix sum of p in LDS: every thread owns a contiguous chunk, sums it from zero, one thread scans
// the chunk sums, and cdf = chunk offset + running chunk sum, which is non-decreasing across chunk borders too; (4) draw b takes
// u = uniform b of the Philox span (seed, offset) and t_b = 1 + #{t : cdf_t <= u cdf_T} by bisection, clamped to [1, T].
constexpr int TSAMPLER_MAX_T = 12288;  // the cdf lives in LDS: 48 KiB
__global__ void __launch_bounds__(256) tsampler_draw_kernel(const float* __restrict__ hist, const int* __restrict__ count, int T, int H, float u0,
                                                            uint64_t seed, uint64_t offset, int B, int64_t* __restrict__ t_out,
                                                            float* __restrict__ w_out, float* __restrict__ p_out) {
    extern __shared__ float cdf[];  // [T + 1]: s_t, then p_t, then the prefix sums; entry 0 stays 0
    __shared__ float red[16];
    __shared__ float chunk_off[257];
    __shared__ int cold;
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) {
        cold = 0;
        cdf[0] = 0.f;
    }
    __syncthreads();
    bool mine_cold = false;
    for (int t = 1 + tid; t <= T; t += nt) mine_cold |= count[t] != H;
    if (mine_cold) cold = 1;  // (every writer stores the same value)
    __syncthreads();
    bool warm = cold == 0;
    float acc = 0.f;
    if (warm) {
        for (int t = 1 + tid; t <= T; t += nt) {
            const float* row = hist + (int64_t)t * H;
            float q = 0.f;
            for (int k = 0; k < H; ++k) q += row[k] * row[k];
            const float s = sqrtf(q / (float)H);
            cdf[t] = s;
            acc += s;
        }
    }
    const float sum_s = block_sum(acc, red);
    warm = warm && sum_s > 0.f && sum_s <= 3.0e38f;  // (false for NaN)
    const float uni = 1.0f / (float)T;
    for (int t = 1 + tid; t <= T; t += nt) {
        const float p = warm ? (1.0f - u0) * cdf[t] / sum_s + u0 / (float)T : uni;
        cdf[t] = p;
        p_out[t] = p;
    }
    if (tid == 0) p_out[0] = 0.f;
    __threadfence_block();
    __syncthreads();
    const int per = (T + nt - 1) / nt, lo = 1 + tid * per, hi = min(T, lo + per - 1);
    float run = 0.f;
    for (int t = lo; t <= hi; ++t) run += cdf[t];
    chunk_off[tid + 1] = run;
    __syncthreads();
    if (tid == 0) {
        chunk_off[0] = 0.f;
        for (int k = 1; k <= nt; ++k) chunk_off[k] = chunk_off[k - 1] + chunk_off[k];
    }
    __syncthreads();
    const float base = chunk_off[tid];
    run = 0.f;
    for (int t = lo; t <= hi; ++t) {
        run += cdf[t];
        cdf[t] = base + run;
    }
    __syncthreads();
    const float top = cdf[T];
    for (int b = tid; b < B; b += nt) {
        uint32_t r[4];
        philox4x32_10(seed, offset + (uint64_t)(b >> 2), r);
        const float x = u01(r[b & 3]) * top;
        int a = 1, e = T + 1;  // first t in [1, T + 1) with cdf[t] > x; T + 1 when there is none
        while (a < e) {
            const int m = (a + e) >> 1;
            if (cdf[m] <= x) a = m + 1; else e = m;
        }
        const int tb = a > T ? T : a;  // 1 + #{t : cdf_t <= x}, kept inside the table
        t_out[b] = tb;
        w_out[b] = warm ? 1.0f / ((float)T * p_out[tb]) : 1.0f;
    }
}
int launch_tsampler_draw(const float* hist, const int* count, int T, int H, float uniform_prob, uint64_t seed, uint64_t offset, int B, int64_t* t,
                         float* weight, float* p, hipStream_t s) {
    DMME_REQUIRE(hist && count && t && weight && p, DMME_ERR_INVALID, "tsampler_draw: null argument");
    DMME_REQUIRE(B > 0 && T >= 1 && H >= 1, DMME_ERR_INVALID, "tsampler_draw: B = %d, T = %d, H = %d", B, T, H);
    DMME_REQUIRE(uniform_prob >= 0.0f && uniform_prob <= 1.0f, DMME_ERR_INVALID, "tsampler_draw: uniform_prob = %g is outside [0, 1]", (double)uniform_prob);
    DMME_REQUIRE(T <= TSAMPLER_MAX_T, DMME_ERR_UNSUPPORTED, "tsampler_draw: T = %d is above %d", T, TSAMPLER_MAX_T);
    hipLaunchKernelGGL(tsampler_draw_kernel, dim3(1), dim3(256), (size_t)(T + 1) * sizeof(float), s, hist, count, T, H, uniform_prob, seed, offset, B,
                       t, weight, p);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// push (t_b, L_b), b = 0 .. B-1, in index order: the thread that owns timestep t walks the batch and is the only writer of row t and
// count[t].  count[t] is clamped to [0, H] before it positions a store.  The owner of t = 1 also flags the entries nobody takes.
__global__ void __launch_bounds__(256) tsampler_update_kernel(float* __restrict__ hist, int* __restrict__ count, int T, int H,
                                                              const int64_t* __restrict__ t, const float* __restrict__ L, int B,
                                                              int* __restrict__ status) {
    const int own = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    if (own > T) return;
    float* row = hist + (int64_t)own * H;
    int c = count[own];
    c = c < 0 ? 0 : (c > H ? H : c);
    bool bad = false;
    for (int b = 0; b < B; ++b) {
        const int64_t tb = t[b];
        const float v = L[b];
        const bool finite = fabsf(v) <= 3.4028234e38f;  // (false for NaN)
        if (own == 1 && (tb < 1 || tb > (int64_t)T || !finite)) bad = true;
        if (tb != (int64_t)own || !finite) continue;
        if (c < H) {
            row[c++] = v;
        } else {
            for (int k = 0; k + 1 < H; ++k) row[k] = row[k + 1];
            row[H - 1] = v;
        }
    }
    count[own] = c;
    if (bad && status) *status = 1;
}
int launch_tsampler_update(float* hist, int* count, int T, int H, const int64_t* t, const float* L, int B, int* status, hipStream_t s) {
    DMME_REQUIRE(hist && count && t && L, DMME_ERR_INVALID, "tsampler_update: null argument");
    DMME_REQUIRE(B > 0 && T >= 1 && H >= 1, DMME_ERR_INVALID, "tsampler_update: B = %d, T = %d, H = %d", B, T, H);
    hipLaunchKernelGGL(tsampler_update_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, hist, count, T, H, t, L, B, status);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}


// Label dropout of classifier-free training: out[b] = K (the null label) where u_b < p, else labels[b]; u_b = u01(word b % 4 of the quad at
// counter offset + b / 4), the layout of a span (seed, offset, B) of the stream (dmme_hip.h).  p >= 1 drops every label (u = 1 is on the grid).
// A label outside [0, K] is copied through and sets *status (nullable).
__global__ void __launch_bounds__(256) label_dropout_kernel(const int64_t* __restrict__ labels, int B, int K, float p, uint64_t seed, uint64_t offset,
                                                            int64_t* __restrict__ out, int* status) {
    const int quads = (B + 3) / 4;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        uint32_t r[4];
        philox4x32_10(seed, offset + (uint64_t)q, r);
        for (int j = 0; j < 4 && q * 4 + j < B; ++j) {
            const int64_t y = labels[q * 4 + j];
            if ((y < 0 || y > (int64_t)K) && status) atomicExch(status, 1);
            out[q * 4 + j] = (u01(r[j]) < p || p >= 1.0f) ? (int64_t)K : y;
        }
    }
}
int launch_label_dropout(const int64_t* labels, int B, int K, float p, uint64_t seed, uint64_t offset, int64_t* out, int* status, hipStream_t s) {
    DMME_REQUIRE(labels && out && B > 0 && K >= 1 && p >= 0.0f && p <= 1.0f, DMME_ERR_INVALID, "label_dropout: bad argument (B = %d, K = %d, p = %g)", B, K, (double)p);
    hipLaunchKernelGGL(label_dropout_kernel, dim3(grid_for((B + 3) / 4)), dim3(256), 0, s, labels, B, K, p, seed, offset, out, status);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ spherical interpolation of latents (dmme_hip.h: dmme_slerp)
// Two launches.  (1) per image pair, <xa, xb>, |xa|^2 and |xb|^2: `parts` blocks per image each leave three partial sums
// (float4 loads, wave / block sums; stores, no atomics: the result does not depend on arrival order).  (2) every block of the
// blend sums its image's partials, turns them and a tile of up to SLERP_TILE weights into the two coefficients per weight
// (the handful of acos / sin per block runs in double), then streams its share of the image: xa and xb are loaded once per
// weight tile and each weight's output is written from registers.
constexpr int SLERP_TILE = 64;
constexpr int SLERP_MAX_PARTS = 256;

__global__ void __launch_bounds__(256) slerp_dots_kernel(const float* __restrict__ xa, const float* __restrict__ xb, int64_t chw4,
                                                         float* __restrict__ partial) {
    __shared__ float red[16];
    const int64_t base = (int64_t)blockIdx.y * chw4 * 4;
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < chw4; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 a = *reinterpret_cast<const float4*>(xa + base + q * 4);
        const float4 b = *reinterpret_cast<const float4*>(xb + base + q * 4);
        ab += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
        aa += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
        bb += b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
    }
    const float s0 = block_sum(ab, red);
    const float s1 = block_sum(aa, red);
    const float s2 = block_sum(bb, red);
    if (threadIdx.x == 0) {
        float* p = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        p[0] = s0;
        p[1] = s1;
        p[2] = s2;
    }
}

__global__ void __launch_bounds__(256) slerp_blend_kernel(const float* __restrict__ xa, const float* __restrict__ xb, const float* __restrict__ w,
                                                          int n, int64_t chw4, const float* __restrict__ partial, int parts,
                                                          float* __restrict__ out) {
    __shared__ float red[16];
    __shared__ float ca[SLERP_TILE], cb[SLERP_TILE];
    const int B = gridDim.y;
    const int64_t img = blockIdx.y, base = img * chw4 * 4;
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int p = threadIdx.x; p < parts; p += blockDim.x) {
        const float* v = partial + (img * parts + p) * 3;
        ab += v[0];
        aa += v[1];
        bb += v[2];
    }
    const float dot = block_sum(ab, red);
    const float na2 = block_sum(aa, red);
    const float nb2 = block_sum(bb, red);
    double cosv = (double)dot / (sqrt((double)na2) * sqrt((double)nb2));  // (a zero image: NaN, which takes the linear form below)
    cosv = cosv > 1.0 ? 1.0 : (cosv < -1.0 ? -1.0 : cosv);
    const double theta = acos(cosv), sn = sin(theta);
    const bool linear = !(sn >= 1e-6);
    for (int j0 = 0; j0 < n; j0 += SLERP_TILE) {
        const int nt = n - j0 < SLERP_TILE ? n - j0 : SLERP_TILE;
        __syncthreads();  // the previous tile's coefficients have been read
        if ((int)threadIdx.x < nt) {
            const double wj = (double)w[j0 + threadIdx.x];
            ca[threadIdx.x] = (float)(linear ? 1.0 - wj : sin((1.0 - wj) * theta) / sn);
            cb[threadIdx.x] = (float)(linear ? wj : sin(wj * theta) / sn);
        }
        __syncthreads();
        for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < chw4; q += (int64_t)gridDim.x * blockDim.x) {
            const float4 a = *reinterpret_cast<const float4*>(xa + base + q * 4);
            const float4 b = *reinterpret_cast<const float4*>(xb + base + q * 4);
            for (int j = 0; j < nt; ++j) {
                const float fa = ca[j], fb = cb[j];
                float4 o;
                o.x = fa * a.x + fb * b.x;
                o.y = fa * a.y + fb * b.y;
                o.z = fa * a.z + fb * b.z;
                o.w = fa * a.w + fb * b.w;
                *reinterpret_cast<float4*>(out + ((int64_t)(j0 + j) * B + img) * chw4 * 4 + q * 4) = o;
            }
        }
    }
}

int slerp_parts(int64_t chw) {
    const int64_t p = (chw / 4 + 255) / 256;
    return (int)(p > SLERP_MAX_PARTS ? SLERP_MAX_PARTS : (p < 1 ? 1 : p));
}

int launch_slerp(const float* xa, const float* xb, const float* w, int n, int B, int64_t chw, float* out, float* scratch, hipStream_t s) {
    DMME_REQUIRE(n > 0 && B > 0 && B <= 65535 && chw > 0, DMME_ERR_INVALID, "slerp: n = %d weights, B = %d images of %lld values", n, B, (long long)chw);
    DMME_REQUIRE(chw % 4 == 0, DMME_ERR_INVALID, "slerp: image size %lld is not a multiple of 4", (long long)chw);
    const int parts = slerp_parts(chw);
    hipLaunchKernelGGL(slerp_dots_kernel, dim3(parts, B), dim3(256), 0, s, xa, xb, chw / 4, scratch);
    DMME_CHECK_LAUNCH();
    hipLaunchKernelGGL(slerp_blend_kernel, dim3(parts, B), dim3(256), 0, s, xa, xb, w, n, chw / 4, (const float*)scratch, parts, out);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ input pipeline: HBM-resident uint8 dataset -> training batch
// out[b][c][y][x] = norm(ToTensor(flip_b(data[idx[b]])))[c][y][x]: torchvision's ToTensor (uint8 -> float / 255) followed by the
// reference's norm, (x - 0.5) * 2 (src/dmme/common/norm.py:4-6), and RandomHorizontalFlip as a per-image bit
// (data_modules/cifar10.py:33-44).  data: [n_images][C][H][W] uint8 (the CIFAR10 pickle's own layout).  One thread per 4 pixels.
__global__ void __launch_bounds__(256) image_batch_kernel(const uint8_t* __restrict__ data, const int64_t* __restrict__ idx,
                                                          const uint8_t* __restrict__ flip, int C, int H, int W, int64_t total4,
                                                          float* __restrict__ out) {
    const int W4 = W / 4;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total4; q += (int64_t)gridDim.x * blockDim.x) {
        const int x4 = (int)(q % W4);
        int64_t r = q / W4;
        const int y = (int)(r % H);
        r /= H;
        const int c = (int)(r % C), b = (int)(r / C);
        const uint8_t* row = data + ((idx[b] * C + c) * H + y) * (int64_t)W;
        const bool fl = flip && flip[b];
        const uint32_t raw = *reinterpret_cast<const uint32_t*>(row + (fl ? W - 4 - 4 * x4 : 4 * x4));
        float4 o;
        float* ov = reinterpret_cast<float*>(&o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t u = (raw >> (8 * (fl ? 3 - j : j))) & 0xffu;
            ov[j] = __fmul_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), 0.5f), 2.0f);
        }
        *reinterpret_cast<float4*>(out + (((int64_t)b * C + c) * H + y) * W + 4 * x4) = o;
    }
}
int launch_image_batch(const uint8_t* data, const int64_t* idx, const uint8_t* flip, int B, int C, int H, int W, float* out, hipStream_t s) {
    DMME_REQUIRE(W % 4 == 0, DMME_ERR_UNSUPPORTED, "image_batch: width %d is not a multiple of 4", W);
    const int64_t total4 = (int64_t)B * C * H * (W / 4);
    if (total4 <= 0) return DMME_OK;
    hipLaunchKernelGGL(image_batch_kernel, dim3(grid_for(total4)), dim3(256), 0, s, data, idx, flip, C, H, W, total4, out);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

// ------------------------------------------------------------------ output side: an image batch into the cells of a grid canvas
// canvas[cg][row*(H+pad)+pad+y][col*(W+pad)+pad+x] = value(x[b][c][y][x]) with cell = cell0 + b*cell_stride, row = cell / xmaps,
// col = cell % xmaps: torchvision's make_grid layout (a single channel written to all three).  value: the reference's denorm,
// clip((x + 1) / 2, 0, 1) (src/dmme/common/norm.py:9-11), or x itself where `raw`; as fp32 or as save_image's byte
// (uint8) clamp(v * 255 + 0.5, 0, 255).  Separately rounded adds and multiplies: both forms match numpy float32 bit for bit.  Image
// pixels only: the padding keeps what the canvas held.  One thread per source pixel; canvas rows have no alignment to rely on
// (width xmaps*(W+pad)+pad), so the stores are scalar.
template <typename OUT>
__global__ void __launch_bounds__(256) grid_tile_kernel(const float* __restrict__ x, int C, int H, int W, int64_t total, int cell0, int cell_stride,
                                                        int xmaps, int pad, int raw, int64_t gw, int64_t plane, OUT* __restrict__ canvas) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int px = (int)(q % W);
        int64_t r = q / W;
        const int py = (int)(r % H);
        r /= H;
        const int c = (int)(r % C), b = (int)(r / C);
        float v = x[q];
        if (!raw) {
            v = __fmul_rn(__fadd_rn(v, 1.0f), 0.5f);
            v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
        }
        OUT o;
        if constexpr (sizeof(OUT) == 1) {
            const float s = __fadd_rn(__fmul_rn(v, 255.0f), 0.5f);
            o = (OUT)(s >= 255.0f ? 255.0f : (s > 0.0f ? s : 0.0f));  // (a NaN becomes 0)
        } else {
            o = v;
        }
        const int64_t cell = cell0 + (int64_t)b * cell_stride;
        const int64_t at = ((cell / xmaps) * (H + pad) + pad + py) * gw + (cell % xmaps) * (int64_t)(W + pad) + pad + px;
        if (C == 1) {
            canvas[at] = o;
            canvas[plane + at] = o;
            canvas[2 * plane + at] = o;
        } else {
            canvas[c * plane + at] = o;
        }
    }
}
int launch_grid_tile(const float* x, int B, int C, int H, int W, int cell0, int cell_stride, int xmaps, int ymaps, int pad, int out_kind, int raw,
                     void* canvas, hipStream_t s) {
    const int64_t total = (int64_t)B * C * H * W;
    const int64_t gw = (int64_t)xmaps * (W + pad) + pad, plane = ((int64_t)ymaps * (H + pad) + pad) * gw;
    if (out_kind == 1)
        hipLaunchKernelGGL(grid_tile_kernel<uint8_t>, dim3(grid_for(total)), dim3(256), 0, s, x, C, H, W, total, cell0, cell_stride, xmaps, pad, raw, gw, plane,
                           (uint8_t*)canvas);
    else
        hipLaunchKernelGGL(grid_tile_kernel<float>, dim3(grid_for(total)), dim3(256), 0, s, x, C, H, W, total, cell0, cell_stride, xmaps, pad, raw, gw, plane,
                           (float*)canvas);
    DMME_CHECK_LAUNCH();
    return DMME_OK;
}

}  // namespace dmme
