// Device pieces shared by the translation units that hold sampler updates (kernels_sampler.hip: the kinds of common.h's table; ilvr.hip,
// ddnm.hip, dps.hip, pfode.hip: the updates of the conditioned chain samplers): the Philox normals, DDPM's mean, the loop state of a
// replayable chain, its cursor and its advance, a step's normals and the eps plane of a network output.  Every translation unit that
// includes this is compiled with -ffp-contract=off (csrc/Makefile).
#pragma once
#include "common.h"

namespace dmme {

// ------------------------------------------------------------------ Philox4x32-10
struct Philox {
    uint32_t c[4];
    uint32_t k[2];
};
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0;
    c[1] = n1;
    c[2] = n2;
    c[3] = n3;
}
__device__ __forceinline__ void philox4x32_10(uint64_t seed, uint64_t ctr, uint32_t (&out)[4]) {
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c[0];
    out[1] = c[1];
    out[2] = c[2];
    out[3] = c[3];
}
__device__ __forceinline__ float u01(uint32_t x) {  // (0, 1]
    return ((float)(x >> 8) + 1.0f) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ void normal4(uint64_t seed, uint64_t ctr, float (&z)[4]) {
    uint32_t r[4];
    philox4x32_10(seed, ctr, r);
    const float r0 = sqrtf(-2.0f * logf(u01(r[0]))), a0 = 6.283185307179586f * u01(r[1]);
    const float r1 = sqrtf(-2.0f * logf(u01(r[2]))), a1 = 6.283185307179586f * u01(r[3]);
    z[0] = r0 * cosf(a0);
    z[1] = r0 * sinf(a0);
    z[2] = r1 * cosf(a1);
    z[3] = r1 * sinf(a1);
}

// DDPM's mean, every operation explicitly rounded (never contracted into fma): c0 = 1/sqrt(alpha_t), c1 = beta_t/sqrt(1-abar_t)
__device__ __forceinline__ float ddpm_mean(float x, float e, float c0, float c1) { return __fmul_rn(c0, __fsub_rn(x, __fmul_rn(c1, e))); }
__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// The replayable chain step (hipGraph-friendly sampling loops): everything that changes from one denoising step to the next lives in DEVICE
// memory, so the launch sequence of a step is the same every time and can be replayed from one captured graph: the loop state {i,
// t = t_table[i], Philox offset and seed, ticket, history flag}, the per-index scalars of the update (`coef[i]`) and the noise itself (drawn
// from the same Philox stream / offsets dmme_randn would use: the chain is bit-identical to the eager loop under the same seed).
struct ChainState {
    long long i;
    long long t;
    unsigned long long offset;
    unsigned long long seed;
    unsigned int ticket, pad;
    unsigned long long history_valid;  // DPM-Solver++ kinds: the history buffer holds the x0 prediction of this chain's previous step
    unsigned long long reserved[2];
};
static_assert(sizeof(ChainState) == 64, "ChainState is eight 64-bit words (dmme_hip.h: dmme_chain_*)");

// The top of a step's kernel, eager or chain: the row of the update's scalars, from the arguments (eager: `eager_row`, index 0, no stream) or
// from the table at the loop state's index (chain), with the Philox stream's place.  Every thread calls this in front of the block's first
// barrier: that all of them have read the state before any block takes its ticket is what chain_advance relies on.
struct ChainCursor {
    const float* row;
    long long i;
    unsigned long long seed, off;
};
__device__ __forceinline__ ChainCursor chain_cursor(const ChainState* st, const float* coef, const float* eager_row) {
    ChainCursor k{eager_row, 0, 0ull, 0ull};
    if (st) {
        k.i = st->i, k.seed = st->seed, k.off = st->offset;
        k.row = coef + 8 * k.i;
    }
    return k;
}

// the normals of stream `stream` for the quad at `element`: from memory where given (zin: [streams][numel]), else the draw at Philox counter
// off + stream n4 + element / 4, which is where dmme_randn over the step's span puts them
__device__ __forceinline__ void chain_noise4(const float* zin, int64_t numel, int64_t n4, unsigned long long seed, unsigned long long off, int stream,
                                             int64_t element, float (&z)[4]) {
    if (zin) {
        const float4 v = load4(zin + stream * numel + element);
        z[0] = v.x, z[1] = v.y, z[2] = v.z, z[3] = v.w;
    } else {
        normal4(seed, off + (uint64_t)stream * (uint64_t)n4 + (uint64_t)(element >> 2), z);
    }
}

// where element e of the images sits in a network output of `planes` chw-sized planes per image, the eps plane first
__device__ __forceinline__ int64_t eps_index(int64_t e, int64_t chw, int planes) { return planes == 1 ? e : e + (e / chw) * (int64_t)(planes - 1) * chw; }

// The end of a chain kernel, after the block's __syncthreads(): every thread of this block has read the state (and is past its loads of it).
// The block that takes the last ticket has, by construction, run after every block read the state (all others took their ticket after
// reading it), and moves it on: i -= 1 (not below 0), t = t_table[i], offset += offset_inc, the history flag raised where asked.
__device__ __forceinline__ void chain_advance(ChainState* st, const long long* __restrict__ t_table, long long i, unsigned long long offset_inc,
                                              bool raise_history) {
    if (threadIdx.x != 0) return;
    const unsigned tk = atomicAdd(&st->ticket, 1u);
    if (tk != gridDim.x - 1) return;
    const long long ni = i > 0 ? i - 1 : 0;
    st->i = ni;
    st->t = t_table[ni];
    if (offset_inc) st->offset += offset_inc;
    if (raise_history) st->history_valid = 1ull;
    atomicExch(&st->ticket, 0u);
}

}  // namespace dmme
