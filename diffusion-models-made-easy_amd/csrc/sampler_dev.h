// Device pieces shared by the translation units that hold sampler updates (kernels_sampler.hip: the kinds of common.h's table; ilvr.hip:
// the plane-wise ILVR update): the Philox normals, DDPM's mean, the loop state of a replayable chain and its advance.  Every translation
// unit that includes this is compiled with -ffp-contract=off (csrc/Makefile).
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
