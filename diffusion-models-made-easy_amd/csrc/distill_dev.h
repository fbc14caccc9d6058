// Device helpers shared by the distillation launches (distill.hip: progressive distillation; consistency.hip: consistency distillation):
// the checked student index, a pair of slots of its table row, and the x0 estimate of a network output.  Both tables have 12 floats per
// row with the same first six slots (p0 p1 | p0' p1' | m0 m1), so dmme_distill_noise and dmme_distill_mid serve both methods.
#pragma once
#include "plan.h"

namespace dmme {

constexpr int kDistillRow = 12;  // floats per row of the table: p0 p1 | p0' p1' | m0 m1 | w1 w2 | q0 q1 | two spare

// the student index of image b, or 0 where it lies outside 1..N: index 0 stands for "no row" (the table's row 0 is NaN)
__device__ __forceinline__ int64_t distill_index(const int64_t* __restrict__ idx, int N, int64_t b) {
    const int64_t i = idx[b];
    return (i < 1 || i > N) ? 0 : i;
}
// slots k, k + 1 of row i.  Index 0 is never used as an address: its pair comes out NaN.
__device__ __forceinline__ float2 distill_pair(const float* __restrict__ rows, int64_t i, int k) {
    if (i == 0) return make_float2(__builtin_nanf(""), __builtin_nanf(""));
    return make_float2(rows[kDistillRow * i + k], rows[kDistillRow * i + k + 1]);
}
__device__ __forceinline__ float distill_axpby(float2 c, float a, float b) { return __fadd_rn(__fmul_rn(c.x, a), __fmul_rn(c.y, b)); }
// the teacher's x0 estimate from its output o at the image z it saw: p.x o + p.y z, clamped to [-1, 1] iff clip (a NaN stays a NaN).
// distill_mid and distill_target both form x1 here, so the target's x1 is the one z_m was built from.
__device__ __forceinline__ float distill_x0(float2 p, float o, float z, int clip) {
    const float x = distill_axpby(p, o, z);
    if (!clip) return x;
    return x < -1.f ? -1.f : (x > 1.f ? 1.f : x);
}

}  // namespace dmme
