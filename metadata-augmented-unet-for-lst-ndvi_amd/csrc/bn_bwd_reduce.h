// bn_bwd_reduce.h -- one element of the BatchNorm + ReLU backward's reduce pass (partial sums of dz and dz * xhat), the ONE copy of
// its rounding, and the workgroup's join of those sums into its slab row: bn.hip's bn_relu_bwd_reduce_kernel and the fused reduce
// kernels of bn_fused.hip all go through them, so a layer's sums have the same bits whichever of them produces them
// (tests/test_gpu_ops.py::test_fused_bn_backward_matches_unfused).  The apply pass's counterpart is bn_bwd_apply.h.
#pragma once
#include "mau_common.h"

namespace mau {

// coefficients of 8 channels starting at c0 (zeros beyond C).  CHECKED: mean / invstd may be null and then give zeros (the forward
// kernels pass none; the fused reduce kernels were measured with the tests in place); load<false> reads all four unconditionally
struct Coef8 {
  float sc[8], sh[8], mu[8], is[8];
  template <bool CHECKED = true>
  __device__ __forceinline__ void load(const float* scale, const float* shift, const float* mean, const float* invstd, int c0, int C) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sc[j] = coef(scale, c0 + j, C);
      sh[j] = coef(shift, c0 + j, C);
      mu[j] = (!CHECKED || mean) ? coef(mean, c0 + j, C) : 0.f;
      is[j] = (!CHECKED || invstd) ? coef(invstd, c0 + j, C) : 0.f;
    }
  }
};

// y and the gradient g arriving at the activation, 8 channels of one pixel:  dz = g where relu(scale * y + shift) is open;
// s1 += dz;  s2 += dz * xhat, xhat = (y - mu) * is -- the product rounded on its own, the sum one explicit FMA
__device__ __forceinline__ void bn_bwd_accumulate8(const Coef8& k, const F8& v, const F8& g, float (&s1)[8], float (&s2)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float act = fmaf(v.v[j], k.sc[j], k.sh[j]);
    const float dz = act > 0.f ? g.v[j] : 0.f;
    s1[j] += dz;
    s2[j] = fmaf(dz, (v.v[j] - k.mu[j]) * k.is[j], s2[j]);
  }
}

// ---- packed fp32 (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 on gfx950): two channels per vector instruction ----
// Every operation below is the IEEE operation its scalar spelling is (fused multiply-add, multiply, add; conversions per element), so a
// kernel written on pairs returns the bits of the scalar one -- what it saves is issue slots: the head's backward reduce ran ~215 vector
// instructions per 8-channel vector (75 of them v_mov shuffling values into and out of the pairs the SLP vectoriser formed), i.e. it was
// bound by VALU issue (~90 us of pure issue at B = 32 x 256 x 256), not by its 302 MB of traffic.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 splat(float v) { return f2{v, v}; }

// bn_bwd_accumulate8 on a pair of channels -- same operations, same order, same bits.  `act` = pk_fma(v, sc, sh) comes from the
// caller (head_bn_bwd_reduce_kernel, which needs it for the head's own sums as well).
__device__ __forceinline__ void bn_bwd_accumulate2(f2 act, f2 v, f2 g, f2 mu, f2 is, f2& s1, f2& s2) {
  const f2 dz = f2{act[0] > 0.f ? g[0] : 0.f, act[1] > 0.f ? g[1] : 0.f};
  s1 += dz;
  s2 = pk_fma(dz, (v - mu) * is, s2);
}

// the LDS join of the reduce kernels: (8 channel vectors) x (32 pixel slots) -> one slab row [2][ldslab] per workgroup
__device__ __forceinline__ void bn_sums_to_slab(float (*red)[32][64 + 1], const float* s1, const float* s2, int cv, int ps, float* slab,
                                                int ldslab) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][ps][cv * 8 + j] = s1[j];
    red[1][ps][cv * 8 + j] = s2[j];
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int which = threadIdx.x >> 6, c = threadIdx.x & 63;
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) s += red[which][r][c];
    const int cc = blockIdx.y * 64 + c;
    if (cc < ldslab) slab[((size_t)blockIdx.x * 2 + which) * ldslab + cc] = s;
  }
}

}  // namespace mau
