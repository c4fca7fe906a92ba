// bn_bwd_apply.h -- one element of the BatchNorm + ReLU backward's apply pass, the ONE copy of its rounding: bn.hip's
// bn_relu_bwd_apply_kernel, the fused apply kernels of bn_fused.hip and the first layer's weight gradient (conv3x3_first.hip, which
// forms dz in its load stage) all round through it, so a layer's dz has the same bits whichever of them produces it.
#pragma once
#include "mau_common.h"

namespace mau {

// data parallel: the all-reduced pixel count travels behind the 2 C sums
__device__ __forceinline__ double bn_bwd_inv_count(const double* __restrict__ sums, double inv_count, int C) {
  return inv_count <= 0.0 ? 1.0 / sums[2 * C] : inv_count;
}

// dy = sc*(dz - m1 - xhat*m2), xhat = (y - mu)*is   ==>   dy = sc*dz - k0 - k1*y, for the 8 channels c0 .. c0 + 7
struct Apply8 {
  float sc[8], sh[8], k0[8], k1[8];
  __device__ __forceinline__ void load(const float* scale, const float* shift, const float* mean, const float* invstd, const double* sums,
                                       double inv_count, int c0, int C) {
    double d1[8], d2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {                        // all 48 loads first, no wait between them (mau_common.h: coef)
      sc[j] = coef(scale, c0 + j, C);
      sh[j] = coef(shift, c0 + j, C);
      k0[j] = coef(mean, c0 + j, C);
      k1[j] = coef(invstd, c0 + j, C);
      d1[j] = coef(sums, c0 + j, C);
      d2[j] = coef(sums + C, c0 + j, C);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float mu = k0[j], is = k1[j];
      const float m1 = (float)(d1[j] * inv_count), m2 = (float)(d2[j] * inv_count);
      // (every product rounded on its own, the difference one explicit FMA: the generic and the fused apply kernels must agree
      //  to the bit -- left to the compiler, "a*b - c*d" contracts differently from kernel to kernel, visible in fp16 outputs)
      k1[j] = __fmul_rn(__fmul_rn(sc[j], m2), is);
      k0[j] = fmaf(sc[j], m1, -__fmul_rn(k1[j], mu));
    }
  }
  __device__ __forceinline__ float dy(int j, float yv, float da) const {
    const float act = fmaf(yv, sc[j], sh[j]);
    const float dz = act > 0.f ? da : 0.f;
    return fmaf(sc[j], dz, -fmaf(k1[j], yv, k0[j]));
  }
};

}  // namespace mau
