// bn_stats.h -- the two steps every BatchNorm statistics launch of bn.hip is made of, ONE copy of each: the fixed-order fp64 column
// sum of a slab (one level of it: reduce_rows_kernel runs it once, the ticket kernels twice) and the finalize of a channel's moments.
#pragma once
#include "mau_common.h"

namespace mau {

// ---- the fixed-order two-accumulator sum of the reductions below, with a group's loads in flight at once ----
//     s0 += v[first], v[first + 8], ...;   s1 += v[first + 4], v[first + 12], ...      (indices < end, ascending)
// is the arithmetic of the plain loop "for (k = first; k + 4 < end; k += 8) { s0 += v[k]; s1 += v[k + 4]; } if (k < end) s0 += v[k];"
// -- same operands, same order, same bits.  As that loop the level was a chain of dependent round trips (each iteration's
// loads were issued after the previous iteration's additions: 16 trips of ~0.65 us through L2 for 128 chunks; the finalize
// launches of the 256^2 / 128^2 layers took 14 us against 5.5 us for the layers with <= 16 chunks).  Here whole groups of 16,
// then of 4 iterations issue their loads back to back and add in order; what is left (< 4 iterations) runs as the plain loop,
// so the short reductions of the deep layers execute exactly what they did before.  (A single 16-wide group with clamped
// indices and predicated additions for every length cost the short ones +3.5 us of instruction issue: 4 waves, one per SIMD.)
template <int G, typename Load>
__device__ __forceinline__ void ordered_group(int& k, int end, Load load, double& s0, double& s1) {
  for (; k + 8 * (G - 1) + 4 < end; k += 8 * G) {          // every index of the group is valid
    double a[G], b[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
      a[i] = load(k + 8 * i);
      b[i] = load(k + 8 * i + 4);
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
      s0 += a[i];
      s1 += b[i];
    }
  }
}
template <typename Load>
__device__ __forceinline__ void ordered_pair_sum(int first, int end, Load load, double& s0, double& s1) {
  int k = first;
  ordered_group<16>(k, end, load, s0, s1);
  ordered_group<4>(k, end, load, s0, s1);
  for (; k + 4 < end; k += 8) {
    s0 += load(k);
    s1 += load(k + 4);
  }
  if (k < end) s0 += load(k);
}

// One level of a column sum, block = 64 columns x 4 row-lanes (each wave reads 64 consecutive columns of one row): lane rl adds
// rows first + rl, first + rl + 4, ... < end of NQ quantities (load(q, row); nothing when !live) and leaves its sums in
// lds[q][rl][column]; the barrier is inside.  join4_* then give a column's sum over the four lanes.
template <int NQ, typename Load>
__device__ __forceinline__ void lane_sums_to_lds(double (*lds)[4][64], bool live, int first, int end, Load load) {
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  double s[NQ][2] = {};
  if (live && first + rl < end) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) ordered_pair_sum(first + rl, end, [&](int r) { return load(q, r); }, s[q][0], s[q][1]);
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) lds[q][rl][cl] = s[q][0] + s[q][1];
  __syncthreads();
}
// The association of the four lanes is part of the pinned bits (the one-launch forms are tested bit for bit against the two-launch
// ones): every sum that is WRITTEN OUT as a sum -- the chunk partials of level 1 and the
// results of reduce_rows_kernel / reduce_rows_fused_kernel -- is the chain; the level 2 that feeds a finalize directly
// (bn_finalize_from_partials_kernel, bn_stats_finalize_fused_kernel) is the tree.
__device__ __forceinline__ double join4_chain(const double (*p)[64], int cl) { return p[0][cl] + p[1][cl] + p[2][cl] + p[3][cl]; }
__device__ __forceinline__ double join4_tree(const double (*p)[64], int cl) { return (p[0][cl] + p[1][cl]) + (p[2][cl] + p[3][cl]); }

// Channel c's sum s and sum of squares q over `count` elements -> scale / shift / mean / invstd, and the running statistics'
// update (biased variance for the normalisation, unbiased for running_var).
__device__ __forceinline__ void bn_finalize_channel(double s, double q, double count, int c, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                                                    float momentum, float eps, float* __restrict__ scale, float* __restrict__ shift,
                                                    float* __restrict__ mean_o, float* __restrict__ invstd_o) {
  const double mean = s / count;
  double var = q / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gamma[c] * invstd;
  scale[c] = sc;
  shift[c] = beta[c] - (float)mean * sc;
  mean_o[c] = (float)mean;
  invstd_o[c] = invstd;
  if (rmean) {
    const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
    rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)mean;
    rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unbiased;
  }
}

}  // namespace mau
