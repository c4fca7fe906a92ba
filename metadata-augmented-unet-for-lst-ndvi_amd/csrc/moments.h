// moments.h -- fp64 moment rows shared by gtstats.hip and tilestats.hip: (n, mean, M2 = sum (x - mean)^2, non-finite count), their
// pairwise merge and the fixed-order workgroup sum.  Nothing here is contracted: the host twins (ground_truth.merge_moments,
// dataset_metrics) repeat the merge operation for operation.
#pragma once
#include "mau_common.h"

#pragma clang fp contract(off)

namespace mau {

struct Moments {
  double n, mean, m2, bad;
};

// Chan et al.'s pairwise update of (n, mean, M2) by a second set; nothing is contracted (the file's pragma), so the host twin
// (ground_truth.merge_moments) repeats it operation for operation.  An empty left side takes the right side as it is.
__device__ __forceinline__ Moments moment_merge(const Moments& a, const Moments& b) {
  if (a.n == 0.0) return b;
  Moments r;
  const double delta = b.mean - a.mean;
  r.n = a.n + b.n;
  r.mean = a.mean + (delta * b.n) / r.n;
  r.m2 = (a.m2 + b.m2) + (delta * delta) * ((a.n * b.n) / r.n);
  r.bad = a.bad + b.bad;
  return r;
}

__device__ __forceinline__ Moments moment_load(const double* p) { return Moments{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void moment_store(double* p, const Moments& m) {
  p[0] = m.n;
  p[1] = m.mean;
  p[2] = m.m2;
  p[3] = m.bad;
}

// the sum of `a` over the workgroup, the same bits in every thread: lanes by xor butterfly, waves in wave order through `slot`
__device__ __forceinline__ double block_sum(double a, double* slot) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) a += __shfl_xor(a, s, 64);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = a;
  __syncthreads();
  return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

}  // namespace mau
