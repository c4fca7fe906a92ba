// eval_row.h -- what the two evaluation-metric kernels (evalmetrics.hip: one model; evalmulti.hip: M models over one target) share,
// written once: the accumulator layout, the chunking, the join of an accumulator and the finished row's entries.  A row of
// evalmulti.hip has the bits of evalmetrics.hip because both walk these.
#pragma once
#include <math.h>
#include "chunk_reduce.h"

namespace mau {

constexpr int EVAL_MAX_CLS = 16;
constexpr int EVAL_HEAD = 11;            // row entries in front of the per-class blocks (include/mau_hip.h)
// per-thread accumulators: 0 sum|d| 1 sum d^2 2,3 sum / sum of squares of lap(p) 4,5 of lap(g) 6,7 non-finite out / tgt
// 8 min p 9 max p 10 min g 11 max g, then NB counts, NB sums |d|, NB sums d^2 (bin NB-1: class ids >= ncls)
constexpr int EVAL_ACC0 = 12;

// image rows of a workgroup: a run of at most CHUNK_PIX pixels (250 x 250: 16 rows, 16 chunks per map); a map wider than
// CHUNK_PIX: one image row
static inline int eval_rows_per_chunk(int W) { return W >= CHUNK_PIX ? 1 : CHUNK_PIX / W; }
static inline int eval_chunks(int H, int W) { return ceil_div(H, eval_rows_per_chunk(W)); }
static inline int eval_bins(int ncls) { return ncls <= 9 ? 10 : EVAL_MAX_CLS + 1; }

struct EvalJoin {
  __device__ __forceinline__ double operator()(int v, double a, double b) const {
    return (v == 8 || v == 10) ? fmin(a, b) : (v == 9 || v == 11) ? fmax(a, b) : a + b;
  }
};

// the pixel's own index and its four neighbours' with the edge sample repeated (an axis of one pixel contributes x + x - 2x)
struct EvalStencil {
  size_t q, qu, qd, ql, qr;
};
__device__ __forceinline__ EvalStencil eval_stencil(int idx, int i0, int H, int W) {
  const int di = idx / W;
  const int i = i0 + di, j = idx - di * W;
  EvalStencil s;
  s.q = (size_t)i * W + j;
  s.qu = i > 0 ? s.q - W : s.q;
  s.qd = i + 1 < H ? s.q + W : s.q;
  s.ql = j > 0 ? s.q - 1 : s.q;
  s.qr = j + 1 < W ? s.q + 1 : s.q;
  return s;
}

// x * sc + sh at the pixel and the 5-point Laplacian of that map there: fp64 from the load on, nothing contracted
__device__ __forceinline__ void eval_value_lap(const float* __restrict__ x, const EvalStencil& s, double sc, double sh, float& raw,
                                               double& v, double& lap) {
#pragma clang fp contract(off)
  raw = x[s.q];
  v = (double)raw * sc + sh;
  lap = ((((double)x[s.qu] * sc + sh) + ((double)x[s.qd] * sc + sh)) + ((double)x[s.ql] * sc + sh)) + ((double)x[s.qr] * sc + sh) - 4.0 * v;
}

// entry e of the finished row from the joined accumulators tot[EVAL_ACC0 + 3 NB]; n = H * W.  A NaN entry is THE quiet NaN: which
// payload and sign survive a chain of sums over NaNs depends on the operand order the compiler chose, which differs from kernel
// to kernel -- the rows of the two kernels are to agree in every bit.
template <int NB>
__device__ __forceinline__ double eval_row_value(const double* tot, int e, int ncls, double n) {
#pragma clang fp contract(off)
  if (e == 0) return tot[0] / n;
  if (e == 1) return sqrt(tot[1] / n);
  if (e == 2 || e == 3) {                  // population variance from the two sums; never below zero
    const double m = tot[2 * e - 2] / n;
    const double val = tot[2 * e - 1] / n - m * m;
    return val < 0.0 ? 0.0 : val;
  }
  if (e < 10) return tot[e + 2];
  if (e == 10) return tot[EVAL_ACC0 + NB - 1];
  const int blk = (e - EVAL_HEAD) / ncls, kk = (e - EVAL_HEAD) - blk * ncls;
  const double cnt = tot[EVAL_ACC0 + kk];
  // an absent class: 0 / 0 = NaN, the host turns it into "no row"
  return blk == 0 ? cnt : blk == 1 ? tot[EVAL_ACC0 + NB + kk] / cnt : sqrt(tot[EVAL_ACC0 + 2 * NB + kk] / cnt);
}

template <int NB>
__device__ __forceinline__ double eval_row_entry(const double* tot, int e, int ncls, double n) {
  const double val = eval_row_value<NB>(tot, e, ncls, n);
  return isnan(val) ? __builtin_nan("") : val;
}

}  // namespace mau
