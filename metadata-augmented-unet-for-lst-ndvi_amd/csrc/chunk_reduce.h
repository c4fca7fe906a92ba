// chunk_reduce.h -- the two-level fixed-order fp64 reduction of the analysis kernels (evalmetrics.hip, evalmulti.hip, scenario.hip, gtstats.hip,
// tilestats.hip, compare.hip, loss_terms.hip; the launch loop also head.hip's mau_head_mean), written once.
//
// A row (a plane, a scenario, a sample) is cut into chunks of CHUNK_PIX consecutive pixels, one 256-thread workgroup each -- the
// chunking is a function of the row's size alone.  The order of every join is fixed:
//   a thread joins its values in index (slot) order -- the caller's loop;
//   the 64 lanes of a wave by an xor butterfly 32..1 (the joins commute: every lane ends with the same bits)   wave_join
//   the four waves in wave order through LDS, into the chunk's partial row of the workspace                   block_join / block_sum
//   the workgroup that draws the row's last ticket (last_block_of) joins the partial rows in chunk order       chunk_join / merge_chunks
// so a row's bits depend on nothing but its own data.  A join is a sum, fmin or fmax (fmin / fmax skip a NaN), chosen per index by
// a functor `op(v, a, b)`: `v` is a constant wherever an accumulator array is walked (everything unrolls, nothing is indexed
// dynamically) and the thread's index where one thread owns one entry.
//
// Moment rows (n, mean, M2 = sum (x - mean)^2, ...) are merged with Chan et al.'s pairwise update, and chunk_moments is the one
// two-pass body over the register-resident values of a chunk (load_plane).  No pragma at file scope: head.hip, ssim.hip and
// loss_terms.hip include this header and keep their own contraction mode; what must not be contracted says so in its body.
#pragma once
#include <math.h>
#include "mau_common.h"

namespace mau {

constexpr int CHUNK_PIX = 4096;          // 250 x 250: 16 chunks per plane; 512 x 512: 64
constexpr int CHUNK_SLOTS = CHUNK_PIX / 256;

static inline int chunks_of(int64_t HW) { return ceil_div(HW, CHUNK_PIX); }

// ---- host: one ticket per row, mau_reduce_tickets_elems() rows per launch ----
// rows whose partials a workspace holds: the launches of one call reuse those of the first
static inline int64_t ticket_ws_rows(int64_t rows) {
  const int64_t per = mau_reduce_tickets_elems();
  return rows < per ? rows : per;
}

// launch(row0, n) for rows [row0, row0 + n), n <= mau_reduce_tickets_elems(), until all `rows` are done or a launch fails
template <typename Launch>
static inline int for_ticket_rows(int rows, const char* what, Launch&& launch) {
  const int per = mau_reduce_tickets_elems();
  for (int row0 = 0; row0 < rows; row0 += per) {
    launch(row0, rows - row0 < per ? rows - row0 : per);
    const int st = check_launch(what);
    if (st != 0) return st;
  }
  return 0;
}

// ---- device: the joins ----
struct SumAll {
  __device__ __forceinline__ double operator()(int, double a, double b) const { return a + b; }
};

// lanes of a wave: xor butterfly, every lane returns the same bits.  op(a, b)
template <typename Op>
__device__ __forceinline__ double wave_join(double v, Op op) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = op(v, __shfl_xor(v, s, 64));
  return v;
}

// the sum of `a` over the workgroup, the same bits in every thread: butterfly, then the waves in wave order through slot[4]
__device__ __forceinline__ double block_sum(double a, double* slot) {
  a = wave_join(a, [](double x, double y) { return x + y; });
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = a;
  __syncthreads();
  return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

// acc[0..NV) of every thread joined over the workgroup: butterfly per value, lane 0 of wave w -> wsum[w], barrier, thread v < NV
// joins the four waves in wave order and writes out[v * ostride].  op(v, a, b)
template <int NV, typename Op>
__device__ __forceinline__ void block_join(double (&acc)[NV], double (*wsum)[NV], Op op, double* out, size_t ostride = 1) {
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = wave_join(acc[v], [&](double a, double b) { return op(v, a, b); });
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) wsum[threadIdx.x >> 6][v] = acc[v];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int v = threadIdx.x;
    double s = wsum[0][v];
    for (int w = 1; w < 4; ++w) s = op(v, s, wsum[w][v]);
    out[v * ostride] = s;
  }
}

// level 2 of one entry: prow[v], prow[stride + v], ... of the row's `chunks` partial rows in chunk order.  op(v, a, b)
template <typename Op>
__device__ __forceinline__ double chunk_join(const double* prow, int chunks, int stride, int v, Op op) {
  double s = prow[v];
  for (int c = 1; c < chunks; ++c) s = op(v, s, prow[(size_t)c * stride + v]);
  return s;
}

// ---- device: moment rows ----
struct Moments {
  double n, mean, m2, bad;
};

// Chan et al.'s pairwise update of (n, mean, M2) by a second set; nothing is contracted, so the host twin
// (ground_truth.merge_moments) repeats it operation for operation.  An empty left side takes the right side as it is.
__device__ __forceinline__ Moments moment_merge(const Moments& a, const Moments& b) {
#pragma clang fp contract(off)
  if (a.n == 0.0) return b;
  Moments r;
  const double delta = b.mean - a.mean;
  r.n = a.n + b.n;
  r.mean = a.mean + (delta * b.n) / r.n;
  r.m2 = (a.m2 + b.m2) + (delta * delta) * ((a.n * b.n) / r.n);
  r.bad = a.bad + b.bad;
  return r;
}

// a moment row in memory: n, mean, M2 at q[0..3), the non-finite count at q[bad_at]
__device__ __forceinline__ Moments moment_load(const double* q, int bad_at = 3) { return Moments{q[0], q[1], q[2], q[bad_at]}; }
__device__ __forceinline__ void moment_store(double* q, const Moments& m, int bad_at = 3) {
  q[0] = m.n;
  q[1] = m.mean;
  q[2] = m.m2;
  q[bad_at] = m.bad;
}

// level 2 of a moment row: the row's `chunks` partial rows merged in chunk order
__device__ __forceinline__ Moments merge_chunks(const double* prow, int chunks, int stride, int bad_at = 3) {
  Moments acc = moment_load(prow, bad_at);
  for (int c = 1; c < chunks; ++c) acc = moment_merge(acc, moment_load(prow + (size_t)c * stride, bad_at));
  return acc;
}

// ---- device: the register-resident values of a chunk ----
// 16 slots per thread.  VEC4 (H * W a multiple of 4 and 16-byte aligned tensors: every plane and chunk base is then aligned): slot
// 4k + j of thread t is pixel (k * 256 + t) * 4 + j of the chunk, one 16-byte load per k (npx is then a multiple of 4: a quad is
// inside or outside as a whole).  Otherwise slot k is pixel k * 256 + t, 4-byte coalesced loads.  A slot outside the (partial,
// last) chunk loads pixel 0 of the chunk -- no exec-masked load -- and is left out of every join.

// bit s: slot s of this thread is a pixel of the chunk
template <bool VEC4>
__device__ __forceinline__ unsigned slot_mask(int npx) {
  unsigned m = 0;
#pragma unroll
  for (int s = 0; s < CHUNK_SLOTS; ++s) {
    const int idx = VEC4 ? ((s >> 2) * 256 + (int)threadIdx.x) * 4 : s * 256 + (int)threadIdx.x;
    m |= idx < npx ? 1u << s : 0u;
  }
  return m;
}

// the thread's 16 values of one plane chunk, doubles from the load on
template <bool VEC4>
__device__ __forceinline__ void load_plane(const float* __restrict__ pc, unsigned ok, double (&v)[CHUNK_SLOTS]) {
  if (VEC4) {
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS / 4; ++k) {
      const int idx = (k * 256 + (int)threadIdx.x) * 4;
      const f32x4 f = *reinterpret_cast<const f32x4*>(pc + ((ok >> (4 * k)) & 1u ? idx : 0));
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = (double)f[j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS; ++k) v[k] = (double)pc[(ok >> k) & 1u ? k * 256 + (int)threadIdx.x : 0];
  }
}

// the thread's 16 class values of one map chunk, four to a word
template <bool VEC4>
__device__ __forceinline__ void load_classes(const unsigned char* __restrict__ pc, unsigned ok, unsigned (&w)[CHUNK_SLOTS / 4]) {
#pragma unroll
  for (int k = 0; k < CHUNK_SLOTS / 4; ++k) {
    if (VEC4) {
      const int idx = (k * 256 + (int)threadIdx.x) * 4;
      w[k] = *reinterpret_cast<const unsigned*>(pc + ((ok >> (4 * k)) & 1u ? idx : 0));
    } else {
      w[k] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int s = 4 * k + j;
        w[k] |= (unsigned)pc[(ok >> s) & 1u ? s * 256 + (int)threadIdx.x : 0] << (8 * j);
      }
    }
  }
}

// entry j of a moment row of 8 (n, mean, M2, min, max, sum |x|, NaNs, non-finite values) or of 4 (n, mean, M2, non-finite values)
struct MomentRowJoin {
  __device__ __forceinline__ double operator()(int j, double a, double b) const { return j == 3 ? fmin(a, b) : j == 4 ? fmax(a, b) : a + b; }
};

// The moment row of the chunk's n values v (register resident) -> out: two passes, the chunk mean, then the squared distances
// to it (not E[x^2] - E[x]^2: with |mean| >> std the one-pass form loses half its digits) and what needs no mean.  FULL: the row
// of 8, otherwise the row of 4.  sm: 4 doubles, sr: 4 rows of FULL ? 6 : 2; the two are written alternately with a barrier
// between any read and the next write, so consecutive planes reuse them.  Returns the chunk mean (the same bits in every thread).
template <bool FULL>
__device__ __forceinline__ double chunk_moments(const double (&v)[CHUNK_SLOTS], unsigned ok, double n, double* sm,
                                                double (*sr)[FULL ? 6 : 2], double* out) {
#pragma clang fp contract(off)
  constexpr int NR = FULL ? 6 : 2;       // the row's entries 2 .. 2 + NR
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < CHUNK_SLOTS; ++k) s += (ok >> k) & 1u ? v[k] : 0.0;
  const double mean = block_sum(s, sm) / n;
  double r[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) r[i] = 0.0;
  if constexpr (FULL) {
    r[1] = INFINITY;
    r[2] = -INFINITY;
  }
#pragma unroll
  for (int k = 0; k < CHUNK_SLOTS; ++k) {
    const bool in = (ok >> k) & 1u;
    const double d = v[k] - mean;
    r[0] += in ? d * d : 0.0;
    r[NR - 1] += in && !isfinite(v[k]) ? 1.0 : 0.0;
    if constexpr (FULL) {
      r[1] = fmin(r[1], in ? v[k] : INFINITY);
      r[2] = fmax(r[2], in ? v[k] : -INFINITY);
      r[3] += in ? fabs(v[k]) : 0.0;
      r[4] += in && isnan(v[k]) ? 1.0 : 0.0;
    }
  }
  if (threadIdx.x == 0) {
    out[0] = n;
    out[1] = mean;
  }
  block_join<NR>(r, sr, [](int i, double a, double b) { return FULL ? MomentRowJoin()(i + 2, a, b) : a + b; }, out + 2);
  return mean;
}

}  // namespace mau
