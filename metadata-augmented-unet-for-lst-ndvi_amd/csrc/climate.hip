// climate.hip -- the climate stage (reference src/data/process_temperature.py: the 1901-1950 baseline of :23-33, the normalised
// anomalies of :48-55, TemperatureQuery.query of :93-114).  x is the reference's concatenation of the year files: (T, G) fp32,
// time-major, the G = lat * lon cells of a month contiguous.
//   baseline_kernel   x (T,G) -> rows (G,4) fp64: n, mean, M2 = sum (x - mean)^2 of a cell's non-NaN months, and its NaN months;
//   normalise_kernel  x (T,G), rows -> out (T,G) fp32: (float)(((double)x - mean) / sqrt(M2 / n)), rounded once;
//   series_kernel     x (the RAW grid), rows, cell[N], keep[N] -> series (N,Tpad) fp32: the first keep[n] anomalies of cell[n], the
//                     same expression (the same bits), then zeros; srows (N,4) fp64: the moment row of those values.
//
// baseline: one thread per cell, consecutive threads on consecutive cells (every time row is read coalesced), two passes over time
// IN TIME ORDER in fp64, BL_UNROLL independent row loads in flight per thread.  A NaN month is skipped and counted (skipna); an
// infinity is not (it propagates, as np.nanmean lets it).  No workspace, no tickets, no atomics: a cell's bits depend on its own
// column only.  normalise: a thread owns one cell (four with 16-byte accesses), loads its coefficients once and walks a slab of
// NORM_SLAB months; the slabs of time are independent workgroups (nothing is summed over time).  series: one workgroup per query,
// the values in registers in the scalar slot layout of chunk_reduce.h (slot k of thread t is month k * 256 + t), chunk_moments<false>
// makes the row: a series is one chunk.  The normalised grid is never materialised for a query.
#include <math.h>
#include "chunk_reduce.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int CL_ROW = 4;                // n, mean, M2, NaN months (baseline) / non-finite values (series)
constexpr int BL_UNROLL = 8;             // row loads in flight per thread of the baseline: 8 KiB per workgroup
constexpr int NORM_SLAB = 64;            // months per workgroup of the normalisation
constexpr int NORM_UNROLL = 8;
constexpr int CL_MAX_MONTHS = CHUNK_PIX; // a series is one chunk

// the standard deviation and the anomaly, written once: the three kernels and the host twin (climate.py) repeat these operations
__device__ __forceinline__ double cell_std(double m2, double n) { return sqrt(m2 / n); }
__device__ __forceinline__ float anomaly(float x, double mean, double std) { return (float)(((double)x - mean) / std); }

__global__ __launch_bounds__(256) void baseline_kernel(const float* __restrict__ x, double* __restrict__ rows, int T, int G) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const bool mine = g < G;
  const float* col = x + (mine ? g : G - 1);     // a thread past the last cell reads the last cell's column and stores nothing
  float v[BL_UNROLL];
  // pass 1: the sum and the number of the non-NaN months
  double sum = 0.0, n = 0.0;
  for (int t0 = 0; t0 < T; t0 += BL_UNROLL) {
#pragma unroll
    for (int u = 0; u < BL_UNROLL; ++u) v[u] = col[(size_t)(t0 + u < T ? t0 + u : T - 1) * G];
#pragma unroll
    for (int u = 0; u < BL_UNROLL; ++u) {
      const bool in = t0 + u < T && !isnan(v[u]);
      sum = in ? sum + (double)v[u] : sum;
      n += in ? 1.0 : 0.0;
    }
  }
  const double mean = sum / n;                   // no month: 0 / 0 = NaN
  // pass 2: the squared distances to the mean
  double m2 = 0.0;
  for (int t0 = 0; t0 < T; t0 += BL_UNROLL) {
#pragma unroll
    for (int u = 0; u < BL_UNROLL; ++u) v[u] = col[(size_t)(t0 + u < T ? t0 + u : T - 1) * G];
#pragma unroll
    for (int u = 0; u < BL_UNROLL; ++u) {
      const bool in = t0 + u < T && !isnan(v[u]);
      const double d = (double)v[u] - mean;
      m2 = in ? m2 + d * d : m2;
    }
  }
  if (!mine) return;
  double* row = rows + (size_t)g * CL_ROW;
  row[0] = n;
  row[1] = mean;
  row[2] = n == 0.0 ? (double)NAN : m2;
  row[3] = (double)T - n;
}

template <bool VEC4>
__global__ __launch_bounds__(256) void normalise_kernel(const float* __restrict__ x, const double* __restrict__ rows,
                                                        float* __restrict__ out, int T, int G) {
  constexpr int W = VEC4 ? 4 : 1;
  const int g = (blockIdx.x * 256 + threadIdx.x) * W;
  if (g >= G) return;                            // VEC4: G % 4 == 0, the four cells are inside or outside together
  double mean[W], std[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const double* row = rows + (size_t)(g + j) * CL_ROW;
    mean[j] = row[1];
    std[j] = cell_std(row[2], row[0]);
  }
  const int t_begin = blockIdx.y * NORM_SLAB, t_end = t_begin + NORM_SLAB < T ? t_begin + NORM_SLAB : T;
  for (int t0 = t_begin; t0 < t_end; t0 += NORM_UNROLL) {
    if (VEC4) {
      f32x4 v[NORM_UNROLL];
#pragma unroll
      for (int u = 0; u < NORM_UNROLL; ++u)
        v[u] = *reinterpret_cast<const f32x4*>(x + (size_t)(t0 + u < t_end ? t0 + u : t_end - 1) * G + g);
#pragma unroll
      for (int u = 0; u < NORM_UNROLL; ++u) {
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = anomaly(v[u][j], mean[j], std[j]);
        if (t0 + u < t_end) *reinterpret_cast<f32x4*>(out + (size_t)(t0 + u) * G + g) = r;
      }
    } else {
      float v[NORM_UNROLL];
#pragma unroll
      for (int u = 0; u < NORM_UNROLL; ++u) v[u] = x[(size_t)(t0 + u < t_end ? t0 + u : t_end - 1) * G + g];
#pragma unroll
      for (int u = 0; u < NORM_UNROLL; ++u)
        if (t0 + u < t_end) out[(size_t)(t0 + u) * G + g] = anomaly(v[u], mean[0], std[0]);
    }
  }
}

__global__ __launch_bounds__(256) void series_kernel(const float* __restrict__ x, const double* __restrict__ rows,
                                                     const int* __restrict__ cell, const int* __restrict__ keep,
                                                     float* __restrict__ series, double* __restrict__ srows, int T, int G, int Tpad) {
  __shared__ double sm[4];
  __shared__ double sr[4][2];
  const size_t q = blockIdx.x;
  const int c = cell[q], k0 = keep[q];
  const bool known = c >= 0 && c < G;            // a cell outside the grid: NaN values and the empty row, nothing read out of bounds
  const int kept = k0 < 0 ? 0 : k0 > T ? T : k0;
  const unsigned ok = slot_mask<false>(kept);
  const float* col = x + (known ? c : 0);
  const double* row = rows + (size_t)(known ? c : 0) * CL_ROW;
  const double mean = row[1], std = cell_std(row[2], row[0]);
  float raw[CHUNK_SLOTS];
#pragma unroll
  for (int k = 0; k < CHUNK_SLOTS; ++k) raw[k] = col[(size_t)((ok >> k) & 1u ? k * 256 + (int)threadIdx.x : 0) * G];
  float* mine = series + q * (size_t)Tpad;
  double v[CHUNK_SLOTS];
#pragma unroll
  for (int k = 0; k < CHUNK_SLOTS; ++k) {
    const float a = known ? anomaly(raw[k], mean, std) : NAN;
    v[k] = (double)a;
    if ((ok >> k) & 1u) mine[k * 256 + (int)threadIdx.x] = a;
  }
  for (int t = kept + (int)threadIdx.x; t < Tpad; t += 256) mine[t] = 0.f;      // pad_sequence's padding
  chunk_moments<false>(v, known ? ok : 0u, known ? (double)kept : 0.0, sm, sr, srows + q * CL_ROW);
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_climate_row_elems(void) { return CL_ROW; }

int mau_climate_series_max_months(void) { return CL_MAX_MONTHS; }

int mau_climate_baseline(const float* x, double* rows, int T, int G, mau_stream_t stream) {
  MAU_REQUIRE(x && rows, "climate_baseline: null pointer");
  MAU_REQUIRE(T > 0 && G > 0, "climate_baseline: non-positive size (T %d, G %d)", T, G);
  MAU_REQUIRE(G <= (1 << 30), "climate_baseline: at most 2^30 cells");
  MAU_REQUIRE((uintptr_t)x % 4 == 0, "climate_baseline: x must be 4-byte aligned");
  MAU_REQUIRE((uintptr_t)rows % 8 == 0, "climate_baseline: rows must be 8-byte aligned");
  MAU_LAUNCH(baseline_kernel, dim3(ceil_div(G, 256)), dim3(256), 0, (hipStream_t)stream, x, rows, T, G);
  return check_launch("baseline_kernel");
}

int mau_climate_normalise(const float* x, const double* rows, float* out, int T, int G, mau_stream_t stream) {
  MAU_REQUIRE(x && rows && out, "climate_normalise: null pointer");
  MAU_REQUIRE(T > 0 && G > 0, "climate_normalise: non-positive size (T %d, G %d)", T, G);
  MAU_REQUIRE(G <= (1 << 30), "climate_normalise: at most 2^30 cells");
  MAU_REQUIRE(T <= 65535 * NORM_SLAB, "climate_normalise: at most %d months", 65535 * NORM_SLAB);
  MAU_REQUIRE(((uintptr_t)x | (uintptr_t)out) % 4 == 0, "climate_normalise: x and out must be 4-byte aligned");
  MAU_REQUIRE((uintptr_t)rows % 8 == 0, "climate_normalise: rows must be 8-byte aligned");
  // 16-byte accesses: every time row of x and of out then starts aligned
  const bool vec4 = G % 4 == 0 && ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
  const int slabs = ceil_div(T, NORM_SLAB);
  if (vec4)
    MAU_LAUNCH(normalise_kernel<true>, dim3(ceil_div(G / 4, 256), slabs), dim3(256), 0, (hipStream_t)stream, x, rows, out, T, G);
  else
    MAU_LAUNCH(normalise_kernel<false>, dim3(ceil_div(G, 256), slabs), dim3(256), 0, (hipStream_t)stream, x, rows, out, T, G);
  return check_launch("normalise_kernel");
}

int mau_climate_series(const float* x, const double* rows, const int* cell, const int* keep, float* series, double* srows, int N, int T,
                       int G, int Tpad, mau_stream_t stream) {
  MAU_REQUIRE(x && rows && cell && keep && series && srows, "climate_series: null pointer");
  MAU_REQUIRE(N > 0 && T > 0 && G > 0, "climate_series: non-positive size (N %d, T %d, G %d)", N, T, G);
  MAU_REQUIRE(G <= (1 << 30), "climate_series: at most 2^30 cells");
  MAU_REQUIRE(N <= (1 << 30), "climate_series: at most 2^30 queries");
  MAU_REQUIRE(T <= CL_MAX_MONTHS, "climate_series: at most %d months (a series is one chunk), got %d", CL_MAX_MONTHS, T);
  MAU_REQUIRE(Tpad >= T, "climate_series: Tpad %d is shorter than the %d months of the grid", Tpad, T);
  MAU_REQUIRE(((uintptr_t)x | (uintptr_t)series | (uintptr_t)cell | (uintptr_t)keep) % 4 == 0,
              "climate_series: x, series, cell and keep must be 4-byte aligned");
  MAU_REQUIRE(((uintptr_t)rows | (uintptr_t)srows) % 8 == 0, "climate_series: rows and srows must be 8-byte aligned");
  MAU_LAUNCH(series_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, x, rows, cell, keep, series, srows, T, G, Tpad);
  return check_launch("series_kernel");
}

}  // extern "C"
