// screen.hip -- placement screening: every candidate stamp ranked from ONE input gradient.  The network's input is one-hot, so a stamp
// of class c changes exactly two channels of a pixel of the second block by +-1, and its first-order effect on a scalar objective is a
// plain sum of input-gradient entries over the stamp's rectangle -- no step size.  Three launches around one forward and one
// data-gradient-only backward (include/mau_hip.h has the definitions: linearisation point, objective, seed, swap term, coefficient):
//   screen_seed_kernel   the objective table and the roi planes -> dout (K,2,H,W) fp32, every element written, and the counts n_k;
//   screen_rows_kernel   the gradient G (K,H,W,ld) and a table of (y0, x0, cls) rows -> four fp64 figures per (row, objective);
//   screen_maps_kernel   for one objective, coef_k * s_k(p, c) for every pixel and class -> (ncls,H,W) fp32.
//
// seed: one workgroup per objective walks the plane (the seed is written once per linearisation point; K is a handful); the count is
// an integer per thread, joined as doubles holding integers -- the same bits in any order.
// rows: one 256-thread workgroup per (row, objective).  Slot i of the UNCLIPPED ph x pw rectangle, row-major, belongs to thread
// i % 256, and a thread joins its slots in increasing i; a slot outside the tile contributes nothing, so the loop visits only the
// rectangle's rows and columns inside the tile (at most H * ceil(W / 256) steps per thread, whatever ph and pw are) and the order is
// that of the unclipped walk.  The join is chunk_reduce.h's: slot order, xor butterfly, wave order.  Every index made from a table
// value (y0, x0, cls, ch, the roi index) is range-checked in 64-bit before it is used; a class id of the tile >= ncls sets no channel
// (scn_pixel.h) and so subtracts nothing.  No float atomics, no workspace: a row's bits depend on its own table row, its objective
// and the tile, not on P, its place in the table or K.
// maps: one thread per pixel; the channel groups of 8 that hold the second one-hot block are read with 16-byte loads (VEC: ld % 8 == 0
// and G 16-byte aligned) or element by element, and stay in registers (statically indexed: no scratch).
#include <math.h>
#include "chunk_reduce.h"
#include "scn_pixel.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int SCR_ROW = 4;               // stamp pixels in the tile, of those changed, predicted change of J_k, non-finite values read
constexpr int SCR_MAX_GROUPS = 3;        // (off % 8 + ncls <= 7 + 16: the second block touches at most three groups of 8 channels)

// the channel offset of the second one-hot block, as scn_store_pixel writes it
__device__ __host__ __forceinline__ int scr_off(int nc) { return nc + SCN_NCONT; }

// the roi plane of an objective: nullptr = the whole tile; *empty: a row that names a plane that is not there
__device__ __forceinline__ const uint8_t* scr_roi(const int* __restrict__ objs, const uint8_t* __restrict__ rois, int R, int k, size_t hw,
                                                  bool* empty) {
  const int r = objs[2 * k + 1];
  *empty = r < -1 || r >= R || (r >= 0 && rois == nullptr);
  return (r >= 0 && !*empty) ? rois + (size_t)r * hw : nullptr;
}

__global__ __launch_bounds__(256) void screen_seed_kernel(const int* __restrict__ objs, const uint8_t* __restrict__ rois, int R, float seed,
                                                          float* __restrict__ dout, double* __restrict__ counts, int64_t HW) {
  __shared__ double wsum[4][1];
  const int k = blockIdx.x, ch = objs[2 * k];
  bool empty;
  const uint8_t* roi = scr_roi(objs, rois, R, k, (size_t)HW, &empty);
  float* d0 = dout + (size_t)k * 2 * HW;
  float* d1 = d0 + HW;
  double acc[1] = {0.0};
  for (int64_t p = threadIdx.x; p < HW; p += 256) {
    const bool in = !empty && (roi == nullptr || roi[p] != 0);
    const float v = in ? seed : 0.f;
    d0[p] = ch == 0 ? v : 0.f;
    d1[p] = ch == 1 ? v : 0.f;
    acc[0] += in ? 1.0 : 0.0;
  }
  block_join<1>(acc, wsum, SumAll(), counts + k);
}

template <typename T>
__global__ __launch_bounds__(256) void screen_rows_kernel(const T* __restrict__ G, int ld, const uint8_t* __restrict__ dw_t2,
                                                          const int* __restrict__ edits, const double* __restrict__ counts,
                                                          const int* __restrict__ objs, double tstd, double seed, double* __restrict__ rows,
                                                          int H, int W, int ph, int pw, int nc) {
  __shared__ double wsum[4][SCR_ROW];
  __shared__ double tot[SCR_ROW];
  const int64_t n = blockIdx.x;
  const int k = blockIdx.y;
  const int64_t y0 = edits[3 * n], x0 = edits[3 * n + 1];
  const int cls = edits[3 * n + 2];
  const bool live = cls >= 0 && cls < nc;
  const int off = scr_off(nc);
  const size_t hw = (size_t)H * W;
  const T* g = G + (size_t)k * hw * ld;
  // the rectangle's rows [r0, r1) and columns [c0, c1) inside the tile
  const int64_t r0 = y0 < 0 ? -y0 : 0, r1 = (int64_t)H - y0 < ph ? (int64_t)H - y0 : ph;
  const int64_t c0 = x0 < 0 ? -x0 : 0, c1 = (int64_t)W - x0 < pw ? (int64_t)W - x0 : pw;

  double acc[SCR_ROW] = {0.0, 0.0, 0.0, 0.0};
  if (c0 < c1) {
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t first = r * pw + c0;                  // slot of column c0; this thread's first column of the row:
      int64_t c = c0 + ((((int64_t)threadIdx.x - first) % 256) + 256) % 256;
      for (; c < c1; c += 256) {
        const size_t ps = (size_t)(y0 + r) * W + (size_t)(x0 + c);
        acc[0] += 1.0;
        if (live) {
          const int cur = dw_t2[ps];
          const T* px = g + ps * ld + off;
          const bool has = cur < nc;
          const float a = (float)px[cls], b = (float)px[has ? cur : 0];
          acc[1] += cur != cls ? 1.0 : 0.0;
          acc[2] += (double)a - (has ? (double)b : 0.0);
          acc[3] += (isfinite(a) ? 0.0 : 1.0) + (has && !isfinite(b) ? 1.0 : 0.0);
        }
      }
    }
  }
  block_join<SCR_ROW>(acc, wsum, SumAll(), tot);
  if (threadIdx.x < SCR_ROW) {
    const int e = threadIdx.x;
    double val = tot[e];                                  // written by this thread
    if (e == 2) {
      const double nk = counts[k];
      const double coef = (objs[2 * k] == 1 ? tstd : 1.0) / (seed * nk);
      val = nk > 0.0 ? (live ? coef * val : 0.0) : NAN;
    }
    rows[((size_t)k * gridDim.x + n) * SCR_ROW + e] = val;
  }
}

// the eight channels [g0, g0 + 8) of a pixel; element by element: a channel at or beyond `lim` is not read (0)
template <typename T, bool VEC>
__device__ __forceinline__ F8 scr_group(const T* __restrict__ px, int g0, int lim) {
  if constexpr (VEC) {
    return load8<T>(px + g0);
  } else {
    F8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = g0 + j < lim;
      const float v = (float)px[in ? g0 + j : 0];
      r.v[j] = in ? v : 0.f;
    }
    return r;
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void screen_maps_kernel(const T* __restrict__ G, int ld, const uint8_t* __restrict__ dw_t2,
                                                          const double* __restrict__ counts, const int* __restrict__ objs, double tstd,
                                                          double seed, float* __restrict__ maps, int k, int64_t HW, int nc) {
  const int64_t ps = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (ps >= HW) return;
  const int off = scr_off(nc), lim = off + nc, gbase = off & ~7;
  const T* px = G + ((size_t)k * HW + ps) * ld;
  F8 f[SCR_MAX_GROUPS];
#pragma unroll
  for (int gi = 0; gi < SCR_MAX_GROUPS; ++gi) f[gi] = gbase + 8 * gi < lim ? scr_group<T, VEC>(px, gbase + 8 * gi, lim) : zero8();
  const int cur = dw_t2[ps];
  double gcur = 0.0;                                      // cur >= nc: no channel is set, nothing is subtracted
#pragma unroll
  for (int gi = 0; gi < SCR_MAX_GROUPS; ++gi)
#pragma unroll
    for (int j = 0; j < 8; ++j) gcur = (cur < nc && gbase + 8 * gi + j == off + cur) ? (double)f[gi].v[j] : gcur;
  const double nk = counts[k];
  const double coef = (objs[2 * k] == 1 ? tstd : 1.0) / (seed * nk);
#pragma unroll
  for (int gi = 0; gi < SCR_MAX_GROUPS; ++gi)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = gbase + 8 * gi + j - off;
      if (c >= 0 && c < nc) maps[(size_t)c * HW + ps] = nk > 0.0 ? (float)(coef * ((double)f[gi].v[j] - gcur)) : NAN;
    }
}

// a positive power of two that a float holds as a normal number
static inline bool scr_scale_ok(double s) {
  int e = 0;
  return s > 0.0 && isfinite(s) && frexp(s, &e) == 0.5 && e >= -125 && e <= 128;
}

}  // namespace mau

using namespace mau;

#define SCR_REQUIRE_TILE(who, H, W, ncls)                                                                                          \
  MAU_REQUIRE((H) > 0 && (W) > 0 && (int64_t)(H) * (W) <= (1 << 30), who ": tiles of 1 to 2^30 pixels, got %d x %d", (H), (W));     \
  MAU_REQUIRE((ncls) >= 1 && (ncls) <= SCN_MAX_CLS, who ": ncls must be in [1,%d], got %d", SCN_MAX_CLS, (ncls))

extern "C" {

int mau_screen_row_elems(void) { return SCR_ROW; }

int mau_screen_seed(const int* objs, const unsigned char* rois, int R, double seed_scale, float* dout, double* counts, int K, int H, int W,
                    mau_stream_t stream) {
  MAU_REQUIRE(objs && dout && counts, "screen_seed: null pointer");
  MAU_REQUIRE(K >= 1 && K <= 65535 && R >= 0, "screen_seed: K must be in [1,65535] and R >= 0, got %d, %d", K, R);
  MAU_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= (1 << 30), "screen_seed: tiles of 1 to 2^30 pixels, got %d x %d", H, W);
  MAU_REQUIRE(scr_scale_ok(seed_scale), "screen_seed: seed_scale must be a positive power of two, got %g", seed_scale);
  MAU_LAUNCH(screen_seed_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, objs, rois, R, (float)seed_scale, dout, counts, (int64_t)H * W);
  return check_launch("screen_seed_kernel");
}

int mau_screen_rows(const void* G, int ld, int dtype, const unsigned char* dw_t2, const int* edits, const double* counts, const int* objs,
                    double temp_std, double seed_scale, double* rows, int K, int P, int H, int W, int ph, int pw, int ncls,
                    mau_stream_t stream) {
  MAU_REQUIRE(G && dw_t2 && edits && counts && objs && rows, "screen_rows: null pointer");
  MAU_REQUIRE(ph >= 1 && pw >= 1, "screen_rows: a stamp of at least 1 x 1, got %d x %d", ph, pw);
  SCR_REQUIRE_TILE("screen_rows", H, W, ncls);
  MAU_REQUIRE(K >= 1 && K <= 65535 && P >= 1, "screen_rows: K must be in [1,65535] and P >= 1, got %d, %d", K, P);
  MAU_REQUIRE(ld >= 2 * ncls + SCN_NCONT, "screen_rows: ld must be at least %d, got %d", 2 * ncls + SCN_NCONT, ld);
  MAU_REQUIRE(scr_scale_ok(seed_scale), "screen_rows: seed_scale must be a positive power of two, got %g", seed_scale);
  MAU_DISPATCH_DTYPE(dtype, MAU_LAUNCH(screen_rows_kernel<T>, dim3(P, K), dim3(256), 0, (hipStream_t)stream, (const T*)G, ld, dw_t2, edits,
                                       counts, objs, temp_std, seed_scale, rows, H, W, ph, pw, ncls));
  return check_launch("screen_rows_kernel");
}

int mau_screen_maps(const void* G, int ld, int dtype, const unsigned char* dw_t2, const double* counts, const int* objs, double temp_std,
                    double seed_scale, float* maps, int k, int K, int H, int W, int ncls, mau_stream_t stream) {
  MAU_REQUIRE(G && dw_t2 && counts && objs && maps, "screen_maps: null pointer");
  SCR_REQUIRE_TILE("screen_maps", H, W, ncls);
  MAU_REQUIRE(K >= 1 && k >= 0 && k < K, "screen_maps: objective %d of %d", k, K);
  MAU_REQUIRE(ld >= 2 * ncls + SCN_NCONT, "screen_maps: ld must be at least %d, got %d", 2 * ncls + SCN_NCONT, ld);
  MAU_REQUIRE(scr_scale_ok(seed_scale), "screen_maps: seed_scale must be a positive power of two, got %g", seed_scale);
  const int64_t HW = (int64_t)H * W;
  const bool vec = ld % 8 == 0 && (uintptr_t)G % 16 == 0;
  const dim3 grid(ceil_div(HW, 256));
  MAU_DISPATCH_DTYPE(dtype, {
    if (vec)
      MAU_LAUNCH((screen_maps_kernel<T, true>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)G, ld, dw_t2, counts, objs, temp_std, seed_scale,
                 maps, k, HW, ncls);
    else
      MAU_LAUNCH((screen_maps_kernel<T, false>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)G, ld, dw_t2, counts, objs, temp_std, seed_scale,
                 maps, k, HW, ncls);
  });
  return check_launch("screen_maps_kernel");
}

}  // extern "C"
