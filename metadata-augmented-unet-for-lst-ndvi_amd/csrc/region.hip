// region.hip -- a forecast for a whole raster at the resolution the network was trained at: overlapping windows through the network
// and a seam-free blend of their outputs (the reference resizes whatever region the user draws to one 512 x 512 tile instead,
// app/gee_utils.py:40-87, app/processing_utils.py:122-128).  The two streaming passes around the forward:
//   region_gather_kernel   B window inputs cut out of ONE resident region (30 B per pixel raw), one launch;
//   region_stitch_kernel   the windows' outputs blended into the region with integer ramp weights, one launch.
//
// gather: grid = (chunks of 256 window pixels, windows), one thread per window pixel, the per-pixel code of scenario_pack_kernel
// (scn_pixel.h): fp64 normalisation rounded to float once, one-hot channels, 16-byte channel-group stores.  The window origins are
// read from DEVICE memory (a captured graph is replayed for the next batch after a device-to-device copy of B rows) and clamped to
// [0, Hr - T] x [0, Wr - T]: no index can leave the region.
//
// stitch: grid = (x chunks, region rows), a thread OWNS V consecutive pixels of a row (V = 4 with 16-byte stores when Wr % 4 == 0 and
// the base is aligned, V = 1 otherwise) in all C channels.  The window set is the Cartesian product ys x xs; per axis a binary
// search finds the first window that reaches the pixel and the next three table entries are tested for cover (the Python wrapper
// refuses tables with more than three windows over a coordinate).  Weights are integers, w = w1(y - y0) * w1(x - x0) with
// w1(i) = min(i + 1, T - i, ramp): every product w * v is exact in fp64 (w < 2^22, v has 24 bits), the numerator is added in the
// order iy ascending, then ix ascending, the denominator is an integer, one fp64 division, one rounding to float.  The order is per
// pixel: both store widths give the same bits, and a pixel under one window gets that window's value bit for bit (w * v / w).  No
// atomics, no LDS.  A window that does not cover the pixel is never read (its NaN must not reach the pixel, and a table entry that
// breaks the wrapper's rules must not move a read outside the buffer): every read is at offsets 0 <= y - y0, x - x0 < T of a window
// whose index is inside the tables.
#include <math.h>
#include "scn_pixel.h"

#pragma clang fp contract(off)

namespace mau {

template <typename T>
__global__ __launch_bounds__(256) void region_gather_kernel(const uint8_t* __restrict__ dw_t1, const uint8_t* __restrict__ dw_t2,
                                                            const float* __restrict__ rgb, const float* __restrict__ ndvi,
                                                            const float* __restrict__ temp, const int* __restrict__ origins,
                                                            const double* __restrict__ norm, T* __restrict__ out, int ld, int Tw, int Hr,
                                                            int Wr, int nc) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= Tw * Tw) return;
  const int n = blockIdx.y;
  int y0 = origins[2 * n], x0 = origins[2 * n + 1];
  y0 = y0 < 0 ? 0 : y0 > Hr - Tw ? Hr - Tw : y0;
  x0 = x0 < 0 ? 0 : x0 > Wr - Tw ? Wr - Tw : x0;
  const int y = p / Tw, x = p - y * Tw;
  const size_t hw = (size_t)Hr * Wr, ps = (size_t)(y0 + y) * Wr + (x0 + x);
  const int a = dw_t1[ps], b = dw_t2[ps];
  float cv[SCN_NCONT];
  scn_norm_planes(rgb, ndvi, temp, norm, hw, ps, cv);
  scn_store_pixel<T>(out + ((size_t)n * Tw * Tw + p) * ld, ld, nc, a, b, cv);
}

constexpr int RGN_COVER = 3;             // windows over one coordinate, at most (overlap <= T / 2, the last origin moved back)

// first index i of the ascending table t (n entries) with t[i] + T > p: the first window that reaches coordinate p
__device__ __forceinline__ int first_reaching(const int* __restrict__ t, int n, int p, int T) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] <= p - T) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the RGN_COVER table entries from i0 on: off[a] = p - t[i0 + a] and w[a] = w1(off[a]) where window i0 + a covers p, w[a] = 0 where not
__device__ __forceinline__ void cover(const int* __restrict__ t, int n, int i0, int p, int T, int ramp, int (&off)[RGN_COVER],
                                      int (&w)[RGN_COVER]) {
#pragma unroll
  for (int a = 0; a < RGN_COVER; ++a) {
    const int i = i0 + a;
    const int s = t[i < n ? i : n - 1];
    const bool in = i < n && s <= p && s > p - T;
    const int o = in ? p - s : 0;
    const int m = o + 1 < T - o ? o + 1 : T - o;
    off[a] = o;
    w[a] = in ? (m < ramp ? m : ramp) : 0;
  }
}

template <int V>
__global__ __launch_bounds__(256) void region_stitch_kernel(const float* __restrict__ win, const int* __restrict__ ys,
                                                            const int* __restrict__ xs, float* __restrict__ out, int C, int T, int ramp,
                                                            int Hr, int Wr, int ny, int nx) {
  const int xb = (blockIdx.x * 256 + threadIdx.x) * V;
  if (xb >= Wr) return;                                   // V == 4 only with Wr % 4 == 0: a thread's pixels are all inside or all outside
  const int y = blockIdx.y;
  const int iy0 = first_reaching(ys, ny, y, T);
  int oy[RGN_COVER], wy[RGN_COVER];
  cover(ys, ny, iy0, y, T, ramp, oy, wy);
  int ix0[V], ox[V][RGN_COVER], wx[V][RGN_COVER], den[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    ix0[j] = first_reaching(xs, nx, xb + j, T);
    cover(xs, nx, ix0[j], xb + j, T, ramp, ox[j], wx[j]);
    den[j] = 0;
#pragma unroll
    for (int a = 0; a < RGN_COVER; ++a)
#pragma unroll
      for (int b = 0; b < RGN_COVER; ++b) den[j] += wy[a] * wx[j][b];
  }
  const size_t tt = (size_t)T * T;
  for (int c = 0; c < C; ++c) {
    float r[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double num = 0.0;
#pragma unroll
      for (int a = 0; a < RGN_COVER; ++a)
#pragma unroll
        for (int b = 0; b < RGN_COVER; ++b) {
          const int w = wy[a] * wx[j][b];
          if (w > 0) {
            const size_t k = (size_t)(iy0 + a) * nx + (ix0[j] + b);
            num += (double)w * (double)win[(k * C + c) * tt + (size_t)oy[a] * T + ox[j][b]];
          }
        }
      r[j] = den[j] > 0 ? (float)(num / (double)den[j]) : NAN;
    }
    float* o = out + ((size_t)c * Hr + y) * Wr + xb;
    if constexpr (V == 4) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = r[j];
      *reinterpret_cast<f32x4*>(o) = v;
    } else {
      o[0] = r[0];
    }
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_region_gather(const unsigned char* dw_t1, const unsigned char* dw_t2, const float* rgb, const float* ndvi, const float* temp,
                      const int* origins, const double* norm, void* out, int ldo, int dtype, int B, int Tw, int Hr, int Wr, int ncls,
                      mau_stream_t stream) {
  MAU_REQUIRE(dw_t1 && dw_t2 && rgb && ndvi && temp && origins && norm && out, "region_gather: null pointer");
  MAU_REQUIRE(B > 0 && Tw > 0 && Hr > 0 && Wr > 0, "region_gather: non-positive dimension (B %d, T %d, region %d x %d)", B, Tw, Hr, Wr);
  MAU_REQUIRE(Tw <= Hr && Tw <= Wr, "region_gather: a window of %d does not fit a region of %d x %d", Tw, Hr, Wr);
  MAU_REQUIRE(ncls >= 1 && ncls <= SCN_MAX_CLS, "region_gather: ncls must be in [1,%d], got %d", SCN_MAX_CLS, ncls);
  MAU_REQUIRE(ldo % 8 == 0 && ldo >= 2 * ncls + SCN_NCONT, "region_gather: ldo must be a multiple of 8 and at least %d, got %d", 2 * ncls + SCN_NCONT, ldo);
  MAU_REQUIRE(Tw <= 4096 && B <= 65535, "region_gather: windows of at most 4096 x 4096, B must fit a grid dimension");
  MAU_REQUIRE((int64_t)Hr * Wr <= (1 << 30), "region_gather: regions of at most 2^30 pixels");
  MAU_REQUIRE((uintptr_t)out % 16 == 0, "region_gather: out must be 16-byte aligned");
  const dim3 grid(ceil_div((int64_t)Tw * Tw, 256), B);
  MAU_DISPATCH_DTYPE(dtype, MAU_LAUNCH(region_gather_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, dw_t1, dw_t2, rgb, ndvi, temp, origins,
                                       norm, (T*)out, ldo, Tw, Hr, Wr, ncls));
  return check_launch("region_gather_kernel");
}

int mau_region_stitch(const float* win, const int* ys, const int* xs, float* out, int C, int T, int ramp, int Hr, int Wr, int ny, int nx,
                      mau_stream_t stream) {
  MAU_REQUIRE(win && ys && xs && out, "region_stitch: null pointer");
  MAU_REQUIRE(C > 0 && T > 0 && Hr > 0 && Wr > 0 && ny > 0 && nx > 0, "region_stitch: non-positive dimension (C %d, T %d, region %d x %d, windows %d x %d)",
              C, T, Hr, Wr, ny, nx);
  MAU_REQUIRE(T <= Hr && T <= Wr && T <= 4096, "region_stitch: a window of %d does not fit a region of %d x %d (or exceeds 4096)", T, Hr, Wr);
  MAU_REQUIRE(ramp >= 1, "region_stitch: ramp must be >= 1, got %d", ramp);
  MAU_REQUIRE(Hr <= 65535, "region_stitch: Hr must fit a grid dimension");
  MAU_REQUIRE((int64_t)Hr * Wr <= (1 << 30) && (int64_t)ny * nx <= (1 << 20), "region_stitch: regions of at most 2^30 pixels and 2^20 windows");
  if (Wr % 4 == 0 && (uintptr_t)out % 16 == 0)
    MAU_LAUNCH(region_stitch_kernel<4>, dim3(ceil_div(Wr / 4, 256), Hr), dim3(256), 0, (hipStream_t)stream, win, ys, xs, out, C, T, ramp, Hr, Wr, ny, nx);
  else
    MAU_LAUNCH(region_stitch_kernel<1>, dim3(ceil_div(Wr, 256), Hr), dim3(256), 0, (hipStream_t)stream, win, ys, xs, out, C, T, ramp, Hr, Wr, ny, nx);
  return check_launch("region_stitch_kernel");
}

}  // extern "C"
