// placement.hip -- placement sweeps: where on a tile does a block of one land-cover class change the forecast most?  A placement is a
// rectangular stamp of ph x pw pixels of one class written into the tile's second class map (the app's canvas edit changes nothing
// else, app/processing_utils.py:70-110); its effect is the forecast with the stamp minus the forecast of the unedited tile.  The two
// streaming passes around the forward:
//   placement_pack_kernel    B stamped inputs from ONE resident tile and a table of (y0, x0, cls) rows in device memory, one launch;
//   placement_result_kernel  the head's output of the B samples against the unedited tile's -> twelve fp64 figures per placement.
//
// pack: grid = (chunks of 256 pixels, samples), one thread per pixel, the per-pixel code of scenario_pack_kernel and
// region_gather_kernel (scn_pixel.h): fp64 normalisation rounded to float once, one-hot channels, 16-byte channel-group stores.  The
// stamp test is made in 64-bit (0 <= y - y0 < ph, 0 <= x - x0 < pw): every int32 in the table is legal, a stamp over an edge is
// clipped, a stamp outside the tile or a class outside [0, ncls) leaves the tile as it is.  Nothing is indexed with a table value.
//
// result: a workgroup owns CHUNK_PIX consecutive pixels of ONE sample -- the chunking is a function of H * W alone.  The temperature
// is two separately rounded fp32 operations, for the sample and for the base alike (as scenario_result_kernel).  Sums are fp64 in the
// fixed order of chunk_reduce.h: a thread joins its 16 slots in slot order, block_join makes the chunk's partial row, and the
// workgroup that draws the sample's last ticket joins the partial rows in chunk order (chunk_join).  Two access forms, chosen by the
// host from H * W and the alignment of the buffers, never from B or the sample's slot:
//   V = 4 (H * W % 4 == 0, out and base 16-byte and roi 4-byte aligned): slot 4k + j of thread t is pixel (k * 256 + t) * 4 + j of
//         the chunk, one 16-byte load per plane and k;
//   V = 1 (otherwise): slot k of thread t is pixel k * 256 + t, 4-byte loads.
// A slot outside the (partial, last) chunk loads pixel 0 of the chunk and joins the identity (0, +inf, -inf).  The two forms add in
// different orders.  No float atomics; a row's bits depend on nothing but its own sample, the base and the roi.
#include <math.h>
#include "chunk_reduce.h"
#include "scn_pixel.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int PLC_ROW = 12;
// per-thread accumulators: 0 stamp pixels  1 sum dT  2 min dT  3 max dT  4 sum dT in the stamp  5 sum dT outside it  6 roi pixels
// 7 sum dT over the roi  8 sum dN  9 sum dN in the stamp  10 sum dN over the roi  11 non-finite values of the two out planes
constexpr int PLC_NV = 12;

// 0 <= p - o < n in 64-bit: o is any int32
__device__ __forceinline__ bool in_span(int p, int o, int n) {
  const int64_t d = (int64_t)p - (int64_t)o;
  return d >= 0 && d < (int64_t)n;
}

template <typename T>
__global__ __launch_bounds__(256) void placement_pack_kernel(const uint8_t* __restrict__ dw_t1, const uint8_t* __restrict__ dw_t2,
                                                             const float* __restrict__ rgb, const float* __restrict__ ndvi,
                                                             const float* __restrict__ temp, const int* __restrict__ edits,
                                                             const double* __restrict__ norm, T* __restrict__ out, int ld, int H, int W,
                                                             int ph, int pw, int nc) {
  const size_t hw = (size_t)H * W;
  const size_t ps = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (ps >= hw) return;
  const int n = blockIdx.y;
  const int y0 = edits[3 * n], x0 = edits[3 * n + 1], cls = edits[3 * n + 2];
  const int y = (int)(ps / (size_t)W), x = (int)(ps - (size_t)y * W);
  const bool stamped = cls >= 0 && cls < nc && in_span(y, y0, ph) && in_span(x, x0, pw);
  const int a = dw_t1[ps], b = stamped ? cls : dw_t2[ps];
  float cv[SCN_NCONT];
  scn_norm_planes(rgb, ndvi, temp, norm, hw, ps, cv);
  scn_store_pixel<T>(out + ((size_t)n * hw + ps) * ld, ld, nc, a, b, cv);
}

struct PlcJoin {
  __device__ __forceinline__ double operator()(int v, double a, double b) const { return v == 2 ? fmin(a, b) : v == 3 ? fmax(a, b) : a + b; }
};

// V consecutive floats at p (16-byte aligned when V == 4)
template <int V>
__device__ __forceinline__ void load_run(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 f = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = f[j];
  } else {
    v[0] = p[0];
  }
}

template <int V>
__global__ __launch_bounds__(256) void placement_result_kernel(const float* __restrict__ out, const float* __restrict__ base,
                                                               const int* __restrict__ edits, const uint8_t* __restrict__ roi, float tstd,
                                                               float tmean, double* part, unsigned* tickets, double* __restrict__ rows,
                                                               int64_t HW, int W, int ph, int pw, int n0) {
  __shared__ double wsum[4][PLC_NV];
  const int n = n0 + blockIdx.y, chunks = gridDim.x;
  const int64_t q0 = (int64_t)blockIdx.x * CHUNK_PIX;
  const int npx = (int)(HW - q0 < CHUNK_PIX ? HW - q0 : CHUNK_PIX);
  const float* o0 = out + (size_t)n * 2 * HW + q0;
  const float* o1 = o0 + HW;
  const float* b0 = base + q0;
  const float* b1 = b0 + HW;
  const int y0 = edits[3 * n], x0 = edits[3 * n + 1];

  double acc[PLC_NV] = {0.0, 0.0, INFINITY, -INFINITY, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4                                          // four k at a time: 20 loads in flight per thread (V = 4: the whole chunk)
  for (int k = 0; k < CHUNK_SLOTS / V; ++k) {
    const int idx = (k * 256 + (int)threadIdx.x) * V;
    const bool ok = idx < npx;                            // V == 4: npx % 4 == 0, a quad is inside or outside as a whole
    const int at = ok ? idx : 0;
    float vo0[V], vo1[V], vb0[V], vb1[V];
    load_run<V>(o0 + at, vo0);
    load_run<V>(o1 + at, vo1);
    load_run<V>(b0 + at, vb0);
    load_run<V>(b1 + at, vb1);
    unsigned rw = 0;
    if (roi != nullptr) {
      if constexpr (V == 4) rw = *reinterpret_cast<const unsigned*>(roi + q0 + at);
      else rw = roi[q0 + at];
    }
    const int64_t q = q0 + at;
    int y = (int)(q / W), x = (int)(q - (int64_t)y * W);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      // the products made opaque: the pair must not become one v_fma_f32 (see scenario_result_kernel)
      const float t = __fadd_rn(opaque(__fmul_rn(vo1[j], tstd)), tmean);
      const float tb = __fadd_rn(opaque(__fmul_rn(vb1[j], tstd)), tmean);
      const double dT = (double)__fsub_rn(t, tb), dN = (double)__fsub_rn(vo0[j], vb0[j]);
      const bool in = ok && in_span(y, y0, ph) && in_span(x, x0, pw);
      const bool inr = ok && ((rw >> (8 * j)) & 0xffu) != 0;
      acc[0] += in ? 1.0 : 0.0;
      acc[1] += ok ? dT : 0.0;
      acc[2] = fmin(acc[2], ok ? dT : INFINITY);          // fmin / fmax: a NaN is skipped (the means carry it)
      acc[3] = fmax(acc[3], ok ? dT : -INFINITY);
      acc[4] += in ? dT : 0.0;
      acc[5] += ok && !in ? dT : 0.0;
      acc[6] += inr ? 1.0 : 0.0;
      acc[7] += inr ? dT : 0.0;
      acc[8] += ok ? dN : 0.0;
      acc[9] += in ? dN : 0.0;
      acc[10] += inr ? dN : 0.0;
      acc[11] += ok ? (isfinite(vo0[j]) ? 0.0 : 1.0) + (isfinite(vo1[j]) ? 0.0 : 1.0) : 0.0;
      if (++x == W) {
        x = 0;
        ++y;
      }
    }
  }

  double* prow = part + (size_t)blockIdx.y * chunks * PLC_NV;
  block_join<PLC_NV>(acc, wsum, PlcJoin(), prow + (size_t)blockIdx.x * PLC_NV);
  if (!last_block_of(tickets + blockIdx.y, (unsigned)chunks)) return;

  // level 2: the sample's chunk partials in chunk order, then the finished row
  if (threadIdx.x < PLC_NV) wsum[0][threadIdx.x] = chunk_join(prow, chunks, PLC_NV, threadIdx.x, PlcJoin());
  __syncthreads();
  if (threadIdx.x < PLC_ROW) {
    const int e = threadIdx.x;
    const double* s = wsum[0];
    const double all = (double)HW, cnt = s[0], rest = all - cnt, nroi = s[6];
    double val;
    switch (e) {
      case 0: val = cnt; break;
      case 1: val = s[1] / all; break;
      case 2: val = s[2]; break;
      case 3: val = s[3]; break;
      case 4: val = cnt > 0.0 ? s[4] / cnt : NAN; break;
      case 5: val = rest > 0.0 ? s[5] / rest : NAN; break;
      case 6: val = nroi; break;
      case 7: val = nroi > 0.0 ? s[7] / nroi : NAN; break;
      case 8: val = s[8] / all; break;
      case 9: val = cnt > 0.0 ? s[9] / cnt : NAN; break;
      case 10: val = nroi > 0.0 ? s[10] / nroi : NAN; break;
      default: val = s[11]; break;
    }
    rows[(size_t)n * PLC_ROW + e] = val;
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_placement_row_elems(void) { return PLC_ROW; }

int mau_placement_chunks(int H, int W) { return H > 0 && W > 0 ? chunks_of((int64_t)H * W) : 0; }

size_t mau_placement_ws_elems(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)ticket_ws_rows(B) * chunks_of((int64_t)H * W) * PLC_NV;
}

int mau_placement_pack(const unsigned char* dw_t1, const unsigned char* dw_t2, const float* rgb, const float* ndvi, const float* temp,
                       const int* edits, const double* norm, void* out, int ldo, int dtype, int B, int H, int W, int ph, int pw, int ncls,
                       mau_stream_t stream) {
  MAU_REQUIRE(dw_t1 && rgb && ndvi && temp && edits && norm && out, "placement_pack: null pointer");
  MAU_REQUIRE(B > 0 && H > 0 && W > 0, "placement_pack: non-positive dimension (B %d, tile %d x %d)", B, H, W);
  MAU_REQUIRE(ph >= 1 && pw >= 1, "placement_pack: a stamp of at least 1 x 1, got %d x %d", ph, pw);
  MAU_REQUIRE(ncls >= 1 && ncls <= SCN_MAX_CLS, "placement_pack: ncls must be in [1,%d], got %d", SCN_MAX_CLS, ncls);
  MAU_REQUIRE(ldo % 8 == 0 && ldo >= 2 * ncls + SCN_NCONT, "placement_pack: ldo must be a multiple of 8 and at least %d, got %d", 2 * ncls + SCN_NCONT, ldo);
  MAU_REQUIRE(B <= 65535, "placement_pack: B must fit a grid dimension");
  MAU_REQUIRE((int64_t)H * W <= (1 << 30), "placement_pack: tiles of at most 2^30 pixels");
  MAU_REQUIRE((uintptr_t)out % 16 == 0, "placement_pack: out must be 16-byte aligned");
  if (dw_t2 == nullptr) dw_t2 = dw_t1;
  const dim3 grid(ceil_div((int64_t)H * W, 256), B);
  MAU_DISPATCH_DTYPE(dtype, MAU_LAUNCH(placement_pack_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, dw_t1, dw_t2, rgb, ndvi, temp, edits,
                                       norm, (T*)out, ldo, H, W, ph, pw, ncls));
  return check_launch("placement_pack_kernel");
}

int mau_placement_result(const float* out, const float* base, const int* edits, const unsigned char* roi, double temp_mean, double temp_std,
                         double* rows, double* ws, unsigned* tickets, int B, int H, int W, int ph, int pw, mau_stream_t stream) {
  MAU_REQUIRE(out && base && edits && rows && ws && tickets, "placement_result: null pointer");
  MAU_REQUIRE(B > 0 && H > 0 && W > 0, "placement_result: non-positive dimension (B %d, tile %d x %d)", B, H, W);
  MAU_REQUIRE(ph >= 1 && pw >= 1, "placement_result: a stamp of at least 1 x 1, got %d x %d", ph, pw);
  MAU_REQUIRE((int64_t)H * W <= (1 << 30), "placement_result: tiles of at most 2^30 pixels");
  const int64_t HW = (int64_t)H * W;
  const int chunks = chunks_of(HW);
  const bool vec4 = HW % 4 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)base % 16 == 0 && (uintptr_t)roi % 4 == 0;
  return for_ticket_rows(B, "placement_result_kernel", [&](int n0, int nn) {
    if (vec4)
      MAU_LAUNCH(placement_result_kernel<4>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, out, base, edits, roi, (float)temp_std,
                 (float)temp_mean, ws, tickets, rows, HW, W, ph, pw, n0);
    else
      MAU_LAUNCH(placement_result_kernel<1>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, out, base, edits, roi, (float)temp_std,
                 (float)temp_mean, ws, tickets, rows, HW, W, ph, pw, n0);
  });
}

}  // extern "C"
