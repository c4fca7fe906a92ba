// compare.hip -- the device side of a model comparison (reference app_dev/pages/1_Model_Comparison.py with
// app_dev/app_src/utils.py:170-271): M heads' outputs of ONE tile against one target.
//   compare_result_kernel  un-normalised predictions and target, the error maps, and per (model, channel) the colour ranges and
//                          error sums of the whole tile and of its four quadrants, one launch for all models;
//   compare_inputs_kernel  the page's views of the compact input sample (RGB as bytes, temperature in degrees C, NDVI, the two
//                          class maps through the palette), one launch per tile.
//
// result: a workgroup owns CHUNK_PIX consecutive pixels of ONE (model, channel) plane -- the chunking is a function of H * W
// alone.  The temperature channel is two separately rounded fp32 operations (numpy on a float32 array with Python-float scalars),
// the error one fp32 subtraction.  A pixel's quadrant follows from its (y, x); the seven accumulators of each quadrant stay in
// registers and are updated through selects (nothing is indexed dynamically).  Joins are those of chunk_reduce.h: a thread joins
// its pixels in slot order, block_join makes the chunk's partial row of 4 x 7 entries, and the workgroup that draws the row's last
// ticket joins the partial rows in chunk order (chunk_join) and then the four quadrants in the order TL, TR, BL, BR into the
// whole-tile entries.  No float atomics; a row's bits depend on nothing but its own plane and the target's.
#include <math.h>
#include "chunk_reduce.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int CMP_REGIONS = 5;           // whole tile, top-left, top-right, bottom-left, bottom-right
constexpr int CMP_ENTRIES = 8;           // pixels, gt min, gt max, pred min, pred max, max |err|, sum |err|, sum err^2
constexpr int CMP_ROW = CMP_REGIONS * CMP_ENTRIES;
constexpr int CMP_NJ = 7;                // accumulators per quadrant: the entries but the pixel count
constexpr int CMP_NV = 4 * CMP_NJ;

// accumulator v = quadrant * 7 + j; j: 0 gt min  1 gt max  2 pred min  3 pred max  4 max |err|  5 sum |err|  6 sum err^2
struct CmpJoin {
  __device__ __forceinline__ double operator()(int v, double a, double b) const {
    const int j = v % CMP_NJ;
    return (j == 0 || j == 2) ? fmin(a, b) : (j == 1 || j == 3 || j == 4) ? fmax(a, b) : a + b;
  }
};

// fl32(fl32(v * std) + mean) where un-normalising, v itself otherwise.  The product is made opaque: __fmul_rn / __fadd_rn are
// inlined with their own contraction flags and the pair otherwise comes out as one v_fma_f32 (see scenario.hip)
__device__ __forceinline__ float unnorm(float v, float tstd, float tmean, bool on) {
  const float t = __fadd_rn(opaque(__fmul_rn(v, tstd)), tmean);
  return on ? t : v;
}

template <bool VEC4>
__global__ __launch_bounds__(256) void compare_result_kernel(const float* __restrict__ out, const float* __restrict__ tgt, float tstd,
                                                             float tmean, float* __restrict__ pred_u, float* __restrict__ gt_u,
                                                             float* __restrict__ err, double* part, unsigned* tickets,
                                                             double* __restrict__ rows, int H, int W, int row0) {
  __shared__ double wsum[4][CMP_NV];
  const int row = row0 + blockIdx.y, chunks = gridDim.x;       // row = model * 2 + channel
  const int c = row & 1;
  const int64_t HW = (int64_t)H * W;
  const int64_t q0 = (int64_t)blockIdx.x * CHUNK_PIX;
  const int npx = (int)(HW - q0 < CHUNK_PIX ? HW - q0 : CHUNK_PIX);
  const float* o = out + (size_t)row * HW + q0;
  const float* g = tgt + (size_t)c * HW + q0;
  float* po = pred_u + (size_t)row * HW + q0;
  float* eo = err + (size_t)row * HW + q0;
  float* go = gt_u + (size_t)c * HW + q0;
  const bool write_gt = row < 2;                               // the target planes are written once, by model 0's workgroups
  const bool un = c == 1;
  const int hy = H / 2, hx = W / 2;
  const unsigned ok = slot_mask<VEC4>(npx);

  double acc[CMP_NV];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k * CMP_NJ + 0] = INFINITY;
    acc[k * CMP_NJ + 1] = -INFINITY;
    acc[k * CMP_NJ + 2] = INFINITY;
    acc[k * CMP_NJ + 3] = -INFINITY;
    acc[k * CMP_NJ + 4] = 0.0;
    acc[k * CMP_NJ + 5] = 0.0;
    acc[k * CMP_NJ + 6] = 0.0;
  }

  // one pixel: its slot is a pixel of the chunk (`in`) or a repeat of the chunk's pixel 0 that joins nothing
  auto pixel = [&](int idx, bool in, float pv, float gv, float ev) {
    const int q = (int)q0 + (in ? idx : 0);                   // H * W <= 2^30
    const int y = q / W, x = q - y * W;
    const int quad = (y >= hy ? 2 : 0) + (x >= hx ? 1 : 0);
    const double gd = (double)gv, pd = (double)pv, ed = (double)ev, ad = fabs(ed);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool on = in && quad == k;
      acc[k * CMP_NJ + 0] = fmin(acc[k * CMP_NJ + 0], on ? gd : INFINITY);      // fmin / fmax: a NaN is skipped
      acc[k * CMP_NJ + 1] = fmax(acc[k * CMP_NJ + 1], on ? gd : -INFINITY);
      acc[k * CMP_NJ + 2] = fmin(acc[k * CMP_NJ + 2], on ? pd : INFINITY);
      acc[k * CMP_NJ + 3] = fmax(acc[k * CMP_NJ + 3], on ? pd : -INFINITY);
      acc[k * CMP_NJ + 4] = fmax(acc[k * CMP_NJ + 4], on ? ad : 0.0);
      acc[k * CMP_NJ + 5] += on ? ad : 0.0;                                     // the sums carry a NaN
      acc[k * CMP_NJ + 6] += on ? ed * ed : 0.0;
    }
  };

  if (VEC4) {
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS / 4; ++k) {
      const bool in = (ok >> (4 * k)) & 1u;                    // npx is a multiple of 4: a quad is inside or outside as a whole
      const int idx = in ? (k * 256 + (int)threadIdx.x) * 4 : 0;
      const f32x4 ov = *reinterpret_cast<const f32x4*>(o + idx);
      const f32x4 tv = *reinterpret_cast<const f32x4*>(g + idx);
      f32x4 pv, gv, ev;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pv[j] = unnorm(ov[j], tstd, tmean, un);
        gv[j] = unnorm(tv[j], tstd, tmean, un);
        ev[j] = __fsub_rn(pv[j], gv[j]);
      }
      if (in) {
        *reinterpret_cast<f32x4*>(po + idx) = pv;
        *reinterpret_cast<f32x4*>(eo + idx) = ev;
        if (write_gt) *reinterpret_cast<f32x4*>(go + idx) = gv;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) pixel(idx + j, in, pv[j], gv[j], ev[j]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS; ++k) {
      const bool in = (ok >> k) & 1u;
      const int idx = in ? k * 256 + (int)threadIdx.x : 0;
      const float pv = unnorm(o[idx], tstd, tmean, un);
      const float gv = unnorm(g[idx], tstd, tmean, un);
      const float ev = __fsub_rn(pv, gv);
      if (in) {
        po[idx] = pv;
        eo[idx] = ev;
        if (write_gt) go[idx] = gv;
      }
      pixel(idx, in, pv, gv, ev);
    }
  }

  double* prow = part + (size_t)blockIdx.y * chunks * CMP_NV;
  block_join<CMP_NV>(acc, wsum, CmpJoin(), prow + (size_t)blockIdx.x * CMP_NV);
  if (!last_block_of(tickets + blockIdx.y, (unsigned)chunks)) return;

  // level 2: the row's chunk partials in chunk order, then the quadrants in the order TL, TR, BL, BR into the whole tile
  if (threadIdx.x < CMP_NV) wsum[0][threadIdx.x] = chunk_join(prow, chunks, CMP_NV, threadIdx.x, CmpJoin());
  __syncthreads();
  if (threadIdx.x < CMP_ROW) {
    const int r = threadIdx.x / CMP_ENTRIES, e = threadIdx.x % CMP_ENTRIES;
    const double* fin = wsum[0];
    double val;
    if (e == 0) {
      const int64_t ny = r == 0 ? H : r <= 2 ? hy : H - hy, nx = r == 0 ? W : (r & 1) ? hx : W - hx;
      val = (double)(ny * nx);
    } else if (r == 0) {
      const int j = e - 1;
      const CmpJoin op;
      val = op(j, op(j, op(j, fin[j], fin[CMP_NJ + j]), fin[2 * CMP_NJ + j]), fin[3 * CMP_NJ + j]);
    } else {
      val = fin[(r - 1) * CMP_NJ + e - 1];
    }
    rows[(size_t)row * CMP_ROW + threadIdx.x] = val;
  }
}

// one thread per pixel; norm: rgb_mean[3], rgb_std[3], temp_mean, temp_std (fp64)
__global__ __launch_bounds__(256) void compare_inputs_kernel(const uint8_t* __restrict__ cls_a, const uint8_t* __restrict__ cls_b,
                                                             const float* __restrict__ cont, const uint8_t* __restrict__ palette,
                                                             const double* __restrict__ norm, uint8_t* __restrict__ rgb8,
                                                             float* __restrict__ temp_c, float* __restrict__ ndvi,
                                                             uint8_t* __restrict__ dw_t1_rgb, uint8_t* __restrict__ dw_t2_rgb,
                                                             int64_t HW, int ncls) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= HW) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // float64, every operation rounded on its own: a float32 array times a float64 array, plus one, times 255.0
    const double v = ((double)cont[j * HW + q] * norm[3 + j] + norm[j]) * 255.0;
    const double cl = v >= 0.0 ? (v > 255.0 ? 255.0 : v) : 0.0;       // clip; a NaN becomes 0
    rgb8[q * 3 + j] = (uint8_t)(int)cl;                               // truncation toward zero
  }
  ndvi[q] = cont[3 * HW + q];
  temp_c[q] = unnorm(cont[4 * HW + q], (float)norm[7], (float)norm[6], true);
  const int a = cls_a[q], b = cls_b[q];
  const int ia = a < ncls ? a : 0, ib = b < ncls ? b : 0;             // unconditional loads, the zero a select
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint8_t pa = palette[3 * ia + j], pb = palette[3 * ib + j];
    dw_t1_rgb[q * 3 + j] = a < ncls ? pa : (uint8_t)0;
    dw_t2_rgb[q * 3 + j] = b < ncls ? pb : (uint8_t)0;
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_compare_row_elems(void) { return CMP_ROW; }

int mau_compare_chunks(int H, int W) { return H > 0 && W > 0 ? chunks_of((int64_t)H * W) : 0; }

size_t mau_compare_ws_elems(int M, int H, int W) {
  if (M <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)ticket_ws_rows((int64_t)M * 2) * chunks_of((int64_t)H * W) * CMP_NV;
}

int mau_compare_result(const float* out, const float* tgt, double temp_mean, double temp_std, float* pred_u, float* gt_u, float* err,
                       double* rows, double* ws, unsigned* tickets, int M, int H, int W, mau_stream_t stream) {
  MAU_REQUIRE(out && tgt && pred_u && gt_u && err && rows && ws && tickets, "compare_result: null pointer");
  MAU_REQUIRE(M > 0 && H > 0 && W > 0, "compare_result: non-positive dimension (M %d, H %d, W %d)", M, H, W);
  MAU_REQUIRE((int64_t)H * W <= (1 << 30), "compare_result: maps of at most 2^30 pixels");
  MAU_REQUIRE(M <= (1 << 20), "compare_result: at most 2^20 models");
  const int64_t HW = (int64_t)H * W;
  const int chunks = chunks_of(HW);
  const bool vec4 = HW % 4 == 0 && ((uintptr_t)out | (uintptr_t)tgt | (uintptr_t)pred_u | (uintptr_t)gt_u | (uintptr_t)err) % 16 == 0;
  return for_ticket_rows(M * 2, "compare_result_kernel", [&](int row0, int n) {
    if (vec4)
      MAU_LAUNCH(compare_result_kernel<true>, dim3(chunks, n), dim3(256), 0, (hipStream_t)stream, out, tgt, (float)temp_std,
                 (float)temp_mean, pred_u, gt_u, err, ws, tickets, rows, H, W, row0);
    else
      MAU_LAUNCH(compare_result_kernel<false>, dim3(chunks, n), dim3(256), 0, (hipStream_t)stream, out, tgt, (float)temp_std,
                 (float)temp_mean, pred_u, gt_u, err, ws, tickets, rows, H, W, row0);
  });
}

int mau_compare_inputs(const unsigned char* cls_a, const unsigned char* cls_b, const float* cont, const unsigned char* palette,
                       const double* norm, unsigned char* rgb8, float* temp_c, float* ndvi, unsigned char* dw_t1_rgb,
                       unsigned char* dw_t2_rgb, int H, int W, int ncls, mau_stream_t stream) {
  MAU_REQUIRE(cls_a && cls_b && cont && palette && norm && rgb8 && temp_c && ndvi && dw_t1_rgb && dw_t2_rgb, "compare_inputs: null pointer");
  MAU_REQUIRE(H > 0 && W > 0, "compare_inputs: non-positive dimension (H %d, W %d)", H, W);
  MAU_REQUIRE(ncls >= 1 && ncls <= mau_scenario_max_classes(), "compare_inputs: ncls must be in [1,%d], got %d", mau_scenario_max_classes(), ncls);
  MAU_REQUIRE((int64_t)H * W <= (1 << 30), "compare_inputs: maps of at most 2^30 pixels");
  const int64_t HW = (int64_t)H * W;
  MAU_LAUNCH(compare_inputs_kernel, dim3(ceil_div(HW, 256)), dim3(256), 0, (hipStream_t)stream, cls_a, cls_b, cont, palette, norm, rgb8,
             temp_c, ndvi, dw_t1_rgb, dw_t2_rgb, HW, ncls);
  return check_launch("compare_inputs_kernel");
}

}  // extern "C"
