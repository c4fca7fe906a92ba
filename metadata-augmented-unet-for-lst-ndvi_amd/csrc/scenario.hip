// scenario.hip -- the two ends of an interactive scenario edit (reference app/Home.py:333-411, app/processing_utils.py:70-181):
//   scenario_pack_kernel    painted RGBA canvases + one base tile -> the network's input and the edited class maps, one launch;
//   scenario_result_kernel  the head's output -> NDVI, temperature in degrees C, its difference to the original raster and
//                           five statistics of that difference per scenario, one launch.
//
// pack: grid = (x chunks, rows, scenarios), one thread per pixel as pack_tile_onehot_kernel (spatial.hip), 16-byte channel-group
// stores.  The canvas is sampled through two index tables (nearest neighbour: source row per destination row, source column per
// destination column); a painted pixel (alpha > 0) takes the palette entry of smallest squared RGB distance, the lowest index on
// a tie -- integer arithmetic, which is what cdist + argmin give (the squares are exact in fp64 and sqrt is monotone).  The five
// continuous planes are normalised in fp64 with IEEE division and rounded to float once: the bits of the reference's float64
// numpy followed by .float() (scn_pixel.h, shared with region_gather_kernel).  A table entry outside the canvas is clamped (no
// read outside the buffer).
//
// result: a workgroup owns CHUNK_PIX consecutive pixels of ONE scenario -- the chunking is a function of H * W alone.  The
// temperature is two separately rounded fp32 operations (numpy on a float32 array with Python-float scalars).  Sums are fp64 in
// the fixed order of chunk_reduce.h: a thread adds its pixels in index order, block_join makes the chunk's partial row, and the
// workgroup that draws the scenario's last ticket joins the partial rows in chunk order (chunk_join).  No float atomics; a row's
// bits depend on nothing but its own scenario.
#include <math.h>
#include "chunk_reduce.h"
#include "scn_pixel.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int SCN_ROW = 5;               // mean, min, max of the difference, edited pixels, mean of the difference over them
// per-thread accumulators: 0 sum d  1 min d  2 max d  3 edited pixels  4 sum d over edited pixels
constexpr int SCN_NV = 5;

template <typename T>
__global__ __launch_bounds__(256) void scenario_pack_kernel(const uint8_t* __restrict__ dw_t1, const float* __restrict__ rgb,
                                                            const float* __restrict__ ndvi, const float* __restrict__ temp,
                                                            const uint8_t* __restrict__ canvas, const int* __restrict__ yidx,
                                                            const int* __restrict__ xidx, const uint8_t* __restrict__ palette,
                                                            const double* __restrict__ norm, T* __restrict__ out,
                                                            uint8_t* __restrict__ dw_t2, int ld, int H, int W, int Hc, int Wc, int nc) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  const int y = blockIdx.y, n = blockIdx.z;
  const size_t hw = (size_t)H * W, ps = (size_t)y * W + x;
  const int a = dw_t1[ps];
  int ys = yidx[y], xs = xidx[x];
  ys = ys < 0 ? 0 : ys >= Hc ? Hc - 1 : ys;
  xs = xs < 0 ? 0 : xs >= Wc ? Wc - 1 : xs;
  const uchar4 p = *reinterpret_cast<const uchar4*>(canvas + (((size_t)n * Hc + ys) * Wc + xs) * 4);
  int b = a;
  if (p.w > 0) {
    int best = 0x7fffffff;
    for (int k = 0; k < nc; ++k) {
      const int dr = (int)p.x - palette[3 * k], dg = (int)p.y - palette[3 * k + 1], db = (int)p.z - palette[3 * k + 2];
      const int d = dr * dr + dg * dg + db * db;
      if (d < best) {                                    // strict: the first minimum wins
        best = d;
        b = k;
      }
    }
  }
  dw_t2[n * hw + ps] = (uint8_t)b;
  float cv[SCN_NCONT];
  scn_norm_planes(rgb, ndvi, temp, norm, hw, ps, cv);
  scn_store_pixel<T>(out + (n * hw + ps) * ld, ld, nc, a, b, cv);
}

struct ScnJoin {
  __device__ __forceinline__ double operator()(int v, double a, double b) const { return v == 1 ? fmin(a, b) : v == 2 ? fmax(a, b) : a + b; }
};

__global__ __launch_bounds__(256) void scenario_result_kernel(const float* __restrict__ out, const float* __restrict__ temp_orig,
                                                              const uint8_t* __restrict__ dw_t1, const uint8_t* __restrict__ dw_t2,
                                                              float tstd, float tmean, float* __restrict__ ndvi,
                                                              float* __restrict__ temp_c, float* __restrict__ delta, double* part,
                                                              unsigned* tickets, double* __restrict__ rows, int64_t HW, int n0) {
  __shared__ double wsum[4][SCN_NV];
  const int n = n0 + blockIdx.y, chunks = gridDim.x;
  const float* o0 = out + (size_t)n * 2 * HW;
  const float* o1 = o0 + HW;
  const uint8_t* e2 = dw_t2 + (size_t)n * HW;
  float* nd = ndvi + (size_t)n * HW;
  float* tc = temp_c + (size_t)n * HW;
  float* dl = delta != nullptr ? delta + (size_t)n * HW : nullptr;
  const bool have = temp_orig != nullptr;
  const int64_t q0 = (int64_t)blockIdx.x * CHUNK_PIX;
  const int npx = (int)(HW - q0 < CHUNK_PIX ? HW - q0 : CHUNK_PIX);

  double acc[SCN_NV] = {0.0, INFINITY, -INFINITY, 0.0, 0.0};
  for (int idx = threadIdx.x; idx < npx; idx += 256) {
    const int64_t q = q0 + idx;
    nd[q] = o0[q];
    // the product made opaque: __fmul_rn / __fadd_rn are inlined from the headers WITH their contraction flags, and the pair
    // came out as one v_fma_f32 (the file's contract(off) does not reach them)
    const float t = __fadd_rn(opaque(__fmul_rn(o1[q], tstd)), tmean);
    tc[q] = t;
    const bool edited = e2[q] != dw_t1[q];
    acc[3] += edited ? 1.0 : 0.0;
    if (have) {
      const float df = __fsub_rn(t, temp_orig[q]);
      dl[q] = df;
      const double d = (double)df;
      acc[0] += d;
      acc[1] = fmin(acc[1], d);                          // fmin / fmax: a NaN is skipped (the mean carries it)
      acc[2] = fmax(acc[2], d);
      acc[4] += edited ? d : 0.0;
    }
  }

  double* prow = part + (size_t)blockIdx.y * chunks * SCN_NV;
  block_join<SCN_NV>(acc, wsum, ScnJoin(), prow + (size_t)blockIdx.x * SCN_NV);
  if (!last_block_of(tickets + blockIdx.y, (unsigned)chunks)) return;

  // level 2: the scenario's chunk partials in chunk order, then the finished row
  if (threadIdx.x < SCN_NV) wsum[0][threadIdx.x] = chunk_join(prow, chunks, SCN_NV, threadIdx.x, ScnJoin());
  __syncthreads();
  if (threadIdx.x < SCN_ROW) {
    const int e = threadIdx.x;
    const double cnt = wsum[0][3];
    double val;
    if (e == 3) val = cnt;
    else if (!have) val = NAN;
    else if (e == 0) val = wsum[0][0] / (double)HW;
    else if (e == 4) val = cnt > 0.0 ? wsum[0][4] / cnt : NAN;
    else val = wsum[0][e];
    rows[(size_t)n * SCN_ROW + e] = val;
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_scenario_max_classes(void) { return SCN_MAX_CLS; }

int mau_scenario_result_row_elems(void) { return SCN_ROW; }

int mau_scenario_result_chunks(int H, int W) { return H > 0 && W > 0 ? chunks_of((int64_t)H * W) : 0; }

size_t mau_scenario_result_ws_elems(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)ticket_ws_rows(N) * chunks_of((int64_t)H * W) * SCN_NV;
}

int mau_scenario_pack(const unsigned char* dw_t1, const float* rgb, const float* ndvi, const float* temp, const unsigned char* canvas,
                      const int* yidx, const int* xidx, const unsigned char* palette, const double* norm, void* out, int ldo,
                      unsigned char* dw_t2, int dtype, int N, int H, int W, int Hc, int Wc, int ncls, mau_stream_t stream) {
  MAU_REQUIRE(dw_t1 && rgb && ndvi && temp && canvas && yidx && xidx && palette && norm && out && dw_t2, "scenario_pack: null pointer");
  MAU_REQUIRE(N > 0 && H > 0 && W > 0 && Hc > 0 && Wc > 0, "scenario_pack: non-positive dimension (N %d, H %d, W %d, canvas %d x %d)", N, H, W, Hc, Wc);
  MAU_REQUIRE(ncls >= 1 && ncls <= SCN_MAX_CLS, "scenario_pack: ncls must be in [1,%d], got %d", SCN_MAX_CLS, ncls);
  MAU_REQUIRE(ldo % 8 == 0 && ldo >= 2 * ncls + SCN_NCONT, "scenario_pack: ldo must be a multiple of 8 and at least %d, got %d", 2 * ncls + SCN_NCONT, ldo);
  MAU_REQUIRE(H <= 65535 && N <= 65535, "scenario_pack: H and N must fit a grid dimension");
  MAU_REQUIRE((int64_t)H * W <= (1 << 30) && (int64_t)Hc * Wc <= (1 << 30), "scenario_pack: tiles and canvases of at most 2^30 pixels");
  MAU_REQUIRE((uintptr_t)canvas % 4 == 0 && (uintptr_t)out % 16 == 0, "scenario_pack: canvas must be 4-byte and out 16-byte aligned");
  const dim3 grid(ceil_div(W, 256), H, N);
  MAU_DISPATCH_DTYPE(dtype, MAU_LAUNCH(scenario_pack_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, dw_t1, rgb, ndvi, temp, canvas, yidx,
                                       xidx, palette, norm, (T*)out, dw_t2, ldo, H, W, Hc, Wc, ncls));
  return check_launch("scenario_pack_kernel");
}

int mau_scenario_result(const float* out, const float* temp_orig, const unsigned char* dw_t1, const unsigned char* dw_t2, double temp_mean,
                        double temp_std, float* ndvi, float* temp_c, float* delta, double* rows, double* ws, unsigned* tickets, int N,
                        int H, int W, mau_stream_t stream) {
  MAU_REQUIRE(out && dw_t1 && dw_t2 && ndvi && temp_c && rows && ws && tickets, "scenario_result: null pointer");
  MAU_REQUIRE(temp_orig == nullptr || delta != nullptr, "scenario_result: delta is needed with temp_orig");
  MAU_REQUIRE(N > 0 && H > 0 && W > 0, "scenario_result: non-positive dimension (N %d, H %d, W %d)", N, H, W);
  MAU_REQUIRE((int64_t)H * W <= (1 << 30), "scenario_result: maps of at most 2^30 pixels");
  const int64_t HW = (int64_t)H * W;
  const int chunks = chunks_of(HW);
  return for_ticket_rows(N, "scenario_result_kernel", [&](int n0, int nn) {
    MAU_LAUNCH(scenario_result_kernel, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, out, temp_orig, dw_t1, dw_t2, (float)temp_std,
               (float)temp_mean, ndvi, temp_c, delta, ws, tickets, rows, HW, n0);
  });
}

}  // extern "C"
