// evalmetrics.hip -- per-(sample, channel) error metrics of the test-split evaluation, per land-cover class, in one launch.
//
// Everything a row of the reference's test/evaluate.py holds is a sum over the pixels of (prediction, target, class id):
//   overall MAE / RMSE, MAE / RMSE and pixel count per class, the population variance of the 5-point Laplacian of both
//   maps (scipy.ndimage.laplace, boundary mode 'reflect': the edge sample repeated), non-finite counts and min / max.
// Grid (row chunks, (sample, channel) rows): a workgroup owns CHUNK_PIX / W (at least one) consecutive image rows of ONE
// map -- the chunking is a function of (H, W) alone.  Every value becomes a double as it is loaded, p = out * scale + shift
// and g = tgt * scale + shift are fp64 products and sums without contraction, and every sum is fp64 in the fixed order of
// chunk_reduce.h: a thread adds its pixels in index order, block_join makes the chunk's partial row, and the workgroup that
// draws the row's last ticket joins the partial rows in chunk order (chunk_join) and writes the finished row.  A row's bits
// depend on nothing but its own maps.
// The class sums are kept in registers: bin k takes `cls == k ? value : 0`, one select per bin and pixel, so that no
// accumulator is indexed dynamically (fp64 rate is not what limits a kernel that reads 9 bytes per pixel).
#include <math.h>
#include "eval_row.h"

#pragma clang fp contract(off)

namespace mau {

template <int NB>
__global__ __launch_bounds__(256) void eval_metrics_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                           const unsigned char* __restrict__ cls, const double* __restrict__ scale,
                                                           const double* __restrict__ shift, double* part, unsigned* tickets,
                                                           double* __restrict__ rows, int C, int H, int W, int ncls, int rpc,
                                                           int row0) {
  constexpr int NV = EVAL_ACC0 + 3 * NB;
  __shared__ double wsum[4][NV];
  __shared__ double tot[NV];
  const int row = row0 + blockIdx.y, chunks = gridDim.x;
  const int b = row / C, c = row - b * C;
  const double sc = scale != nullptr ? scale[c] : 1.0, sh = shift != nullptr ? shift[c] : 0.0;
  const size_t HW = (size_t)H * W;
  const float* o = out + (size_t)row * HW;
  const float* t = tgt + (size_t)row * HW;
  const unsigned char* k = cls + (size_t)b * HW;
  const int i0 = blockIdx.x * rpc;
  const int i1 = i0 + rpc < H ? i0 + rpc : H;
  const int npx = (i1 - i0) * W;

  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
  acc[8] = acc[10] = INFINITY;
  acc[9] = acc[11] = -INFINITY;

  for (int idx = threadIdx.x; idx < npx; idx += 256) {
    const EvalStencil s = eval_stencil(idx, i0, H, W);
    const size_t q = s.q;
    float of, tf;
    double p, lp, g, lg;
    eval_value_lap(o, s, sc, sh, of, p, lp);
    eval_value_lap(t, s, sc, sh, tf, g, lg);
    const double d = p - g;
    const double a = fabs(d), d2 = d * d;
    acc[0] += a;
    acc[1] += d2;
    acc[2] += lp;
    acc[3] += lp * lp;
    acc[4] += lg;
    acc[5] += lg * lg;
    acc[6] += isfinite(of) ? 0.0 : 1.0;
    acc[7] += isfinite(tf) ? 0.0 : 1.0;
    acc[8] = fmin(acc[8], p);             // fmin / fmax: a NaN is skipped (it is counted above)
    acc[9] = fmax(acc[9], p);
    acc[10] = fmin(acc[10], g);
    acc[11] = fmax(acc[11], g);
    const int id = k[q];
    const int bin = id < ncls ? id : NB - 1;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const bool m = bin == n;
      acc[EVAL_ACC0 + n] += m ? 1.0 : 0.0;
      acc[EVAL_ACC0 + NB + n] += m ? a : 0.0;
      acc[EVAL_ACC0 + 2 * NB + n] += m ? d2 : 0.0;
    }
  }

  double* prow = part + (size_t)blockIdx.y * chunks * NV;
  block_join<NV>(acc, wsum, EvalJoin(), prow + (size_t)blockIdx.x * NV);
  if (!last_block_of(tickets + blockIdx.y, (unsigned)chunks)) return;

  // level 2: the row's chunk partials in chunk order, then the finished row
  if (threadIdx.x < NV) tot[threadIdx.x] = chunk_join(prow, chunks, NV, threadIdx.x, EvalJoin());
  __syncthreads();
  const int relems = EVAL_HEAD + 3 * ncls;
  double* r = rows + (size_t)row * relems;
  const double n = (double)HW;
  const int e = threadIdx.x;
  if (e < relems) r[e] = eval_row_entry<NB>(tot, e, ncls, n);
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_eval_metrics_row_elems(int ncls) { return ncls >= 1 && ncls <= EVAL_MAX_CLS ? EVAL_HEAD + 3 * ncls : 0; }

int mau_eval_metrics_chunks(int H, int W) { return H > 0 && W > 0 ? eval_chunks(H, W) : 0; }

size_t mau_eval_metrics_ws_elems(int B, int C, int H, int W, int ncls) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || ncls < 1 || ncls > EVAL_MAX_CLS) return 0;
  return (size_t)ticket_ws_rows((int64_t)B * C) * eval_chunks(H, W) * (EVAL_ACC0 + 3 * eval_bins(ncls));
}

int mau_eval_metrics(const float* out, const float* tgt, const unsigned char* cls, const double* scale, const double* shift,
                     double* rows, double* ws, unsigned* tickets, int B, int C, int H, int W, int ncls, mau_stream_t stream) {
  MAU_REQUIRE(out && tgt && cls && rows && ws && tickets, "eval_metrics: null pointer");
  MAU_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "eval_metrics: non-positive dimension (B %d, C %d, H %d, W %d)", B, C, H, W);
  MAU_REQUIRE(ncls >= 1 && ncls <= EVAL_MAX_CLS, "eval_metrics: ncls must be in [1,%d], got %d", EVAL_MAX_CLS, ncls);
  MAU_REQUIRE((int64_t)H * W <= (1 << 30), "eval_metrics: maps of at most 2^30 pixels");
  MAU_REQUIRE((int64_t)B * C <= (1 << 30), "eval_metrics: at most 2^30 (sample, channel) rows");
  const int rpc = eval_rows_per_chunk(W), chunks = eval_chunks(H, W);
  const dim3 block(256);
  const hipStream_t st = (hipStream_t)stream;
  return for_ticket_rows(B * C, "eval_metrics_kernel", [&](int row0, int nn) {
    const dim3 grid(chunks, nn);
    if (eval_bins(ncls) == 10)
      MAU_LAUNCH(eval_metrics_kernel<10>, grid, block, 0, st, out, tgt, cls, scale, shift, ws, tickets, rows, C, H, W, ncls, rpc, row0);
    else
      MAU_LAUNCH(eval_metrics_kernel<EVAL_MAX_CLS + 1>, grid, block, 0, st, out, tgt, cls, scale, shift, ws, tickets, rows, C, H, W, ncls, rpc, row0);
  });
}

}  // extern "C"
