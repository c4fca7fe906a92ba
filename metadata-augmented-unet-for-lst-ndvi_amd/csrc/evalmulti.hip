// evalmulti.hip -- the evaluation metrics of M models' outputs against ONE target and class map, in one launch (the statistical
// comparison of checkpoints, mau_amd.statistics).  Row [m][b * C + c] has the bits mau_eval_metrics gives for out[m]: the chunking,
// the per-thread pixel order, block_join, the last-ticket chunk_join in chunk order and the finished row are eval_row.h's and
// chunk_reduce.h's, shared with evalmetrics.hip.
//
// Grid (row chunks, (sample, channel) rows), as evalmetrics.hip: a workgroup owns one chunk of one (sample, channel) and walks the
// M models over it.  What depends on the target alone is formed ONCE, in the first pass: the un-normalised target g, its Laplacian
// and the class bin of the thread's <= 16 pixels stay in registers (32 + 32 + 4 VGPRs), the target-only accumulators (sums of
// lap(g), non-finite targets, min / max of g, class counts) are joined once and written into every model's row.  A pass of a model
// then reads 4 bytes per pixel (and its stencil neighbours from cache) instead of 9.
// Registers, not LDS: a thread only ever needs its own 16 pixels again, so LDS would buy no sharing, and 64 KiB of it per
// workgroup would leave two workgroups per CU.  The model accumulators are 7 + 2 NB doubles (27 / 41) instead of the 42 / 63 of
// the one-model kernel, which pays for the kept values.
// A map wider than CHUNK_PIX (one image row per chunk, more than 16 pixels per thread) cannot be kept: the target values are then
// formed again per model, tile by tile -- the same bits, the one-model kernel's traffic.
#include <math.h>
#include "eval_row.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int EVAL_MULTI_MAX = 8;
constexpr int EVAL_TGT0 = 5;             // target-only accumulators: lap(g) sum, sum of squares, non-finite tgt, min g, max g, then NB counts
constexpr int EVAL_MOD0 = 7;             // per-model: sum|d|, sum d^2, lap(p) sum, sum of squares, non-finite out, min p, max p, then 2 NB sums

// index of a compact accumulator in the one-model kernel's layout (eval_row.h)
__device__ __forceinline__ int eval_tgt_index(int i) { return i == 0 ? 4 : i == 1 ? 5 : i == 2 ? 7 : i == 3 ? 10 : i == 4 ? 11 : EVAL_ACC0 + i - EVAL_TGT0; }
template <int NB>
__device__ __forceinline__ int eval_mod_index(int i) { return i < 4 ? i : i == 4 ? 6 : i == 5 ? 8 : i == 6 ? 9 : EVAL_ACC0 + NB + i - EVAL_MOD0; }

struct EvalTgtJoin {
  __device__ __forceinline__ double operator()(int i, double a, double b) const { return EvalJoin()(eval_tgt_index(i), a, b); }
};
template <int NB>
struct EvalModJoin {
  __device__ __forceinline__ double operator()(int i, double a, double b) const { return EvalJoin()(eval_mod_index<NB>(i), a, b); }
};

template <int NB>
__global__ __launch_bounds__(256) void eval_metrics_multi_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                                 const unsigned char* __restrict__ cls, const double* __restrict__ scale,
                                                                 const double* __restrict__ shift, double* part, unsigned* tickets,
                                                                 double* __restrict__ rows, int M, int nrows, int C, int H, int W,
                                                                 int ncls, int rpc, int row0) {
  constexpr int NV = EVAL_ACC0 + 3 * NB, TV = EVAL_TGT0 + NB, MV = EVAL_MOD0 + 2 * NB;
  __shared__ double wsum_t[4][TV];
  __shared__ double wsum_m[4][MV];
  __shared__ double tot[NV];
  const int row = row0 + blockIdx.y, chunks = gridDim.x;
  const int b = row / C, c = row - b * C;
  const double sc = scale != nullptr ? scale[c] : 1.0, sh = shift != nullptr ? shift[c] : 0.0;
  const size_t HW = (size_t)H * W;
  const float* t = tgt + (size_t)row * HW;
  const unsigned char* k = cls + (size_t)b * HW;
  const int i0 = blockIdx.x * rpc;
  const int i1 = i0 + rpc < H ? i0 + rpc : H;
  const int npx = (i1 - i0) * W;
  const bool keep = npx <= CHUNK_PIX;      // every map at most CHUNK_PIX wide
  const int pstride = TV + M * MV;         // a chunk's partials: the target's, then the M models'
  double* prow = part + (size_t)blockIdx.y * chunks * pstride;
  double* pchunk = prow + (size_t)blockIdx.x * pstride;

  double g[CHUNK_SLOTS], lg[CHUNK_SLOTS];  // the thread's target values of the tile, slot s = pixel base + s * 256 + thread
  unsigned bins[CHUNK_SLOTS / 4];          // their class bins, four to a word
  double tacc[TV];
#pragma unroll
  for (int v = 0; v < TV; ++v) tacc[v] = 0.0;
  tacc[3] = INFINITY;
  tacc[4] = -INFINITY;

  for (int m = 0; m < M; ++m) {
    const float* o = out + ((size_t)m * nrows + row) * HW;
    double acc[MV];
#pragma unroll
    for (int v = 0; v < MV; ++v) acc[v] = 0.0;
    acc[5] = INFINITY;
    acc[6] = -INFINITY;
    for (int base = 0; base < npx; base += CHUNK_PIX) {
      if (m == 0 || !keep) {
#pragma unroll
        for (int w = 0; w < CHUNK_SLOTS / 4; ++w) bins[w] = 0;
#pragma unroll
        for (int s = 0; s < CHUNK_SLOTS; ++s) {
          const int idx = base + s * 256 + (int)threadIdx.x;
          g[s] = lg[s] = 0.0;
          if (idx < npx) {
            const EvalStencil st = eval_stencil(idx, i0, H, W);
            float tf;
            eval_value_lap(t, st, sc, sh, tf, g[s], lg[s]);
            const int id = k[st.q];
            const int bin = id < ncls ? id : NB - 1;
            bins[s >> 2] |= (unsigned)bin << (8 * (s & 3));
            if (m == 0) {
              tacc[0] += lg[s];
              tacc[1] += lg[s] * lg[s];
              tacc[2] += isfinite(tf) ? 0.0 : 1.0;
              tacc[3] = fmin(tacc[3], g[s]);     // fmin / fmax: a NaN is skipped (it is counted above)
              tacc[4] = fmax(tacc[4], g[s]);
#pragma unroll
              for (int n = 0; n < NB; ++n) tacc[EVAL_TGT0 + n] += bin == n ? 1.0 : 0.0;
            }
          }
        }
      }
#pragma unroll
      for (int s = 0; s < CHUNK_SLOTS; ++s) {
        const int idx = base + s * 256 + (int)threadIdx.x;
        if (idx < npx) {
          const EvalStencil st = eval_stencil(idx, i0, H, W);
          float of;
          double p, lp;
          eval_value_lap(o, st, sc, sh, of, p, lp);
          const double d = p - g[s];
          const double a = fabs(d), d2 = d * d;
          acc[0] += a;
          acc[1] += d2;
          acc[2] += lp;
          acc[3] += lp * lp;
          acc[4] += isfinite(of) ? 0.0 : 1.0;
          acc[5] = fmin(acc[5], p);
          acc[6] = fmax(acc[6], p);
          const int bin = (bins[s >> 2] >> (8 * (s & 3))) & 0xff;
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            const bool in = bin == n;
            acc[EVAL_MOD0 + n] += in ? a : 0.0;
            acc[EVAL_MOD0 + NB + n] += in ? d2 : 0.0;
          }
        }
      }
    }
    if (m == 0) block_join<TV>(tacc, wsum_t, EvalTgtJoin(), pchunk);
    if (m > 0) __syncthreads();            // the previous model's partials have been read out of wsum_m
    block_join<MV>(acc, wsum_m, EvalModJoin<NB>(), pchunk + TV + (size_t)m * MV);
  }
  if (!last_block_of(tickets + blockIdx.y, (unsigned)chunks)) return;

  // level 2: the row's chunk partials in chunk order -- the target's once, then model by model -- and the finished rows
  const int relems = EVAL_HEAD + 3 * ncls;
  const double n = (double)HW;
  const int e = threadIdx.x;
  if (e < TV) tot[eval_tgt_index(e)] = chunk_join(prow, chunks, pstride, e, EvalTgtJoin());
  for (int m = 0; m < M; ++m) {
    if (e < MV) tot[eval_mod_index<NB>(e)] = chunk_join(prow + TV + (size_t)m * MV, chunks, pstride, e, EvalModJoin<NB>());
    __syncthreads();
    if (e < relems) rows[((size_t)m * nrows + row) * relems + e] = eval_row_entry<NB>(tot, e, ncls, n);
    __syncthreads();
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_eval_metrics_multi_max_models(void) { return EVAL_MULTI_MAX; }

size_t mau_eval_metrics_multi_ws_elems(int M, int B, int C, int H, int W, int ncls) {
  if (M < 1 || M > EVAL_MULTI_MAX || B <= 0 || C <= 0 || H <= 0 || W <= 0 || ncls < 1 || ncls > EVAL_MAX_CLS) return 0;
  const int nb = eval_bins(ncls);
  return (size_t)ticket_ws_rows((int64_t)B * C) * eval_chunks(H, W) * ((EVAL_TGT0 + nb) + (size_t)M * (EVAL_MOD0 + 2 * nb));
}

int mau_eval_metrics_multi(const float* out, const float* tgt, const unsigned char* cls, const double* scale, const double* shift,
                           double* rows, double* ws, unsigned* tickets, int M, int B, int C, int H, int W, int ncls,
                           mau_stream_t stream) {
  MAU_REQUIRE(out && tgt && cls && rows && ws && tickets, "eval_metrics_multi: null pointer");
  MAU_REQUIRE(M >= 1 && M <= EVAL_MULTI_MAX, "eval_metrics_multi: M must be in [1,%d], got %d", EVAL_MULTI_MAX, M);
  MAU_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "eval_metrics_multi: non-positive dimension (B %d, C %d, H %d, W %d)", B, C, H, W);
  MAU_REQUIRE(ncls >= 1 && ncls <= EVAL_MAX_CLS, "eval_metrics_multi: ncls must be in [1,%d], got %d", EVAL_MAX_CLS, ncls);
  MAU_REQUIRE((int64_t)H * W <= (1 << 30), "eval_metrics_multi: maps of at most 2^30 pixels");
  MAU_REQUIRE((int64_t)B * C <= (1 << 30), "eval_metrics_multi: at most 2^30 (sample, channel) rows");
  const int rpc = eval_rows_per_chunk(W), chunks = eval_chunks(H, W);
  const dim3 block(256);
  const hipStream_t st = (hipStream_t)stream;
  return for_ticket_rows(B * C, "eval_metrics_multi_kernel", [&](int row0, int nn) {
    const dim3 grid(chunks, nn);
    if (eval_bins(ncls) == 10)
      MAU_LAUNCH(eval_metrics_multi_kernel<10>, grid, block, 0, st, out, tgt, cls, scale, shift, ws, tickets, rows, M, B * C, C, H, W, ncls, rpc, row0);
    else
      MAU_LAUNCH(eval_metrics_multi_kernel<EVAL_MAX_CLS + 1>, grid, block, 0, st, out, tgt, cls, scale, shift, ws, tickets, rows, M, B * C, C, H, W, ncls, rpc, row0);
  });
}

}  // extern "C"
