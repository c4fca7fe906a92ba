// tilestats.hip -- dataset survey (reference src/utils/visualize_npz.py extract_metrics): everything the per-tile CSV row needs
// from the pixels of a compact batch, ONE launch, every byte read once.
//   tile_stats_kernel  cls_a, cls_b (B,H,W) uint8 + cont (B,5,H,W) fp32 + targets (B,2,H,W) fp32 -> per sample one fp64 row:
//     [0,16) pixels per class of cls_a   [16,32) of cls_b   [32], [33] values >= num_classes in cls_a, cls_b
//     [34 + 8p, 34 + 8p + 8) the plane row  n, mean, M2 = sum (x - mean)^2, min, max, sum |x|, NaNs, non-finite values  of plane p:
//     p = 0..4 cont (r, g, b, ndvi_t1, temp_t1), 5, 6 targets (ndvi_t2, temp_t2), 7 = ndvi_t2 - ndvi_t1, 8 = temp_t2 - temp_t1.
//
// Grid (chunks of CHUNK_PIX consecutive pixels, samples): the chunking is a function of H * W alone.  A workgroup walks the planes
// of its chunk one at a time -- the two that form a difference together: a[16], b[16] doubles per thread, then a := b - a in fp64
// (the difference is never stored).  Loader, two-pass moments and the fixed order of every sum are chunk_reduce.h's (load_plane,
// chunk_moments<true>); min / max / counts are exact in any order.  The chunk's results are a row of the same layout in the
// workspace; the workgroup that draws the sample's last ticket joins them IN CHUNK ORDER (merge_chunks; chunk_join with fmin /
// fmax / plain sums), one thread per entry.
// A row's bits depend on nothing but the sample's own bytes.  A NaN is counted and left to propagate into mean and M2; fmin /
// fmax skip it (the host turns min / max into NaN when the NaN count is not zero, as np.min does).
#include <math.h>
#include "chunk_reduce.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int TS_MAX_CLASSES = 16;
constexpr int TS_OOR = 2 * TS_MAX_CLASSES;    // [32], [33]: class values >= num_classes
constexpr int TS_PLANES0 = TS_OOR + 2;
constexpr int TS_PLANE_ROW = 8;               // n, mean, M2, min, max, sum |x|, NaN, non-finite
constexpr int TS_NPLANES = 9;
constexpr int TS_ROW = TS_PLANES0 + TS_NPLANES * TS_PLANE_ROW;
constexpr int TS_CONT = 5, TS_TGT = 2;
constexpr int TS_RED = TS_PLANE_ROW - 2;       // values of chunk_moments' second reduction: the row without n and mean

// pixels per class of the wave's 1024 slots (a ballot per slot and class: wave-uniform integers), lane 0 -> hist[0..17)
__device__ __forceinline__ void class_counts(const unsigned (&w)[CHUNK_SLOTS / 4], unsigned ok, int num_classes, unsigned* hist) {
#pragma unroll
  for (int c = 0; c <= TS_MAX_CLASSES; ++c) {
    unsigned cnt = 0;
#pragma unroll
    for (int s = 0; s < CHUNK_SLOTS; ++s) {
      const unsigned val = (w[s >> 2] >> (8 * (s & 3))) & 0xffu;
      const bool in = (ok >> s) & 1u;
      const bool hit = c < TS_MAX_CLASSES ? (int)val == c && c < num_classes : (int)val >= num_classes;
      cnt += (unsigned)__popcll(__ballot(in && hit));
    }
    if ((threadIdx.x & 63) == 0) hist[c] = cnt;
  }
}

template <bool VEC4>
__global__ __launch_bounds__(256) void tile_stats_kernel(const unsigned char* __restrict__ cls_a, const unsigned char* __restrict__ cls_b,
                                                         const float* __restrict__ cont, const float* __restrict__ targets, double* part,
                                                         unsigned* tickets, double* __restrict__ rows, int64_t HW, int num_classes,
                                                         int sample0) {
  __shared__ double sm[4];
  __shared__ double sr[4][TS_RED];
  __shared__ unsigned hist[4][2][TS_MAX_CLASSES + 1];
  const int chunks = gridDim.x;
  const size_t sample = (size_t)sample0 + blockIdx.y;
  const int64_t q0 = (int64_t)blockIdx.x * CHUNK_PIX;
  const int npx = (int)(HW - q0 < CHUNK_PIX ? HW - q0 : CHUNK_PIX);
  const double n = (double)npx;
  const unsigned ok = slot_mask<VEC4>(npx);
  double* prow = part + (size_t)blockIdx.y * chunks * TS_ROW;
  double* mine = prow + (size_t)blockIdx.x * TS_ROW;

  // the two class maps
  {
    unsigned wa[CHUNK_SLOTS / 4], wb[CHUNK_SLOTS / 4];
    load_classes<VEC4>(cls_a + sample * HW + q0, ok, wa);
    load_classes<VEC4>(cls_b + sample * HW + q0, ok, wb);
    class_counts(wa, ok, num_classes, hist[threadIdx.x >> 6][0]);
    class_counts(wb, ok, num_classes, hist[threadIdx.x >> 6][1]);
    __syncthreads();
    if (threadIdx.x < 2 * (TS_MAX_CLASSES + 1)) {
      const int m = threadIdx.x / (TS_MAX_CLASSES + 1), c = threadIdx.x % (TS_MAX_CLASSES + 1);
      const unsigned cnt = hist[0][m][c] + hist[1][m][c] + hist[2][m][c] + hist[3][m][c];
      mine[c < TS_MAX_CLASSES ? m * TS_MAX_CLASSES + c : TS_OOR + m] = (double)cnt;
    }
  }

  // r, g, b
  double a[CHUNK_SLOTS], b[CHUNK_SLOTS];
  for (int p = 0; p < 3; ++p) {
    load_plane<VEC4>(cont + (sample * TS_CONT + p) * HW + q0, ok, a);
    chunk_moments<true>(a, ok, n, sm, sr, mine + TS_PLANES0 + p * TS_PLANE_ROW);
  }
  // (ndvi_t1, ndvi_t2), (temp_t1, temp_t2) and their differences
  for (int p = 0; p < 2; ++p) {
    load_plane<VEC4>(cont + (sample * TS_CONT + 3 + p) * HW + q0, ok, a);
    load_plane<VEC4>(targets + (sample * TS_TGT + p) * HW + q0, ok, b);
    chunk_moments<true>(a, ok, n, sm, sr, mine + TS_PLANES0 + (3 + p) * TS_PLANE_ROW);
    chunk_moments<true>(b, ok, n, sm, sr, mine + TS_PLANES0 + (5 + p) * TS_PLANE_ROW);
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS; ++k) a[k] = b[k] - a[k];
    chunk_moments<true>(a, ok, n, sm, sr, mine + TS_PLANES0 + (7 + p) * TS_PLANE_ROW);
  }

  if (!last_block_of(tickets + blockIdx.y, (unsigned)chunks)) return;

  // level 2: the sample's chunk rows in chunk order, one thread per entry
  double* row = rows + sample * TS_ROW;
  const int t = threadIdx.x;
  if (t < TS_NPLANES) {
    const int at = TS_PLANES0 + t * TS_PLANE_ROW;
    moment_store(row + at, merge_chunks(prow + at, chunks, TS_ROW, 7), 7);
  } else if (t >= 64 && t < 64 + TS_ROW) {
    // the class counts, and min, max, sum |x| and the NaN count of every plane row
    const int e = t - 64, j = e < TS_PLANES0 ? 0 : (e - TS_PLANES0) % TS_PLANE_ROW;
    if (e < TS_PLANES0 || (j >= 3 && j <= 6))
      row[e] = chunk_join(prow, chunks, TS_ROW, e, [j](int, double x, double y) { return MomentRowJoin()(j, x, y); });
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_tile_stats_row_elems(void) { return TS_ROW; }

size_t mau_tile_stats_ws_elems(int B, int64_t HW) {
  if (B <= 0 || HW <= 0 || HW > (1 << 30)) return 0;
  return (size_t)ticket_ws_rows(B) * chunks_of(HW) * TS_ROW;
}

int mau_tile_stats(const unsigned char* cls_a, const unsigned char* cls_b, const float* cont, const float* targets, double* rows,
                   double* ws, unsigned* tickets, int B, int64_t HW, int num_classes, mau_stream_t stream) {
  MAU_REQUIRE(cls_a && cls_b && cont && targets && rows && ws && tickets, "tile_stats: null pointer");
  MAU_REQUIRE(B > 0 && HW > 0, "tile_stats: non-positive size (B %d, H*W %lld)", B, (long long)HW);
  MAU_REQUIRE(HW <= (1 << 30), "tile_stats: planes of at most 2^30 pixels");
  MAU_REQUIRE(B <= (1 << 24), "tile_stats: at most 2^24 samples");
  MAU_REQUIRE(num_classes >= 1 && num_classes <= TS_MAX_CLASSES, "tile_stats: num_classes must be in [1,%d], got %d", TS_MAX_CLASSES,
              num_classes);
  MAU_REQUIRE((uintptr_t)cont % 4 == 0 && (uintptr_t)targets % 4 == 0, "tile_stats: cont and targets must be 4-byte aligned");
  MAU_REQUIRE((uintptr_t)rows % 8 == 0 && (uintptr_t)ws % 8 == 0, "tile_stats: rows and ws must be 8-byte aligned");
  const int chunks = chunks_of(HW);
  // 16-byte loads of the fp32 planes and 4-byte loads of the class maps: every plane and chunk base is then aligned
  const bool vec4 = HW % 4 == 0 && (uintptr_t)cont % 16 == 0 && (uintptr_t)targets % 16 == 0 && (uintptr_t)cls_a % 4 == 0 &&
                    (uintptr_t)cls_b % 4 == 0;
  return for_ticket_rows(B, "tile_stats_kernel", [&](int s0, int nn) {
    if (vec4)
      MAU_LAUNCH(tile_stats_kernel<true>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, cls_a, cls_b, cont, targets, ws, tickets, rows,
                 HW, num_classes, s0);
    else
      MAU_LAUNCH(tile_stats_kernel<false>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, cls_a, cls_b, cont, targets, ws, tickets,
                 rows, HW, num_classes, s0);
  });
}

}  // extern "C"
