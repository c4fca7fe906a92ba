// tilestats.hip -- dataset survey (reference src/utils/visualize_npz.py extract_metrics): everything the per-tile CSV row needs
// from the pixels of a compact batch, ONE launch, every byte read once.
//   tile_stats_kernel  cls_a, cls_b (B,H,W) uint8 + cont (B,5,H,W) fp32 + targets (B,2,H,W) fp32 -> per sample one fp64 row:
//     [0,16) pixels per class of cls_a   [16,32) of cls_b   [32], [33] values >= num_classes in cls_a, cls_b
//     [34 + 8p, 34 + 8p + 8) the plane row  n, mean, M2 = sum (x - mean)^2, min, max, sum |x|, NaNs, non-finite values  of plane p:
//     p = 0..4 cont (r, g, b, ndvi_t1, temp_t1), 5, 6 targets (ndvi_t2, temp_t2), 7 = ndvi_t2 - ndvi_t1, 8 = temp_t2 - temp_t1.
//
// Grid (chunks of GT_CHUNK_PIX consecutive pixels, samples), as plane_moments_kernel: the chunking is a function of H * W alone.
// A workgroup walks the planes of its chunk one at a time -- the two that form a difference together: a[16], b[16] doubles per
// thread, then a := b - a in fp64 (the difference is never stored) -- and keeps gtstats.hip's conventions: doubles from the load
// on, two passes over register-resident values (chunk mean, then squared distances), sums in slot order, xor butterfly, wave order.
// min / max / counts are exact in any order.  The chunk's results are a row of the same layout in the workspace; the workgroup
// that draws the sample's last ticket merges them IN CHUNK ORDER (moment_merge; fmin / fmax; plain sums), one thread per entry.
// A row's bits depend on nothing but the sample's own bytes.  A NaN is counted and left to propagate into mean and M2; fmin /
// fmax skip it (the host turns min / max into NaN when the NaN count is not zero, as np.min does).
#include <math.h>
#include "mau_common.h"
#include "moments.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int TS_CHUNK_PIX = 4096;            // gtstats.hip's GT_CHUNK_PIX: 250 x 250 = 16 chunks
constexpr int TS_SLOTS = TS_CHUNK_PIX / 256;
constexpr int TS_MAX_CLASSES = 16;
constexpr int TS_OOR = 2 * TS_MAX_CLASSES;    // [32], [33]: class values >= num_classes
constexpr int TS_PLANES0 = TS_OOR + 2;
constexpr int TS_PLANE_ROW = 8;               // n, mean, M2, min, max, sum |x|, NaN, non-finite
constexpr int TS_NPLANES = 9;
constexpr int TS_ROW = TS_PLANES0 + TS_NPLANES * TS_PLANE_ROW;
constexpr int TS_CONT = 5, TS_TGT = 2;
constexpr int TS_RED = 6;                     // values of the second reduction: M2, sum |x|, NaN, non-finite, min, max

static inline int ts_chunks(int64_t HW) { return ceil_div(HW, TS_CHUNK_PIX); }

// bit s: slot s of this thread is a pixel of the (partial, last) chunk.  VEC4: slot 4k + j of thread t is pixel (k * 256 + t) * 4 + j
// (npx is then a multiple of 4: a quad is inside or outside as a whole); otherwise slot k is pixel k * 256 + t.
template <bool VEC4>
__device__ __forceinline__ unsigned slot_mask(int npx) {
  unsigned m = 0;
#pragma unroll
  for (int s = 0; s < TS_SLOTS; ++s) {
    const int idx = VEC4 ? ((s >> 2) * 256 + (int)threadIdx.x) * 4 : s * 256 + (int)threadIdx.x;
    m |= idx < npx ? 1u << s : 0u;
  }
  return m;
}

// the thread's 16 values of one plane chunk as doubles; a slot outside the chunk loads pixel 0 of the chunk (no exec-masked load)
template <bool VEC4>
__device__ __forceinline__ void load_plane(const float* __restrict__ pc, unsigned ok, double (&v)[TS_SLOTS]) {
  if (VEC4) {
#pragma unroll
    for (int k = 0; k < TS_SLOTS / 4; ++k) {
      const int idx = (k * 256 + (int)threadIdx.x) * 4;
      const f32x4 f = *reinterpret_cast<const f32x4*>(pc + ((ok >> (4 * k)) & 1u ? idx : 0));
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = (double)f[j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < TS_SLOTS; ++k) v[k] = (double)pc[(ok >> k) & 1u ? k * 256 + (int)threadIdx.x : 0];
  }
}

// the plane row of the chunk's values v (register resident), written by thread 0 to out[0..8).  sm: 4 doubles for the mean's
// block_sum, sr: 4 x TS_RED for the second reduction; the two are written alternately, a barrier between any read and the next
// write, so consecutive planes reuse them.
__device__ __forceinline__ void plane_row(const double (&v)[TS_SLOTS], unsigned ok, double n, double* sm, double (*sr)[TS_RED],
                                          double* __restrict__ out) {
  // pass one: the chunk mean
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < TS_SLOTS; ++k) s += (ok >> k) & 1u ? v[k] : 0.0;
  const double mean = block_sum(s, sm) / n;
  // pass two: the squared distances to it, and what needs no mean
  double r[TS_RED] = {0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY};
#pragma unroll
  for (int k = 0; k < TS_SLOTS; ++k) {
    const bool in = (ok >> k) & 1u;
    const double d = v[k] - mean;
    r[0] += in ? d * d : 0.0;
    r[1] += in ? fabs(v[k]) : 0.0;
    r[2] += in && isnan(v[k]) ? 1.0 : 0.0;
    r[3] += in && !isfinite(v[k]) ? 1.0 : 0.0;
    r[4] = fmin(r[4], in ? v[k] : INFINITY);
    r[5] = fmax(r[5], in ? v[k] : -INFINITY);
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] += __shfl_xor(r[i], sh, 64);
    r[4] = fmin(r[4], __shfl_xor(r[4], sh, 64));
    r[5] = fmax(r[5], __shfl_xor(r[5], sh, 64));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < TS_RED; ++i) sr[threadIdx.x >> 6][i] = r[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const auto waves = [&](int i) { return ((sr[0][i] + sr[1][i]) + sr[2][i]) + sr[3][i]; };
    out[0] = n;
    out[1] = mean;
    out[2] = waves(0);
    out[5] = waves(1);
    out[6] = waves(2);
    out[7] = waves(3);
    out[3] = fmin(fmin(sr[0][4], sr[1][4]), fmin(sr[2][4], sr[3][4]));
    out[4] = fmax(fmax(sr[0][5], sr[1][5]), fmax(sr[2][5], sr[3][5]));
  }
}

// the thread's 16 class values of one map chunk, four to a word
template <bool VEC4>
__device__ __forceinline__ void load_classes(const unsigned char* __restrict__ pc, unsigned ok, unsigned (&w)[TS_SLOTS / 4]) {
#pragma unroll
  for (int k = 0; k < TS_SLOTS / 4; ++k) {
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

// pixels per class of the wave's 1024 slots (a ballot per slot and class: wave-uniform integers), lane 0 -> hist[0..17)
__device__ __forceinline__ void class_counts(const unsigned (&w)[TS_SLOTS / 4], unsigned ok, int num_classes, unsigned* hist) {
#pragma unroll
  for (int c = 0; c <= TS_MAX_CLASSES; ++c) {
    unsigned cnt = 0;
#pragma unroll
    for (int s = 0; s < TS_SLOTS; ++s) {
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
  const int64_t q0 = (int64_t)blockIdx.x * TS_CHUNK_PIX;
  const int npx = (int)(HW - q0 < TS_CHUNK_PIX ? HW - q0 : TS_CHUNK_PIX);
  const double n = (double)npx;
  const unsigned ok = slot_mask<VEC4>(npx);
  double* prow = part + (size_t)blockIdx.y * chunks * TS_ROW;
  double* mine = prow + (size_t)blockIdx.x * TS_ROW;

  // the two class maps
  {
    unsigned wa[TS_SLOTS / 4], wb[TS_SLOTS / 4];
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
  double a[TS_SLOTS], b[TS_SLOTS];
  for (int p = 0; p < 3; ++p) {
    load_plane<VEC4>(cont + (sample * TS_CONT + p) * HW + q0, ok, a);
    plane_row(a, ok, n, sm, sr, mine + TS_PLANES0 + p * TS_PLANE_ROW);
  }
  // (ndvi_t1, ndvi_t2), (temp_t1, temp_t2) and their differences
  for (int p = 0; p < 2; ++p) {
    load_plane<VEC4>(cont + (sample * TS_CONT + 3 + p) * HW + q0, ok, a);
    load_plane<VEC4>(targets + (sample * TS_TGT + p) * HW + q0, ok, b);
    plane_row(a, ok, n, sm, sr, mine + TS_PLANES0 + (3 + p) * TS_PLANE_ROW);
    plane_row(b, ok, n, sm, sr, mine + TS_PLANES0 + (5 + p) * TS_PLANE_ROW);
#pragma unroll
    for (int k = 0; k < TS_SLOTS; ++k) a[k] = b[k] - a[k];
    plane_row(a, ok, n, sm, sr, mine + TS_PLANES0 + (7 + p) * TS_PLANE_ROW);
  }

  if (!last_block_of(tickets + blockIdx.y, (unsigned)chunks)) return;

  // level 2: the sample's chunk rows in chunk order, one thread per entry
  double* row = rows + sample * TS_ROW;
  const int t = threadIdx.x;
  if (t < TS_NPLANES) {
    const double* q = prow + TS_PLANES0 + t * TS_PLANE_ROW;
    Moments acc = Moments{q[0], q[1], q[2], q[7]};
    double mn = q[3], mx = q[4], l1 = q[5], nan = q[6];
    for (int c = 1; c < chunks; ++c) {
      q += TS_ROW;
      acc = moment_merge(acc, Moments{q[0], q[1], q[2], q[7]});
      mn = fmin(mn, q[3]);
      mx = fmax(mx, q[4]);
      l1 += q[5];
      nan += q[6];
    }
    double* o = row + TS_PLANES0 + t * TS_PLANE_ROW;
    o[0] = acc.n;
    o[1] = acc.mean;
    o[2] = acc.m2;
    o[3] = mn;
    o[4] = mx;
    o[5] = l1;
    o[6] = nan;
    o[7] = acc.bad;
  } else if (t >= 64 && t < 64 + TS_PLANES0) {
    const int e = t - 64;
    double cnt = prow[e];
    for (int c = 1; c < chunks; ++c) cnt += prow[(size_t)c * TS_ROW + e];
    row[e] = cnt;
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_tile_stats_row_elems(void) { return TS_ROW; }

size_t mau_tile_stats_ws_elems(int B, int64_t HW) {
  if (B <= 0 || HW <= 0 || HW > (1 << 30)) return 0;
  // the launches of one call reuse the partials of the first mau_reduce_tickets_elems() samples
  const int per = mau_reduce_tickets_elems();
  return (size_t)(B < per ? B : per) * ts_chunks(HW) * TS_ROW;
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
  const int chunks = ts_chunks(HW);
  // 16-byte loads of the fp32 planes and 4-byte loads of the class maps: every plane and chunk base is then aligned
  const bool vec4 = HW % 4 == 0 && (uintptr_t)cont % 16 == 0 && (uintptr_t)targets % 16 == 0 && (uintptr_t)cls_a % 4 == 0 &&
                    (uintptr_t)cls_b % 4 == 0;
  // one ticket per sample: mau_reduce_tickets_elems() samples per launch
  const int per = mau_reduce_tickets_elems();
  for (int s0 = 0; s0 < B; s0 += per) {
    const int nn = B - s0 < per ? B - s0 : per;
    if (vec4)
      MAU_LAUNCH(tile_stats_kernel<true>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, cls_a, cls_b, cont, targets, ws, tickets, rows,
                 HW, num_classes, s0);
    else
      MAU_LAUNCH(tile_stats_kernel<false>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, cls_a, cls_b, cont, targets, ws, tickets,
                 rows, HW, num_classes, s0);
    const int st = check_launch("tile_stats_kernel");
    if (st != 0) return st;
  }
  return 0;
}

}  // extern "C"
