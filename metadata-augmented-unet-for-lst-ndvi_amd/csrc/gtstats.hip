// gtstats.hip -- ground-truth sensitivity (reference test/generate_ground_truth_sensitivity.py): mean and standard deviation of the
// targets of a split, binned by latitude and by longitude, without keeping a target on the host.
//   plane_moments_kernel  (B,C,H,W) fp32 -> per (sample, channel) plane the moment row (n, mean, M2 = sum (x - mean)^2, non-finite);
//   bin_moments_kernel    the B*C rows of a batch merged into a device-resident table [axes][bins][C] of such rows.
//
// plane moments: grid (chunks of CHUNK_PIX consecutive pixels of ONE plane, planes) -- the chunking is a function of H * W alone.
// Loader, two-pass moments and the fixed order of every sum are chunk_reduce.h's: a workgroup keeps its <= 16 values per thread
// in registers, as doubles from the load on (load_plane), chunk_moments makes the chunk's moment row (a temperature in physical
// units has |mean| >> std: two passes), and the workgroup that draws the plane's last ticket merges the chunk rows IN CHUNK ORDER
// with the pairwise update (merge_chunks).  A row's bits depend on nothing but its own plane.  A non-finite value is counted
// and its arithmetic left to propagate (a NaN pixel gives a NaN mean and M2, as np.mean / np.std do).
//
// bin moments: one workgroup, one thread per (axis, bin, channel).  The bin of every (axis, sample) is np.digitize's (the number
// of edges <= x) and is staged in LDS; a thread then walks the samples IN SAMPLE ORDER and merges those of its bin into its table
// entry with the same update.  No atomics, no tickets: the table after any sequence of batches has the bits of the table after
// the same samples in one batch.
#include <math.h>
#include "chunk_reduce.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int GT_ROW = 4;                // n, mean, M2, non-finite values
constexpr int GT_MAX_AXES = 4;
constexpr int GT_MAX_THREADS = 1024;     // (axis, bin, channel) entries of a table: one workgroup
constexpr int GT_TILE = 1024;            // samples whose bins are staged in LDS at a time

template <bool VEC4>
__global__ __launch_bounds__(256) void plane_moments_kernel(const float* __restrict__ x, double* part, unsigned* tickets,
                                                            double* __restrict__ rows, int64_t HW, int row0) {
  __shared__ double sm[4];
  __shared__ double sr[4][2];
  const int plane = row0 + blockIdx.y, chunks = gridDim.x;
  const int64_t q0 = (int64_t)blockIdx.x * CHUNK_PIX;
  const int npx = (int)(HW - q0 < CHUNK_PIX ? HW - q0 : CHUNK_PIX);
  const unsigned ok = slot_mask<VEC4>(npx);
  double v[CHUNK_SLOTS];
  load_plane<VEC4>(x + (size_t)plane * HW + q0, ok, v);
  double* prow = part + (size_t)blockIdx.y * chunks * GT_ROW;
  chunk_moments<false>(v, ok, (double)npx, sm, sr, prow + (size_t)blockIdx.x * GT_ROW);
  if (!last_block_of(tickets + blockIdx.y, (unsigned)chunks)) return;

  // level 2: the plane's chunk rows in chunk order, then the finished row
  if (threadIdx.x == 0) moment_store(rows + (size_t)plane * GT_ROW, merge_chunks(prow, chunks, GT_ROW));
}

struct BinAxes {
  int col[GT_MAX_AXES];
  double std[GT_MAX_AXES], mean[GT_MAX_AXES];
};

__global__ __launch_bounds__(GT_MAX_THREADS) void bin_moments_kernel(const double* __restrict__ rows, const float* __restrict__ meta,
                                                                     int pitch, BinAxes ax, const double* __restrict__ edges,
                                                                     double* __restrict__ table, int B, int C, int axes, int bins) {
  __shared__ int sbin[GT_MAX_AXES][GT_TILE];
  const int tid = threadIdx.x;
  const int entries = axes * bins * C;
  const int a = tid / (bins * C), mybin = (tid - a * bins * C) / C, c = tid % C;
  const bool mine = tid < entries;
  Moments acc = mine ? moment_load(table + (size_t)tid * GT_ROW) : Moments{0.0, 0.0, 0.0, 0.0};
  for (int b0 = 0; b0 < B; b0 += GT_TILE) {
    const int nb = B - b0 < GT_TILE ? B - b0 : GT_TILE;
    // np.digitize(x, edges): k = number of edges <= x (ascending edges); kept iff 1 <= k <= bins, bin k - 1.  A NaN compares
    // false with every edge: k = 0, dropped.
    for (int i = tid; i < axes * nb; i += blockDim.x) {
      const int ai = i / nb, b = i - ai * nb;
      const double xc = (double)meta[(size_t)(b0 + b) * pitch + ax.col[ai]] * ax.std[ai] + ax.mean[ai];
      const double* e = edges + (size_t)ai * (bins + 1);
      int lo = 0, hi = bins + 1;                          // e[i] <= xc for i < lo, e[i] > xc (or xc is NaN) for i >= hi
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= xc) lo = mid + 1;
        else hi = mid;
      }
      sbin[ai][b] = lo >= 1 && lo <= bins ? lo - 1 : -1;
    }
    __syncthreads();
    if (mine) {
      for (int b = 0; b < nb; ++b)
        if (sbin[a][b] == mybin) acc = moment_merge(acc, moment_load(rows + ((size_t)(b0 + b) * C + c) * GT_ROW));
    }
    __syncthreads();
  }
  if (mine) moment_store(table + (size_t)tid * GT_ROW, acc);
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_moments_row_elems(void) { return GT_ROW; }

int mau_plane_moments_chunks(int64_t HW) { return HW > 0 && HW <= (1 << 30) ? chunks_of(HW) : 0; }

size_t mau_plane_moments_ws_elems(int B, int C, int64_t HW) {
  if (B <= 0 || C <= 0 || HW <= 0 || HW > (1 << 30)) return 0;
  return (size_t)ticket_ws_rows((int64_t)B * C) * chunks_of(HW) * GT_ROW;
}

int mau_plane_moments(const float* x, double* rows, double* ws, unsigned* tickets, int B, int C, int64_t HW, mau_stream_t stream) {
  MAU_REQUIRE(x && rows && ws && tickets, "plane_moments: null pointer");
  MAU_REQUIRE(B > 0 && C > 0 && HW > 0, "plane_moments: non-positive size (B %d, C %d, H*W %lld)", B, C, (long long)HW);
  MAU_REQUIRE(HW <= (1 << 30), "plane_moments: planes of at most 2^30 pixels");
  MAU_REQUIRE((int64_t)B * C <= (1 << 30), "plane_moments: at most 2^30 planes");
  MAU_REQUIRE((uintptr_t)x % 4 == 0, "plane_moments: x must be 4-byte aligned");
  const int chunks = chunks_of(HW);
  const bool vec4 = HW % 4 == 0 && (uintptr_t)x % 16 == 0;
  return for_ticket_rows(B * C, "plane_moments_kernel", [&](int row0, int nn) {
    if (vec4)
      MAU_LAUNCH(plane_moments_kernel<true>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, x, ws, tickets, rows, HW, row0);
    else
      MAU_LAUNCH(plane_moments_kernel<false>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, x, ws, tickets, rows, HW, row0);
  });
}

int mau_bin_moments_max_entries(void) { return GT_MAX_THREADS; }

int mau_bin_moments(const double* rows, const float* meta, int meta_pitch, const int* cols_host, const double* std_host,
                    const double* mean_host, const double* edges, double* table, int B, int C, int axes, int bins,
                    mau_stream_t stream) {
  MAU_REQUIRE(rows && meta && cols_host && std_host && mean_host && edges && table, "bin_moments: null pointer");
  MAU_REQUIRE(B > 0 && C > 0 && bins > 0, "bin_moments: non-positive size (B %d, C %d, bins %d)", B, C, bins);
  MAU_REQUIRE(axes >= 1 && axes <= GT_MAX_AXES, "bin_moments: axes must be in [1,%d], got %d", GT_MAX_AXES, axes);
  MAU_REQUIRE((int64_t)axes * bins * C <= GT_MAX_THREADS, "bin_moments: axes * bins * C = %lld entries, at most %d (one thread each)",
              (long long)axes * bins * C, GT_MAX_THREADS);
  MAU_REQUIRE(meta_pitch > 0, "bin_moments: non-positive metadata pitch %d", meta_pitch);
  BinAxes ax = {};
  for (int a = 0; a < axes; ++a) {
    MAU_REQUIRE(cols_host[a] >= 0 && cols_host[a] < meta_pitch, "bin_moments: column %d of axis %d is outside a row of %d", cols_host[a], a, meta_pitch);
    ax.col[a] = cols_host[a];
    ax.std[a] = std_host[a];
    ax.mean[a] = mean_host[a];
  }
  const int threads = round_up(axes * bins * C, 64);
  MAU_LAUNCH(bin_moments_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, rows, meta, meta_pitch, ax, edges, table, B, C, axes, bins);
  return check_launch("bin_moments_kernel");
}

}  // extern "C"
