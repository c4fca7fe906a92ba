// rawtiles.hip -- dataset build (reference src/data/processing_10m/process.py: the filter check and running statistics of :37-50 /
// :84-115, the normalisation of :175-183): everything the build needs from the pixels of a batch of RAW samples, ONE launch, every
// byte read once.
//   raw_tile_kernel  dw_t1, dw_t2 (B,H,W) uint8 + rgb (B,3,H,W) fp32 (raw 0..255) + ndvi_t1, ndvi_t2, temp_t1, temp_t2 (B,H,W) fp32
//     -> rows (optional): per sample one fp64 row
//          [0,16)  pixels where (dw_t1 == c) != (dw_t2 == c), per class c < num_classes (count / HW = the reference's per-channel
//                  mean |ohe2 - ohe1|)                      [16], [17] values >= num_classes in dw_t1, dw_t2
//          [18] sum |ndvi_t2 - ndvi_t1|  [19] non-finite values of that difference   [20], [21] the same of temp_t2 - temp_t1
//          [22 + 4p, 22 + 4p + 4) n, mean, M2 = sum (x - mean)^2, non-finite values of p = 0..2: r / 255, g / 255, b / 255 (the
//                  division in fp64), p = 3: temp_t1
//     -> cont (B,5,H,W), targets (B,2,H,W) fp32 (optional, both or neither; they need norm = rgb_mean[3], rgb_std[3], temp_mean,
//        temp_std as 8 fp64 on the device): the normalised planes, numpy's arithmetic for float32 rasters operation for operation
//          cont[0..2] = (float)(((double)rgb / 255.0 - mean_c) / std_c)        cont[3] = ndvi_t1, targets[0] = ndvi_t2 (bits unchanged)
//          cont[4], targets[1] = (t - (float)temp_mean) / (float)temp_std in fp32, the division correctly rounded
//
// Grid (chunks of CHUNK_PIX consecutive pixels, samples), the slots of a thread, the two load paths, the ticket per sample and the
// level-2 join in chunk order are tilestats.hip's; moments are chunk_moments<false>, the differences are formed in fp64 from the
// loaded floats (exact) and never stored; counts come from ballots.  No float atomics.  A row's bits and a plane's bits depend on
// nothing but the sample's own bytes.  A non-finite value is counted and left to propagate into the sums it enters.
#include <math.h>
#include "chunk_reduce.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int RT_MAX_CLASSES = 16;
constexpr int RT_OOR = RT_MAX_CLASSES;         // [16], [17]: class values >= num_classes
constexpr int RT_DIFF0 = RT_OOR + 2;           // [18..22): sum |d|, non-finite d of the NDVI and of the temperature difference
constexpr int RT_MOM0 = RT_DIFF0 + 4;          // four moment rows of 4
constexpr int RT_NMOM = 4;
constexpr int RT_ROW = RT_MOM0 + 4 * RT_NMOM;
constexpr int RT_HIST = RT_MAX_CLASSES + 2;
constexpr int RT_CONT = 5, RT_TGT = 2, RT_NORM = 8;

// the thread's 16 values of one plane chunk as stored (load_plane's slots; the bits pass through untouched)
template <bool VEC4>
__device__ __forceinline__ void load_raw(const float* __restrict__ pc, unsigned ok, float (&v)[CHUNK_SLOTS]) {
  if (VEC4) {
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS / 4; ++k) {
      const int idx = (k * 256 + (int)threadIdx.x) * 4;
      const f32x4 f = *reinterpret_cast<const f32x4*>(pc + ((ok >> (4 * k)) & 1u ? idx : 0));
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = f[j];
    }
  } else {
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS; ++k) v[k] = pc[(ok >> k) & 1u ? k * 256 + (int)threadIdx.x : 0];
  }
}

// the inverse: only the slots inside the chunk are written
template <bool VEC4>
__device__ __forceinline__ void store_raw(float* __restrict__ pc, unsigned ok, const float (&v)[CHUNK_SLOTS]) {
  if (VEC4) {
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS / 4; ++k) {
      f32x4 f;
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = v[4 * k + j];
      if ((ok >> (4 * k)) & 1u) *reinterpret_cast<f32x4*>(pc + (k * 256 + (int)threadIdx.x) * 4) = f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS; ++k)
      if ((ok >> k) & 1u) pc[k * 256 + (int)threadIdx.x] = v[k];
  }
}

// per class the wave's pixels that are of that class in exactly one of the two maps, and the values >= num_classes of either
// map (a ballot per slot and class: wave-uniform integers), lane 0 -> hist[0..18)
__device__ __forceinline__ void change_counts(const unsigned (&wa)[CHUNK_SLOTS / 4], const unsigned (&wb)[CHUNK_SLOTS / 4], unsigned ok,
                                              int num_classes, unsigned* hist) {
#pragma unroll
  for (int c = 0; c < RT_HIST; ++c) {
    unsigned cnt = 0;
#pragma unroll
    for (int s = 0; s < CHUNK_SLOTS; ++s) {
      const int va = (int)((wa[s >> 2] >> (8 * (s & 3))) & 0xffu), vb = (int)((wb[s >> 2] >> (8 * (s & 3))) & 0xffu);
      const bool in = (ok >> s) & 1u;
      const bool hit = c < RT_MAX_CLASSES ? c < num_classes && ((va == c) != (vb == c)) : (c == RT_OOR ? va : vb) >= num_classes;
      cnt += (unsigned)__popcll(__ballot(in && hit));
    }
    if ((threadIdx.x & 63) == 0) hist[c] = cnt;
  }
}

// sum |b - a| and the non-finite values of b - a over the chunk -> out[0], out[1]; the difference in fp64, never stored
__device__ __forceinline__ void chunk_abs_diff(const float (&a)[CHUNK_SLOTS], const float (&b)[CHUNK_SLOTS], unsigned ok, double (*sd)[2],
                                               double* out) {
  double r[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < CHUNK_SLOTS; ++k) {
    const bool in = (ok >> k) & 1u;
    const double d = (double)b[k] - (double)a[k];
    r[0] += in ? fabs(d) : 0.0;
    r[1] += in && !isfinite(d) ? 1.0 : 0.0;
  }
  block_join<2>(r, sd, SumAll(), out);
}

template <bool VEC4>
__global__ __launch_bounds__(256) void raw_tile_kernel(const unsigned char* __restrict__ dw_t1, const unsigned char* __restrict__ dw_t2,
                                                       const float* __restrict__ rgb, const float* __restrict__ ndvi_t1,
                                                       const float* __restrict__ ndvi_t2, const float* __restrict__ temp_t1,
                                                       const float* __restrict__ temp_t2, const double* __restrict__ norm, double* part,
                                                       unsigned* tickets, double* __restrict__ rows, float* __restrict__ cont,
                                                       float* __restrict__ targets, int64_t HW, int num_classes, int sample0) {
  __shared__ double sm[4];
  __shared__ double sr[4][2];
  __shared__ double sd[2][4][2];
  __shared__ unsigned hist[4][RT_HIST];
  const int chunks = gridDim.x;
  const size_t sample = (size_t)sample0 + blockIdx.y;
  const int64_t q0 = (int64_t)blockIdx.x * CHUNK_PIX;
  const int npx = (int)(HW - q0 < CHUNK_PIX ? HW - q0 : CHUNK_PIX);
  const double n = (double)npx;
  const unsigned ok = slot_mask<VEC4>(npx);
  const bool want_rows = rows != nullptr, want_planes = cont != nullptr;
  double* prow = want_rows ? part + (size_t)blockIdx.y * chunks * RT_ROW : nullptr;
  double* mine = want_rows ? prow + (size_t)blockIdx.x * RT_ROW : nullptr;
  const size_t plane = sample * HW + q0;       // this chunk in a (B,H,W) tensor

  // the two class maps
  if (want_rows) {
    unsigned wa[CHUNK_SLOTS / 4], wb[CHUNK_SLOTS / 4];
    load_classes<VEC4>(dw_t1 + plane, ok, wa);
    load_classes<VEC4>(dw_t2 + plane, ok, wb);
    change_counts(wa, wb, ok, num_classes, hist[threadIdx.x >> 6]);
    __syncthreads();
    if (threadIdx.x < RT_HIST) {
      const int c = threadIdx.x;
      mine[c] = (double)(hist[0][c] + hist[1][c] + hist[2][c] + hist[3][c]);
    }
  }

  float a[CHUNK_SLOTS], b[CHUNK_SLOTS];
  double v[CHUNK_SLOTS];
  // r, g, b
  for (int p = 0; p < 3; ++p) {
    load_raw<VEC4>(rgb + (sample * 3 + p) * HW + q0, ok, a);
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS; ++k) v[k] = (double)a[k] / 255.0;
    if (want_rows) chunk_moments<false>(v, ok, n, sm, sr, mine + RT_MOM0 + 4 * p);
    if (want_planes) {
      const double mean = norm[p], std = norm[3 + p];
#pragma unroll
      for (int k = 0; k < CHUNK_SLOTS; ++k) a[k] = (float)((v[k] - mean) / std);
      store_raw<VEC4>(cont + (sample * RT_CONT + p) * HW + q0, ok, a);
    }
  }
  // ndvi_t1, ndvi_t2: passed through, and their difference
  load_raw<VEC4>(ndvi_t1 + plane, ok, a);
  load_raw<VEC4>(ndvi_t2 + plane, ok, b);
  if (want_rows) chunk_abs_diff(a, b, ok, sd[0], mine + RT_DIFF0);
  if (want_planes) {
    store_raw<VEC4>(cont + (sample * RT_CONT + 3) * HW + q0, ok, a);
    store_raw<VEC4>(targets + (sample * RT_TGT + 0) * HW + q0, ok, b);
  }
  // temp_t1, temp_t2: the moments of temp_t1, the difference, and both normalised in fp32
  load_raw<VEC4>(temp_t1 + plane, ok, a);
  load_raw<VEC4>(temp_t2 + plane, ok, b);
  if (want_rows) {
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS; ++k) v[k] = (double)a[k];
    chunk_moments<false>(v, ok, n, sm, sr, mine + RT_MOM0 + 4 * 3);
    chunk_abs_diff(a, b, ok, sd[1], mine + RT_DIFF0 + 2);
  }
  if (want_planes) {
    const float mean = (float)norm[6], std = (float)norm[7];
#pragma unroll
    for (int k = 0; k < CHUNK_SLOTS; ++k) {
      a[k] = __fdiv_rn(a[k] - mean, std);
      b[k] = __fdiv_rn(b[k] - mean, std);
    }
    store_raw<VEC4>(cont + (sample * RT_CONT + 4) * HW + q0, ok, a);
    store_raw<VEC4>(targets + (sample * RT_TGT + 1) * HW + q0, ok, b);
  }

  if (!want_rows) return;
  if (!last_block_of(tickets + blockIdx.y, (unsigned)chunks)) return;

  // level 2: the sample's chunk rows in chunk order, one thread per entry
  double* row = rows + sample * RT_ROW;
  const int t = threadIdx.x;
  if (t < RT_NMOM) {
    const int at = RT_MOM0 + 4 * t;
    moment_store(row + at, merge_chunks(prow + at, chunks, RT_ROW));
  } else if (t >= 64 && t < 64 + RT_MOM0) {
    row[t - 64] = chunk_join(prow, chunks, RT_ROW, t - 64, SumAll());
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_raw_tile_row_elems(void) { return RT_ROW; }

size_t mau_raw_tile_ws_elems(int B, int64_t HW) {
  if (B <= 0 || HW <= 0 || HW > (1 << 30)) return 0;
  return (size_t)ticket_ws_rows(B) * chunks_of(HW) * RT_ROW;
}

int mau_raw_tile_process(const unsigned char* dw_t1, const unsigned char* dw_t2, const float* rgb, const float* ndvi_t1,
                         const float* ndvi_t2, const float* temp_t1, const float* temp_t2, const double* norm, double* rows, float* cont,
                         float* targets, double* ws, unsigned* tickets, int B, int64_t HW, int num_classes, mau_stream_t stream) {
  MAU_REQUIRE(dw_t1 && dw_t2 && rgb && ndvi_t1 && ndvi_t2 && temp_t1 && temp_t2, "raw_tile_process: null pointer (an input)");
  MAU_REQUIRE(rows || cont || targets, "raw_tile_process: nothing asked for (rows, cont and targets are all NULL)");
  MAU_REQUIRE((cont != nullptr) == (targets != nullptr), "raw_tile_process: cont and targets come together (one of them is NULL)");
  MAU_REQUIRE(!cont || norm, "raw_tile_process: cont / targets need norm (rgb_mean[3], rgb_std[3], temp_mean, temp_std)");
  MAU_REQUIRE(!rows || (ws && tickets), "raw_tile_process: null pointer (rows need ws and tickets)");
  MAU_REQUIRE(B > 0 && HW > 0, "raw_tile_process: non-positive size (B %d, H*W %lld)", B, (long long)HW);
  MAU_REQUIRE(HW <= (1 << 30), "raw_tile_process: planes of at most 2^30 pixels");
  MAU_REQUIRE(B <= (1 << 24), "raw_tile_process: at most 2^24 samples");
  MAU_REQUIRE(num_classes >= 1 && num_classes <= RT_MAX_CLASSES, "raw_tile_process: num_classes must be in [1,%d], got %d", RT_MAX_CLASSES,
              num_classes);
  const uintptr_t planes = (uintptr_t)rgb | (uintptr_t)ndvi_t1 | (uintptr_t)ndvi_t2 | (uintptr_t)temp_t1 | (uintptr_t)temp_t2 |
                           (uintptr_t)cont | (uintptr_t)targets;
  MAU_REQUIRE(planes % 4 == 0, "raw_tile_process: the fp32 planes must be 4-byte aligned");
  MAU_REQUIRE(((uintptr_t)rows | (uintptr_t)ws | (uintptr_t)norm) % 8 == 0, "raw_tile_process: rows, ws and norm must be 8-byte aligned");
  MAU_REQUIRE((uintptr_t)tickets % 4 == 0, "raw_tile_process: tickets must be 4-byte aligned");
  const int chunks = chunks_of(HW);
  // 16-byte loads and stores of the fp32 planes and 4-byte loads of the class maps: every plane and chunk base is then aligned
  const bool vec4 = HW % 4 == 0 && planes % 16 == 0 && ((uintptr_t)dw_t1 | (uintptr_t)dw_t2) % 4 == 0;
  return for_ticket_rows(B, "raw_tile_kernel", [&](int s0, int nn) {
    if (vec4)
      MAU_LAUNCH(raw_tile_kernel<true>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, dw_t1, dw_t2, rgb, ndvi_t1, ndvi_t2, temp_t1,
                 temp_t2, norm, ws, tickets, rows, cont, targets, HW, num_classes, s0);
    else
      MAU_LAUNCH(raw_tile_kernel<false>, dim3(chunks, nn), dim3(256), 0, (hipStream_t)stream, dw_t1, dw_t2, rgb, ndvi_t1, ndvi_t2, temp_t1,
                 temp_t2, norm, ws, tickets, rows, cont, targets, HW, num_classes, s0);
  });
}

}  // extern "C"
