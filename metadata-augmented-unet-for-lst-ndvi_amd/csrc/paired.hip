// paired.hip -- the joint moments behind the paired tests of M checkpoints (reference test/statistical_tests.py, the numeric part
// of app_dev/pages/3_Statistical_Comparison.py): a device-resident table merged batch by batch, read back once.
//
// Table [group][channel][slot] of entries; a slot is one metric of the `overall` row (mae, rmse, laplacian_var_pred,
// laplacian_var_gt) or of a class (mae, rmse): 4 + 2 ncls slots.  An entry holds n, the number of samples skipped for a non-finite
// value, mean[M] and the upper triangle of the co-moment matrix Cm[i][j] = sum (x_i - mean_i)(x_j - mean_j), where x is the
// M-vector of the slot's metric in the M models' rows (mau_eval_metrics_multi) of one sample.
// One thread per entry walks the samples of the batch IN SAMPLE ORDER with Welford's update, fp64, nothing contracted:
//   n' = n + 1;  d_i = x_i - mean_i;  mean_i' = mean_i + d_i / n';  Cm_ij' = Cm_ij + d_i * (x_j - mean_j')
// Every element depends on its own i, j only.  No atomics, no tickets: the table after any sequence of batches has the bits of the
// table after the same samples in one batch (the host twin, statistics.paired_accumulate_host, repeats it operation for operation).
#include <math.h>
#include "eval_row.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int PAIRED_GROUPS = 8;         // is_known_city (2) x temporal distance (4)
constexpr int PAIRED_MAX_MODELS = 8;
constexpr int PAIRED_OVERALL = 4;        // slots of the overall row; then (mae, rmse) per class

static inline int paired_entry_elems(int M) { return 2 + M + M * (M + 1) / 2; }
static inline int paired_slots(int ncls) { return PAIRED_OVERALL + 2 * ncls; }

template <int M>
__global__ __launch_bounds__(256) void paired_accumulate_kernel(const double* __restrict__ rows, const unsigned char* __restrict__ gid,
                                                                double* __restrict__ table, int B, int C, int ncls) {
  constexpr int EE = 2 + M + M * (M + 1) / 2;
  const int slots = PAIRED_OVERALL + 2 * ncls, relems = EVAL_HEAD + 3 * ncls;
  const int tid = blockIdx.x * 256 + threadIdx.x;
  if (tid >= PAIRED_GROUPS * C * slots) return;
  const int grp = tid / (C * slots), c = (tid - grp * C * slots) / slots, slot = tid % slots;
  // the row entry the slot reads, and for a class slot the entry that holds the class's pixel count
  const int kk = slot < PAIRED_OVERALL ? -1 : (slot - PAIRED_OVERALL) >> 1;
  const int col = kk < 0 ? slot : EVAL_HEAD + ncls * (1 + ((slot - PAIRED_OVERALL) & 1)) + kk;
  double* e = table + (size_t)tid * EE;
  double n = e[0], skipped = e[1], mean[M], cm[M * (M + 1) / 2];
#pragma unroll
  for (int i = 0; i < M; ++i) mean[i] = e[2 + i];
#pragma unroll
  for (int p = 0; p < M * (M + 1) / 2; ++p) cm[p] = e[2 + M + p];

  for (int b = 0; b < B; ++b) {
    if (gid[b] != grp) continue;
    const double* r = rows + ((size_t)b * C + c) * relems;             // model m: + m * B * C * relems
    if (kk >= 0 && !(r[EVAL_HEAD + kk] > 0.0)) continue;              // the class has no pixel in this sample (the same for every model)
    double x[M];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      x[i] = r[(size_t)i * B * C * relems + col];
      ok = ok && isfinite(x[i]);
    }
    if (!ok) {
      skipped += 1.0;
      continue;
    }
    n += 1.0;
    double d[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      d[i] = x[i] - mean[i];
      mean[i] = mean[i] + d[i] / n;
    }
    int p = 0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
      for (int j = i; j < M; ++j, ++p) cm[p] = cm[p] + d[i] * (x[j] - mean[j]);
    }
  }

  e[0] = n;
  e[1] = skipped;
#pragma unroll
  for (int i = 0; i < M; ++i) e[2 + i] = mean[i];
#pragma unroll
  for (int p = 0; p < M * (M + 1) / 2; ++p) e[2 + M + p] = cm[p];
}

template <int M>
static void paired_launch(const double* rows, const unsigned char* gid, double* table, int B, int C, int ncls, hipStream_t st) {
  const int threads = PAIRED_GROUPS * C * paired_slots(ncls);
  MAU_LAUNCH(paired_accumulate_kernel<M>, dim3(ceil_div(threads, 256)), dim3(256), 0, st, rows, gid, table, B, C, ncls);
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_paired_groups(void) { return PAIRED_GROUPS; }

int mau_paired_entry_elems(int M) { return M >= 1 && M <= PAIRED_MAX_MODELS ? paired_entry_elems(M) : 0; }

size_t mau_paired_table_elems(int M, int C, int ncls) {
  if (M < 1 || M > PAIRED_MAX_MODELS || C <= 0 || ncls < 1 || ncls > EVAL_MAX_CLS) return 0;
  return (size_t)PAIRED_GROUPS * C * paired_slots(ncls) * paired_entry_elems(M);
}

int mau_paired_accumulate(const double* rows, const unsigned char* group, double* table, int M, int B, int C, int ncls,
                          mau_stream_t stream) {
  MAU_REQUIRE(rows && group && table, "paired_accumulate: null pointer");
  MAU_REQUIRE(M >= 1 && M <= PAIRED_MAX_MODELS, "paired_accumulate: M must be in [1,%d], got %d", PAIRED_MAX_MODELS, M);
  MAU_REQUIRE(B > 0 && C > 0, "paired_accumulate: non-positive size (B %d, C %d)", B, C);
  MAU_REQUIRE(ncls >= 1 && ncls <= EVAL_MAX_CLS, "paired_accumulate: ncls must be in [1,%d], got %d", EVAL_MAX_CLS, ncls);
  MAU_REQUIRE((int64_t)B * C <= (1 << 30), "paired_accumulate: at most 2^30 (sample, channel) rows");
  MAU_REQUIRE((int64_t)C * paired_slots(ncls) <= (1 << 20), "paired_accumulate: at most 2^20 entries per group");
  const hipStream_t st = (hipStream_t)stream;
  switch (M) {
    case 1: paired_launch<1>(rows, group, table, B, C, ncls, st); break;
    case 2: paired_launch<2>(rows, group, table, B, C, ncls, st); break;
    case 3: paired_launch<3>(rows, group, table, B, C, ncls, st); break;
    case 4: paired_launch<4>(rows, group, table, B, C, ncls, st); break;
    case 5: paired_launch<5>(rows, group, table, B, C, ncls, st); break;
    case 6: paired_launch<6>(rows, group, table, B, C, ncls, st); break;
    case 7: paired_launch<7>(rows, group, table, B, C, ncls, st); break;
    default: paired_launch<8>(rows, group, table, B, C, ncls, st); break;
  }
  return check_launch("paired_accumulate_kernel");
}

}  // extern "C"
