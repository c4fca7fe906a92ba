// rankstats.hip -- the rank tests of M checkpoints (app_dev/pages/3_Statistical_Comparison.py: section 7, the pairwise Wilcoxon
// signed-rank tests; section 3, Mann-Whitney U of known against unknown cities per model; sections 1-2, the pooled minimum and the
// 98th percentile that set the axis range), from a device-resident column store, as EXACT INTEGERS.
//
// Ranks come from counting, not from sorting.  For element i of a multiset v
//   less_i = #{j : v_j < v_i},  eq_i = #{j : v_j == v_i} (i itself included),  twice its mid-rank = 2 less_i + eq_i + 1,
// the tie term sum over tie groups (t^3 - t) = sum_i (eq_i^2 - 1), and i is the k-th order statistic iff less_i <= k < less_i + eq_i.
// Every output is an int64 sum of such integers (or the bit pattern of an input value): any summation order gives the same bits,
// so the partial sums of the workgroups meet in the table through integer atomic adds and the numpy twin
// (rank_tests.rank_tests_host) reproduces the table to the bit.
//
// The compare is O(n^2) and trivially parallel: a thread owns one i, the workgroup stages RANK_TILE values of j in LDS, every thread
// reads the tile (a broadcast read).  A j that does not take part (beyond the end, a dropped sample, a zero difference) is staged as
// NaN: both compares are false for it, so ragged tiles need no branch and every thread reaches every barrier.
#include <math.h>
#include "mau_common.h"

namespace mau {

constexpr int RANK_TILE = 256;           // values of j per LDS tile = threads per workgroup
constexpr int RANK_MAX_MODELS = 8;
constexpr int RANK_MAX_Q = 4096;
constexpr int RANK_MAX_N = 1 << 20;      // sum eq^2 <= 2^60 stays inside int64
constexpr int RANK_PAIR = 7;             // n_used, n_zero, skipped, 2 W+, 2 W-, tie term, the tie groups of a small sample
constexpr int RANK_SMALL = 13;           // kept samples up to which the tie groups are written (4 bits per rank position)
constexpr int RANK_MODEL = 4;            // n_known, n_unknown, 2 R_known, tie term
constexpr int RANK_POOL = 4;             // n, minimum, order statistics lo and hi (bit patterns)

static inline int rank_pairs(int M) { return M * (M - 1) / 2; }
static inline int rank_q_elems(int M) { return RANK_PAIR * rank_pairs(M) + RANK_MODEL * M + RANK_POOL; }

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void rank_zero_kernel(u64* __restrict__ a, size_t na, u64* __restrict__ b, size_t nb) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < na) a[i] = 0;
  if (i < nb) b[i] = 0;
}

// acc[0..NV) of every thread summed over the workgroup and added to out[0..NV): butterfly per value, the four waves through LDS,
// one atomic per value and workgroup
template <int NV>
__device__ __forceinline__ void block_add(long long (&acc)[NV], long long (*wsum)[NV], u64* out) {
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc[v] += __shfl_xor(acc[v], s, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) wsum[threadIdx.x >> 6][v] = acc[v];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int v = threadIdx.x;
    const long long s = ((wsum[0][v] + wsum[1][v]) + wsum[2][v]) + wsum[3][v];
    if (s != 0) atomicAdd(out + v, (u64)s);
  }
}

// less / eq of vi against value(j), j in [0, nJ); nJ is the same in every thread of the workgroup
template <typename Value>
__device__ __forceinline__ void count_against(double vi, int nJ, Value value, double* tile, int& less, int& eq) {
  less = 0;
  eq = 0;
  for (int j0 = 0; j0 < nJ; j0 += RANK_TILE) {
    tile[threadIdx.x] = value(j0 + (int)threadIdx.x);
    __syncthreads();
#pragma unroll 16
    for (int t = 0; t < RANK_TILE; ++t) {
      const double vj = tile[t];
      less += vj < vi ? 1 : 0;
      eq += vj == vi ? 1 : 0;
    }
    __syncthreads();
  }
}

// keep[q][n] = every model's value of sample n is finite; kept[q] = their number
__global__ __launch_bounds__(256) void rank_keep_kernel(const double* __restrict__ cols, unsigned char* __restrict__ keep, u64* __restrict__ kept,
                                                        int M, int N, int Ncap) {
  __shared__ long long wsum[4][1];
  const int q = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < N;
  const int at = in ? i : 0;
  bool ok = in;
  for (int m = 0; m < M; ++m) ok = ok && isfinite(cols[((size_t)q * M + m) * Ncap + at]);
  if (in) keep[(size_t)q * N + i] = ok ? 1 : 0;
  long long acc[1] = {ok ? 1 : 0};
  block_add<1>(acc, wsum, kept + q);
}

// job < P: the Wilcoxon entry of pair (a, b), a < b in row-major order; job >= P: the Mann-Whitney entry of model job - P
__global__ __launch_bounds__(256) void rank_tests_kernel(const double* __restrict__ cols, const unsigned char* __restrict__ known,
                                                         const unsigned char* __restrict__ keep, const u64* __restrict__ nkept,
                                                         u64* __restrict__ table, int M, int N, int Ncap) {
  __shared__ double tile[RANK_TILE];
  __shared__ long long wsum[4][RANK_PAIR];
  const int P = M * (M - 1) / 2, q = blockIdx.z, job = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < N;
  const unsigned char* kq = keep + (size_t)q * N;
  u64* tq = table + (size_t)q * (RANK_PAIR * P + RANK_MODEL * M + RANK_POOL);
  int less, eq;
  if (job < P) {                                                     // (the same branch in every thread of the workgroup)
    int a = 0, first = 0;
    while (job >= first + (M - 1 - a)) {
      first += M - 1 - a;
      ++a;
    }
    const int b = a + 1 + (job - first);
    const double* xa = cols + ((size_t)q * M + a) * Ncap;
    const double* xb = cols + ((size_t)q * M + b) * Ncap;
    // |d| of a sample that takes part, NaN otherwise (d of a kept sample is finite)
    auto value = [&](int j) {
      const int at = j < N ? j : 0;
      const double d = xa[at] - xb[at];
      return j < N && kq[at] && d != 0.0 ? fabs(d) : (double)NAN;
    };
    const int at = in ? i : 0;
    const bool kept = in && kq[at];
    const double d = xa[at] - xb[at];
    const bool used = kept && d != 0.0;
    count_against(used ? fabs(d) : (double)NAN, N, value, tile, less, eq);
    const long long twice_rank = 2LL * less + eq + 1;
    long long acc[RANK_PAIR];
    acc[0] = used ? 1 : 0;
    acc[1] = kept && !used ? 1 : 0;
    acc[2] = in && !kept ? 1 : 0;
    acc[3] = used && d > 0.0 ? twice_rank : 0;
    acc[4] = used && d < 0.0 ? twice_rank : 0;
    acc[5] = used ? (long long)eq * eq - 1 : 0;
    // a sample of at most 13: the size of the tie group that starts at rank position p, in bits [4 p, 4 p + 4)
    acc[6] = used && nkept[q] <= (u64)RANK_SMALL ? 1LL << (4 * (less & 15)) : 0;
    block_add<RANK_PAIR>(acc, wsum, tq + (size_t)RANK_PAIR * job);
  } else {
    const int m = job - P;
    const double* x = cols + ((size_t)q * M + m) * Ncap;
    auto value = [&](int j) {
      const int at = j < N ? j : 0;
      const double v = x[at];
      return j < N && kq[at] ? v : (double)NAN;
    };
    const int at = in ? i : 0;
    const bool kept = in && kq[at];
    const bool kn = known[at] != 0;
    const double xi = x[at];
    count_against(kept ? xi : (double)NAN, N, value, tile, less, eq);
    long long acc[RANK_PAIR];
    acc[0] = kept && kn ? 1 : 0;
    acc[1] = kept && !kn ? 1 : 0;
    acc[2] = kept && kn ? 2LL * less + eq + 1 : 0;
    acc[3] = kept ? (long long)eq * eq - 1 : 0;
    acc[4] = 0;
    acc[5] = 0;
    acc[6] = 0;                                                      // (a zero sum issues no atomic)
    block_add<RANK_PAIR>(acc, wsum, tq + (size_t)RANK_PAIR * P + (size_t)RANK_MODEL * m);
  }
}

// the kept values of all M models pooled: n = M kept[q], the order statistics 0, lo = floor(0.98 (n - 1)) and min(lo + 1, n - 1) as
// the bit patterns of the values (x + 0.0: a negative zero is written as +0.0, so tied elements write the same bits)
__global__ __launch_bounds__(256) void rank_pool_kernel(const double* __restrict__ cols, const unsigned char* __restrict__ keep,
                                                        const u64* __restrict__ kept, u64* __restrict__ table, int M, int N, int Ncap) {
  __shared__ double tile[RANK_TILE];
  const int P = M * (M - 1) / 2, q = blockIdx.y, total = M * N;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned char* kq = keep + (size_t)q * N;
  const double* xq = cols + (size_t)q * M * Ncap;
  u64* out = table + (size_t)q * (RANK_PAIR * P + RANK_MODEL * M + RANK_POOL) + RANK_PAIR * P + RANK_MODEL * M;
  auto value = [&](int j) {
    const int jj = j < total ? j : 0;
    const int m = jj / N, s = jj - m * N;
    const double v = xq[(size_t)m * Ncap + s] + 0.0;
    return j < total && kq[s] ? v : (double)NAN;
  };
  const double vi = value(i);
  int less, eq;
  count_against(vi, total, value, tile, less, eq);
  const long long n = (long long)M * (long long)kept[q];
  const long long lo = n > 0 ? (n - 1) * 49 / 50 : 0, hi = lo + 1 < n ? lo + 1 : lo;
  if (i == 0) out[0] = (u64)n;
  if (eq > 0) {                                                      // (vi takes part: it equals itself)
    const u64 pattern = (u64)__double_as_longlong(vi);
    if (less == 0) out[1] = pattern;
    if (less <= lo && lo < (long long)less + eq) out[2] = pattern;
    if (less <= hi && hi < (long long)less + eq) out[3] = pattern;
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

int mau_rank_tile(void) { return RANK_TILE; }

int mau_rank_max_samples(void) { return RANK_MAX_N; }

size_t mau_rank_table_elems(int M, int Q) {
  if (M < 1 || M > RANK_MAX_MODELS || Q < 1 || Q > RANK_MAX_Q) return 0;
  return (size_t)Q * rank_q_elems(M);
}

size_t mau_rank_ws_elems(int Q, int N) {
  if (Q < 1 || Q > RANK_MAX_Q || N < 1 || N > RANK_MAX_N) return 0;
  return (size_t)Q + ((size_t)Q * N + 7) / 8;
}

int mau_rank_tests(const double* cols, const unsigned char* known, int64_t* table, int64_t* ws, int M, int Q, int N, int Ncap,
                   mau_stream_t stream) {
  MAU_REQUIRE(cols && known && table && ws, "rank_tests: null pointer");
  MAU_REQUIRE(M >= 1 && M <= RANK_MAX_MODELS, "rank_tests: M must be in [1,%d], got %d", RANK_MAX_MODELS, M);
  MAU_REQUIRE(Q >= 1 && Q <= RANK_MAX_Q, "rank_tests: Q must be in [1,%d], got %d", RANK_MAX_Q, Q);
  MAU_REQUIRE(N >= 1, "rank_tests: no sample (N %d)", N);
  MAU_REQUIRE(N <= RANK_MAX_N, "rank_tests: at most 2^20 samples, got %d", N);
  MAU_REQUIRE(Ncap >= N, "rank_tests: the column capacity %d is below N = %d", Ncap, N);
  const hipStream_t st = (hipStream_t)stream;
  u64* tab = reinterpret_cast<u64*>(table);
  u64* kept = reinterpret_cast<u64*>(ws);
  unsigned char* keep = reinterpret_cast<unsigned char*>(ws + Q);
  const size_t telems = (size_t)Q * rank_q_elems(M);
  const size_t zmax = telems > (size_t)Q ? telems : (size_t)Q;
  MAU_LAUNCH(rank_zero_kernel, dim3(ceil_div((int64_t)zmax, 256)), dim3(256), 0, st, tab, telems, kept, (size_t)Q);
  int rc = check_launch("rank_zero_kernel");
  if (rc != 0) return rc;
  MAU_LAUNCH(rank_keep_kernel, dim3(ceil_div(N, 256), Q), dim3(256), 0, st, cols, keep, kept, M, N, Ncap);
  rc = check_launch("rank_keep_kernel");
  if (rc != 0) return rc;
  MAU_LAUNCH(rank_tests_kernel, dim3(ceil_div(N, RANK_TILE), rank_pairs(M) + M, Q), dim3(256), 0, st, cols, known, keep, kept, tab, M, N, Ncap);
  rc = check_launch("rank_tests_kernel");
  if (rc != 0) return rc;
  MAU_LAUNCH(rank_pool_kernel, dim3(ceil_div((int64_t)M * N, RANK_TILE), Q), dim3(256), 0, st, cols, keep, kept, tab, M, N, Ncap);
  return check_launch("rank_pool_kernel");
}

}  // extern "C"
