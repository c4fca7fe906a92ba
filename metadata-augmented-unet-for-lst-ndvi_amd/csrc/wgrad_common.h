// wgrad_common.h -- the split-K scaffold shared by the two 16-bit weight-gradient kernels (conv3x3_wgrad_bf16.hip: 8 x 16 pixel
// tiles on v_mfma_f32_32x32x16; conv3x3_wgrad16.hip: 4 x 32 ones on v_mfma_f32_16x16x32): operand fragment reads, the work-item
// order, the pixel-tile cursor, the hand-over between two wave groups and the launch.  Operand images, swizzles, DMA slot tables,
// schedules, MFMA wrappers and the slab-store lane maps differ and stay with their kernel.
#pragma once
#include "igemm_bf16_util.h"

namespace mau {
namespace wgrad {

constexpr int BCI = 64;                             // input channels per workgroup (both kernels)

using igemm::u32x4;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// one k16 operand fragment = two transposed 8-byte reads (k 0..3 | 4..7 of the lane half's 8 pixels), joined into the
// MFMA's 4-register operand AT THE READ: joined later (after the counted wait had taken the two halves as separate
// in/out operands) the halves lived in unrelated register pairs and every fragment cost 2-4 v_mov -- 97 copies per stage
// next to 72 MFMAs, in a kernel whose clock falls with every vector instruction.
struct Frag {
  u32x4 v;
};
template <int OFF, int HI>
__device__ __forceinline__ void tr_read(Frag& f, unsigned addr) {
  static_assert(OFF >= 0 && OFF + HI < 65536, "ds offset field");
  u32x2 lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4"
               : "=&v"(lo), "=&v"(hi)       // early-clobber: the second read still needs the address register (conv3x3_first.hip tr_frag)
               : "v"(addr), "n"(OFF), "n"(OFF + HI));
  f.v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
}

// ---- work item: (pixel split, output tile) from the 1-D workgroup id; false = surplus workgroup, leave (before any barrier) ----
// The workgroups of one split stream the SAME pixels (dY tile shared by the ci tiles, X halo shared by the co tiles).
// Hardware deals workgroup ids round-robin over the XCDs (id % 8; speed only): with xcd_shift > 0 (nsplit a multiple of the XCD
// count) XCD k owns the splits = k (mod 8) and walks their tiles in order, so all tiles of a split are resident on ONE
// XCD at about the same time and its L2 serves the re-reads.  With id = split + nsplit * tile (the other form), a split
// count like 85 or 21 scattered the tiles of a split over all XCDs: conv0_1.conv1 read its 268 MB dY three times.
__device__ __forceinline__ bool work_item(int id, int nsplit, int xcd_shift, int tilesOut, int& split, int& tile_id) {
  if (xcd_shift > 0) {
    const int k = id & ((1 << xcd_shift) - 1), j = id >> xcd_shift;
    tile_id = j % tilesOut;
    split = ((j / tilesOut) << xcd_shift) + k;
  } else if (xcd_shift < 0) {
    // any other split count: the (split, tile) list in split-major order is cut into one contiguous run per XCD -- the tiles of a
    // split are still resident on one XCD (two at a run boundary) at about the same time.  The grid is rounded up to a whole number
    // of workgroups per XCD; the (at most XCDs - 1) surplus workgroups leave.
    const int sh = -xcd_shift, k = id & ((1 << sh) - 1), j = id >> sh;
    const int total = nsplit * tilesOut, per = (total + (1 << sh) - 1) >> sh;
    const int w = k * per + j;
    if (w >= total) return false;
    split = w / tilesOut;
    tile_id = w - split * tilesOut;
  } else {
    split = id % nsplit;
    tile_id = id / nsplit;
  }
  return true;
}

// ---- split-K: the pixel tiles [t0, t1) of a split (none if the split count does not divide the tiles), and the cursor (lcur; n = ln,
// ty = lty, tx = ltx) of the tile being LOADED, advanced incrementally (wave-uniform scalars); past the last tile the cursor stays
// there: the tile is re-fetched into an idle buffer (nobody reads it), which keeps the DMA count per stage fixed.  The cursor is
// four ints of the kernel, not a struct: as members they cost the kernels a different (no better) instruction order ----
__device__ __forceinline__ void split_range(int split, int nsplit, int nTiles, int& t0, int& t1) {
  const int per = (nTiles + nsplit - 1) / nsplit;
  t0 = split * per;
  t1 = min(nTiles, t0 + per);
}
__device__ __forceinline__ void first_tile(int t0, int tilesX, int tilesY, int& lcur, int& ltx, int& lty, int& ln) {
  lcur = t0;
  ltx = t0 % tilesX;
  lty = (t0 / tilesX) % tilesY;
  ln = t0 / (tilesX * tilesY);
}
__device__ __forceinline__ void advance(int& lcur, int& ltx, int& lty, int& ln, int t1, int tilesX, int tilesY) {
  if (lcur + 1 < t1) {
    ++lcur;
    if (++ltx == tilesX) {
      ltx = 0;
      if (++lty == tilesY) {
        lty = 0;
        ++ln;
      }
    }
  }
}

// ---- KG = 2: the two wave groups add their accumulators (16 floats per tap per lane) through LDS in a fixed order, group 0 +
// group 1: one of the three rounds of 3 taps each.  red = the wave pair's area of hand_over_floats; the sum is left in group 0's
// registers.  The caller unrolls the rounds after one s_barrier (every wave is done with the stage buffers red overlays) ----
constexpr int hand_over_floats = 3 * 16 * 64;      // per wave pair
__device__ __forceinline__ void wave_groups_round(float (&acc)[9][16], float* red, int round, int kg, int lane) {
  if (kg == 1) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(t * 16 + r) * 64 + lane] = acc[round * 3 + t][r];
  }
  __syncthreads();
  if (kg == 0) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[round * 3 + t][r] += red[(t * 16 + r) * 64 + lane];
  }
  __syncthreads();
}

// ---- launch: LDS = the kernel's stage buffers or, if larger, the hand-over area of wave_groups_round ----
template <auto KERNEL, size_t STAGES, int NW, int KG>
static int launch(const char* name, const WgradP& p, const WgPlan& pl, hipStream_t st) {
  constexpr size_t red = KG == 2 ? (size_t)(NW / 2) * hand_over_floats * sizeof(float) : 0;
  constexpr size_t lds = STAGES > red ? STAGES : red;
  static_assert(lds <= 160 * 1024, "LDS budget");
  MAU_LDS_ATTR(lds, KERNEL);
  MAU_LAUNCH(KERNEL, dim3(pl.grid), dim3(NW * 64), lds, st, p, pl.nsplit, pl.xcd_shift);
  return check_launch(name);
}

}  // namespace wgrad
}  // namespace mau
