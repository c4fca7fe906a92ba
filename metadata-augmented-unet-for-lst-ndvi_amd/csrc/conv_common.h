// conv_common.h -- declarations shared by the convolution translation units.
#pragma once
#include <stdlib.h>
#include "mau_common.h"

namespace mau {

// Test hooks: the only environment variables the library reads.  They exist for the tests and the A/B scripts, which run both
// sides of a dispatch rule on the same library; no product path sets them.
//   MAU_CONV_KG=0    no K-group launches (k_groups_rule)          MAU_CONV_M16=0  the 32x32x16 loop on the big tiles too
//   MAU_CONV_L0=0|1  force <64,4,8> | <64,4,4> on 64-channel tiles  MAU_WGRAD16=0   the 32x32x16 weight gradient everywhere
//   MAU_WGRAD_SPLITS_FORCE=s   the weight gradient's split count (clipped by wgrad_splits)
// The first four are read once per process; the split count is read per call (a test walks several counts in one process).
// So an A/B of one of the first four needs a process per side: changing os.environ after the first launch does nothing
// (scripts/wgrad_ab.py flips its variable inside one process -- it can compare split counts only).
struct TestHooks {
  bool conv_kg, conv_m16, wgrad16;
  int conv_l0;                               // -1: the rule decides
  static int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
  }
  static int wgrad_splits_force() { return env_int("MAU_WGRAD_SPLITS_FORCE", 0); }   // < 1: the rule decides
};
inline const TestHooks& test_hooks() {
  static const TestHooks h = {TestHooks::env_int("MAU_CONV_KG", 1) != 0, TestHooks::env_int("MAU_CONV_M16", 1) != 0,
                              TestHooks::env_int("MAU_WGRAD16", 1) != 0, TestHooks::env_int("MAU_CONV_L0", -1)};
  return h;
}

// 16 zero bytes in global memory: DMA source of padding pixels / channels (one copy per translation unit)
static __device__ __attribute__((aligned(16))) unsigned int g_zero_page[4] = {0u, 0u, 0u, 0u};

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// 16-bit operand fragments travel as raw 128-bit registers (typed bf16x8); F16 selects how the matrix core reads them
template <bool F16>
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

struct ConvP {
  const void* x;
  int ldx, C0;
  const void* x1;       // optional second tensor source: input channels [C0, C0 + C1) (virtual channel concat), else nullptr
  int ldx1, C1;
  const float* emb;     // fp32 (N,E) broadcast source (float kernels)
  const void* emb_lp;   // the same in the activation dtype (bf16 kernel), filled by the C entry point
  int E;
  const void* w;
  const float* bias;
  const float* post_scale;   // optional: out = relu(post_scale[co] * (conv + bias) + post_shift[co])  (eval-mode BN + ReLU)
  const float* post_shift;
  void* y;
  int ldy, Cout, CoutPad;
  float* slab;
  int N, H, W, tilesX, tilesY, nChunks;
  int xcdShift;         // log2(XCDs of the device) for the XCD-contiguous work-item order (bf16 kernel, set by its launcher)
  int fast;             // (bf16 kernel, set by its launcher) every 16-channel stage lies inside one tensor: buffer-addressed loader
  void* pool = nullptr; // optional (inference epilogue of the 16x16x32 tilings): MaxPool2d(2,2) of the activation, (N, H/2, W/2, ldpool)
  int ldpool = 0;
};

// C/D layout of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }


// ------------------------------------------------------------------------------------------
// weight gradient
// ------------------------------------------------------------------------------------------
struct WgradP {
  const void* x;
  int ldx, C0;
  const void* x1;       // optional second tensor source (channels [C0, C0 + C1) of the convolution's input)
  int ldx1, C1;
  const float* emb;
  const void* emb_lp;   // embedding in the activation dtype (bf16 kernel)
  int E;
  const void* dy;
  int lddy, Cout, CoutPad, Cin, CinPad;
  float* acc;
  int N, H, W, tilesX, tilesY, nTiles;
};

// packed-weight K-chunk per dtype (both 16: one k16 bf16 MFMA step / eight k2 fp32 MFMA steps per tap)
template <typename T>
struct PackKC {
  static constexpr int value = 16;
};

int launch_conv_bf16_v2(const ConvP& p, bool f16, hipStream_t st);   // 16-bit kernels: bf16 or (f16 = true) fp16 operands
int conv_bf16_v2_num_pixel_tiles(int N, int H, int W, int Cout);
void conv_bf16_v2_variant(int N, int H, int W, int Cin, int Cout, int* th, int* nw, int* bn, int* kg);
// The launch plan of one 16-bit weight gradient (make_wg_plan, conv3x3_wgrad_bf16.hip): the split-count query reads it, the
// launchers of both kernels execute it.
struct WgPlan {
  bool k16;             // the 16x16x32 kernel on 4 x 32 pixel tiles (conv3x3_wgrad16.hip), else the 32x32x16 kernel on 8 x 16 ones
  int th, tw;           // pixel tile
  int bco;              // output channels per workgroup
  int outTiles;         // (output-channel block, 64-input-channel block) work items per split
  int tilesX, tilesY, nTiles;
  int nsplit;           // partial slabs = workgroups along the split axis
  int xcd_shift, grid;  // the kernels' work-item order (wgrad_xcd_shift) and the grid that goes with it
  bool mixed;           // some 64-channel block of input channels straddles two sources
};
int launch_wgrad_bf16_v2(const WgradP& p, bool f16, hipStream_t st);      // writes nsplit partial slabs (plain stores)
int launch_wgrad16(const WgradP& q, bool f16, const WgPlan& pl, hipStream_t st);
int wgrad_bf16_v2_splits(int N, int H, int W, int Cout, int Cin);

}  // namespace mau
