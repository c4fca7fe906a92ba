// head_shared.h -- what the entry points of head.hip's head kernels and of their BatchNorm-fused forms in bn_fused.hip have in common,
// ONE copy of each: the Co -> instantiation dispatch, the forward's pixels per workgroup, the argument check.  (The LDS join of the
// dW / db partials stays written out in head_bwd_kernel and in head_bn_bwd_reduce_kernel: the latter keeps 158 / 168 registers only by
// spilling, and through a shared function, however it was called, three of its twelve forms spilled differently.)
#pragma once
#include "mau_common.h"

namespace mau {

// MAU_HEAD_DISPATCH(Co, statement): runs the statement with the names MC_ and EX_ -- which the statement uses as template arguments,
// as MAU_DISPATCH_DTYPE's statement uses T -- bound to the instantiation that serves Co output channels.  The reference's head has two
// outputs: MC_ = 2 holds half the weight / accumulator registers of the general form; EX_: Co == MC_ (no per-term `o < Co` selects).
#define MAU_HEAD_CASE(MC, EX, ...) \
  {                                \
    constexpr int MC_ = MC;        \
    constexpr bool EX_ = EX;       \
    __VA_ARGS__;                   \
  }
#define MAU_HEAD_DISPATCH(Co, ...) /* Co: an int variable */                      \
  do {                                                                               \
    if (Co == 2) MAU_HEAD_CASE(2, true, __VA_ARGS__)                                 \
    else if (Co == 1) MAU_HEAD_CASE(2, false, __VA_ARGS__)                           \
    else if (Co == HEAD_MAX_CO) MAU_HEAD_CASE(HEAD_MAX_CO, true, __VA_ARGS__)        \
    else MAU_HEAD_CASE(HEAD_MAX_CO, false, __VA_ARGS__)                              \
  } while (0)

// pixels per workgroup of head_bn_fwd_kernel
static inline int head_fwd_pixb(int64_t npix) { return npix >= ((int64_t)1 << 20) ? 1024 : 128; }

// the conditions the BatchNorm-fused head entry points share, in the order they are reported (ld_good: the entry point's own
// leading-dimension conditions); `who` names the entry point in the message
static inline int head_bn_check(const char* who, int N, int HW, int C, int Co, bool ld_good) {
  MAU_REQUIRE(Co >= 1 && Co <= HEAD_MAX_CO && C <= mau_head_bn_max_channels(), "%s: out_channels in [1,%d], C <= %d", who, HEAD_MAX_CO,
              mau_head_bn_max_channels());
  MAU_REQUIRE(ld_good, "%s: bad ld", who);
  MAU_REQUIRE(HW >= 32 && (int64_t)N * HW < ((int64_t)1 << 31), "%s: images of at least 32 pixels, fewer than 2^31 pixels in all", who);
  return MAU_OK;
}

}  // namespace mau
