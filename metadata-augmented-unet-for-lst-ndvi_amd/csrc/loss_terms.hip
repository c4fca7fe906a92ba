// loss_terms.hip -- every term of the reference's compute_all_loss (src/utils/losses.py:101-115) for one (outputs, targets)
// pair in ONE launch: mse (:33), pixel = L1 (:67), the two halves of gradient_loss (:14-25), the SSIM loss (:72-89) and the
// two totals (:51, :92).  The validation pass (src/train.py:20-60) needs all of them per batch and none carries a gradient.
//
// What one workgroup owns.  Grid (tilesX, tilesY, B*C), as ssim_tiles_kernel: a workgroup is one 16x16 tile of the SSIM map of one
// (image, channel) plane.  With f the pooling factor of ssim.hip it owns
//   * the SSIM pixels [16 by, 16 by + 16) x [16 bx, 16 bx + 16) of the (H/f - 10) x (W/f - 10) map: ssim_tile.h's tile with the
//     reference's channel preparation (:72-84), the function ssim_tiles_kernel calls;
//   * the full-resolution rectangle rows [16 f by, 16 f (by + 1)) x columns [16 f bx, 16 f (bx + 1)) for the element-wise terms; the
//     last tile of an axis extends to H (to W): it picks up the 10 f pixel margin of the window and the H mod f (W mod f) remainder
//     that the pooling drops.  The rectangles of a plane are disjoint and cover it;
//   * of the finite differences, the pair (y, y + 1) in column x and the pair (x, x + 1) in row y belong to the owner of pixel
//     (y, x): a pair that straddles two tiles is counted once, by the upper / left one (the partner comes from the neighbour's
//     rectangle through the cache -- the window load of this workgroup or of the neighbour has just brought it in).
// Every per-element value is the fp32 expression of mse_kernel / l1_gradient_loss_kernel (head.hip); sums are fp64 in a fixed
// order: a thread adds its elements in index order and chunk_reduce.h's block_join (xor butterfly, waves in wave order) sends
// the five partials of the workgroup to `ws`.  The workgroup that draws the last ticket (last_block_of) adds the
// partials -- lane l of a wave takes partials l, l + 64, ... in index order, then the same butterfly -- and writes terms,
// ssim_per_image and the optional accumulator.  No float atomics; the bits do not depend on which workgroup finishes last.
#include <math.h>
#include "chunk_reduce.h"
#include "ssim_tile.h"

namespace mau {

constexpr int LT_T = SS_T;
constexpr int LT_PART = 5;                                    // partials per workgroup: ssim, (o-t)^2, |o-t|, dy, dx

// lanes of one wave: partials p[0 .. n) in index order per lane, then the butterfly (every lane returns the same bits)
__device__ __forceinline__ double lt_wave_reduce(const double* p, int n, int lane) {
  double s = 0.0;
  for (int i = lane; i < n; i += 64) s += p[i];
  return wave_join(s, [](double a, double b) { return a + b; });
}

// the scalars of the batch from the finished sums; fp32 in the reference's order of operations, nothing contracted
__device__ void lt_finish(const double* el, double ssim_tot, float* __restrict__ terms, double* __restrict__ acc, float lambda_grad,
                          float lambda_ssim, int B, double inv_n, double inv_ny, double inv_nx) {
#pragma clang fp contract(off)
  float t[8];
  t[0] = (float)(el[0] * inv_n);                         // F.mse_loss, losses.py:33
  t[1] = (float)(el[1] * inv_n);                         // F.l1_loss, :67
  t[2] = (float)(el[2] * inv_ny);                        // dy_loss, :22
  t[3] = (float)(el[3] * inv_nx);                        // dx_loss, :23
  t[4] = t[2] + t[3];                                    // :25
  t[5] = (float)(1.0 - ssim_tot / (double)B);            // :89
  const float lg = lambda_grad * t[4];
  t[6] = t[0] + lg;                                      // :51
  const float ls = lambda_ssim * t[5];
  t[7] = (t[1] + lg) + ls;                               // :92
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    terms[k] = t[k];
    if (acc != nullptr) acc[k] = acc[k] + (double)B * (double)t[k];      // src/train.py:42,48: v.item() * len(batch)
  }
}

__global__ __launch_bounds__(256) void loss_terms_kernel(const float* __restrict__ out, const float* __restrict__ tgt, double* ws,
                                                         unsigned* tickets, float* __restrict__ terms, float* __restrict__ per_image,
                                                         double* __restrict__ acc, SsimW w, float lambda_grad, float lambda_ssim, int C,
                                                         int H, int W, int f, int Ho, int Wo) {
  __shared__ double wsum[4][LT_PART];
  __shared__ double fin[4 + 4];
  const int tilesX = gridDim.x, tilesY = gridDim.y;
  const int bc = blockIdx.z, c = bc % C;
  const int ty0 = blockIdx.y * LT_T, tx0 = blockIdx.x * LT_T;
  const float* ob = out + (size_t)bc * H * W;
  const float* tb = tgt + (size_t)bc * H * W;

  double part[LT_PART] = {0.0, 0.0, 0.0, 0.0, 0.0};
  part[0] = ssim_tile_value(ob, tb, w, c, 1, ty0, tx0, H, W, f, Ho, Wo);

  // ---- element-wise terms of the owned rectangle ----
  {
    const int Y0 = ty0 * f, X0 = tx0 * f;
    const int Y1 = (int)blockIdx.y == tilesY - 1 ? H : Y0 + LT_T * f;
    const int X1 = (int)blockIdx.x == tilesX - 1 ? W : X0 + LT_T * f;
    const int rw = X1 - X0, npx = (Y1 - Y0) * rw;
    for (int idx = threadIdx.x; idx < npx; idx += 256) {
      const int ry = idx / rw;
      const int y = Y0 + ry, x = X0 + (idx - ry * rw);
      const size_t q = (size_t)y * W + x;
      const float o = ob[q], t = tb[q];
      const float d = o - t;
      part[1] += (double)(d * d);
      part[2] += fabsf(d);
      if (y + 1 < H) {
        const float a = ob[q + W] - o, b = tb[q + W] - t;
        part[3] += fabsf(fabsf(a) - fabsf(b));
      }
      if (x + 1 < W) {
        const float a = ob[q + 1] - o, b = tb[q + 1] - t;
        part[4] += fabsf(fabsf(a) - fabsf(b));
      }
    }
  }

  // ---- the workgroup's five partials ----
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntiles = tilesX * tilesY;
  const size_t nb = (size_t)ntiles * gridDim.z;
  block_join<LT_PART>(part, wsum, SumAll(), ws + (size_t)bc * ntiles + blockIdx.y * tilesX + blockIdx.x, nb);
  if (!last_block_of(tickets, (unsigned)nb)) return;

  // ---- level 2: wave k adds element-wise quantity k; then the waves take the images in turn ----
  {
    const double s = lt_wave_reduce(ws + (size_t)(1 + wave) * nb, (int)nb, lane);
    if (lane == 0) fin[wave] = s;
  }
  const int B = gridDim.z / C;
  const double inv_pix = 1.0 / ((double)Ho * Wo);
  double tot = 0.0;
  for (int b = wave; b < B; b += 4) {
    double sb = 0.0;
    for (int ch = 0; ch < C; ++ch) sb += lt_wave_reduce(ws + ((size_t)b * C + ch) * ntiles, ntiles, lane) * inv_pix;
    sb /= (double)C;
    if (lane == 0) per_image[b] = (float)sb;
    tot += sb;
  }
  if (lane == 0) fin[4 + wave] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = (double)gridDim.z * H * W;
    lt_finish(fin, ((fin[4] + fin[5]) + fin[6]) + fin[7], terms, acc, lambda_grad, lambda_ssim, B, 1.0 / n,
              1.0 / ((double)gridDim.z * (H - 1) * W), 1.0 / ((double)gridDim.z * H * (W - 1)));
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

size_t mau_loss_terms_ws_elems(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const SsimGeometry g = ssim_geometry(H, W);
  return (size_t)LT_PART * B * C * g.tx * g.ty;
}

int mau_loss_terms(const float* out, const float* tgt, double* ws, unsigned* tickets, float* terms, float* ssim_per_image, double* acc,
                   float lambda_grad, float lambda_ssim, int B, int C, int H, int W, mau_stream_t stream) {
  MAU_REQUIRE(out && tgt && ws && tickets && terms && ssim_per_image, "loss_terms: null pointer");
  MAU_REQUIRE(B > 0 && H > 0 && W > 0, "loss_terms: non-positive dimension (B %d, H %d, W %d)", B, H, W);
  MAU_REQUIRE(C == 2, "loss_terms: the channel preparation is defined for (NDVI, temperature) only: C must be 2, got %d", C);
  const SsimGeometry g = ssim_geometry(H, W);
  MAU_REQUIRE(g.Ho > 0 && g.Wo > 0, "loss_terms: image %dx%d is smaller than the 11x11 window after downsampling by %d", H, W, g.f);
  MAU_REQUIRE((int64_t)B * C <= 65535 && g.ty <= 65535, "loss_terms: B*C and tile rows must fit a grid dimension");
  MAU_REQUIRE((int64_t)H * W <= (1 << 30) && (int64_t)B * C * g.tx * g.ty <= (1 << 30), "loss_terms: at most 2^30 pixels per map and 2^30 tiles");
  MAU_LAUNCH(loss_terms_kernel, dim3(g.tx, g.ty, B * C), dim3(256), 0, (hipStream_t)stream, out, tgt, ws, tickets, terms, ssim_per_image, acc,
             ssim_window(), lambda_grad, lambda_ssim, C, H, W, g.f, g.Ho, g.Wo);
  return check_launch("loss_terms_kernel");
}

}  // extern "C"
