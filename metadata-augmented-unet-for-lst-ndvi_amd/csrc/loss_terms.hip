// loss_terms.hip -- every term of the reference's compute_all_loss (src/utils/losses.py:101-115) for one (outputs, targets)
// pair in ONE launch: mse (:33), pixel = L1 (:67), the two halves of gradient_loss (:14-25), the SSIM loss (:72-89) and the
// two totals (:51, :92).  The validation pass (src/train.py:20-60) needs all of them per batch and none carries a gradient.
//
// What one workgroup owns.  Grid (tilesX, tilesY, B*C), as ssim_tiles_kernel: a workgroup is one 16x16 tile of the SSIM map of one
// (image, channel) plane.  With f the pooling factor of ssim.hip it owns
//   * the SSIM pixels [16 by, 16 by + 16) x [16 bx, 16 bx + 16) of the (H/f - 10) x (W/f - 10) map: 26x26 pooled window in LDS, the
//     reference's channel preparation (:72-84) applied while loading, separable 11-tap Gaussian -- the per-pixel arithmetic is
//     ssim_tiles_kernel's, expression for expression;
//   * the full-resolution rectangle rows [16 f by, 16 f (by + 1)) x columns [16 f bx, 16 f (bx + 1)) for the element-wise terms; the
//     last tile of an axis extends to H (to W): it picks up the 10 f pixel margin of the window and the H mod f (W mod f) remainder
//     that the pooling drops.  The rectangles of a plane are disjoint and cover it;
//   * of the finite differences, the pair (y, y + 1) in column x and the pair (x, x + 1) in row y belong to the owner of pixel
//     (y, x): a pair that straddles two tiles is counted once, by the upper / left one (the partner comes from the neighbour's
//     rectangle through the cache -- the window load of this workgroup or of the neighbour has just brought it in).
// Every per-element value is the fp32 expression of mse_kernel / l1_gradient_loss_kernel (head.hip); sums are fp64 in a fixed
// order: a thread adds its elements in index order, a wave joins its lanes by an xor butterfly, the four waves are added in wave
// order and the five partials of the workgroup go to `ws`.  The workgroup that draws the last ticket (last_block_of) adds the
// partials -- lane l of a wave takes partials l, l + 64, ... in index order, then the same butterfly -- and writes terms,
// ssim_per_image and the optional accumulator.  No float atomics; the bits do not depend on which workgroup finishes last.
#include <math.h>
#include "mau_common.h"

namespace mau {

constexpr int LT_K = 11, LT_T = 16, LT_IN = LT_T + LT_K - 1;   // 26
constexpr int LT_PART = 5;                                    // partials per workgroup: ssim, (o-t)^2, |o-t|, dy, dx

struct LtW {
  float g[LT_K];
};

__device__ __forceinline__ double lt_wave_sum(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// lanes of one wave: partials p[0 .. n) in index order per lane, then the butterfly (every lane returns the same bits)
__device__ __forceinline__ double lt_wave_reduce(const double* p, int n, int lane) {
  double s = 0.0;
  for (int i = lane; i < n; i += 64) s += p[i];
  return lt_wave_sum(s);
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
                                                         double* __restrict__ acc, LtW w, float lambda_grad, float lambda_ssim, int C,
                                                         int H, int W, int f, int Ho, int Wo) {
  __shared__ float xs[LT_IN][LT_IN + 1], ys[LT_IN][LT_IN + 1];
  __shared__ float hz[5][LT_IN][LT_T + 1];
  __shared__ double wsum[4][LT_PART];
  __shared__ double fin[4 + 4];
  const int tilesX = gridDim.x, tilesY = gridDim.y;
  const int bc = blockIdx.z, c = bc % C;
  const int ty0 = blockIdx.y * LT_T, tx0 = blockIdx.x * LT_T;
  const float* ob = out + (size_t)bc * H * W;
  const float* tb = tgt + (size_t)bc * H * W;
  const int Hd = H / f, Wd = W / f;
  const float inv = 1.f / (float)(f * f);

  // ---- SSIM tile (ssim_tiles_kernel with prep != 0) ----
  for (int i = threadIdx.x; i < LT_IN * LT_IN; i += 256) {
    const int r = i / LT_IN, cc = i % LT_IN;
    const int y = ty0 + r, x = tx0 + cc;
    float xv = 0.f, yv = 0.f;
    if (y < Hd && x < Wd) {
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) {
          float a = ob[(size_t)(y * f + dy) * W + x * f + dx], b = tb[(size_t)(y * f + dy) * W + x * f + dx];
          if (c == 0) {
            a = (a + 1.f) * 0.5f;
            b = (b + 1.f) * 0.5f;
          } else {
            a = fminf(fmaxf(a, 0.f), 1.f);
            b = fminf(fmaxf(b, 0.f), 1.f);
          }
          xv += a;
          yv += b;
        }
      xv *= inv;
      yv *= inv;
    }
    xs[r][cc] = xv;
    ys[r][cc] = yv;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LT_IN * LT_T; i += 256) {
    const int r = i / LT_T, cc = i % LT_T;
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < LT_K; ++k) {
      const float a = xs[r][cc + k], b = ys[r][cc + k], g = w.g[k];
      s[0] = fmaf(g, a, s[0]);
      s[1] = fmaf(g, b, s[1]);
      s[2] = fmaf(g, a * a, s[2]);
      s[3] = fmaf(g, b * b, s[3]);
      s[4] = fmaf(g, a * b, s[4]);
    }
#pragma unroll
    for (int m = 0; m < 5; ++m) hz[m][r][cc] = s[m];
  }
  __syncthreads();
  double part[LT_PART] = {0.0, 0.0, 0.0, 0.0, 0.0};
  {
    const int r = threadIdx.x / LT_T, cc = threadIdx.x % LT_T;
    if (ty0 + r < Ho && tx0 + cc < Wo) {
      float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < LT_K; ++k) {
        const float g = w.g[k];
#pragma unroll
        for (int m = 0; m < 5; ++m) s[m] = fmaf(g, hz[m][r + k][cc], s[m]);
      }
      const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
      const float mx = s[0], my = s[1];
      const float sxx = s[2] - mx * mx, syy = s[3] - my * my, sxy = s[4] - mx * my;
      const float cs = (2.f * sxy + c2) / (sxx + syy + c2);
      part[0] = (double)((2.f * mx * my + c1) / (mx * mx + my * my + c1) * cs);
    }
  }

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
#pragma unroll
  for (int v = 0; v < LT_PART; ++v) part[v] = lt_wave_sum(part[v]);
  if (lane == 0) {
#pragma unroll
    for (int v = 0; v < LT_PART; ++v) wsum[wave][v] = part[v];
  }
  __syncthreads();
  const int ntiles = tilesX * tilesY;
  const size_t nb = (size_t)ntiles * gridDim.z;
  const size_t blk = (size_t)bc * ntiles + blockIdx.y * tilesX + blockIdx.x;
  if (threadIdx.x < LT_PART) {
    const int v = threadIdx.x;
    ws[(size_t)v * nb + blk] = ((wsum[0][v] + wsum[1][v]) + wsum[2][v]) + wsum[3][v];
  }
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

// geometry of ssim.hip: f = max(1, round-half-even(min(H, W) / 256)), valid 11x11 windows on the H/f x W/f pooled image
static void lt_geometry(int H, int W, int* f, int* Ho, int* Wo, int* tx, int* ty) {
  const int m = H < W ? H : W;
  int ff = (int)nearbyint(m / 256.0);
  if (ff < 1) ff = 1;
  *f = ff;
  *Ho = H / ff - (LT_K - 1);
  *Wo = W / ff - (LT_K - 1);
  *tx = *Wo > 0 ? ceil_div(*Wo, LT_T) : 0;
  *ty = *Ho > 0 ? ceil_div(*Ho, LT_T) : 0;
}

size_t mau_loss_terms_ws_elems(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  int f, Ho, Wo, tx, ty;
  lt_geometry(H, W, &f, &Ho, &Wo, &tx, &ty);
  return (size_t)LT_PART * B * C * tx * ty;
}

int mau_loss_terms(const float* out, const float* tgt, double* ws, unsigned* tickets, float* terms, float* ssim_per_image, double* acc,
                   float lambda_grad, float lambda_ssim, int B, int C, int H, int W, mau_stream_t stream) {
  MAU_REQUIRE(out && tgt && ws && tickets && terms && ssim_per_image, "loss_terms: null pointer");
  MAU_REQUIRE(B > 0 && H > 0 && W > 0, "loss_terms: non-positive dimension (B %d, H %d, W %d)", B, H, W);
  MAU_REQUIRE(C == 2, "loss_terms: the channel preparation is defined for (NDVI, temperature) only: C must be 2, got %d", C);
  int f, Ho, Wo, tx, ty;
  lt_geometry(H, W, &f, &Ho, &Wo, &tx, &ty);
  MAU_REQUIRE(Ho > 0 && Wo > 0, "loss_terms: image %dx%d is smaller than the 11x11 window after downsampling by %d", H, W, f);
  MAU_REQUIRE((int64_t)B * C <= 65535 && ty <= 65535, "loss_terms: B*C and tile rows must fit a grid dimension");
  MAU_REQUIRE((int64_t)H * W <= (1 << 30) && (int64_t)B * C * tx * ty <= (1 << 30), "loss_terms: at most 2^30 pixels per map and 2^30 tiles");
  LtW w;
  double sum = 0.0, g[LT_K];
  for (int i = 0; i < LT_K; ++i) {
    const double d = i - (LT_K - 1) / 2.0;
    g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += g[i];
  }
  for (int i = 0; i < LT_K; ++i) w.g[i] = (float)(g[i] / sum);
  MAU_LAUNCH(loss_terms_kernel, dim3(tx, ty, B * C), dim3(256), 0, (hipStream_t)stream, out, tgt, ws, tickets, terms, ssim_per_image, acc, w,
             lambda_grad, lambda_ssim, C, H, W, f, Ho, Wo);
  return check_launch("loss_terms_kernel");
}

}  // extern "C"
