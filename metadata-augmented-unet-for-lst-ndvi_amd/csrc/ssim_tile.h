// ssim_tile.h -- one 16x16 tile of the SSIM map of one (image, channel) plane, shared by ssim_tiles_kernel (ssim.hip) and
// loss_terms_kernel (loss_terms.hip); its window, geometry and prepared, pooled load also serve ssim_grad_kernel (ssim.hip): piq.ssim's published defaults (11x11 Gaussian window, sigma 1.5, k1 0.01, k2 0.03, "valid"
// windows, average-pool downsampling by max(1, round(min(H, W) / 256))).  26x26 pooled window in LDS with the reference's channel
// preparation (src/utils/losses.py:72-84: channel 0 -> (v + 1) / 2, channel 1 -> clamp(v, 0, 1)) applied while loading, separable
// Gaussian (horizontal pass to LDS, vertical pass in registers) over x, y, x^2, y^2, xy.  No pragma here: the fp32 expressions
// take the including file's contraction mode, the same in both.
#pragma once
#include <math.h>
#include "mau_common.h"

namespace mau {

constexpr int SS_K = 11, SS_T = 16, SS_IN = SS_T + SS_K - 1;   // 26

struct SsimW {
  float g[SS_K];
};

static inline SsimW ssim_window() {
  SsimW w;
  double sum = 0.0, g[SS_K];
  for (int i = 0; i < SS_K; ++i) {
    const double d = i - (SS_K - 1) / 2.0;
    g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += g[i];
  }
  for (int i = 0; i < SS_K; ++i) w.g[i] = (float)(g[i] / sum);
  return w;
}

// f = max(1, round-half-even(min(H, W) / 256)) as Python's round() in piq's downsampling factor, valid 11x11 windows on the
// H/f x W/f pooled image: an Ho x Wo map in tx x ty tiles (0 tiles when the image is smaller than the window)
struct SsimGeometry {
  int f, Ho, Wo, tx, ty;
};
static inline SsimGeometry ssim_geometry(int H, int W) {
  SsimGeometry g;
  const int m = H < W ? H : W;
  g.f = (int)nearbyint(m / 256.0);
  if (g.f < 1) g.f = 1;
  g.Ho = H / g.f - (SS_K - 1);
  g.Wo = W / g.f - (SS_K - 1);
  g.tx = g.Wo > 0 ? ceil_div(g.Wo, SS_T) : 0;
  g.ty = g.Ho > 0 ? ceil_div(g.Ho, SS_T) : 0;
  return g;
}

// The N x N window of prepared, pooled pixels of the planes ob (output) and tb (target) of channel c whose first pixel is (y0, x0)
// of the Hd x Wd = H/f x W/f pooled image, into xs and ys; 0.0 where the window leaves that image (y0 and x0 may be negative).
// Every thread of the 256-thread workgroup calls it; no barrier inside.
template <int N>
__device__ __forceinline__ void ssim_load_window(float (*xs)[N + 1], float (*ys)[N + 1], const float* __restrict__ ob,
                                                 const float* __restrict__ tb, int c, int prep, int y0, int x0, int H, int W, int f) {
  const int Hd = H / f, Wd = W / f;
  const float inv = 1.f / (float)(f * f);
  for (int i = threadIdx.x; i < N * N; i += 256) {
    const int r = i / N, cc = i % N;
    const int y = y0 + r, x = x0 + cc;
    float xv = 0.f, yv = 0.f;
    if (y >= 0 && x >= 0 && y < Hd && x < Wd) {
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) {
          float a = ob[(size_t)(y * f + dy) * W + x * f + dx], b = tb[(size_t)(y * f + dy) * W + x * f + dx];
          if (prep) {
            if (c == 0) {
              a = (a + 1.f) * 0.5f;
              b = (b + 1.f) * 0.5f;
            } else if (c == 1) {
              a = fminf(fmaxf(a, 0.f), 1.f);
              b = fminf(fmaxf(b, 0.f), 1.f);
            }
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
}

// The SSIM value of map pixel (ty0 + threadIdx.x / 16, tx0 + threadIdx.x % 16) of the planes ob (output) and tb (target) of
// channel c, 0.0 outside the Ho x Wo map.  Every thread of the 256-thread workgroup calls it; two barriers inside.
__device__ __forceinline__ double ssim_tile_value(const float* __restrict__ ob, const float* __restrict__ tb, const SsimW& w, int c,
                                                  int prep, int ty0, int tx0, int H, int W, int f, int Ho, int Wo) {
  __shared__ float xs[SS_IN][SS_IN + 1], ys[SS_IN][SS_IN + 1];
  __shared__ float hz[5][SS_IN][SS_T + 1];
  ssim_load_window<SS_IN>(xs, ys, ob, tb, c, prep, ty0, tx0, H, W, f);
  __syncthreads();
  for (int i = threadIdx.x; i < SS_IN * SS_T; i += 256) {
    const int r = i / SS_T, cc = i % SS_T;
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < SS_K; ++k) {
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
  const int r = threadIdx.x / SS_T, cc = threadIdx.x % SS_T;
  if (ty0 + r >= Ho || tx0 + cc >= Wo) return 0.0;
  float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < SS_K; ++k) {
    const float g = w.g[k];
#pragma unroll
    for (int m = 0; m < 5; ++m) s[m] = fmaf(g, hz[m][r + k][cc], s[m]);
  }
  const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
  const float mx = s[0], my = s[1];
  const float sxx = s[2] - mx * mx, syy = s[3] - my * my, sxy = s[4] - mx * my;
  const float cs = (2.f * sxy + c2) / (sxx + syy + c2);
  return (double)((2.f * mx * my + c1) / (mx * mx + my * my + c1) * cs);
}

}  // namespace mau
