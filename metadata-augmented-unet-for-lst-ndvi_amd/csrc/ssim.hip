// ssim.hip -- the SSIM term of compute_loss_l1_grad_ssim (reference src/utils/losses.py:70-97: piq.ssim(outputs_ssim,
// targets_ssim, data_range=1.0, reduction='none') per sample, then 1 - mean) as one fused HIP reduction.
//
// piq is not available in the build environment; the kernel follows piq.ssim's published defaults (11x11 Gaussian window,
// sigma 1.5, k1 0.01, k2 0.03, "valid" windows, average-pool downsampling by max(1, round(min(H, W) / 256))) -- the same
// formula the torch-op version in mau_amd/losses.py::ssim_value_torch spells out.  PARITY UNPINNED (no fixture from the
// reference exists for this scalar); it carries no gradient in the reference (torch.Tensor(ssim_vals) at :96 detaches it).
//
// One block = one 16x16 tile of SSIM-map pixels of one (image, channel): the per-pixel value is ssim_tile.h's (channel
// preparation :72-84 fused into the tile load when prep != 0), block sum in fp64.
//
// ssim_grad_kernel is that loss's adjoint, for whoever opts in to train on the term (mau_ssim_loss_grad; closed form checked against
// tests/ssim_grad_ref.py): one pixel-owned launch, see the kernel.
#include <math.h>
#include "ssim_tile.h"

namespace mau {

__global__ __launch_bounds__(256) void ssim_tiles_kernel(const float* __restrict__ out, const float* __restrict__ tgt, double* __restrict__ part,
                                                         SsimW w, int C, int H, int W, int f, int Ho, int Wo, int tilesX, int tilesY,
                                                         int prep) {
  __shared__ double red[256];
  const int bc = blockIdx.z;
  const double v = ssim_tile_value(out + (size_t)bc * H * W, tgt + (size_t)bc * H * W, w, bc % C, prep, blockIdx.y * SS_T,
                                   blockIdx.x * SS_T, H, W, f, Ho, Wo);
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if (threadIdx.x < s2) red[threadIdx.x] += red[threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)bc * tilesX * tilesY + blockIdx.y * tilesX + blockIdx.x] = red[0];
}

// per_image[b] = mean over channels of (sum of the tiles of (b, c) / (Ho*Wo)); loss[0] = 1 - mean over images
__global__ void ssim_finalize_kernel(const double* __restrict__ part, float* __restrict__ per_image, float* __restrict__ loss, int B, int C,
                                     int ntiles, double inv_pix) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double tot = 0.0;
  for (int b = 0; b < B; ++b) {
    double sb = 0.0;
    for (int c = 0; c < C; ++c) {
      double s = 0.0;
      for (int t = 0; t < ntiles; ++t) s += part[((size_t)b * C + c) * ntiles + t];
      sb += s * inv_pix;
    }
    sb /= (double)C;
    per_image[b] = (float)sb;
    tot += sb;
  }
  loss[0] = (float)(1.0 - tot / (double)B);
}

// ---- the adjoint: d(1 - mean SSIM) / d out, pixel-owned ----
// One block owns a 16x16 tile of POOLED input pixels q of one (image, channel) and writes the 16f x 16f output cells below it (the
// last tile of an axis also writes the zeros of the rows / columns avg_pool2d drops).  Map pixel p reaches q when 0 <= q - p <= 10
// in both axes, so the tile needs a0/a2/a4 (dS/ds0, dS/ds2, dS/ds4 with the chain through sxx, syy, sxy folded in) on the 26x26
// map pixels from q0 - 10 on, hence the five moments there, hence the 36x36 pooled window from q0 - 10 on: the moments are
// recomputed (36/16)^2 = 5x, nothing is accumulated across blocks -- no atomics, no second launch, the same bits every time.
//   dS/dx(q) = (G^T*a0)(q) + 2 x(q) (G^T*a2)(q) + y(q) (G^T*a4)(q)
// LDS: 2*36*37 + 5*36*27 + 3*26*27 + 3*26*17 + 16*17 floats = 44928 bytes of the 64 KB a workgroup may take; every row length is
// odd, so the column walks of the vertical passes and the row-strided walks of the horizontal ones spread over the 32 banks.
constexpr int SG_IN = SS_T + 2 * (SS_K - 1);   // 36
constexpr int SG_MAP = SS_IN;                  // 26

__global__ __launch_bounds__(256) void ssim_grad_kernel(const float* __restrict__ out, const float* __restrict__ tgt, float* __restrict__ dout,
                                                        SsimW w, float scale, float coef, int C, int H, int W, int f, int Ho, int Wo,
                                                        int prep) {
  __shared__ float xs[SG_IN][SG_IN + 1], ys[SG_IN][SG_IN + 1];
  __shared__ float hz[5][SG_IN][SG_MAP + 1];
  __shared__ float am[3][SG_MAP][SG_MAP + 1];
  __shared__ float ht[3][SG_MAP][SS_T + 1];
  __shared__ float res[SS_T][SS_T + 1];
  const int bc = blockIdx.z, c = bc % C;
  const float* ob = out + (size_t)bc * H * W;
  const float* tb = tgt + (size_t)bc * H * W;
  float* db = dout + (size_t)bc * H * W;
  const int qy0 = blockIdx.y * SS_T, qx0 = blockIdx.x * SS_T;       // first pooled pixel of the tile
  const int py0 = qy0 - (SS_K - 1), px0 = qx0 - (SS_K - 1);         // first map pixel that reaches it = first pooled pixel loaded
  ssim_load_window<SG_IN>(xs, ys, ob, tb, c, prep, py0, px0, H, W, f);
  __syncthreads();
  // horizontal pass: the five moments' row sums on 36 rows x 26 map columns
  for (int i = threadIdx.x; i < SG_IN * SG_MAP; i += 256) {
    const int r = i / SG_MAP, cc = i % SG_MAP;
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
  // vertical pass: the moments of 26x26 map pixels, then a0/a2/a4 there; zero outside the Ho x Wo map (image borders, ragged tiles)
  for (int i = threadIdx.x; i < SG_MAP * SG_MAP; i += 256) {
    const int r = i / SG_MAP, cc = i % SG_MAP;
    const int py = py0 + r, px = px0 + cc;
    float a0 = 0.f, a2 = 0.f, a4 = 0.f;
    if (py >= 0 && px >= 0 && py < Ho && px < Wo) {
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
      const float ld = mx * mx + my * my + c1, cd = sxx + syy + c2;
      const float l = (2.f * mx * my + c1) / ld, cs = (2.f * sxy + c2) / cd;
      a2 = -l * cs / cd;
      a4 = 2.f * l / cd;
      a0 = cs * (2.f * my - 2.f * mx * l) / ld - 2.f * mx * a2 - my * a4;
    }
    am[0][r][cc] = a0;
    am[1][r][cc] = a2;
    am[2][r][cc] = a4;
  }
  __syncthreads();
  // transposed horizontal pass: pooled column qx0 + j collects map columns qx0 + j - k, k = 0..10 (local index j + 10 - k)
  for (int i = threadIdx.x; i < SG_MAP * SS_T; i += 256) {
    const int r = i / SS_T, j = i % SS_T;
    float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < SS_K; ++k) {
      const float g = w.g[k];
#pragma unroll
      for (int m = 0; m < 3; ++m) t[m] = fmaf(g, am[m][r][j + (SS_K - 1) - k], t[m]);
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) ht[m][r][j] = t[m];
  }
  __syncthreads();
  // transposed vertical pass in registers, one pooled pixel per thread
  {
    const int i = threadIdx.x / SS_T, j = threadIdx.x % SS_T;
    float u[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < SS_K; ++k) {
      const float g = w.g[k];
#pragma unroll
      for (int m = 0; m < 3; ++m) u[m] = fmaf(g, ht[m][i + (SS_K - 1) - k][j], u[m]);
    }
    const float x = xs[i + SS_K - 1][j + SS_K - 1], y = ys[i + SS_K - 1][j + SS_K - 1];
    // coef = -1 / (B C Ho Wo f^2), halved on the prepared channel 0 = (v + 1) / 2; the caller's scale is the LAST factor, so a
    // power of two scales the bits exactly
    const float cf = prep && c == 0 ? 0.5f * coef : coef;
    res[i][j] = scale * (cf * (u[0] + 2.f * x * u[1] + y * u[2]));
  }
  __syncthreads();
  // write the output cells below the tile: every element, +0.0 where pooling dropped the pixel or clamp() cut channel 1 off
  const int Hd = H / f, Wd = W / f;
  const int oy0 = qy0 * f, ox0 = qx0 * f;
  const int oy1 = blockIdx.y == gridDim.y - 1 ? H : (qy0 + SS_T) * f, ox1 = blockIdx.x == gridDim.x - 1 ? W : (qx0 + SS_T) * f;
  const int wr = ox1 - ox0, n = (oy1 - oy0) * wr;
  const bool clamped = prep && c == 1;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int oy = oy0 + i / wr, ox = ox0 + i % wr;
    const int qy = oy / f, qx = ox / f;
    float v = 0.f;
    if (qy < Hd && qx < Wd) {
      v = res[qy - qy0][qx - qx0];
      if (clamped) {
        const float o = ob[(size_t)oy * W + ox];
        if (!(o >= 0.f && o <= 1.f)) v = 0.f;       // torch.clamp's backward: gradient on the bounds, none outside
      }
    }
    db[(size_t)oy * W + ox] = v;
  }
}

}  // namespace mau

using namespace mau;

extern "C" {

size_t mau_ssim_ws_elems(int B, int C, int H, int W) {
  const SsimGeometry g = ssim_geometry(H, W);
  return (size_t)B * C * g.tx * g.ty;
}

int mau_ssim_loss(const float* out, const float* tgt, double* ws, float* per_image, float* loss, int prep, int B, int C, int H, int W,
                  mau_stream_t stream) {
  MAU_REQUIRE(out && tgt && ws && per_image && loss && B > 0 && C > 0, "ssim_loss: bad arguments");
  const SsimGeometry g = ssim_geometry(H, W);
  MAU_REQUIRE(g.Ho > 0 && g.Wo > 0, "ssim_loss: image %dx%d is smaller than the 11x11 window after downsampling by %d", H, W, g.f);
  MAU_REQUIRE((int64_t)B * C <= 65535 && g.ty <= 65535, "ssim_loss: B*C and tile rows must fit a grid dimension");
  hipStream_t st = (hipStream_t)stream;
  MAU_LAUNCH(ssim_tiles_kernel, dim3(g.tx, g.ty, B * C), dim3(256), 0, st, out, tgt, ws, ssim_window(), C, H, W, g.f, g.Ho, g.Wo, g.tx, g.ty, prep);
  MAU_LAUNCH(ssim_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, per_image, loss, B, C, g.tx * g.ty, 1.0 / ((double)g.Ho * g.Wo));
  return check_launch("ssim_tiles_kernel");
}

int mau_ssim_loss_grad(const float* out, const float* tgt, float* dout, float scale, int prep, int B, int C, int H, int W,
                       mau_stream_t stream) {
  MAU_REQUIRE(out && tgt && dout && B > 0 && C > 0, "ssim_loss_grad: bad arguments");
  const SsimGeometry g = ssim_geometry(H, W);
  MAU_REQUIRE(g.Ho > 0 && g.Wo > 0, "ssim_loss_grad: image %dx%d is smaller than the 11x11 window after downsampling by %d", H, W, g.f);
  const int gx = ceil_div(W / g.f, SS_T), gy = ceil_div(H / g.f, SS_T);        // tiles of POOLED pixels, not of the map
  MAU_REQUIRE((int64_t)B * C <= 65535 && gy <= 65535, "ssim_loss_grad: B*C and tile rows must fit a grid dimension");
  const float coef = (float)(-1.0 / ((double)B * C * g.Ho * g.Wo * g.f * g.f));      // d(1 - mean) / dS, and the pooling's 1/f^2
  hipStream_t st = (hipStream_t)stream;
  MAU_LAUNCH(ssim_grad_kernel, dim3(gx, gy, B * C), dim3(256), 0, st, out, tgt, dout, ssim_window(), scale, coef, C, H, W, g.f, g.Ho, g.Wo,
             prep);
  return check_launch("ssim_grad_kernel");
}

}  // extern "C"
