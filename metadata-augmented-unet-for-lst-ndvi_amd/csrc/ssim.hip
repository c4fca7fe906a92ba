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

}  // extern "C"
