// scn_pixel.h -- one pixel of the network's input from raw planes, written once and shared by scenario_pack_kernel (scenario.hip)
// and region_gather_kernel (region.hip): the five continuous planes normalised in fp64 with IEEE division and rounded to float once
// (the reference's float64 numpy followed by .float(), app/processing_utils.py:136-139, :149), and the channel vector
// [one-hot a | rgb | ndvi | temp | one-hot b | zeros up to ld] as 16-byte channel-group stores, cast as pack_tile_onehot_kernel does.
#pragma once
#include "mau_common.h"

#pragma clang fp contract(off)

namespace mau {

constexpr int SCN_MAX_CLS = 16;
constexpr int SCN_NCONT = 5;             // rgb (3) + ndvi + temperature

// ps: the pixel's index in a plane of hw pixels; norm: rgb_mean[3], rgb_std[3], temp_mean, temp_std
__device__ __forceinline__ void scn_norm_planes(const float* __restrict__ rgb, const float* __restrict__ ndvi, const float* __restrict__ temp,
                                                const double* __restrict__ norm, size_t hw, size_t ps, float (&cv)[SCN_NCONT]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) cv[j] = (float)(((double)rgb[j * hw + ps] / 255.0 - norm[j]) / norm[3 + j]);
  cv[3] = ndvi[ps];
  cv[4] = (float)(((double)temp[ps] - norm[6]) / norm[7]);
}

// a, b: the two class ids (an id >= nc sets no channel); o: the pixel's ld channels, 16-byte aligned
template <typename T>
__device__ __forceinline__ void scn_store_pixel(T* __restrict__ o, int ld, int nc, int a, int b, const float (&cv)[SCN_NCONT]) {
  for (int g = 0; g < ld; g += 8) {
    F8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = g + j;
      float f = 0.f;
      if (c < nc) f = (a == c) ? 1.f : 0.f;
      else if (c < nc + SCN_NCONT) {
        const int k = c - nc;
        f = k == 0 ? cv[0] : k == 1 ? cv[1] : k == 2 ? cv[2] : k == 3 ? cv[3] : cv[4];
      } else if (c < 2 * nc + SCN_NCONT) f = (b == c - nc - SCN_NCONT) ? 1.f : 0.f;
      v.v[j] = f;
    }
    store8<T>(o + g, v);
  }
}

}  // namespace mau
