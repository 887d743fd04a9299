// Device functions shared by the loss epilogues that work on the FINE (label) grid from the coarse logits without ever
// writing the up-sampled volume (occ_loss.hip, lovasz.hip): the x2 trilinear taps (align_corners=False), the up-sampled
// logits of one fine voxel and the 20-way softmax in registers.
#pragma once
#include "common.h"

namespace {

constexpr int NC = 20;                       // classes (asserted by the host wrappers)

__device__ __forceinline__ void src_taps2(int o, int in_size, int* i0, int* i1, float* l0, float* l1) {
  float s = 0.5f * ((float)o + 0.5f) - 0.5f;
  s = s < 0.0f ? 0.0f : s;
  const int a = (int)s;
  *i0 = a;
  *i1 = a + (a < in_size - 1 ? 1 : 0);
  *l1 = s - (float)a;
  *l0 = 1.0f - *l1;
}

// up-sampled logits of fine voxel (od, oh, ow) -> z[NC]
__device__ __forceinline__ void upsampled_logits(const float* __restrict__ x, int b, int D, int H, int W, int od, int oh,
                                                 int ow, float* z) {
  int d0, d1, h0, h1, w0, w1;
  float ld0, ld1, lh0, lh1, lw0, lw1;
  src_taps2(od, D, &d0, &d1, &ld0, &ld1);
  src_taps2(oh, H, &h0, &h1, &lh0, &lh1);
  src_taps2(ow, W, &w0, &w1, &lw0, &lw1);
#pragma unroll
  for (int c = 0; c < NC; ++c) z[c] = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dd = (k & 4) ? d1 : d0, hh = (k & 2) ? h1 : h0, ww = (k & 1) ? w1 : w0;
    const float wt = ((k & 4) ? ld1 : ld0) * ((k & 2) ? lh1 : lh0) * ((k & 1) ? lw1 : lw0);
    const float4* src = reinterpret_cast<const float4*>(x + ((((size_t)b * D + dd) * H + hh) * W + ww) * NC);
#pragma unroll
    for (int q = 0; q < NC / 4; ++q) {
      const float4 v = src[q];
      z[4 * q + 0] += wt * v.x; z[4 * q + 1] += wt * v.y; z[4 * q + 2] += wt * v.z; z[4 * q + 3] += wt * v.w;
    }
  }
}

__device__ __forceinline__ float softmax_inplace(float* z, int* amax) {
  float m = z[0];
  int am = 0;
#pragma unroll
  for (int c = 1; c < NC; ++c) if (z[c] > m) { m = z[c]; am = c; }
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) { z[c] = __expf(z[c] - m); s += z[c]; }
  const float inv = 1.0f / s;
#pragma unroll
  for (int c = 0; c < NC; ++c) z[c] *= inv;
  *amax = am;
  return m + __logf(s);     // logsumexp (of the raw logits)
}

}  // namespace
