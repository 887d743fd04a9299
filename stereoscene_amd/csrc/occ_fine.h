// Shared by the voxel-loss epilogues that work on the FINE (label) grid from the coarse logits without ever writing the
// up-sampled volume (occ_loss.hip, occ_extra.hip, lovasz.hip, ohem.hip, frustum.hip):
//   device  the x2 trilinear taps (align_corners=False), the logits of one fine voxel in registers (on the label grid or
//           up-sampled), the 20-way softmax with the fast __expf (softmax_inplace) and the max-subtracted exponentials with the
//           accurate expf (exp_inplace).  The two are different functions with different bits: each loss keeps its own.
//   host    workspace alignment, the capped one-thread-per-voxel grid, the common part of the dims checks and the tail of the
//           backward entry points (fine gradient, then ssbev_trilinear2x_bwd).
// The fixed-order folds of the partial sums (wave_sum, block_fold256) are in common.h.
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

// 20 consecutive floats (16-byte aligned) <-> registers
__device__ __forceinline__ void load20(const float* src, float* z) {
  const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
  for (int q = 0; q < NC / 4; ++q) {
    const float4 t = s4[q];
    z[4 * q + 0] = t.x; z[4 * q + 1] = t.y; z[4 * q + 2] = t.z; z[4 * q + 3] = t.w;
  }
}
__device__ __forceinline__ void store20(float* dst, const float* v) {
  float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
  for (int q = 0; q < NC / 4; ++q) d4[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
__device__ __forceinline__ void zero20(float* dst) {
  float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
  for (int q = 0; q < NC / 4; ++q) d4[q] = make_float4(0, 0, 0, 0);
}

// logits of voxel v of sample b -> z[NC].  UP: (D, H, W) is the coarse grid and v lives on [2D, 2H, 2W] (Ns = 8 D H W);
// otherwise the logits sit on the label grid.  int arithmetic: for the kernels that walk (sample, voxel).
template <bool UP>
__device__ __forceinline__ void fine_logits(const float* __restrict__ x, int b, int v, int Ns, int D, int H, int W, float* z) {
  if (UP) {
    int r = v;
    const int ow = r % (2 * W); r /= 2 * W;
    const int oh = r % (2 * H); r /= 2 * H;
    upsampled_logits(x, b, D, H, W, r, oh, ow, z);
  } else {
    load20(x + ((size_t)b * Ns + v) * NC, z);
  }
}

// the same for flat voxel i of the batch ([B, 2D, 2H, 2W] when UP): for the kernels that walk the batch in one long index
template <bool UP>
__device__ __forceinline__ void fine_logits_flat(const float* __restrict__ x, long i, int D, int H, int W, float* z) {
  if (UP) {
    long r = i;
    const int ow = (int)(r % (2 * W)); r /= 2 * W;
    const int oh = (int)(r % (2 * H)); r /= 2 * H;
    const int od = (int)(r % (2 * D));
    const int b = (int)(r / (2 * D));
    upsampled_logits(x, b, D, H, W, od, oh, ow, z);
  } else {
    load20(x + (size_t)i * NC, z);
  }
}

// z -> exp(z - max) in place with the ACCURATE expf; returns the sum, *mx the maximum
__device__ __forceinline__ float exp_inplace(float* z, float* mx) {
  float m = z[0];
#pragma unroll
  for (int c = 1; c < NC; ++c) m = z[c] > m ? z[c] : m;
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < NC; ++c) { z[c] = expf(z[c] - m); s += z[c]; }
  *mx = m;
  return s;
}

// 20-way softmax in place with the FAST __expf / __logf
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

// ---------------------------------------------------------------- host side of the entry points
size_t ws_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// one thread per voxel, grid-stride behind a cap
unsigned voxel_grid(long long n, int threads = 256, long long cap = 4096) {
  const long long b = (n + threads - 1) / threads;
  return (unsigned)(b < cap ? b : cap);
}

// what every dims struct with B, D, H, W, C, upsample must satisfy: positive sizes, 20 classes, 20 x fine voxels < 2^31
template <class Dims>
bool fine_dims_ok(const Dims* d) {
  if (!d || d->B <= 0 || d->D <= 0 || d->H <= 0 || d->W <= 0 || d->C != NC) return false;
  if (d->upsample != 0 && d->upsample != 1) return false;
  const long long n = (long long)d->B * d->D * d->H * d->W * (d->upsample ? 8 : 1);
  return n * NC < (1ll << 31);
}

// Tail of a backward entry point whose kernel has just written the gradient at the label resolution to gfine: on the label
// grid that was grad_logits itself; up-sampled, gfine is the workspace and the x2 pull-back to the coarse grid (B, D, H, W)
// follows.
int finish_fine_grad(const float* gfine, float* grad_logits, int B, int D, int H, int W, ssbev_stream_t stream) {
  if (gfine == grad_logits) return ssbev_launch_status();
  ssbev_upsample_dims u = {B, D, H, W, NC};
  const int rc = ssbev_trilinear2x_bwd(gfine, grad_logits, &u, stream);
  return rc != SSBEV_OK ? rc : ssbev_launch_status();
}

}  // namespace
