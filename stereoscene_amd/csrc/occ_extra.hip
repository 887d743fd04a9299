// The two remaining voxel losses of the head (occhead.py:331-343), gfx950:
//
//   voxel_dice  SoftDiceLossWithProb (utils/dice_loss.py:36-66) of the occupied probability 1 - p_0 against [t > 0] over the
//               labelled voxels.  It is a function of four sums the fused epilogue (occ_loss.hip) already produces, so it needs
//               no pass over the logits: one scalar kernel gives the value and its Jacobian row over (ce_num, sum_p, nom), and
//               the gradient rides the coefficient vector of ssbev_occ_loss_bwd.
//   voxel_lga   PositionAwareLoss (utils/pal_loss.py): class-weighted cross entropy with the per-voxel factor alpha + beta * lga.
//               lga depends on the labels only and is a multiple of 0.5 in [0, 6]: ssbev_lga_weights writes 2 * lga as one byte
//               per voxel, exactly.  The loss pass has the shape of the fused epilogue: x2 trilinear taps from the coarse logits,
//               a 20-way softmax in registers, per-wave float sums folded in wave order into per-workgroup double partials and a
//               fixed-order fold.  No float atomics, nothing read back, the up-sampled volume is never written.
#include "common.h"
#include "occ_fine.h"     // NC, fine_logits_flat, softmax_inplace, the host helpers

namespace {

constexpr int LGA_BLOCKS = 2048;             // cap of the forward grid = rows of the partial table

// ---- Dice: sums = ce_num, ce_den, M, sum_p[NC], nom[NC], cnt[NC], ... (the layout of ssbev_occ_loss_fwd)
__global__ void __launch_bounds__(64)
occ_dice_tail_kernel(const double* __restrict__ sums, float smooth, float* __restrict__ out, double* __restrict__ jac) {
  constexpr int ND = 1 + 2 * NC;               // differentiable sums: ce_num, sum_p[NC], nom[NC]
  const int c = threadIdx.x;
  const double M = sums[2], sp0 = sums[3], nm0 = sums[3 + NC], ct0 = sums[3 + 2 * NC];
  const double occ_t = M - ct0;                // sum [t > 0]
  const double inter = occ_t - (sp0 - nm0);    // sum (1 - p_0) [t > 0]
  const double num = 2.0 * inter + (double)smooth;
  const double den = (M - sp0) + occ_t + (double)smooth;
  if (c < ND) {
    double j = 0.0;
    if (c == 1) j = (2.0 * den - num) / (den * den);       // d/d sum_p[0]: d num = -2, d den = -1
    if (c == 1 + NC) j = -2.0 / den;                        // d/d nom[0]:   d num = +2
    jac[c] = j;
  }
  if (c == 0) out[0] = (float)(1.0 - num / den);
}

// ---- LGA weights: one thread per voxel of [B, X, Y, Z]
__device__ __forceinline__ int lga_pair(int a, int b) {    // (is(a) + is(b)) [a != b]
  return a != b ? (a < NC) + (b < NC) : 0;
}
// contribution (x2) of one axis: position p of n (n >= 2), element stride s around index i
__device__ __forceinline__ int lga_axis(const uint8_t* __restrict__ t, long i, int p, int n, long s) {
  if (p == 0) return 2 * lga_pair(t[i], t[i + s]);
  if (p == n - 1) return 2 * lga_pair(t[i - s], t[i]);
  return lga_pair(t[i - s], t[i + s]);
}

__global__ void __launch_bounds__(256)
lga_weights_kernel(const uint8_t* __restrict__ label, uint8_t* __restrict__ lga2, int B, int X, int Y, int Z) {
  const long total = (long)B * X * Y * Z;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    long r = i;
    const int z = (int)(r % Z); r /= Z;
    const int y = (int)(r % Y); r /= Y;
    const int x = (int)(r % X);
    const int v = lga_axis(label, i, x, X, (long)Y * Z) + lga_axis(label, i, y, Y, Z) + lga_axis(label, i, z, Z, 1);
    lga2[i] = (uint8_t)v;
  }
}

// ---- LGA-weighted cross entropy, forward: partial[block] = (num, den)
__global__ void __launch_bounds__(256)
occ_lga_fwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ label, const uint8_t* __restrict__ lga2,
                   const float* __restrict__ cw, float alpha, float beta, double* __restrict__ partial, int B, int D, int H,
                   int W) {
  __shared__ float wred[4][2];                   // one slot per wave, folded in wave order (deterministic)
  const long total = (long)B * 8 * D * H * W;
  float num = 0.0f, den = 0.0f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = label[i];
    if (t >= NC) continue;                       // 255 = ignore
    float z[NC];
    fine_logits_flat<true>(x, i, D, H, W, z);
    float zt_raw = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) zt_raw = (c == t) ? z[c] : zt_raw;
    int am;
    const float lse = softmax_inplace(z, &am);
    const float w = cw[t];
    const float fac = alpha + beta * (0.5f * (float)lga2[i]);
    num += (w * (lse - zt_raw)) * fac;
    den += w;
  }
  num = wave_sum(num); den = wave_sum(den);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { wred[wave][0] = num; wred[wave][1] = den; }
  __syncthreads();
  if (threadIdx.x < 2)
    partial[(size_t)blockIdx.x * 2 + threadIdx.x] = (double)wred[0][threadIdx.x] + (double)wred[1][threadIdx.x] +
                                                    (double)wred[2][threadIdx.x] + (double)wred[3][threadIdx.x];
}

// numden = sums over the blocks in a fixed order; loss = num / den, 0 when nothing is labelled
__global__ void __launch_bounds__(256)
occ_lga_reduce_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ numden, float* __restrict__ loss) {
  double nd[2];
  block_fold256(partial, nblocks, 2, nd);
  if (threadIdx.x == 0) {
    numden[0] = nd[0]; numden[1] = nd[1];
    loss[0] = nd[1] > 0.0 ? (float)(nd[0] / nd[1]) : 0.0f;
  }
}

// One thread per FINE voxel writes gout / den * w[t] (alpha + beta lga) (p - onehot) (zero where ignored or den == 0); the x2
// pull-back to the coarse grid is ssbev_trilinear2x_bwd.
__global__ void __launch_bounds__(256)
occ_lga_bwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ label, const uint8_t* __restrict__ lga2,
                   const float* __restrict__ cw, float alpha, float beta, const double* __restrict__ numden,
                   const float* __restrict__ gout, float* __restrict__ gfine, int B, int D, int H, int W) {
  const double den = numden[1];
  const float scale = den > 0.0 ? (float)((double)gout[0] / den) : 0.0f;
  const long total = (long)B * 8 * D * H * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = label[i];
    float* dst = gfine + (size_t)i * NC;
    if (t >= NC || scale == 0.0f) {
      zero20(dst);
      continue;
    }
    float z[NC];
    fine_logits_flat<true>(x, i, D, H, W, z);
    int am;
    softmax_inplace(z, &am);
    const float k = scale * cw[t] * (alpha + beta * (0.5f * (float)lga2[i]));
    float g[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) g[c] = k * (z[c] - (c == t ? 1.0f : 0.0f));
    store20(dst, g);
  }
}

// fine voxels of refused dims: 0
long lga_fine(const ssbev_occloss_dims* d) {
  if (!d || d->B <= 0 || d->D <= 0 || d->H <= 0 || d->W <= 0 || d->C != NC) return 0;
  const double n = (double)d->B * 8.0 * d->D * d->H * d->W;
  return n * NC < 2147483648.0 ? (long)n : 0;
}

}  // namespace

extern "C" {

int ssbev_occ_dice_tail(const double* sums, float smooth, float* out1, double* jac41, ssbev_stream_t stream) {
  if (!sums || !out1 || !jac41) return SSBEV_EINVAL;
  hipLaunchKernelGGL(occ_dice_tail_kernel, dim3(1), dim3(64), 0, as_stream(stream), sums, smooth, out1, jac41);
  return ssbev_launch_status();
}

int ssbev_lga_weights(const uint8_t* label, uint8_t* lga2, int B, int X, int Y, int Z, ssbev_stream_t stream) {
  if (!label || !lga2 || B < 1 || X < 2 || Y < 2 || Z < 2) return SSBEV_EINVAL;
  const double n = (double)B * X * Y * Z;
  if (n >= 2147483648.0) return SSBEV_EINVAL;
  const long total = (long)n;
  hipLaunchKernelGGL(lga_weights_kernel, dim3((unsigned)min((long)cdiv(total, 256), 65535L)), dim3(256), 0, as_stream(stream),
                     label, lga2, B, X, Y, Z);
  return ssbev_launch_status();
}

size_t ssbev_occ_lga_workspace(const ssbev_occloss_dims* d) {
  return lga_fine(d) ? (size_t)LGA_BLOCKS * 2 * sizeof(double) : 0;
}

int ssbev_occ_lga_fwd(const float* logits, const uint8_t* label, const uint8_t* lga2, const float* class_weight, float alpha,
                      float beta, double* numden, float* loss, const ssbev_occloss_dims* d, void* ws, size_t ws_bytes,
                      ssbev_stream_t stream) {
  const long fine = lga_fine(d);
  if (!fine || !logits || !label || !lga2 || !class_weight || !numden || !loss || !ws) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_occ_lga_workspace(d)) return SSBEV_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  double* partial = static_cast<double*>(ws);
  const int nblocks = (int)min((long)cdiv(fine, 256), (long)LGA_BLOCKS);
  hipLaunchKernelGGL(occ_lga_fwd_kernel, dim3(nblocks), dim3(256), 0, st, logits, label, lga2, class_weight, alpha, beta,
                     partial, d->B, d->D, d->H, d->W);
  hipLaunchKernelGGL(occ_lga_reduce_kernel, dim3(1), dim3(256), 0, st, partial, nblocks, numden, loss);
  return ssbev_launch_status();
}

size_t ssbev_occ_lga_bwd_workspace(const ssbev_occloss_dims* d) {
  return (size_t)lga_fine(d) * NC * sizeof(float);
}

int ssbev_occ_lga_bwd(const float* logits, const uint8_t* label, const uint8_t* lga2, const float* class_weight, float alpha,
                      float beta, const double* numden, const float* grad_out, float* grad_logits,
                      const ssbev_occloss_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  const long fine = lga_fine(d);
  if (!fine || !logits || !label || !lga2 || !class_weight || !numden || !grad_out || !grad_logits || !ws) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_occ_lga_bwd_workspace(d)) return SSBEV_EWORKSPACE;
  float* gfine = static_cast<float*>(ws);
  hipLaunchKernelGGL(occ_lga_bwd_kernel, dim3((unsigned)min((long)cdiv(fine, 256), 4096L)), dim3(256), 0, as_stream(stream),
                     logits, label, lga2, class_weight, alpha, beta, numden, grad_out, gfine, d->B, d->D, d->H, d->W);
  return finish_fine_grad(gfine, grad_logits, d->B, d->D, d->H, d->W, stream);
}

}  // extern "C"
