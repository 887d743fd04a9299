// Image-view segmentation loss of the view transformer (ViewTransformerLSSVoxel.py:418-430 get_seg_loss), gfx950.
//
// The reference up-samples the head's [BN, K, h, w] logits to the [BN, H, W] label map (F.interpolate, nearest) and runs a
// class-weighted cross entropy with ignore_index = 0 on [BN, K, H, W].  Every image pixel of a coarse cell reads that cell's
// logits, so the loss is a per-cell class histogram of the labels times ONE log-softmax per cell:
//
//   forward   one wavefront per cell: the cell's pixel rectangle from the index rule, the labels counted into K bins (lane c
//             keeps bin c; a ballot per class and pass, no LDS, no atomics), one max-subtracted log-sum-exp, (num, den) of the
//             cell in double; a one-workgroup launch folds the cells in a fixed order.
//   backward  one wavefront per cell from the saved counts: every element of the gradient is written exactly once.
//
// Nothing of size K x H x W exists, no float atomics, nothing read back.
#include "common.h"

namespace {

constexpr int MAXK = 32;                       // bins per cell in the workspace (K <= 32)
constexpr int CELLS_PER_BLOCK = 4;             // 256 threads = four wavefronts = four cells
constexpr double MAX_CELLS = 16777216.0;       // BN h w < 2^24

// torch's `nearest` source index of destination index i: min(floor(i * scale), n_in - 1), scale = (float)n_in / n_out.
__device__ __forceinline__ int nearest_src(int i, float scale, int n_in) {
  return min((int)floorf((float)i * scale), n_in - 1);
}

// Smallest destination index in [0, n_out] whose source index is >= c (n_out when there is none): the first row / column of
// cell c.  nearest_src is non-decreasing in i, so [first(c), first(c + 1)) are the cell's rows and the cells tile [0, n_out).
// The exact-ratio guess is corrected with the fp32 rule itself, one or two steps.
__device__ int first_at_least(int c, float scale, int n_in, int n_out) {
  if (c <= 0) return 0;
  if (c >= n_in) return n_out;
  int i = (int)min(((long)c * n_out + n_in - 1) / n_in, (long)n_out);
  while (i > 0 && nearest_src(i - 1, scale, n_in) >= c) --i;
  while (i < n_out && nearest_src(i, scale, n_in) < c) ++i;
  return i;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Lane c < K: logit c of the cell; returns exp(z - max) (0 on the other lanes), the maximum and the sum of the exponentials.
__device__ __forceinline__ float cell_softmax_terms(float z, bool live, float* zmax, float* esum) {
  const float m = wave_max(live ? z : -INFINITY);
  const float e = live ? expf(z - m) : 0.0f;
  *zmax = m;
  *esum = wave_sum(e);
  return e;
}

// partial[cell] = (num, den) in double, counts[cell][c] = valid pixels of class c (bin 0 stays 0)
__global__ void __launch_bounds__(64 * CELLS_PER_BLOCK)
imgseg_ce_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ labels, const float* __restrict__ cw,
                     double* __restrict__ partial, unsigned* __restrict__ counts, int BN, int K, int h, int w, int H, int W,
                     float s_h, float s_w) {
  const int lane = threadIdx.x & 63;
  const long cell = (long)blockIdx.x * CELLS_PER_BLOCK + (threadIdx.x >> 6);     // wave-uniform
  if (cell >= (long)BN * h * w) return;
  const int cx = (int)(cell % w), cy = (int)((cell / w) % h), bn = (int)(cell / ((long)w * h));
  const int y0 = first_at_least(cy, s_h, h, H), y1 = first_at_least(cy + 1, s_h, h, H);
  const int x0 = first_at_least(cx, s_w, w, W), x1 = first_at_least(cx + 1, s_w, w, W);
  const int rw = x1 - x0;
  const long npix = (long)(y1 - y0) * rw;
  const float* lab = labels + (size_t)bn * H * W;
  unsigned n = 0;                                                                  // lane c: pixels of class c
  for (long p0 = 0; p0 < npix; p0 += 64) {                                         // wave-uniform trip count
    const long p = p0 + lane;
    int l = 0;
    if (p < npix) {
      const float v = lab[(size_t)(y0 + (int)(p / rw)) * W + (x0 + (int)(p % rw))];
      if (v >= 1.0f && v < (float)K) l = (int)v;                                   // NaN, 0 and everything outside [1, K): ignored
    }
    if (__ballot(l != 0) == 0) continue;
    for (int c = 1; c < K; ++c) {
      const unsigned long long hit = __ballot(l == c);
      if (lane == c) n += (unsigned)__popcll(hit);
    }
  }
  const bool live = lane < K;
  const float z = live ? logits[(((size_t)bn * K + lane) * h + cy) * w + cx] : 0.0f;
  float m, esum;
  cell_softmax_terms(z, live, &m, &esum);
  const double nw = live ? (double)n * (double)cw[lane] : 0.0;
  const double nll = ((double)m - (double)z) + (double)logf(esum);                // lse - z_c
  const double num = wave_sum(nw * nll), den = wave_sum(nw);
  if (live) counts[(size_t)cell * MAXK + lane] = n;
  if (lane == 0) { partial[(size_t)cell * 2] = num; partial[(size_t)cell * 2 + 1] = den; }
}

// numden = the cells' partials folded in a fixed order; loss = weight * (num / den), 0 when nothing is labelled
__global__ void __launch_bounds__(256)
imgseg_ce_reduce_kernel(const double* __restrict__ partial, long cells, float weight, double* __restrict__ numden,
                        float* __restrict__ loss) {
  double nd[2];
  block_fold256(partial, cells, 2, nd);
  if (threadIdx.x == 0) {
    numden[0] = nd[0]; numden[1] = nd[1];
    loss[0] = nd[1] > 0.0 ? (float)((double)weight * (nd[0] / nd[1])) : 0.0f;
  }
}

// grad[c, cell] = gout * weight / den * (softmax_c * den_cell - n_c w_c); exact zeros for a cell without a valid pixel
__global__ void __launch_bounds__(64 * CELLS_PER_BLOCK)
imgseg_ce_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ cw, const float* __restrict__ gout,
                     const double* __restrict__ numden, const unsigned* __restrict__ counts, float* __restrict__ grad, int BN,
                     int K, int h, int w, float weight) {
  const int lane = threadIdx.x & 63;
  const long cell = (long)blockIdx.x * CELLS_PER_BLOCK + (threadIdx.x >> 6);
  if (cell >= (long)BN * h * w) return;
  const int cx = (int)(cell % w), cy = (int)((cell / w) % h), bn = (int)(cell / ((long)w * h));
  const double den = numden[1];
  const double scale = den > 0.0 ? (double)gout[0] * ((double)weight / den) : 0.0;
  const bool live = lane < K;
  const size_t at = (((size_t)bn * K + (live ? lane : 0)) * h + cy) * w + cx;
  const float z = live ? logits[at] : 0.0f;
  float m, esum;
  const float e = cell_softmax_terms(z, live, &m, &esum);
  const double nw = live ? (double)counts[(size_t)cell * MAXK + lane] * (double)cw[lane] : 0.0;
  const double den_cell = wave_sum(nw);
  if (live) grad[at] = den_cell != 0.0 ? (float)(scale * (((double)e / (double)esum) * den_cell - nw)) : 0.0f;
}

// cells of accepted dims, 0 for refused ones
long imgseg_cells(int BN, int h, int w) {
  if (BN <= 0 || h <= 0 || w <= 0) return 0;
  const double n = (double)BN * h * w;
  return n < MAX_CELLS ? (long)n : 0;
}

bool imgseg_dims_ok(int BN, int K, int h, int w, int H, int W) {
  return imgseg_cells(BN, h, w) && K >= 2 && K <= MAXK && H >= h && W >= w;
}

// workspace: (num, den) | (num, den) per cell | MAXK counts per cell
size_t imgseg_counts_offset(long cells) { return (size_t)(1 + cells) * 2 * sizeof(double); }

}  // namespace

extern "C" {

size_t ssbev_imgseg_ce_workspace(int BN, int h, int w) {
  const long cells = imgseg_cells(BN, h, w);
  return cells ? imgseg_counts_offset(cells) + (size_t)cells * MAXK * sizeof(unsigned) : 0;
}

int ssbev_imgseg_ce_fwd(const float* logits, const float* labels, const float* class_w, int BN, int K, int h, int w, int H, int W,
                        float weight, float* loss_out, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  if (!logits || !labels || !class_w || !loss_out || !ws || !imgseg_dims_ok(BN, K, h, w, H, W)) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_imgseg_ce_workspace(BN, h, w)) return SSBEV_EINVAL;
  const long cells = imgseg_cells(BN, h, w);
  hipStream_t st = as_stream(stream);
  double* numden = static_cast<double*>(ws);
  double* partial = numden + 2;
  unsigned* counts = reinterpret_cast<unsigned*>(static_cast<char*>(ws) + imgseg_counts_offset(cells));
  hipLaunchKernelGGL(imgseg_ce_fwd_kernel, dim3(cdiv(cells, CELLS_PER_BLOCK)), dim3(64 * CELLS_PER_BLOCK), 0, st, logits, labels,
                     class_w, partial, counts, BN, K, h, w, H, W, (float)h / (float)H, (float)w / (float)W);
  hipLaunchKernelGGL(imgseg_ce_reduce_kernel, dim3(1), dim3(256), 0, st, partial, cells, weight, numden, loss_out);
  return ssbev_launch_status();
}

int ssbev_imgseg_ce_bwd(const float* logits, const float* labels, const float* class_w, const float* grad_loss, int BN, int K,
                        int h, int w, int H, int W, float weight, float* grad_logits, const void* ws, ssbev_stream_t stream) {
  if (!logits || !labels || !class_w || !grad_loss || !grad_logits || !ws || !imgseg_dims_ok(BN, K, h, w, H, W))
    return SSBEV_EINVAL;
  const long cells = imgseg_cells(BN, h, w);
  const double* numden = static_cast<const double*>(ws);
  const unsigned* counts = reinterpret_cast<const unsigned*>(static_cast<const char*>(ws) + imgseg_counts_offset(cells));
  hipLaunchKernelGGL(imgseg_ce_bwd_kernel, dim3(cdiv(cells, CELLS_PER_BLOCK)), dim3(64 * CELLS_PER_BLOCK), 0, as_stream(stream),
                     logits, class_w, grad_loss, numden, counts, grad_logits, BN, K, h, w, weight);
  return ssbev_launch_status();
}

}  // extern "C"
