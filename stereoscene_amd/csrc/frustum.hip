// Frustum-proportion voxel loss (compute_frustum_dist_loss, utils/semkitti.py:218-244 of the reference) and the loader step that
// produces its inputs (CreateRelationLabels, datasets/pipelines/voxel_labels.py:65-265), gfx950.
//
// The reference takes a dense bool tensor [B, 64, X, Y, Z] (134 MB per sample at the KITTI grid), multiplies the whole softmax
// volume by one mask at a time and reads two scalars back per frustum.  The 64 masks of a sample are pairwise disjoint (a voxel
// centre projects into at most one half-open image patch), so one byte per voxel (the frustum id, 255 = none) holds the same
// information and ONE pass over the coarse logits yields all F x 20 sums.  Here:
//   accumulate  one thread per fine voxel, FR_TILE voxels per workgroup: skip id 255; up-sample (occ_fine.h); softmax with the
//               ACCURATE expf; per distinct id of the wave (ballot, broadcast of the first pending lane's id) a cross-lane sum of
//               the 20 probabilities, added in double to the wave's own row table in LDS (an id held by one lane alone adds its
//               probabilities directly).  The four wave tables are folded in a fixed order into the workgroup's partial table
//               [F][20] (double).  Which voxels a wave sees and in which order is a function of the dims alone.
//   fold        one workgroup per frustum: the partial tables of the batch in eight strided slices, then a fixed-order sum:
//               cum[f][c] (double).
//   final       one wave, one lane per frustum: counts pooled over the batch; a frustum counts if both totals are > 0; its term
//               is sum over t_c != 0 of t_c (log t_c - log q_c) in double; loss = sum of the terms / counted frusta (0 when none
//               counts); g[f][c] = d loss / d cum[f][c] = (1 / P_f - [t_c != 0] t_c / cum[f][c]) / counted for backward.
//   backward    per fine voxel: the row g[id] through the softmax Jacobian, p_k (g_k - sum_j g_j p_j), times the incoming scalar;
//               zeros for id 255.  The x2 case is written once at the fine resolution and pulled back by ssbev_trilinear2x_bwd.
//   labels      one thread per voxel: centre -> (x d, y d, d) by a 3x4 matrix, divide, 2x2 post-rotation + translation, the
//               half-open patch on both axes; id = py * frustum_size + px when d > 0 and the voxel is labelled; class counts per
//               frustum by integer atomics (LDS, then global): exact and order-free.
// No float atomics and no host read-back anywhere: every run gives the same bits.
#include "common.h"
#include "occ_fine.h"

namespace {

constexpr int FR_T = 256;                    // threads of a workgroup
constexpr int FR_WAVES = FR_T / 64;
constexpr int FR_ROWS = 32;                  // rows of FR_T voxels per workgroup
constexpr int FR_TILE = FR_T * FR_ROWS;
constexpr int FR_MAXF = 64;                  // frusta (frustum_size <= 8)
constexpr int FR_SLICES = 8;                 // strided slices of the fold
constexpr int FR_NONE = 255;

struct FrPlan {
  long long N;                               // fine voxels of the batch
  int Ns;                                    // fine voxels of a sample
  int nblk;                                  // workgroups (= partial tables) per sample
  size_t part, cum, bytes;
};

struct FrCam {                               // kernel argument of the label pass
  float o[3], s[3];                          // centre of voxel (0, 0, 0), voxel size
  float m[12];                               // centre -> (x d, y d, d)
  float pr[4], pt[2];                        // post-rotation (row-major 2x2), post-translation
  float ex[9], ey[9];                        // patch edges along the image width / height
  int fs;
};

bool fr_ok(const ssbev_frustum_dims* d) { return fine_dims_ok(d) && d->F >= 1 && d->F <= FR_MAXF; }

FrPlan fr_plan(const ssbev_frustum_dims* d) {
  FrPlan p;
  p.Ns = d->D * d->H * d->W * (d->upsample ? 8 : 1);
  p.N = (long long)d->B * p.Ns;
  p.nblk = (p.Ns + FR_TILE - 1) / FR_TILE;
  size_t o = 0;
  p.part = o;  o += ws_align256((size_t)d->B * p.nblk * d->F * NC * sizeof(double));
  p.cum = o;   o += ws_align256((size_t)d->F * NC * sizeof(double));
  p.bytes = o;
  return p;
}

// softmax of voxel v of sample b -> p[NC] (accurate expf; fine_logits: UP = the logits are on the coarse grid)
template <bool UP>
__device__ __forceinline__ void fr_softmax(const float* __restrict__ x, int b, int v, int Ns, int D, int H, int W, float* p) {
  fine_logits<UP>(x, b, v, Ns, D, H, W, p);
  float m;
  const float inv = 1.0f / exp_inplace(p, &m);
#pragma unroll
  for (int c = 0; c < NC; ++c) p[c] *= inv;
}

// ---------------------------------------------------------------- forward, pass 1: part[b * nblk + block][f][c]
template <bool UP>
__global__ void __launch_bounds__(FR_T)
frustum_accum_kernel(const float* __restrict__ x, const uint8_t* __restrict__ ids, double* __restrict__ part, int D, int H, int W,
                     int Ns, int F) {
  __shared__ double rows[FR_WAVES][FR_MAXF * NC];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < FR_WAVES * FR_MAXF * NC; i += FR_T) (&rows[0][0])[i] = 0.0;
  __syncthreads();
  double* my = rows[wave];
  const int base = blockIdx.x * FR_TILE;
  for (int j = 0; j < FR_ROWS; ++j) {
    if (base + j * FR_T >= Ns) break;            // (the same for the whole workgroup)
    const int v = base + j * FR_T + tid;
    int id = v < Ns ? (int)ids[(size_t)b * Ns + v] : FR_NONE;
    if (id >= F) id = FR_NONE;                   // 255, and anything that names no row of the table
    float p[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = 0.0f;
    if (id != FR_NONE) fr_softmax<UP>(x, b, v, Ns, D, H, W, p);
    unsigned long long todo = __ballot(id != FR_NONE);
    while (todo) {                               // one round per distinct id of the wave, lowest pending lane first
      const int leader = __ffsll((long long)todo) - 1;
      const int cur = __shfl(id, leader, 64);
      const bool mine = id == cur;
      const unsigned long long m = __ballot(mine);
      if (__popcll(m) == 1) {
        if (mine) {
#pragma unroll
          for (int c = 0; c < NC; ++c) my[cur * NC + c] += (double)p[c];
        }
      } else {
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float s = wave_sum(mine ? p[c] : 0.0f);
          acc = lane == c ? s : acc;
        }
        if (lane < NC) my[cur * NC + lane] += (double)acc;
      }
      todo &= ~m;
      // the next round may add to the same row from other lanes (a single holder writes all 20 entries, a group writes them from
      // lanes 0..19): keep the wave's LDS accesses of two rounds in program order
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  double* dst = part + ((size_t)b * gridDim.x + blockIdx.x) * F * NC;
  for (int i = tid; i < F * NC; i += FR_T) dst[i] = ((rows[0][i] + rows[1][i]) + rows[2][i]) + rows[3][i];
}

// ---------------------------------------------------------------- forward, pass 2a: cum[f][c] = sum of the partial tables
__global__ void __launch_bounds__(FR_T)
frustum_fold_kernel(const double* __restrict__ part, double* __restrict__ cum, int nparts, int F) {
  __shared__ double red[FR_SLICES][32];
  const int f = blockIdx.x, tid = threadIdx.x, c = tid & 31, s = tid >> 5;
  double a = 0.0;
  if (c < NC)
    for (int p = s; p < nparts; p += FR_SLICES) a += part[((size_t)p * F + f) * NC + c];
  red[s][c] = a;
  __syncthreads();
  if (tid < NC) {
    double t = red[0][tid];
#pragma unroll
    for (int k = 1; k < FR_SLICES; ++k) t += red[k][tid];
    cum[f * NC + tid] = t;
  }
}

// ---------------------------------------------------------------- forward, pass 2b: the loss and g = d loss / d cum
__global__ void __launch_bounds__(64)
frustum_final_kernel(const double* __restrict__ cum, const float* __restrict__ dists, float* __restrict__ loss,
                     float* __restrict__ g, int B, int F) {
  const int f = threadIdx.x;
  const bool in = f < F;
  double cnt[NC], cm[NC], tc = 0.0, tp = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double n = 0.0;
    if (in)
      for (int b = 0; b < B; ++b) n += (double)dists[((size_t)b * F + f) * NC + c];
    cnt[c] = n;
    cm[c] = in ? cum[f * NC + c] : 0.0;
    tc += n;
    tp += cm[c];
  }
  const bool counted = in && tp > 0.0 && tc > 0.0;
  double term = 0.0;
  if (counted) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (cnt[c] != 0.0) {
        const double t = cnt[c] / tc;
        term += t * (log(t) - log(cm[c] / tp));
      }
  }
  const int n = __popcll(__ballot(counted));
  const double sum = wave_sum(term);
  if (f == 0) loss[0] = n ? (float)(sum / (double)n) : 0.0f;
  if (in) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      double v = 0.0;
      if (counted) v = (1.0 / tp - (cnt[c] != 0.0 ? (cnt[c] / tc) / cm[c] : 0.0)) / (double)n;
      g[f * NC + c] = (float)v;
    }
  }
}

// ---------------------------------------------------------------- backward
template <bool UP>
__global__ void __launch_bounds__(FR_T)
frustum_bwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ ids, const float* __restrict__ g,
                   const float* __restrict__ grad_out, float* __restrict__ gdst, int D, int H, int W, int Ns, long N, int F) {
  __shared__ float gs[FR_MAXF * NC];             // grad_out * g
  for (int i = threadIdx.x; i < F * NC; i += FR_T) gs[i] = grad_out[0] * g[i];
  __syncthreads();
  for (long i = (long)blockIdx.x * FR_T + threadIdx.x; i < N; i += (long)gridDim.x * FR_T) {
    float* dst = gdst + (size_t)i * NC;
    const int id = ids[i];
    if (id >= F) {
      zero20(dst);
      continue;
    }
    float p[NC];
    fr_softmax<UP>(x, (int)(i / Ns), (int)(i % Ns), Ns, D, H, W, p);
    const float* row = gs + id * NC;
    float dot = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) dot += row[c] * p[c];
    float o[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] = p[c] * (row[c] - dot);
    store20(dst, o);
  }
}

// ---------------------------------------------------------------- the loader step: frustum id per voxel, class counts per frustum
__global__ void __launch_bounds__(FR_T)
frustum_labels_kernel(const uint8_t* __restrict__ labels, uint8_t* __restrict__ ids, int32_t* __restrict__ counts, int Y, int Z,
                      long N, FrCam cam) {
  __shared__ int cnt[FR_MAXF * NC];
  for (int i = threadIdx.x; i < FR_MAXF * NC; i += FR_T) cnt[i] = 0;
  __syncthreads();
  for (long v = (long)blockIdx.x * FR_T + threadIdx.x; v < N; v += (long)gridDim.x * FR_T) {
    const int iz = (int)(v % Z), iy = (int)((v / Z) % Y), ix = (int)(v / ((long)Z * Y));
    const float cx = cam.o[0] + (float)ix * cam.s[0], cy = cam.o[1] + (float)iy * cam.s[1], cz = cam.o[2] + (float)iz * cam.s[2];
    const float xd = cam.m[0] * cx + cam.m[1] * cy + cam.m[2] * cz + cam.m[3];
    const float yd = cam.m[4] * cx + cam.m[5] * cy + cam.m[6] * cz + cam.m[7];
    const float d = cam.m[8] * cx + cam.m[9] * cy + cam.m[10] * cz + cam.m[11];
    const float u0 = xd / d, v0 = yd / d;
    const float pu = cam.pr[0] * u0 + cam.pr[1] * v0 + cam.pt[0];
    const float pv = cam.pr[2] * u0 + cam.pr[3] * v0 + cam.pt[1];
    int px = -1, py = -1;
    for (int i = 0; i < cam.fs; ++i) {           // half-open patches; a NaN falls into none
      if (pu >= cam.ex[i] && pu < cam.ex[i + 1]) px = i;
      if (pv >= cam.ey[i] && pv < cam.ey[i + 1]) py = i;
    }
    const int lab = labels[v];
    int id = FR_NONE;
    if (px >= 0 && py >= 0 && d > 0.0f && lab < NC) {
      id = py * cam.fs + px;
      atomicAdd(&cnt[id * NC + lab], 1);
    }
    ids[v] = (uint8_t)id;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cam.fs * cam.fs * NC; i += FR_T) {
    const int c = cnt[i];
    if (c) atomicAdd(&counts[i], c);
  }
}

}  // namespace

extern "C" {

size_t ssbev_frustum_dist_workspace(const ssbev_frustum_dims* d) { return fr_ok(d) ? fr_plan(d).bytes : 0; }

int ssbev_frustum_dist_fwd(const float* logits, const uint8_t* ids, const float* dists, float* loss, float* g,
                           const ssbev_frustum_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  if (!fr_ok(d) || !logits || !ids || !dists || !loss || !g || !ws) return SSBEV_EINVAL;
  const FrPlan p = fr_plan(d);
  if (ws_bytes < p.bytes) return SSBEV_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  char* w = static_cast<char*>(ws);
  double* part = reinterpret_cast<double*>(w + p.part);
  double* cum = reinterpret_cast<double*>(w + p.cum);
  const dim3 grid(p.nblk, d->B);
  if (d->upsample)
    hipLaunchKernelGGL(frustum_accum_kernel<true>, grid, dim3(FR_T), 0, st, logits, ids, part, d->D, d->H, d->W, p.Ns, d->F);
  else
    hipLaunchKernelGGL(frustum_accum_kernel<false>, grid, dim3(FR_T), 0, st, logits, ids, part, d->D, d->H, d->W, p.Ns, d->F);
  hipLaunchKernelGGL(frustum_fold_kernel, dim3(d->F), dim3(FR_T), 0, st, part, cum, d->B * p.nblk, d->F);
  hipLaunchKernelGGL(frustum_final_kernel, dim3(1), dim3(64), 0, st, cum, dists, loss, g, d->B, d->F);
  return ssbev_launch_status();
}

size_t ssbev_frustum_dist_bwd_workspace(const ssbev_frustum_dims* d) {
  if (!fr_ok(d)) return 0;
  return d->upsample ? (size_t)fr_plan(d).N * NC * sizeof(float) : 0;
}

int ssbev_frustum_dist_bwd(const float* logits, const uint8_t* ids, const float* g, const float* grad_out, float* grad_logits,
                           const ssbev_frustum_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  if (!fr_ok(d) || !logits || !ids || !g || !grad_out || !grad_logits) return SSBEV_EINVAL;
  if (d->upsample && !ws) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_frustum_dist_bwd_workspace(d)) return SSBEV_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const FrPlan p = fr_plan(d);
  float* gfine = d->upsample ? static_cast<float*>(ws) : grad_logits;
  if (!d->upsample)
    hipLaunchKernelGGL(frustum_bwd_kernel<false>, dim3(voxel_grid(p.N)), dim3(FR_T), 0, st, logits, ids, g, grad_out, gfine, d->D,
                       d->H, d->W, p.Ns, (long)p.N, d->F);
  else
    hipLaunchKernelGGL(frustum_bwd_kernel<true>, dim3(voxel_grid(p.N)), dim3(FR_T), 0, st, logits, ids, g, grad_out, gfine, d->D,
                       d->H, d->W, p.Ns, (long)p.N, d->F);
  return finish_fine_grad(gfine, grad_logits, d->B, d->D, d->H, d->W, stream);
}

int ssbev_frustum_labels(const uint8_t* labels, uint8_t* ids, int32_t* counts, int X, int Y, int Z, const float* params,
                         int img_h, int img_w, int frustum_size, ssbev_stream_t stream) {
  if (!labels || !ids || !counts || !params) return SSBEV_EINVAL;
  if (X <= 0 || Y <= 0 || Z <= 0 || img_h <= 0 || img_w <= 0 || frustum_size < 1 || frustum_size > 8) return SSBEV_EINVAL;
  const long long n = (long long)X * Y * Z;
  if (n >= (1ll << 31)) return SSBEV_EINVAL;
  FrCam cam;
  for (int i = 0; i < 3; ++i) { cam.o[i] = params[i]; cam.s[i] = params[3 + i]; }
  for (int i = 0; i < 12; ++i) cam.m[i] = params[6 + i];
  for (int i = 0; i < 4; ++i) cam.pr[i] = params[18 + i];
  for (int i = 0; i < 2; ++i) cam.pt[i] = params[22 + i];
  for (int i = 0; i < 9; ++i) {                  // the reference's (i / frustum_size) * size in double, compared in fp32
    const int k = i <= frustum_size ? i : frustum_size;
    cam.ex[i] = (float)((double)k / (double)frustum_size * (double)img_w);
    cam.ey[i] = (float)((double)k / (double)frustum_size * (double)img_h);
  }
  cam.fs = frustum_size;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(counts, 0, (size_t)frustum_size * frustum_size * NC * sizeof(int32_t), st) != hipSuccess) return SSBEV_ELAUNCH;
  hipLaunchKernelGGL(frustum_labels_kernel, dim3(voxel_grid(n)), dim3(FR_T), 0, st, labels, ids, counts, Y, Z, (long)n, cam);
  return ssbev_launch_status();
}

}  // extern "C"
