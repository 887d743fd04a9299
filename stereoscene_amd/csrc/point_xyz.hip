// Lifted-point position encoder (point_xyz_channel of ViewTransformerLiftSplatShootVoxel, VT:432-476), fused per voxel.
//
// The reference runs Linear(3, M) -> BatchNorm1d(M) -> ReLU -> Linear(M, Cxyz) on one row per kept frustum point and pools the
// rows into the voxels.  Nothing here has a row per point:
//   * the batch statistics of h = W1 u + b1 follow from ten moments of the unit positions u (count, sum u, sum u u^T):
//     point_xyz_moments_kernel, one pass over geom + vox, double accumulation, fixed-order folds;
//   * the second Linear commutes with the voxel sum, so the kernels below produce S[v] = sum_{p in v} relu(gamma hhat_p + beta)
//     ([NV, M], channels-last) and the host multiplies S by W2 on the GEMM path;
//   * the backward pass re-walks the lists, recomputes the ReLU mask by the SAME expression (point_act) and reduces five sums per
//     channel (sum gz, sum gz hhat, sum gz u), from which the parameter gradients follow in closed form on the host.
// A point costs 12 bytes (geom) + 4 (order); a voxel 4 M bytes of S (forward) or gS (backward).
//
// Walk: a voxel is owned by Q = M / 4 neighbouring lanes (one float4 of channels each); they read the same order[] / geom entries
// (a broadcast) and add the points of the list in ascending order, sequentially in fp32.  Lists of more than 32 points come
// from the compacted long-voxel list of ssbev_pool_prepare2 in the forward pass: a wave per voxel, 64 / Q point slices, folded in
// slice order through LDS.  The backward pass needs an order of the CHANNEL sums that does not depend on the (atomically built,
// hence unordered) long list: every workgroup owns a contiguous voxel range and walks the long lists of that range itself.
//
// Built without FMA contraction (build.py): u is the reference's separately rounded (g - lo) / (hi - lo) - 0.5, times 2, and the
// pre-activation is the explicit fmaf chain of point_act in both directions, so the masks agree bit for bit.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int PXYZ_LONG = 32;          // = POOL_LONG of voxel_pool.hip: what ssbev_pool_prepare2 lists as long
constexpr int PXYZ_MAX_M = 256;
constexpr int PXYZ_MOM_BLOCKS = 512;   // workgroups of the moment pass (fixed: part of the fold order)
constexpr int PXYZ_BWD_BLOCKS = 1024;  // upper bound of the backward grid (fixed: part of the fold order)

struct Range {
  float lo[3], span[3];
};

__device__ __forceinline__ void unit_pos(const float* __restrict__ geom, long p, const Range& r, float (&u)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
    u[k] = __fmul_rn(__fsub_rn(__fdiv_rn(__fsub_rn(geom[3 * p + k], r.lo[k]), r.span[k]), 0.5f), 2.0f);
}

// Per-channel coefficients, [6][M]: c0..c2 = w_m / s_m, c3 = (b1_m - mu_m) / s_m, c4 = gamma_m, c5 = beta_m.
struct Coef4 {
  float4 c[6];
};
__device__ __forceinline__ Coef4 load_coef(const float* __restrict__ coef, int M, int q) {
  Coef4 k;
#pragma unroll
  for (int j = 0; j < 6; ++j) k.c[j] = ld4(coef + (size_t)j * M + 4 * q);
  return k;
}
__device__ __forceinline__ float hhat1(float c0, float c1, float c2, float c3, const float (&u)[3]) {
  return fmaf(c0, u[0], fmaf(c1, u[1], fmaf(c2, u[2], c3)));
}
// hhat and z = gamma hhat + beta of the lane's four channels: the one expression both directions evaluate.
__device__ __forceinline__ void point_act(const Coef4& k, const float (&u)[3], float (&hh)[4], float (&z)[4]) {
  hh[0] = hhat1(k.c[0].x, k.c[1].x, k.c[2].x, k.c[3].x, u);
  hh[1] = hhat1(k.c[0].y, k.c[1].y, k.c[2].y, k.c[3].y, u);
  hh[2] = hhat1(k.c[0].z, k.c[1].z, k.c[2].z, k.c[3].z, u);
  hh[3] = hhat1(k.c[0].w, k.c[1].w, k.c[2].w, k.c[3].w, u);
  z[0] = fmaf(k.c[4].x, hh[0], k.c[5].x);
  z[1] = fmaf(k.c[4].y, hh[1], k.c[5].y);
  z[2] = fmaf(k.c[4].z, hh[2], k.c[5].z);
  z[3] = fmaf(k.c[4].w, hh[3], k.c[5].w);
}

// ---------------------------------------------------------------- (a) moments
// partial[block][10]: n, sum u (3), sum u u^T (xx, xy, xz, yy, yz, zz) over the kept points of the block's strided share.
__global__ void __launch_bounds__(256)
point_xyz_moments_kernel(const float* __restrict__ geom, const int32_t* __restrict__ vox, long total, Range r,
                         double* __restrict__ partial) {
  __shared__ double red[10][256];
  const int tid = threadIdx.x;
  double a[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) a[j] = 0.0;
  for (long p = (long)blockIdx.x * 256 + tid; p < total; p += (long)gridDim.x * 256) {
    if (vox[p] < 0) continue;
    float uf[3];
    unit_pos(geom, p, r, uf);
    const double x = uf[0], y = uf[1], z = uf[2];
    a[0] += 1.0; a[1] += x; a[2] += y; a[3] += z;
    a[4] += x * x; a[5] += x * y; a[6] += x * z; a[7] += y * y; a[8] += y * z; a[9] += z * z;
  }
#pragma unroll
  for (int j = 0; j < 10; ++j) red[j][tid] = a[j];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int j = 0; j < 10; ++j) red[j][tid] += red[j][tid + off];
    }
    __syncthreads();
  }
  if (tid < 10) partial[(size_t)blockIdx.x * 10 + tid] = red[tid][0];
}

__global__ void __launch_bounds__(256) point_xyz_moments_fold_kernel(const double* __restrict__ partial, int n,
                                                                      double* __restrict__ moments) {
  double out[10];
  block_fold256<10>(partial, n, 10, out);
  if (threadIdx.x < 10) moments[threadIdx.x] = out[threadIdx.x];
}

// ---------------------------------------------------------------- (b) forward
// Lists of at most PXYZ_LONG points (all lists when there is no long list), and the zeros of the empty voxels.
__global__ void __launch_bounds__(256)
point_xyz_fwd_short_kernel(const float* __restrict__ geom, const int32_t* __restrict__ starts, const int32_t* __restrict__ order,
                           const float* __restrict__ coef, float* __restrict__ S, int nv, int M, long total, int skip_long,
                           Range r) {
  const int Q = M >> 2, vpb = 256 / Q;
  const int vs = threadIdx.x / Q, q = threadIdx.x - vs * Q;
  if (vs >= vpb) return;
  const long v = (long)blockIdx.x * vpb + vs;
  if (v >= nv) return;
  const int s = starts[v], e = starts[v + 1];
  if (skip_long && e - s > PXYZ_LONG) return;
  const Coef4 k = load_coef(coef, M, q);
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int i = s; i < e; ++i) {
    const long p = order[i];
    if ((unsigned long)p >= (unsigned long)total) continue;
    float u[3], hh[4], z[4];
    unit_pos(geom, p, r, u);
    point_act(k, u, hh, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = __fadd_rn(acc[c], fmaxf(z[c], 0.0f));
  }
  st4(S + (size_t)v * M + 4 * q, make_float4(acc[0], acc[1], acc[2], acc[3]));
}

// Long lists: a wave per listed voxel, lane = (slice, q); slice j adds points j, j + nsl, ... of the list in that order, lane
// (0, q) then adds the slices 0 .. nsl - 1 in order.
__global__ void __launch_bounds__(256)
point_xyz_fwd_long_kernel(const float* __restrict__ geom, const int32_t* __restrict__ starts, const int32_t* __restrict__ order,
                          const int32_t* __restrict__ long_list, const float* __restrict__ coef, float* __restrict__ S, int nv,
                          int M, long total, int list_cap, Range r) {
  __shared__ float part[4][64 * 4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int Q = M >> 2, nsl = 64 / Q;
  const int sl = lane / Q, q = lane - sl * Q;
  const bool active = sl < nsl;
  const int nlong = min(long_list[0], list_cap);
  Coef4 k;
  if (active) k = load_coef(coef, M, q);
  for (int i = blockIdx.x * 4 + w; i < nlong; i += gridDim.x * 4) {       // wave-uniform
    const int v = long_list[1 + i];
    if ((unsigned)v >= (unsigned)nv) continue;
    const int s = starts[v], e = starts[v + 1];
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (active) {
      for (int j = s + sl; j < e; j += nsl) {
        const long p = order[j];
        if ((unsigned long)p >= (unsigned long)total) continue;
        float u[3], hh[4], z[4];
        unit_pos(geom, p, r, u);
        point_act(k, u, hh, z);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = __fadd_rn(acc[c], fmaxf(z[c], 0.0f));
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) part[w][lane * 4 + c] = acc[c];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0): the wave's LDS writes have landed
    if (active && sl == 0) {
      float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int j = 0; j < nsl; ++j) {
#pragma unroll
        for (int c = 0; c < 4; ++c) t[c] = __fadd_rn(t[c], part[w][(j * Q + q) * 4 + c]);
      }
      st4(S + (size_t)v * M + 4 * q, make_float4(t[0], t[1], t[2], t[3]));
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);      // the reads are done before the next voxel overwrites part[w]
  }
}

// ---------------------------------------------------------------- (d) backward
// Workgroup b owns the voxels [b per, (b + 1) per).  Phase 1: slot (vs, q) walks the lists of at most PXYZ_LONG points of voxels
// vs, vs + vpb, ... of the range.  Phase 2: the workgroup visits the long lists of its range in voxel order; slot (vs, q) takes
// the points vs, vs + vpb, ... of each.  Every lane keeps 5 x 4 double sums; the slots are then folded in slot order and
// the workgroup writes partial[b][5][M].
__global__ void __launch_bounds__(256)
point_xyz_bwd_kernel(const float* __restrict__ geom, const int32_t* __restrict__ starts, const int32_t* __restrict__ order,
                     const float* __restrict__ coef, const float* __restrict__ gS, double* __restrict__ partial, int nv, int M,
                     long total, int per, Range r) {
  __shared__ double red[5 * 1024];          // [slot][5][M], slot < vpb, vpb M <= 1024
  const int Q = M >> 2, vpb = 256 / Q;
  const int vs = threadIdx.x / Q, q = threadIdx.x - vs * Q;
  const bool active = vs < vpb;
  const long v0 = (long)blockIdx.x * per, v1 = min((long)nv, v0 + per);
  double a[5][4];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) a[j][c] = 0.0;
  Coef4 k;
  if (active) k = load_coef(coef, M, q);

  auto add_point = [&](long p, const float (&g)[4]) {
    float u[3], hh[4], z[4];
    unit_pos(geom, p, r, u);
    point_act(k, u, hh, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double gz = z[c] > 0.0f ? (double)g[c] : 0.0;
      a[0][c] += gz;
      a[1][c] += gz * (double)hh[c];
      a[2][c] += gz * (double)u[0];
      a[3][c] += gz * (double)u[1];
      a[4][c] += gz * (double)u[2];
    }
  };

  if (active) {
    for (long v = v0 + vs; v < v1; v += vpb) {
      const int s = starts[v], e = starts[v + 1];
      if (e == s || e - s > PXYZ_LONG) continue;
      const float4 g4 = ld4(gS + (size_t)v * M + 4 * q);
      const float g[4] = {g4.x, g4.y, g4.z, g4.w};
      for (int i = s; i < e; ++i) {
        const long p = order[i];
        if ((unsigned long)p < (unsigned long)total) add_point(p, g);
      }
    }
    for (long v = v0; v < v1; ++v) {                 // workgroup-uniform scan of the range's list lengths
      const int s = starts[v], e = starts[v + 1];
      if (e - s <= PXYZ_LONG) continue;
      const float4 g4 = ld4(gS + (size_t)v * M + 4 * q);
      const float g[4] = {g4.x, g4.y, g4.z, g4.w};
      for (int i = s + vs; i < e; i += vpb) {
        const long p = order[i];
        if ((unsigned long)p < (unsigned long)total) add_point(p, g);
      }
    }
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) red[((size_t)vs * 5 + j) * M + 4 * q + c] = a[j][c];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 5 * M; idx += 256) {
    double t = 0.0;
    for (int sidx = 0; sidx < vpb; ++sidx) t += red[(size_t)sidx * 5 * M + idx];
    partial[(size_t)blockIdx.x * 5 * M + idx] = t;
  }
}

// sums[5][M] = the partials of the workgroups, added in workgroup order.
__global__ void __launch_bounds__(256) point_xyz_bwd_fold_kernel(const double* __restrict__ partial, int nblk, int n,
                                                                  double* __restrict__ sums) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  double t = 0.0;
  for (int b = 0; b < nblk; ++b) t += partial[(size_t)b * n + idx];
  sums[idx] = t;
}

bool dims_ok(const ssbev_point_xyz_dims* d) {
  if (!d || d->B < 1 || d->P < 1 || d->nx < 1 || d->ny < 1 || d->nz < 1) return false;
  if (d->M < 4 || d->M > PXYZ_MAX_M || d->M % 4) return false;
  if ((long long)d->B * d->P >= (1ll << 31) || (long long)d->B * d->nx * d->ny * d->nz >= (1ll << 31)) return false;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(d->lo[k]) || !std::isfinite(d->hi[k]) || !(d->hi[k] - d->lo[k] > 0.0f)) return false;
  return true;
}

Range range_of(const ssbev_point_xyz_dims* d) {
  Range r;
  for (int k = 0; k < 3; ++k) {
    r.lo[k] = d->lo[k];
    r.span[k] = d->hi[k] - d->lo[k];           // fp32, as the reference's tensor expression forms it
  }
  return r;
}

int bwd_per(int nv, int M) {                   // voxels per workgroup of the backward pass: a multiple of its slot count
  const int vpb = 256 / (M / 4);
  const int per = (int)(((long long)nv + PXYZ_BWD_BLOCKS - 1) / PXYZ_BWD_BLOCKS);
  return (per + vpb - 1) / vpb * vpb;
}

}  // namespace

extern "C" {

size_t ssbev_point_xyz_workspace(const ssbev_point_xyz_dims* d) {
  if (!dims_ok(d)) return 0;
  const int nv = d->B * d->nx * d->ny * d->nz;
  const size_t bwd = (size_t)cdiv((size_t)nv, (size_t)bwd_per(nv, d->M)) * 5 * d->M * sizeof(double);
  const size_t mom = (size_t)PXYZ_MOM_BLOCKS * 10 * sizeof(double);
  return bwd > mom ? bwd : mom;
}

int ssbev_point_xyz_moments(const float* geom, const int32_t* vox, double* moments, const ssbev_point_xyz_dims* d, void* ws,
                            size_t ws_bytes, ssbev_stream_t stream) {
  if (!dims_ok(d) || !geom || !vox || !moments || !ws) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_point_xyz_workspace(d)) return SSBEV_EWORKSPACE;
  const long total = (long)d->B * d->P;
  const int nblk = (int)std::min<long>(PXYZ_MOM_BLOCKS, (total + 255) / 256);
  double* partial = static_cast<double*>(ws);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(point_xyz_moments_kernel, dim3(nblk), dim3(256), 0, st, geom, vox, total, range_of(d), partial);
  hipLaunchKernelGGL(point_xyz_moments_fold_kernel, dim3(1), dim3(256), 0, st, partial, nblk, moments);
  return ssbev_launch_status();
}

int ssbev_point_xyz_fwd(const float* geom, const int32_t* starts, const int32_t* order, const int32_t* long_list,
                        const float* coef, float* S, const ssbev_point_xyz_dims* d, ssbev_stream_t stream) {
  if (!dims_ok(d) || !geom || !starts || !order || !coef || !S) return SSBEV_EINVAL;
  const int nv = d->B * d->nx * d->ny * d->nz, M = d->M;
  const long total = (long)d->B * d->P;
  const int vpb = 256 / (M / 4);
  hipStream_t st = as_stream(stream);
  const Range r = range_of(d);
  hipLaunchKernelGGL(point_xyz_fwd_short_kernel, dim3(cdiv((size_t)nv, (size_t)vpb)), dim3(256), 0, st, geom, starts, order, coef,
                     S, nv, M, total, long_list ? 1 : 0, r);
  if (long_list) {
    const int cap = (int)(total / (PXYZ_LONG + 1)) + 1;          // entries behind the count (ssbev_pool_long_list_elems - 1)
    const int grid = std::max(1, std::min(1024, (cap + 3) / 4));
    hipLaunchKernelGGL(point_xyz_fwd_long_kernel, dim3(grid), dim3(256), 0, st, geom, starts, order, long_list, coef, S, nv, M,
                       total, cap, r);
  }
  return ssbev_launch_status();
}

int ssbev_point_xyz_bwd(const float* geom, const int32_t* starts, const int32_t* order, const float* coef, const float* gS,
                        double* sums, const ssbev_point_xyz_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  if (!dims_ok(d) || !geom || !starts || !order || !coef || !gS || !sums || !ws) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_point_xyz_workspace(d)) return SSBEV_EWORKSPACE;
  const int nv = d->B * d->nx * d->ny * d->nz, M = d->M;
  const long total = (long)d->B * d->P;
  const int per = bwd_per(nv, M);
  const int nblk = (int)cdiv((size_t)nv, (size_t)per);
  double* partial = static_cast<double*>(ws);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(point_xyz_bwd_kernel, dim3(nblk), dim3(256), 0, st, geom, starts, order, coef, gS, partial, nv, M, total, per,
                     range_of(d));
  hipLaunchKernelGGL(point_xyz_bwd_fold_kernel, dim3(cdiv((size_t)5 * M, 256)), dim3(256), 0, st, partial, nblk, 5 * M, sums);
  return ssbev_launch_status();
}

}  // extern "C"
