// Point-level branch of the occupancy head (occhead.py:171-236 sample_point_feats + feature_sampling), gfx950.
//
// The reference samples every labelled LiDAR point trilinearly from the voxel feature maps and bilinearly from the image
// features (F.grid_sample, zero padding, align_corners=False).  Here:
//
//   forward   one wavefront per point for the whole batch and all levels: the lanes cover the channels in 16-byte pieces
//             over the 8 (4) corners of the channels-last maps.  Corners outside the map are skipped, never clamped.  The
//             source index is ATen's fp32 expression ((g + 1) * S - 1) / 2, the corner weights its differences and the
//             corners are added in its order, so the rows equal grid_sample's up to the rounding of the multiply-adds.
//             The same pass writes one (key, weight) pair per corner: key = destination cell of the gradient, -1 for a
//             corner that was skipped.
//   backward  the host sorts the keys into a CSR table (ssbev_pool_prepare2: a stable sort, invalid keys dropped); one
//             wavefront per cell adds weight * row gradient over the cell's list in list order and writes the cell, zeros
//             for an empty list.  Every element of the gradient is written exactly once: no memset, no float atomics, the
//             same bits on every run.
#include "common.h"

namespace {

constexpr int PH_LEVELS = 4;                   // voxel levels of one launch
constexpr int PH_WAVES = 4;                    // wavefronts (= points or cells) per workgroup

struct LevelArgs {
  const float* feat[PH_LEVELS];
  int X[PH_LEVELS], Y[PH_LEVELS], Z[PH_LEVELS];
  int base[PH_LEVELS + 1];                     // first key of the level: sum of B X Y Z over the levels before it
};

struct GradArgs {
  float* out[PH_LEVELS];
  int base[PH_LEVELS + 1];
};

__device__ __forceinline__ int sample_of(const int32_t* __restrict__ offs, int B, int n) {
  int b = 0;
  while (b + 1 < B && n >= offs[b + 1]) ++b;
  return b;
}

// ATen's grid_sampler_unnormalize for align_corners=False
__device__ __forceinline__ float unnormalize(float g, int size) { return ((g + 1.f) * (float)size - 1.f) / 2.f; }

__device__ __forceinline__ void fma4(float4& a, float w, const float4& v) {
  a.x += w * v.x; a.y += w * v.y; a.z += w * v.z; a.w += w * v.w;
}

// rows[(l N + n) C ..] (per_level) or rows[n C ..] (the sum over the levels, level 0 first); keys / wts [(l N + n) 8 + k]
__global__ void __launch_bounds__(64 * PH_WAVES)
point_sample_fwd_kernel(const float* __restrict__ pts, const int32_t* __restrict__ offs, LevelArgs a, float* __restrict__ rows,
                        int32_t* __restrict__ keys, float* __restrict__ wts, int B, int N, int C, int L, int axis_xyz,
                        int per_level) {
  const int lane = threadIdx.x & 63;
  const long nl = (long)blockIdx.x * PH_WAVES + (threadIdx.x >> 6);        // wave-uniform
  if (nl >= N) return;
  const int n = (int)nl;
  const int b = sample_of(offs, B, n);
  const float gx = pts[(size_t)n * 3], gy = pts[(size_t)n * 3 + 1], gz = pts[(size_t)n * 3 + 2];
  const int C4 = C >> 2;
  for (int l = 0; l < L; ++l) {
    const int X = a.X[l], Y = a.Y[l], Z = a.Z[l];
    // grid_sample's first grid coordinate walks the LAST axis: reference order hands it the point's x, "xyz" its z
    const float ix = unnormalize(axis_xyz ? gz : gx, Z), iy = unnormalize(gy, Y), iz = unnormalize(axis_xyz ? gx : gz, X);
    const bool inside = ix > -1.f && ix < (float)Z && iy > -1.f && iy < (float)Y && iz > -1.f && iz < (float)X;   // NaN: false
    const float fx = inside ? floorf(ix) : 0.f, fy = inside ? floorf(iy) : 0.f, fz = inside ? floorf(iz) : 0.f;
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const float wx[2] = {(fx + 1.f) - ix, ix - fx}, wy[2] = {(fy + 1.f) - iy, iy - fy}, wz[2] = {(fz + 1.f) - iz, iz - fz};
    long cell[8];
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int xi = x0 + (k & 1), yi = y0 + ((k >> 1) & 1), zi = z0 + (k >> 2);
      const bool ok = inside && xi >= 0 && xi < Z && yi >= 0 && yi < Y && zi >= 0 && zi < X;
      w[k] = wx[k & 1] * wy[(k >> 1) & 1] * wz[k >> 2];
      cell[k] = ok ? (((long)b * X + zi) * Y + yi) * Z + xi : -1;
    }
    if (lane < 8) {
      float wl = 0.f;
      long cl = -1;
#pragma unroll
      for (int k = 0; k < 8; ++k) if (lane == k) { wl = w[k]; cl = cell[k]; }
      const size_t at = ((size_t)l * N + n) * 8 + lane;
      keys[at] = cl >= 0 ? (int32_t)(a.base[l] + cl) : -1;
      wts[at] = wl;
    }
    const float* feat = a.feat[l];
    float* dst = rows + ((per_level ? (size_t)l * N : 0) + n) * C;
    for (int q = lane; q < C4; q += 64) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (cell[k] >= 0) fma4(acc, w[k], reinterpret_cast<const float4*>(feat + (size_t)cell[k] * C)[q]);
      float4* d4 = reinterpret_cast<float4*>(dst) + q;
      if (!per_level && l > 0) {                 // this lane wrote the piece at the level before
        const float4 o = *d4;
        acc.x = o.x + acc.x; acc.y = o.y + acc.y; acc.z = o.z + acc.z; acc.w = o.w + acc.w;
      }
      *d4 = acc;
    }
  }
}

// img [B, cams, H, W, C]; uv [N, cams, 3] = (u, v, depth); rows [N, C] = sum over the cameras with depth > 1e-5 and u, v strictly
// inside (-1, 1) of the bilinear sample; keys / wts [(n cams + cam) 4 + k], -1 for masked pairs and skipped corners
__global__ void __launch_bounds__(64 * PH_WAVES)
point_img_fwd_kernel(const float* __restrict__ img, const float* __restrict__ uv, const int32_t* __restrict__ offs,
                     float* __restrict__ rows, int32_t* __restrict__ keys, float* __restrict__ wts, int B, int N, int cams, int C,
                     int H, int W) {
  const int lane = threadIdx.x & 63;
  const long nl = (long)blockIdx.x * PH_WAVES + (threadIdx.x >> 6);
  if (nl >= N) return;
  const int n = (int)nl;
  const int b = sample_of(offs, B, n);
  const int C4 = C >> 2;
  for (int q0 = 0; q0 < C4; q0 += 64) {          // (wave-uniform trip count; the corner data is recomputed per 256 channels)
    const int q = q0 + lane;
    float4 total = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int cam = 0; cam < cams; ++cam) {
      const float* p = uv + ((size_t)n * cams + cam) * 3;
      const float u = p[0], v = p[1], dep = p[2];
      const bool keep = dep > 1e-5f && u > -1.f && u < 1.f && v > -1.f && v < 1.f;
      const float ix = unnormalize(u, W), iy = unnormalize(v, H);
      const float fx = keep ? floorf(ix) : 0.f, fy = keep ? floorf(iy) : 0.f;
      const int x0 = (int)fx, y0 = (int)fy;
      const float wx[2] = {(fx + 1.f) - ix, ix - fx}, wy[2] = {(fy + 1.f) - iy, iy - fy};
      long cell[4];
      float w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int xi = x0 + (k & 1), yi = y0 + (k >> 1);
        const bool ok = keep && xi >= 0 && xi < W && yi >= 0 && yi < H;
        w[k] = wx[k & 1] * wy[k >> 1];
        cell[k] = ok ? (((long)b * cams + cam) * H + yi) * W + xi : -1;
      }
      if (q0 == 0 && lane < 4) {
        float wl = 0.f;
        long cl = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (lane == k) { wl = w[k]; cl = cell[k]; }
        const size_t at = ((size_t)n * cams + cam) * 4 + lane;
        keys[at] = (int32_t)cl;
        wts[at] = wl;
      }
      if (q < C4) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (cell[k] >= 0) fma4(acc, w[k], reinterpret_cast<const float4*>(img + (size_t)cell[k] * C)[q]);
        total.x += acc.x; total.y += acc.y; total.z += acc.z; total.w += acc.w;
      }
    }
    if (q < C4) reinterpret_cast<float4*>(rows + (size_t)n * C)[q] = total;
  }
}

// cell v of the key space: out[v] = sum over its list, in list order, of wts[j] * grad[row(j)], row(j) = (j / kpp) % rowmod
__global__ void __launch_bounds__(64 * PH_WAVES)
point_cell_grad_kernel(const float* __restrict__ grad, const int32_t* __restrict__ starts, const int32_t* __restrict__ order,
                       const float* __restrict__ wts, GradArgs a, int nv, int nseg, int C, int kpp, int rowmod) {
  const int lane = threadIdx.x & 63;
  const long vl = (long)blockIdx.x * PH_WAVES + (threadIdx.x >> 6);
  if (vl >= nv) return;
  const int v = (int)vl;
  int s = 0;
  while (s + 1 < nseg && v >= a.base[s + 1]) ++s;
  float* dst = a.out[s] + (size_t)(v - a.base[s]) * C;
  const int e0 = starts[v], e1 = starts[v + 1];
  const int C4 = C >> 2;
  for (int q = lane; q < C4; q += 64) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = e0; e < e1; ++e) {
      const int j = order[e];
      fma4(acc, wts[j], reinterpret_cast<const float4*>(grad + (size_t)((j / kpp) % rowmod) * C)[q]);
    }
    reinterpret_cast<float4*>(dst)[q] = acc;
  }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// keys of a voxel launch (L 8 N), 0 for refused dims
long head_keys(const ssbev_point_head_dims* d) {
  if (!d || d->B <= 0 || d->N <= 0 || d->C <= 0 || d->C % 4 || d->L <= 0 || d->L > PH_LEVELS) return 0;
  if ((d->axis_xyz != 0 && d->axis_xyz != 1) || (d->per_level != 0 && d->per_level != 1)) return 0;
  long long cells = 0;
  for (int l = 0; l < d->L; ++l) {
    if (d->X[l] <= 0 || d->Y[l] <= 0 || d->Z[l] <= 0) return 0;
    cells += (long long)d->B * d->X[l] * d->Y[l] * d->Z[l];
    if (cells >= (1ll << 31)) return 0;
  }
  const long long nk = (long long)d->L * 8 * d->N;
  return nk < (1ll << 31) ? (long)nk : 0;
}

long img_keys(const ssbev_point_img_dims* d) {
  if (!d || d->B <= 0 || d->N <= 0 || d->cams <= 0 || d->C <= 0 || d->C % 4 || d->H <= 0 || d->W <= 0) return 0;
  if ((long long)d->B * d->cams * d->H * d->W >= (1ll << 31)) return 0;
  const long long nk = (long long)d->N * d->cams * 4;
  return nk < (1ll << 31) ? (long)nk : 0;
}

void level_bases(const ssbev_point_head_dims* d, int* base) {
  base[0] = 0;
  for (int l = 0; l < PH_LEVELS; ++l)
    base[l + 1] = base[l] + (l < d->L ? d->B * d->X[l] * d->Y[l] * d->Z[l] : 0);
}

}  // namespace

extern "C" {

// workspace = keys int32 [nk] | weights fp32 [nk], each part rounded up to 256 bytes
size_t ssbev_point_sample_workspace(const ssbev_point_head_dims* d) { return 2 * align256((size_t)head_keys(d) * 4); }
size_t ssbev_point_img_workspace(const ssbev_point_img_dims* d) { return 2 * align256((size_t)img_keys(d) * 4); }

int ssbev_point_sample_fwd(const float* points, const int32_t* offsets, const float* f0, const float* f1, const float* f2,
                           const float* f3, float* rows, const ssbev_point_head_dims* d, void* ws, size_t ws_bytes,
                           ssbev_stream_t stream) {
  const long nk = head_keys(d);
  if (!nk || !points || !offsets || !rows || !ws) return SSBEV_EINVAL;
  const float* f[PH_LEVELS] = {f0, f1, f2, f3};
  for (int l = 0; l < d->L; ++l) if (!f[l]) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_point_sample_workspace(d)) return SSBEV_EWORKSPACE;
  LevelArgs a;
  for (int l = 0; l < PH_LEVELS; ++l) {
    a.feat[l] = l < d->L ? f[l] : nullptr;
    a.X[l] = l < d->L ? d->X[l] : 1; a.Y[l] = l < d->L ? d->Y[l] : 1; a.Z[l] = l < d->L ? d->Z[l] : 1;
  }
  level_bases(d, a.base);
  int32_t* keys = static_cast<int32_t*>(ws);
  float* wts = reinterpret_cast<float*>(static_cast<char*>(ws) + align256((size_t)nk * 4));
  hipLaunchKernelGGL(point_sample_fwd_kernel, dim3(cdiv((size_t)d->N, PH_WAVES)), dim3(64 * PH_WAVES), 0, as_stream(stream),
                     points, offsets, a, rows, keys, wts, d->B, d->N, d->C, d->L, d->axis_xyz, d->per_level);
  return ssbev_launch_status();
}

int ssbev_point_sample_bwd(const float* grad_rows, const int32_t* starts, const int32_t* order, const void* ws, float* g0,
                           float* g1, float* g2, float* g3, const ssbev_point_head_dims* d, ssbev_stream_t stream) {
  const long nk = head_keys(d);
  if (!nk || !grad_rows || !starts || !order || !ws) return SSBEV_EINVAL;
  float* g[PH_LEVELS] = {g0, g1, g2, g3};
  for (int l = 0; l < d->L; ++l) if (!g[l]) return SSBEV_EINVAL;
  GradArgs a;
  for (int l = 0; l < PH_LEVELS; ++l) a.out[l] = l < d->L ? g[l] : nullptr;
  level_bases(d, a.base);
  const int nv = a.base[d->L];
  const float* wts = reinterpret_cast<const float*>(static_cast<const char*>(ws) + align256((size_t)nk * 4));
  hipLaunchKernelGGL(point_cell_grad_kernel, dim3(cdiv((size_t)nv, PH_WAVES)), dim3(64 * PH_WAVES), 0, as_stream(stream),
                     grad_rows, starts, order, wts, a, nv, d->L, d->C, 8, d->per_level ? d->L * d->N : d->N);
  return ssbev_launch_status();
}

int ssbev_point_img_fwd(const float* img, const float* uv, const int32_t* offsets, float* rows, const ssbev_point_img_dims* d,
                        void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  const long nk = img_keys(d);
  if (!nk || !img || !uv || !offsets || !rows || !ws) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_point_img_workspace(d)) return SSBEV_EWORKSPACE;
  int32_t* keys = static_cast<int32_t*>(ws);
  float* wts = reinterpret_cast<float*>(static_cast<char*>(ws) + align256((size_t)nk * 4));
  hipLaunchKernelGGL(point_img_fwd_kernel, dim3(cdiv((size_t)d->N, PH_WAVES)), dim3(64 * PH_WAVES), 0, as_stream(stream), img, uv,
                     offsets, rows, keys, wts, d->B, d->N, d->cams, d->C, d->H, d->W);
  return ssbev_launch_status();
}

int ssbev_point_img_bwd(const float* grad_rows, const int32_t* starts, const int32_t* order, const void* ws, float* grad_img,
                        const ssbev_point_img_dims* d, ssbev_stream_t stream) {
  const long nk = img_keys(d);
  if (!nk || !grad_rows || !starts || !order || !ws || !grad_img) return SSBEV_EINVAL;
  GradArgs a;
  for (int l = 0; l < PH_LEVELS; ++l) a.out[l] = l == 0 ? grad_img : nullptr;
  const int nv = d->B * d->cams * d->H * d->W;
  for (int l = 0; l <= PH_LEVELS; ++l) a.base[l] = l == 0 ? 0 : nv;
  const float* wts = reinterpret_cast<const float*>(static_cast<const char*>(ws) + align256((size_t)nk * 4));
  hipLaunchKernelGGL(point_cell_grad_kernel, dim3(cdiv((size_t)nv, PH_WAVES)), dim3(64 * PH_WAVES), 0, as_stream(stream),
                     grad_rows, starts, order, wts, a, nv, 1, d->C, 4 * d->cams, d->N);
  return ssbev_launch_status();
}

}  // extern "C"
