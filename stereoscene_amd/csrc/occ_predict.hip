// Fused INFERENCE epilogue of the occupancy head (the twin of occ_loss.hip without the losses), gfx950:
//   trilinear x2 upsample of the coarse logits (align_corners=False) -> argmax over the 20 classes -> label volume,
//   raw SemanticKITTI ids and the per-sample 20x20 confusion counts, in ONE pass over the 21 MB of coarse logits.
// The reference (bevdepth_occupancy.py:293 -> semantic_kitti_lss_dataset.py:231-287 / apis/test.py:49-64) writes the 168 MB of
// up-sampled logits, reads them back for the argmax and runs ~15 tensor ops over the 2.1 M labels.
//
// Arithmetic per fine voxel is that of trilinear2x_fwd_kernel (trilinear.hip) / upsampled_logits (occ_loss.hip): the same eight
// taps in the same order (k = 4 d + 2 h + w), the same weight product (ld * lh) * lw, acc = fma(wt, v, acc) from zero.  What is shared
// is LOADS only: a thread owns four consecutive fine voxels along w, which reference coarse columns 2j-1 .. 2j+2 of four (d, h)
// rows -- 16 float4 per channel quad instead of 32 -- and it packs its four labels into one 32-bit store.
#include "common.h"

namespace {

constexpr int NC = 20;                       // classes
constexpr int NH = NC * NC + 1;              // conf[NC][NC] ([gt][pred]) + the ignored count
constexpr int MAX_BLOCKS = 2048;             // per sample (8 per CU at B = 1)

struct remap_table { uint16_t v[NC]; };

// source index / weights of PyTorch's area_pixel_compute_source_index for scale 1/2, align_corners=False (trilinear.hip)
__device__ __forceinline__ void src_taps2(int o, int in_size, int* i0, int* i1, float* l0, float* l1) {
  float s = 0.5f * ((float)o + 0.5f) - 0.5f;
  s = s < 0.0f ? 0.0f : s;
  const int a = (int)s;
  *i0 = a;
  *i1 = a + (a < in_size - 1 ? 1 : 0);
  *l1 = s - (float)a;
  *l0 = 1.0f - *l1;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (blocks per sample, B).  VEC: 2W % 4 == 0 and label / pred / raw are aligned for the packed accesses.
template <bool VEC>
__global__ void __launch_bounds__(256)
occ_predict_kernel(const float* __restrict__ x, const uint8_t* __restrict__ label, remap_table remap,
                   uint8_t* __restrict__ pred, uint16_t* __restrict__ raw, int* __restrict__ partial, int D, int H, int W) {
  __shared__ int hist[NH];
  if (partial) {
    for (int i = threadIdx.x; i < NH; i += 256) hist[i] = 0;
    __syncthreads();
  }
  const int b = blockIdx.y;
  const int W2 = 2 * W, NQ = (W2 + 3) >> 2;                       // quads of fine voxels per (od, oh) row
  const long nquads = (long)4 * D * H * NQ;
  const float* xb = x + (size_t)b * D * H * W * NC;
  const size_t fine0 = (size_t)b * 8 * D * H * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nquads; i += (long)gridDim.x * 256) {
    long r = i;
    const int j = (int)(r % NQ); r /= NQ;
    const int oh = (int)(r % (2 * H));
    const int od = (int)(r / (2 * H));
    const int nv = min(4, W2 - 4 * j);                            // 4, or 2 in the last quad of an odd W
    int d0, d1, h0, h1;
    float ld0, ld1, lh0, lh1;
    src_taps2(od, D, &d0, &d1, &ld0, &ld1);
    src_taps2(oh, H, &h0, &h1, &lh0, &lh1);
    // weights and (register) columns of the four voxels.  Columns held: t = 0..3 <-> coarse w = clamp(2j - 1 + t).  Voxel k's
    // taps are (2j-1, 2j), (2j, 2j+1), (2j, 2j+1), (2j+1, 2j+2) = columns (0,1), (1,2), (1,2), (2,3); the clamp reproduces
    // src_taps' upper edge, and at the lower edge (ow = 0: taps (0, min(1, W-1)), weights (1, 0)) voxel 0 takes column 2 as
    // its second tap.
    float lw0[4], lw1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int a0, a1;
      src_taps2(4 * j + k, W, &a0, &a1, &lw0[k], &lw1[k]);
    }
    const float wdh[4] = {ld0 * lh0, ld0 * lh1, ld1 * lh0, ld1 * lh1};       // (ld * lh), rows in tap order
    const float* row[4] = {xb + ((size_t)d0 * H + h0) * W * NC, xb + ((size_t)d0 * H + h1) * W * NC,
                           xb + ((size_t)d1 * H + h0) * W * NC, xb + ((size_t)d1 * H + h1) * W * NC};
    int coff[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) coff[t] = clampi(2 * j - 1 + t, 0, W - 1) * NC;
    const bool low_edge = j == 0;
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int am[4] = {0, 0, 0, 0};
    // one channel quad per trip, NOT unrolled: 64 registers of taps in flight instead of 320 (one wave per SIMD)
#pragma unroll 1
    for (int q = 0; q < NC / 4; ++q) {
      float4 v[4][4];                                             // [row][column]
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int t = 0; t < 4; ++t) v[rr][t] = *reinterpret_cast<const float4*>(row[rr] + coff[t] + 4 * q);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ta = k == 0 ? 0 : (k == 3 ? 2 : 1);
        float4 acc = make_float4(0, 0, 0, 0);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float4 va = v[rr][ta];
          float4 vb = v[rr][ta + 1];
          if (k == 0 && low_edge) vb = v[rr][2];
          const float wa = wdh[rr] * lw0[k], wb = wdh[rr] * lw1[k];
          // explicit fma: trilinear2x_fwd_kernel's `acc += wt * v` compiles to v_pk_fma_f32 for all eight taps, and contraction
          // is the compiler's choice per site (here it would split most of them into multiply + add)
          acc.x = __builtin_fmaf(wa, va.x, acc.x); acc.y = __builtin_fmaf(wa, va.y, acc.y);
          acc.z = __builtin_fmaf(wa, va.z, acc.z); acc.w = __builtin_fmaf(wa, va.w, acc.w);
          acc.x = __builtin_fmaf(wb, vb.x, acc.x); acc.y = __builtin_fmaf(wb, vb.y, acc.y);
          acc.z = __builtin_fmaf(wb, vb.z, acc.z); acc.w = __builtin_fmaf(wb, vb.w, acc.w);
        }
        // first maximum in class order (the z[c] > m scan of occ_loss.hip)
        if (q == 0 || acc.x > m[k]) { m[k] = acc.x; am[k] = 4 * q; }
        if (acc.y > m[k]) { m[k] = acc.y; am[k] = 4 * q + 1; }
        if (acc.z > m[k]) { m[k] = acc.z; am[k] = 4 * q + 2; }
        if (acc.w > m[k]) { m[k] = acc.w; am[k] = 4 * q + 3; }
      }
    }
    const size_t f = fine0 + ((size_t)od * 2 * H + oh) * W2 + 4 * j;         // first fine voxel of the quad
    if (pred) {
      if (VEC) *reinterpret_cast<uint32_t*>(pred + f) = (uint32_t)am[0] | ((uint32_t)am[1] << 8) | ((uint32_t)am[2] << 16) | ((uint32_t)am[3] << 24);
      else
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < nv) pred[f + k] = (uint8_t)am[k];
    }
    if (raw) {
      uint32_t rv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        rv[k] = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) rv[k] = am[k] == c ? (uint32_t)remap.v[c] : rv[k];
      }
      if (VEC) *reinterpret_cast<uint2*>(raw + f) = make_uint2(rv[0] | (rv[1] << 16), rv[2] | (rv[3] << 16));
      else
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < nv) raw[f + k] = (uint16_t)rv[k];
    }
    if (partial) {
      int key[4];                                                 // bin of voxel k: conf[t][am], NC * NC = ignored, -1 = no voxel
      if (VEC) {
        const uint32_t lab = *reinterpret_cast<const uint32_t*>(label + f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int t = (int)((lab >> (8 * k)) & 0xffu);
          key[k] = t < NC ? t * NC + am[k] : NC * NC;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int t = k < nv ? (int)label[f + k] : -1;
          key[k] = t < 0 ? -1 : (t < NC ? t * NC + am[k] : NC * NC);
        }
      }
      // equal bins of the quad go out as one LDS atomic (neighbouring voxels mostly agree: the empty class dominates)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        bool first = key[k] >= 0;
        int n = 1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (e < k && key[e] == key[k]) first = false;
          if (e > k && key[e] == key[k]) ++n;
        }
        if (first) atomicAdd(&hist[key[k]], n);
      }
    }
  }
  if (partial) {
    __syncthreads();
    int* out = partial + ((size_t)b * gridDim.x + blockIdx.x) * NH;
    for (int i = threadIdx.x; i < NH; i += 256) out[i] = hist[i];
  }
}

// conf[b][i] / n_ignored[b] = sum over the sample's blocks.  grid (ceil(NH / 64), B), 1024 threads: wave w adds blocks
// w, w + 16, ... of 64 consecutive bins (coalesced rows of the partials), the 16 waves are folded through LDS.  Integers: exact.
__global__ void __launch_bounds__(1024)
occ_predict_reduce_kernel(const int* __restrict__ partial, int nblocks, int64_t* __restrict__ conf,
                          int64_t* __restrict__ n_ignored) {
  __shared__ long long red[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane, b = blockIdx.y;
  long long a = 0;
  if (i < NH)
    for (int k = wave; k < nblocks; k += 16) a += partial[((size_t)b * nblocks + k) * NH + i];
  red[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && i < NH) {
#pragma unroll
    for (int w = 1; w < 16; ++w) a += red[w][lane];
    if (i < NC * NC) { if (conf) conf[(size_t)b * NC * NC + i] = a; }
    else if (n_ignored) n_ignored[b] = a;
  }
}

bool pred_ok(const ssbev_upsample_dims* d) {
  // one sample's fine voxels must fit the 32-bit per-block counters
  return d && d->B > 0 && d->D > 0 && d->H > 0 && d->W > 0 && d->C == NC && d->B <= 65535 &&
         (long long)8 * d->D * d->H * d->W < (1LL << 31);
}

int blocks_per_sample(const ssbev_upsample_dims* d) {
  const long long nquads = (long long)4 * d->D * d->H * ((2 * d->W + 3) / 4);
  const long long n = (nquads + 255) / 256;
  return (int)(n < MAX_BLOCKS ? n : MAX_BLOCKS);
}

}  // namespace

extern "C" {

size_t ssbev_occ_predict_workspace(const ssbev_upsample_dims* d) {
  return pred_ok(d) ? (size_t)d->B * blocks_per_sample(d) * NH * sizeof(int) : 0;
}

int ssbev_occ_predict(const float* logits, const uint8_t* label, const uint16_t* remap, uint8_t* pred, uint16_t* raw,
                      int64_t* conf, int64_t* n_ignored, const ssbev_upsample_dims* d, void* ws, size_t ws_bytes,
                      ssbev_stream_t stream) {
  const bool counts = conf || n_ignored;
  if (!pred_ok(d) || !logits || (!pred && !raw && !counts)) return SSBEV_EINVAL;
  if ((counts && !label) || (raw && !remap)) return SSBEV_EINVAL;
  if (counts && !ws) return SSBEV_EINVAL;
  if (counts && ws_bytes < ssbev_occ_predict_workspace(d)) return SSBEV_EWORKSPACE;
  remap_table tab = {};
  if (raw) for (int c = 0; c < NC; ++c) tab.v[c] = remap[c];
  hipStream_t st = as_stream(stream);
  const int nb = blocks_per_sample(d);
  int* partial = counts ? static_cast<int*>(ws) : nullptr;
  const uint8_t* lab = counts ? label : nullptr;
  const bool vec = (2 * d->W) % 4 == 0 && ((uintptr_t)lab & 3) == 0 && ((uintptr_t)pred & 3) == 0 && ((uintptr_t)raw & 7) == 0;
  if (vec)
    hipLaunchKernelGGL(occ_predict_kernel<true>, dim3(nb, d->B), dim3(256), 0, st, logits, lab, tab, pred, raw, partial, d->D,
                       d->H, d->W);
  else
    hipLaunchKernelGGL(occ_predict_kernel<false>, dim3(nb, d->B), dim3(256), 0, st, logits, lab, tab, pred, raw, partial, d->D,
                       d->H, d->W);
  if (counts)
    hipLaunchKernelGGL(occ_predict_reduce_kernel, dim3(cdiv(NH, 64), d->B), dim3(1024), 0, st, partial, nb, conf, n_ignored);
  return ssbev_launch_status();
}

}  // extern "C"
