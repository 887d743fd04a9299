// Input-side image operators (LoadMultiViewImageFromFiles_SemanticKitti, datasets/pipelines/
// loading_semkitti.py:76-302): Pillow's antialiased resize (`img.resize(resize_dims)`: bicubic, 8 bits per channel) and
// crop + flip + mmcv `imnormalize` + HWC -> CHW, on the GPU.  The resize is BYTE-EXACT with Pillow: the reference's
// pixels are whatever libImaging's fixed-point convolution produces (Resample.c: coefficients normalised in double,
// converted to 22-bit fixed point with round-half-away, accumulator seeded with 1 << 21, shifted and clamped to 0..255;
// horizontal pass to an 8-bit intermediate, then vertical), so the kernels consume the host-computed integer
// coefficient tables and do the same integer arithmetic.  Pure byte work, HBM-bound; one thread per output byte triple.
#include <cfloat>

#include "common.h"

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;

__device__ __forceinline__ unsigned char clip8(int v) {
  v >>= kPrecisionBits;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// dst[y][x][c] = clip8(half + sum_k src[y][xmin + k][c] * kk[x][k]),   src [H][Ws][C], dst [H][Wd][C]
__global__ void __launch_bounds__(256)
resample_h_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, const int* __restrict__ kk,
                  const int* __restrict__ bounds, int ksize, int H, int Ws, int Wd, int C) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * Wd) return;
  const int x = (int)(i % Wd), y = (int)(i / Wd);
  const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
  const int* k = kk + (long)x * ksize;
  const unsigned char* row = src + ((long)y * Ws + xmin) * C;
  for (int c = 0; c < C; ++c) {
    int ss = 1 << (kPrecisionBits - 1);
    for (int j = 0; j < n; ++j) ss += (int)row[j * C + c] * k[j];
    dst[i * C + c] = clip8(ss);
  }
}

// dst[y][x][c] = clip8(half + sum_k src[ymin + k][x][c] * kk[y][k]),   src [Hs][W][C], dst [Hd][W][C]
__global__ void __launch_bounds__(256)
resample_v_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, const int* __restrict__ kk,
                  const int* __restrict__ bounds, int ksize, int Hs, int Hd, int W, int C) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)Hd * W) return;
  const int x = (int)(i % W), y = (int)(i / W);
  const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
  const int* k = kk + (long)y * ksize;
  const unsigned char* col = src + ((long)ymin * W + x) * C;
  for (int c = 0; c < C; ++c) {
    int ss = 1 << (kPrecisionBits - 1);
    for (int j = 0; j < n; ++j) ss += (int)col[(long)j * W * C + c] * k[j];
    dst[i * C + c] = clip8(ss);
  }
}

struct NormParams { float mean[3], stdinv[3]; int x0, y0, flip, swap_rb; };

// out[c][y][x] = (src[y0 + y][x0 + (flip ? w - 1 - x : x)][swap ? 2 - c : c] - mean[c]) * stdinv[c]
__global__ void __launch_bounds__(256)
crop_normalize_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, NormParams p, int Hs, int Ws, int h, int w) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)h * w) return;
  const int x = (int)(i % w), y = (int)(i / w);
  const int sx = p.x0 + (p.flip ? w - 1 - x : x), sy = p.y0 + y;
  const bool in = sx >= 0 && sx < Ws && sy >= 0 && sy < Hs;            // PIL's crop pads with zeros outside the image
  const unsigned char* px = src + ((long)sy * Ws + sx) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = in ? (float)px[p.swap_rb ? 2 - c : c] : 0.0f;
    dst[(long)c * h * w + i] = (v - p.mean[c]) * p.stdinv[c];
  }
}

struct RotParams { NormParams n; long long a[6]; };

// Pillow's `img.rotate(angle)` (nearest, expand=False, black fill) of the cropped + flipped w x h image, fused with the crop /
// flip / normalise above: output (x, y) reads intermediate pixel (xi, yi) = ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16)
// (libImaging Geometry.c `affine_fixed`: 16.16 fixed point, arithmetic shift = floor); 0 outside [0,w) x [0,h) (rotate fill),
// then the same read and normalise as crop_normalize_kernel (0 outside the source = crop fill).
__global__ void __launch_bounds__(256)
crop_rotate_normalize_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, RotParams r, int Hs, int Ws, int h,
                             int w) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)h * w) return;
  const int x = (int)(i % w), y = (int)(i / w);
  const long long xx = r.a[2] + y * r.a[1] + x * r.a[0], yy = r.a[5] + y * r.a[4] + x * r.a[3];
  const long long xi = xx >> 16, yi = yy >> 16;
  const NormParams& p = r.n;
  bool in = xi >= 0 && xi < w && yi >= 0 && yi < h;
  const int sx = in ? p.x0 + (p.flip ? w - 1 - (int)xi : (int)xi) : 0, sy = in ? p.y0 + (int)yi : 0;
  in = in && sx >= 0 && sx < Ws && sy >= 0 && sy < Hs;
  const unsigned char* px = src + ((long)sy * Ws + sx) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = in ? (float)px[p.swap_rb ? 2 - c : c] : 0.0f;
    dst[(long)c * h * w + i] = (v - p.mean[c]) * p.stdinv[c];
  }
}

struct RotJitterParams { RotParams r; ssbev_jitter_params j; };

// PhotoMetricDistortionMultiViewImage (loading_bevdet.py:532-620) on one pixel, in the upstream's BGR order, steps 1-8 of
// include/ssbev.h.  numpy rounds every fp32 product and sum on its own, so nothing here may fuse into an FMA; the divisions are
// IEEE (hipcc's default).  The colour conversions restate OpenCV's scalar float path (cvtColor, float32, hrange 360):
// RGB2HSV_f's hue factor 60 / (diff + FLT_EPSILON) is a double quotient rounded to fp32, which equals the fp32 quotient (double
// has more than 2 * 24 + 2 bits, so the second rounding is innocuous), and its hscale 360 * (1.f / 360) is exactly 1.
__device__ __forceinline__ void photometric_bgr(float& b, float& g, float& r, const ssbev_jitter_params& j) {
#pragma clang fp contract(off)
  const bool contrast = (j.flags & SSBEV_JITTER_CONTRAST) != 0;
  if (j.flags & SSBEV_JITTER_BRIGHTNESS) { b = b + j.delta; g = g + j.delta; r = r + j.delta; }
  if (contrast && j.mode == 1) { b = b * j.alpha; g = g * j.alpha; r = r * j.alpha; }
  // BGR -> HSV
  float v = r, mn = r;
  if (v < g) v = g;
  if (v < b) v = b;
  if (mn > g) mn = g;
  if (mn > b) mn = b;
  const float diff = v - mn;
  float s = diff / (fabsf(v) + FLT_EPSILON);
  const float k = 60.0f / (diff + FLT_EPSILON);
  float hue = v == r ? (g - b) * k : (v == g ? (b - r) * k + 120.0f : (r - g) * k + 240.0f);
  if (hue < 0.0f) hue = hue + 360.0f;
  if (j.flags & SSBEV_JITTER_SATURATION) s = s * j.saturation;
  if (j.flags & SSBEV_JITTER_HUE) {
    hue = hue + j.hue;
    if (hue > 360.0f) hue = hue - 360.0f;                 // the upstream's two masked updates, in its order
    if (hue < 0.0f) hue = hue + 360.0f;
  }
  // HSV -> BGR.  |g - b| <= diff bounds the hue to (-60, 360) before the jitter, and |j.hue| <= 360 (host check) keeps it in
  // [0, 360] after the wrap: the loops below run at most once.
  if (s == 0.0f) {
    b = g = r = v;
  } else {
    float hh = hue * (6.0f / 360.0f);
    while (hh < 0.0f) hh = hh + 6.0f;
    while (hh >= 6.0f) hh = hh - 6.0f;
    int sector = (int)floorf(hh);
    hh = hh - (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; hh = 0.0f; }
    const float t1 = v * (1.0f - s), t2 = v * (1.0f - s * hh), t3 = v * (1.0f - s * (1.0f - hh));
    switch (sector) {                                      // OpenCV's sector_data {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}
      case 0: b = t1; g = t3; r = v; break;
      case 1: b = t1; g = v; r = t2; break;
      case 2: b = t3; g = v; r = t1; break;
      case 3: b = v; g = t2; r = t1; break;
      case 4: b = v; g = t1; r = t3; break;
      default: b = t2; g = t1; r = v; break;
    }
  }
  if (contrast && j.mode == 0) { b = b * j.alpha; g = g * j.alpha; r = r * j.alpha; }
  if (j.flags & SSBEV_JITTER_SWAP) {
    const float x[3] = {b, g, r};
    const int p0 = j.perm[0], p1 = j.perm[1], p2 = j.perm[2];
    b = p0 == 0 ? x[0] : (p0 == 1 ? x[1] : x[2]);
    g = p1 == 0 ? x[0] : (p1 == 1 ? x[1] : x[2]);
    r = p2 == 0 ? x[0] : (p2 == 1 ? x[1] : x[2]);
  }
}

// numpy's float32 -> uint8 on x86-64: truncate toward zero to int32, keep the low 8 bits (no clipping: -3.5 -> 253, 300.2 -> 44).
// |x| stays far below 2^31 for the host-checked parameter ranges.
__device__ __forceinline__ float wrap_u8(float x) { return (float)(unsigned char)(unsigned)(int)x; }

// crop_rotate_normalize_kernel's fetch (crop, flip and rotate fill read 0), then the colour jitter of the uint8 pixel, then the
// same normalise.  c0..c2 is the pixel in the order the normalise writes (RGB); the jitter sees it as BGR = (c2, c1, c0).
__global__ void __launch_bounds__(256)
crop_rotate_jitter_normalize_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, RotJitterParams q, int Hs,
                                    int Ws, int h, int w) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)h * w) return;
  const int x = (int)(i % w), y = (int)(i / w);
  const RotParams& rp = q.r;
  const long long xx = rp.a[2] + y * rp.a[1] + x * rp.a[0], yy = rp.a[5] + y * rp.a[4] + x * rp.a[3];
  const long long xi = xx >> 16, yi = yy >> 16;
  const NormParams& p = rp.n;
  bool in = xi >= 0 && xi < w && yi >= 0 && yi < h;
  const int sx = in ? p.x0 + (p.flip ? w - 1 - (int)xi : (int)xi) : 0, sy = in ? p.y0 + (int)yi : 0;
  in = in && sx >= 0 && sx < Ws && sy >= 0 && sy < Hs;
  const unsigned char* px = src + ((long)sy * Ws + sx) * 3;
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = in ? (float)px[p.swap_rb ? 2 - k : k] : 0.0f;
  float b = c[2], g = c[1], r = c[0];
  photometric_bgr(b, g, r, q.j);
  c[0] = wrap_u8(r); c[1] = wrap_u8(g); c[2] = wrap_u8(b);
#pragma unroll
  for (int k = 0; k < 3; ++k) dst[(long)k * h * w + i] = (c[k] - p.mean[k]) * p.stdinv[k];
}

}  // namespace

extern "C" {

int ssbev_resize_pil_u8(const uint8_t* src, int Hs, int Ws, int C, const int32_t* kk_h, const int32_t* bounds_h, int ksize_h,
                        const int32_t* kk_v, const int32_t* bounds_v, int ksize_v, uint8_t* tmp, uint8_t* dst, int Hd, int Wd,
                        ssbev_stream_t stream) {
  if (!src || !dst || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || C <= 0 || C > 4) return SSBEV_EINVAL;
  const bool need_h = Wd != Ws, need_v = Hd != Hs;
  if ((need_h && (!kk_h || !bounds_h || ksize_h <= 0)) || (need_v && (!kk_v || !bounds_v || ksize_v <= 0))) return SSBEV_EINVAL;
  if (need_h && need_v && !tmp) return SSBEV_EINVAL;
  hipStream_t st = as_stream(stream);
  const uint8_t* cur = src;
  if (need_h) {
    uint8_t* out = need_v ? tmp : dst;
    hipLaunchKernelGGL(resample_h_kernel, dim3(cdiv((size_t)Hs * Wd, 256)), dim3(256), 0, st, cur, out, kk_h, bounds_h, ksize_h,
                       Hs, Ws, Wd, C);
    cur = out;
  }
  if (need_v)
    hipLaunchKernelGGL(resample_v_kernel, dim3(cdiv((size_t)Hd * Wd, 256)), dim3(256), 0, st, cur, dst, kk_v, bounds_v, ksize_v,
                       Hs, Hd, Wd, C);
  if (!need_h && !need_v && hipMemcpyAsync(dst, src, (size_t)Hs * Ws * C, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return SSBEV_ELAUNCH;
  return ssbev_launch_status();
}

int ssbev_crop_normalize_u8(const uint8_t* src, int Hs, int Ws, float* dst, int x0, int y0, int w, int h, int flip,
                            const float* mean, const float* stdinv, int swap_rb, ssbev_stream_t stream) {
  if (!src || !dst || !mean || !stdinv || Hs <= 0 || Ws <= 0 || w <= 0 || h <= 0) return SSBEV_EINVAL;
  NormParams p;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean[c]; p.stdinv[c] = stdinv[c]; }       // host pointers (3 floats each)
  p.x0 = x0; p.y0 = y0; p.flip = flip ? 1 : 0; p.swap_rb = swap_rb ? 1 : 0;
  hipLaunchKernelGGL(crop_normalize_kernel, dim3(cdiv((size_t)h * w, 256)), dim3(256), 0, as_stream(stream), src, dst, p, Hs, Ws,
                     h, w);
  return ssbev_launch_status();
}

int ssbev_crop_rotate_normalize_u8(const uint8_t* src, int Hs, int Ws, float* dst, int x0, int y0, int w, int h, int flip,
                                   const int32_t* affine6, const float* mean, const float* stdinv, int swap_rb,
                                   ssbev_stream_t stream) {
  if (!src || !dst || !affine6 || !mean || !stdinv || Hs <= 0 || Ws <= 0 || w <= 0 || h <= 0) return SSBEV_EINVAL;
  RotParams r;
  for (int c = 0; c < 3; ++c) { r.n.mean[c] = mean[c]; r.n.stdinv[c] = stdinv[c]; }   // host pointers (3 floats each)
  for (int k = 0; k < 6; ++k) r.a[k] = affine6[k];                                       // host pointer (6 int32)
  r.n.x0 = x0; r.n.y0 = y0; r.n.flip = flip ? 1 : 0; r.n.swap_rb = swap_rb ? 1 : 0;
  hipLaunchKernelGGL(crop_rotate_normalize_kernel, dim3(cdiv((size_t)h * w, 256)), dim3(256), 0, as_stream(stream), src, dst, r,
                     Hs, Ws, h, w);
  return ssbev_launch_status();
}

int ssbev_crop_rotate_jitter_normalize_u8(const uint8_t* src, int Hs, int Ws, float* dst, int x0, int y0, int w, int h, int flip,
                                          const int32_t* affine6, const ssbev_jitter_params* jitter, const float* mean,
                                          const float* stdinv, int swap_rb, ssbev_stream_t stream) {
  if (!src || !dst || !affine6 || !jitter || !mean || !stdinv || Hs <= 0 || Ws <= 0 || w <= 0 || h <= 0) return SSBEV_EINVAL;
  const ssbev_jitter_params j = *jitter;                                                // host pointer
  const int known = SSBEV_JITTER_BRIGHTNESS | SSBEV_JITTER_CONTRAST | SSBEV_JITTER_SATURATION | SSBEV_JITTER_HUE |
                    SSBEV_JITTER_SWAP;
  if ((j.flags & ~known) != 0 || (j.mode != 0 && j.mode != 1)) return SSBEV_EINVAL;
  unsigned seen = 0;
  for (int k = 0; k < 3; ++k) {
    if (j.perm[k] < 0 || j.perm[k] > 2) return SSBEV_EINVAL;
    seen |= 1u << j.perm[k];
  }
  if (seen != 7u) return SSBEV_EINVAL;
  // ranges that keep every intermediate finite and far inside int32 (and the hue wrap to one turn); written so NaN fails
  if (!(fabsf(j.delta) <= 255.0f && j.alpha >= 0.0f && j.alpha <= 8.0f && j.saturation >= 0.0f && j.saturation <= 8.0f &&
        fabsf(j.hue) <= 360.0f))
    return SSBEV_EINVAL;
  RotJitterParams q;
  for (int c = 0; c < 3; ++c) { q.r.n.mean[c] = mean[c]; q.r.n.stdinv[c] = stdinv[c]; }   // host pointers (3 floats each)
  for (int k = 0; k < 6; ++k) q.r.a[k] = affine6[k];                                       // host pointer (6 int32)
  q.r.n.x0 = x0; q.r.n.y0 = y0; q.r.n.flip = flip ? 1 : 0; q.r.n.swap_rb = swap_rb ? 1 : 0;
  q.j = j;
  hipLaunchKernelGGL(crop_rotate_jitter_normalize_kernel, dim3(cdiv((size_t)h * w, 256)), dim3(256), 0, as_stream(stream), src,
                     dst, q, Hs, Ws, h, w);
  return ssbev_launch_status();
}

}  // extern "C"
