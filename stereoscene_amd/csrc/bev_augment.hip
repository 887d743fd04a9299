// BEV augmentation of the voxel labels (loading_semkitti.py:304-356 bev_transform): scipy.ndimage.rotate(order=0,
// mode='constant', reshape=False) over every (X, Y) plane of a uint8 [X,Y,Z] grid, then the two flips, widened to int64.
//
// Three steps, all over the X*Y raster of one plane (the source map does not depend on z):
//   1. source map: output p = i*Y + j reads source (floor(ci + 0.5), floor(cj + 0.5)) or the fill value, scipy's rule, in IEEE
//      double with every product and sum rounded on its own (this file is built with -ffp-contract=off as well);
//   2. chain resolution, only for the upstream's IN-PLACE rotation (rotate(lab, output=lab)): scipy walks a plane in raster order
//      and does not guard against the aliasing, so an output whose source index m[p] is below p reads what was WRITTEN there:
//      out[p] = out[m[p]].  The chains are collapsed by pointer jumping, ceil(log2(X*Y)) rounds between two tables;
//   3. gather: a Z column is contiguous, so the column of source voxel q moves as one piece to the (flipped) place of p.
//
// Table entries (int32): v >= 0 "same as entry v" (only before resolution, always v < p); v == -1 the fill value;
// v <= -2 source column -2 - v.
#include <math.h>

#include "common.h"

namespace {

constexpr int kFill = -1;
__host__ __device__ constexpr int src_code(int q) { return -2 - q; }

struct BevMap { double m00, m01, m10, m11, off0, off1; };

// inplace != 0: an entry whose source lies before it in raster order points at that entry (it was overwritten before it is read)
__global__ void bev_source_map_kernel(int* __restrict__ table, BevMap c, int X, int Y, int inplace) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (unsigned)(X * Y)) return;
  const int p = (int)t;
  const double i = (double)(p / Y), j = (double)(p % Y);
  const double ci = __dadd_rn(__dadd_rn(__dmul_rn(c.m00, i), __dmul_rn(c.m01, j)), c.off0);
  const double cj = __dadd_rn(__dadd_rn(__dmul_rn(c.m10, i), __dmul_rn(c.m11, j)), c.off1);
  int v = kFill;
  if (ci >= 0.0 && ci <= (double)(X - 1) && cj >= 0.0 && cj <= (double)(Y - 1)) {       // (false for NaN)
    const int q = (int)floor(__dadd_rn(ci, 0.5)) * Y + (int)floor(__dadd_rn(cj, 0.5));
    v = (inplace && q < p) ? q : src_code(q);
  }
  table[p] = v;
}

// One round of pointer jumping: an unresolved entry takes what the entry it points at holds (a resolved code, or a pointer
// twice as far down the chain).  a and b are distinct tables, so a round reads nothing it writes.
__global__ void bev_chain_jump_kernel(const int* __restrict__ a, int* __restrict__ b, int n) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (unsigned)n) return;
  const int v = a[p];
  b[p] = v >= 0 ? a[v] : v;
}

template <int V> struct Bytes;
template <> struct Bytes<1> { typedef uint8_t type; };
template <> struct Bytes<4> { typedef uint32_t type; };
template <> struct Bytes<8> { typedef uint64_t type; };

template <int V>
__device__ __forceinline__ void store_labels(uint8_t* dst, size_t at, typename Bytes<V>::type w) {
  *reinterpret_cast<typename Bytes<V>::type*>(dst + at) = w;
}
template <int V>
__device__ __forceinline__ void store_labels(int64_t* dst, size_t at, typename Bytes<V>::type w) {
  if constexpr (V == 1) {
    dst[at] = (int64_t)w;
  } else {
#pragma unroll
    for (int k = 0; k < V; k += 2)
      *reinterpret_cast<longlong2*>(dst + at + k) = make_longlong2((long long)((w >> (8 * k)) & 0xff), (long long)((w >> (8 * k + 8)) & 0xff));
  }
}

// One thread moves V consecutive z of one column (V divides Z; V > 1 needs src aligned to V and an int64 dst to 16 bytes).
// table == nullptr: no rotation, column p reads column p.
template <int V, typename Out>
__global__ void bev_gather_kernel(const uint8_t* __restrict__ src, Out* __restrict__ dst, const int* __restrict__ table, int X,
                                  int Y, int Z, int flip_dx, int flip_dy, int fill) {
  typedef typename Bytes<V>::type W;
  const int per_col = Z / V;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)X * Y * per_col) return;
  const int p = (int)(t / per_col), k = (int)(t % per_col) * V;
  const int code = table ? table[p] : src_code(p);
  W w;
  if (code == kFill) {
    w = (W)((W)fill * (W)((W)~(W)0 / 0xff));          // the byte in every lane of the word
  } else {
    w = *reinterpret_cast<const W*>(src + (size_t)(-2 - code) * Z + k);
  }
  const int i = p / Y, j = p % Y;
  const int oi = flip_dx ? X - 1 - i : i, oj = flip_dy ? Y - 1 - j : j;
  store_labels<V>(dst, ((size_t)oi * Y + oj) * Z + k, w);
}

int chain_rounds(int n) {
  int r = 0;
  while (((int64_t)1 << r) < n) ++r;      // ceil(log2(n)): a chain has fewer than n links, and each round halves what is left
  return r;
}

bool dims_ok(int X, int Y, int Z) { return X >= 1 && Y >= 1 && Z >= 1 && (int64_t)X * Y <= (int64_t)INT32_MAX - 2; }

template <typename Out>
int bev_label_transform(const uint8_t* src, Out* dst, int X, int Y, int Z, const double* coeffs6, int inplace, int flip_dx,
                        int flip_dy, int fill, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  if (!src || !dst || !dims_ok(X, Y, Z) || fill < 0 || fill > 255) return SSBEV_EINVAL;
  const size_t total = (size_t)X * Y * Z;
  if ((total + 255) / 256 > (size_t)INT32_MAX) return SSBEV_EINVAL;                    // one launch: the grid's x extent
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  if (s0 < d0 + total * sizeof(Out) && d0 < s0 + total) return SSBEV_EINVAL;           // the gather is not an in-place pass
  BevMap c = {};
  if (coeffs6) {
    for (int k = 0; k < 6; ++k)
      if (!isfinite(coeffs6[k])) return SSBEV_EINVAL;                                  // host pointer (6 doubles)
    c = BevMap{coeffs6[0], coeffs6[1], coeffs6[2], coeffs6[3], coeffs6[4], coeffs6[5]};
    if (!ws) return SSBEV_EINVAL;
    if (ws_bytes < ssbev_bev_label_workspace(X, Y, 1, inplace)) return SSBEV_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int n = X * Y;
  const int* table = nullptr;
  if (coeffs6) {
    int* a = static_cast<int*>(ws);
    int* b = a + n;
    hipLaunchKernelGGL(bev_source_map_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a, c, X, Y, inplace ? 1 : 0);
    if (inplace) {
      for (int r = chain_rounds(n); r > 0; --r) {
        hipLaunchKernelGGL(bev_chain_jump_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a, b, n);
        int* t = a; a = b; b = t;
      }
    }
    table = a;
  }
  const bool wide_dst = sizeof(Out) == 1 ? true : ((uintptr_t)dst % 16 == 0);
  const int al = (int)(((uintptr_t)src | (sizeof(Out) == 1 ? (uintptr_t)dst : 0)) % 8);
  const int V = (wide_dst && Z % 8 == 0 && al == 0) ? 8 : (wide_dst && Z % 4 == 0 && al % 4 == 0) ? 4 : 1;
  const dim3 grid(cdiv((size_t)n * (Z / V), 256)), block(256);
  const int fx = flip_dx ? 1 : 0, fy = flip_dy ? 1 : 0;
  if (V == 8)
    hipLaunchKernelGGL((bev_gather_kernel<8, Out>), grid, block, 0, st, src, dst, table, X, Y, Z, fx, fy, fill);
  else if (V == 4)
    hipLaunchKernelGGL((bev_gather_kernel<4, Out>), grid, block, 0, st, src, dst, table, X, Y, Z, fx, fy, fill);
  else
    hipLaunchKernelGGL((bev_gather_kernel<1, Out>), grid, block, 0, st, src, dst, table, X, Y, Z, fx, fy, fill);
  return ssbev_launch_status();
}

}  // namespace

extern "C" {

size_t ssbev_bev_label_workspace(int X, int Y, int rotate, int inplace) {
  if (X < 1 || Y < 1 || (int64_t)X * Y > (int64_t)INT32_MAX - 2 || !rotate) return 0;
  return (size_t)X * Y * sizeof(int) * (inplace && chain_rounds(X * Y) > 0 ? 2 : 1);
}

int ssbev_bev_label_transform(const uint8_t* src, int64_t* dst, int X, int Y, int Z, const double* coeffs6, int inplace,
                              int flip_dx, int flip_dy, int fill, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  return bev_label_transform(src, dst, X, Y, Z, coeffs6, inplace, flip_dx, flip_dy, fill, ws, ws_bytes, stream);
}

int ssbev_bev_label_transform_u8(const uint8_t* src, uint8_t* dst, int X, int Y, int Z, const double* coeffs6, int inplace,
                                 int flip_dx, int flip_dy, int fill, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  return bev_label_transform(src, dst, X, Y, Z, coeffs6, inplace, flip_dx, flip_dy, fill, ws, ws_bytes, stream);
}

}  // extern "C"
