// Lovasz-softmax voxel loss (lovasz_softmax.py:21-33, 156-225 of the reference head; classes='present', per_image=False), gfx950.
//
// The reference materialises the up-sampled softmax volume (168 MB at the KITTI grid) and runs one torch.sort + cumsum + gather
// chain per class over up to 2.1 M voxels.  Here:
//   key pass   one thread per fine voxel: up-sample (occ_fine.h, shared with occ_loss.hip), 20-way softmax in registers, and
//              for every class c one 31-bit sort key   ((0x3F800000 - bits(e)) << 1) | fg,   e = |fg - p_c| in [0, 1]:
//              ascending key order is descending e, and the key alone gives e and fg back exactly.  Ignored voxels write an
//              invalid key.  Per-class label counts and M by integer atomics (exact, order-free).
//   sort       per class segment, stable LSD radix sort in four 8-bit passes (tile histogram -> per-digit scan -> placement).
//              The rank of an element among the lanes of its wave with the same digit is a popcount of a match mask (one
//              ballot per digit bit; the scheme of the CSR partition in voxel_pool.hip), the running offsets live in LDS: no
//              order-dependent atomics, ties stay in voxel order, every run gives the same bits.  The first pass drops the
//              invalid keys (later passes see M elements) and takes the voxel index from the position; blocks of absent
//              classes and of tiles past the live length leave at once on the device-side counts -- the host never learns
//              them.
//   scan + dot inclusive integer scan of fg along each sorted segment (tile counts, then in-tile), J and dJ in double,
//              e * dJ reduced per tile in double and folded in tile order; dJ is scattered to [voxel][class] for backward.
//   backward   per fine voxel: rebuild p, G_c = s dJ / n_present over the present classes (s = -1 fg, +1 non-fg, 0 where
//              e == 0), g_k = p_k (G_k - sum_c G_c p_c) times the incoming gradient, written once at the fine resolution
//              and pulled back by ssbev_trilinear2x_bwd.  No float atomics anywhere.
#include "common.h"
#include "occ_fine.h"

namespace {

constexpr int LV_T = 256;                    // threads of a workgroup
constexpr int LV_WAVES = LV_T / 64;
constexpr int LV_ITEMS = 8;                  // rows of 64 elements per wave
constexpr int LV_TILE = LV_T * LV_ITEMS;     // elements of a tile
constexpr int LV_BITS = 8;
constexpr int LV_ND = 1 << LV_BITS;
constexpr int LV_PASSES = 4;                 // 31 key bits
constexpr unsigned LV_INVALID = 0xFFFFFFFFu; // ignored voxel (valid keys have bit 31 clear)
constexpr unsigned LV_ONE = 0x3F800000u;
constexpr int LV_NCNT = NC + 2;              // counts: cnt[NC], M, n_present

struct LvPlan {
  long long N;                               // fine voxels
  int nblk;                                  // tiles per class segment
  size_t totals, hist, tilefg, partial, closs, keys_a, keys_b, ids_a, ids_b, bytes;
};

LvPlan lv_plan(const ssbev_lovasz_dims* d) {
  LvPlan p;
  p.N = (long long)d->B * d->D * d->H * d->W * (d->upsample ? 8 : 1);
  p.nblk = (int)((p.N + LV_TILE - 1) / LV_TILE);
  size_t o = 0;
  p.totals = o;  o += ws_align256((size_t)LV_PASSES * NC * LV_ND * sizeof(int));
  p.hist = o;    o += ws_align256((size_t)NC * LV_ND * p.nblk * sizeof(int));
  p.tilefg = o;  o += ws_align256((size_t)NC * p.nblk * sizeof(int));
  p.partial = o; o += ws_align256((size_t)NC * p.nblk * sizeof(double));
  p.closs = o;   o += ws_align256((size_t)NC * sizeof(double));
  const size_t seg = ws_align256((size_t)NC * p.N * sizeof(unsigned));
  p.keys_a = o;  o += seg;
  p.keys_b = o;  o += seg;
  p.ids_a = o;   o += seg;
  p.ids_b = o;   o += seg;
  p.bytes = o;
  return p;
}

// lanes of this wave that hold the same digit (among the valid ones): one ballot per digit bit
__device__ __forceinline__ unsigned long long lv_match(int digit, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < LV_BITS; ++b) {
    const bool bit = (digit >> b) & 1;
    const unsigned long long bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// live length of class c's segment: the first pass walks all N slots (ignored voxels hold LV_INVALID), later ones the M
// compacted elements; an absent class has none
template <bool FIRST>
__device__ __forceinline__ int lv_live(const int32_t* __restrict__ counts, int c, int N) {
  if (counts[c] == 0) return 0;
  return FIRST ? N : counts[NC];
}

// ---------------------------------------------------------------- key pass
// softmax of flat voxel i -> z[NC] (fine_logits_flat: UP = the logits are on the coarse grid)
template <bool UP>
__device__ __forceinline__ void lv_probs(const float* __restrict__ x, long i, int D, int H, int W, float* z) {
  fine_logits_flat<UP>(x, i, D, H, W, z);
  int am;
  softmax_inplace(z, &am);
}

template <bool UP>
__global__ void __launch_bounds__(LV_T)
lovasz_key_kernel(const float* __restrict__ x, const uint8_t* __restrict__ label, unsigned* __restrict__ keys,
                  int32_t* __restrict__ counts, int D, int H, int W, long N, int ignore) {
  __shared__ int cnt[NC + 1];
  if (threadIdx.x <= NC) cnt[threadIdx.x] = 0;
  __syncthreads();
  for (long i = (long)blockIdx.x * LV_T + threadIdx.x; i < N; i += (long)gridDim.x * LV_T) {
    const int t = label[i];
    if (t == ignore) {
#pragma unroll
      for (int c = 0; c < NC; ++c) keys[(size_t)c * N + i] = LV_INVALID;
      continue;
    }
    float p[NC];
    lv_probs<UP>(x, i, D, H, W, p);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const unsigned fg = (c == t) ? 1u : 0u;
      const float e = fabsf((fg ? 1.0f : 0.0f) - p[c]);
      unsigned bits = __float_as_uint(e);
      bits = bits > LV_ONE ? LV_ONE : bits;      // (a NaN sorts in front; e <= 1 otherwise)
      keys[(size_t)c * N + i] = ((LV_ONE - bits) << 1) | fg;
    }
    if (t < NC) atomicAdd(&cnt[t], 1);
    atomicAdd(&cnt[NC], 1);
  }
  __syncthreads();
  if (threadIdx.x <= NC && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], cnt[threadIdx.x]);
}

// ---------------------------------------------------------------- segmented stable LSD radix sort, one 8-bit pass
// hist[(c * ND + d) * nblk + tile] = elements of the tile whose digit is d; totals[c * ND + d] += the same (zeroed by the host)
template <bool FIRST>
__global__ void __launch_bounds__(LV_T)
lovasz_hist_kernel(const unsigned* __restrict__ keys, const int32_t* __restrict__ counts, int N, int shift, int nblk,
                   int32_t* __restrict__ hist, int32_t* __restrict__ totals) {
  __shared__ int cnt[LV_ND];
  const int c = blockIdx.y, tid = threadIdx.x;
  const int n = lv_live<FIRST>(counts, c, N);
  const long base = (long)blockIdx.x * LV_TILE;
  if (base >= n) return;
  cnt[tid] = 0;
  __syncthreads();
  const unsigned* seg = keys + (size_t)c * N;
  unsigned k[LV_ITEMS];
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long e = base + j * LV_T + tid;
    k[j] = e < n ? seg[e] : LV_INVALID;
  }
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j)
    if (k[j] != LV_INVALID) atomicAdd(&cnt[(k[j] >> shift) & (LV_ND - 1)], 1);
  __syncthreads();
  const int v = cnt[tid];
  hist[((size_t)c * LV_ND + tid) * nblk + blockIdx.x] = v;
  if (v) atomicAdd(&totals[c * LV_ND + tid], v);
}

// one workgroup per (digit d, class c): hist[c][d][live tiles] -> exclusive offsets, starting at the number of elements of the
// class with a smaller digit
template <bool FIRST>
__global__ void __launch_bounds__(LV_T)
lovasz_scan_kernel(int32_t* __restrict__ hist, const int32_t* __restrict__ totals, const int32_t* __restrict__ counts, int N,
                   int nblk) {
  __shared__ int wsum[LV_WAVES];
  __shared__ int carry_s;
  const int d = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lv_live<FIRST>(counts, c, N);
  if (n == 0) return;
  const int live = (n + LV_TILE - 1) / LV_TILE;
  int part = tid < d ? totals[c * LV_ND + tid] : 0;
  part = wave_incl_scan(part, lane);
  if (lane == 63) wsum[wave] = part;
  __syncthreads();
  if (tid == 0) carry_s = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  int32_t* row = hist + ((size_t)c * LV_ND + d) * nblk;
  for (int c0 = 0; c0 < live; c0 += LV_T) {
    const int i = c0 + tid;
    const int v = i < live ? row[i] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = carry_s;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (i < live) row[i] = before + incl - v;
    __syncthreads();
    if (tid == 0) carry_s += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}

// stable placement of a tile's elements behind the offsets of lovasz_scan_kernel.  A wave owns LV_ITEMS consecutive rows of 64
// elements; its rows stay in registers between the counting and the placing phase.  FIRST: the id is the position (= the voxel).
template <bool FIRST>
__global__ void __launch_bounds__(LV_T)
lovasz_place_kernel(const unsigned* __restrict__ keys, const int32_t* __restrict__ ids, const int32_t* __restrict__ counts,
                    int N, int shift, int nblk, const int32_t* __restrict__ offsets, unsigned* __restrict__ keys_out,
                    int32_t* __restrict__ ids_out) {
  __shared__ int cnt[LV_WAVES * LV_ND];
  const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lv_live<FIRST>(counts, c, N);
  if ((long)blockIdx.x * LV_TILE >= n) return;
  for (int d = tid; d < LV_WAVES * LV_ND; d += LV_T) cnt[d] = 0;
  __syncthreads();
  const size_t seg = (size_t)c * N;
  const long sub = ((long)blockIdx.x * LV_WAVES + wave) * 64 * LV_ITEMS;
  int* mine = cnt + wave * LV_ND;
  unsigned kk[LV_ITEMS];
  int ii[LV_ITEMS];
  unsigned long long mm[LV_ITEMS];
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long e = sub + j * 64 + lane;
    kk[j] = e < n ? keys[seg + e] : LV_INVALID;
    ii[j] = FIRST ? (int)e : (e < n ? ids[seg + e] : 0);
  }
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const bool valid = kk[j] != LV_INVALID;
    const int digit = valid ? (int)((kk[j] >> shift) & (LV_ND - 1)) : 0;
    mm[j] = lv_match(digit, valid);
    if (valid && lane == 63 - __clzll(mm[j])) atomicAdd(&mine[digit], __popcll(mm[j]));
  }
  __syncthreads();
  {
    const int d = tid;                             // LV_T == LV_ND: one digit per thread
    int run = offsets[((size_t)c * LV_ND + d) * nblk + blockIdx.x];
#pragma unroll
    for (int w = 0; w < LV_WAVES; ++w) {
      const int v = cnt[w * LV_ND + d];
      cnt[w * LV_ND + d] = run;
      run += v;
    }
  }
  __syncthreads();
  volatile int* run = mine;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const unsigned k = kk[j];
    const bool valid = k != LV_INVALID;
    const int digit = valid ? (int)((k >> shift) & (LV_ND - 1)) : 0;
    const unsigned long long m = mm[j];
    int old = 0;
    if (valid) {
      old = run[digit];
      const int pos = old + __popcll(m & below);   // < live length of the class: offsets partition [0, #valid)
      keys_out[seg + pos] = k;
      ids_out[seg + pos] = ii[j];
    }
    __builtin_amdgcn_wave_barrier();
    if (valid && lane == 63 - __clzll(m)) run[digit] = old + __popcll(m);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------- scan + dot over the sorted segments
// tilefg[c * nblk + tile] = foreground elements of the tile
__global__ void __launch_bounds__(LV_T)
lovasz_tilefg_kernel(const unsigned* __restrict__ keys, const int32_t* __restrict__ counts, int N, int nblk,
                     int32_t* __restrict__ tilefg) {
  __shared__ int wsum[LV_WAVES];
  const int c = blockIdx.y, tid = threadIdx.x;
  const int n = lv_live<false>(counts, c, N);
  const long base = (long)blockIdx.x * LV_TILE;
  if (base >= n) return;
  const unsigned* seg = keys + (size_t)c * N;
  int f = 0;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long e = base + j * LV_T + tid;
    f += e < n ? (int)(seg[e] & 1u) : 0;
  }
  f = wave_sum(f);
  if ((tid & 63) == 0) wsum[tid >> 6] = f;
  __syncthreads();
  if (tid == 0) tilefg[(size_t)c * nblk + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Jaccard index after the first n sorted elements of which f are foreground, G foreground in all (G >= 1)
__device__ __forceinline__ double lv_jaccard(double G, double n, double f) { return 1.0 - (G - f) / (G + (n - f)); }

// partial[c * nblk + tile] = sum over the tile of e_(i) * dJ_i;  dj[voxel * NC + c] = dJ_i
__global__ void __launch_bounds__(LV_T)
lovasz_dot_kernel(const unsigned* __restrict__ keys, const int32_t* __restrict__ ids, const int32_t* __restrict__ counts,
                  const int32_t* __restrict__ tilefg, int N, int nblk, float* __restrict__ dj, double* __restrict__ partial) {
  __shared__ int wsum[LV_WAVES];
  __shared__ double dsum[LV_WAVES];
  __shared__ int carry_s;
  const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lv_live<false>(counts, c, N);
  const long base = (long)blockIdx.x * LV_TILE;
  if (base >= n) return;
  const double G = (double)counts[c];
  // foreground elements in front of this tile
  int before = 0;
  for (int b = tid; b < (int)blockIdx.x; b += LV_T) before += tilefg[(size_t)c * nblk + b];
  before = wave_sum(before);
  if (lane == 0) wsum[wave] = before;
  __syncthreads();
  if (tid == 0) carry_s = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  const unsigned* kseg = keys + (size_t)c * N;
  const int32_t* iseg = ids + (size_t)c * N;
  double acc = 0.0;
  for (int j = 0; j < LV_ITEMS; ++j) {
    const long e = base + j * LV_T + tid;
    const bool valid = e < n;
    const unsigned k = valid ? kseg[e] : 0u;
    const int fg = (int)(k & 1u);
    const int incl = wave_incl_scan(fg, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int f = carry_s + incl;
    for (int w = 0; w < wave; ++w) f += wsum[w];
    if (valid) {
      const double J = lv_jaccard(G, (double)(e + 1), (double)f);
      const double Jp = e == 0 ? 0.0 : lv_jaccard(G, (double)e, (double)(f - fg));
      const double d = J - Jp;
      acc += (double)__uint_as_float(LV_ONE - (k >> 1)) * d;
      dj[(size_t)iseg[e] * NC + c] = (float)d;
    }
    __syncthreads();
    if (tid == 0) carry_s += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  acc = wave_sum(acc);
  if (lane == 0) dsum[wave] = acc;
  __syncthreads();
  if (tid == 0) partial[(size_t)c * nblk + blockIdx.x] = ((dsum[0] + dsum[1]) + dsum[2]) + dsum[3];
}

// closs[c] = sum of the class's live tile partials (fixed order: strided per thread, then a tree)
__global__ void __launch_bounds__(LV_T)
lovasz_class_kernel(const double* __restrict__ partial, const int32_t* __restrict__ counts, int N, int nblk,
                    double* __restrict__ closs) {
  const int c = blockIdx.x;
  const int n = lv_live<false>(counts, c, N);
  const int live = (n + LV_TILE - 1) / LV_TILE;
  double a[1];
  block_fold256(partial + (size_t)c * nblk, live, 1, a);
  if (threadIdx.x == 0) closs[c] = a[0];
}

// loss = mean of closs over the present classes (0 when none); counts[NC + 1] = n_present
__global__ void __launch_bounds__(64)
lovasz_final_kernel(const double* __restrict__ closs, int32_t* __restrict__ counts, float* __restrict__ loss) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  int np = 0;
  for (int c = 0; c < NC; ++c)
    if (counts[c] > 0) { s += closs[c]; ++np; }
  counts[NC + 1] = np;
  loss[0] = np > 0 ? (float)(s / (double)np) : 0.0f;
}

// ---------------------------------------------------------------- backward
template <bool UP>
__global__ void __launch_bounds__(LV_T)
lovasz_bwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ label, const float* __restrict__ dj,
                  const int32_t* __restrict__ counts, const float* __restrict__ grad_out, float* __restrict__ gdst, int D,
                  int H, int W, long N, int ignore) {
  __shared__ float scale[NC];                    // grad_out / n_present for a present class, 0 for an absent one
  __shared__ int present[NC];
  if (threadIdx.x < NC) {
    const int np = counts[NC + 1];
    present[threadIdx.x] = counts[threadIdx.x] > 0;
    scale[threadIdx.x] = counts[threadIdx.x] > 0 ? grad_out[0] / (float)np : 0.0f;
  }
  __syncthreads();
  for (long i = (long)blockIdx.x * LV_T + threadIdx.x; i < N; i += (long)gridDim.x * LV_T) {
    const int t = label[i];
    float* dst = gdst + (size_t)i * NC;
    if (t == ignore) {
      zero20(dst);
      continue;
    }
    float p[NC], g[NC];
    lv_probs<UP>(x, i, D, H, W, p);
    load20(dj + (size_t)i * NC, g);
    float dot = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      // d|fg - p| / dp: -1 for fg, +1 for non-fg, 0 where the error is exactly 0 (torch's abs)
      const float s = (c == t) ? (p[c] < 1.0f ? -1.0f : 0.0f) : (p[c] > 0.0f ? 1.0f : 0.0f);
      g[c] = present[c] ? s * g[c] * scale[c] : 0.0f;      // (dj of an absent class was never written: select, not multiply)
      dot += g[c] * p[c];
    }
    float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
    for (int q = 0; q < NC / 4; ++q)
      d4[q] = make_float4(p[4 * q] * (g[4 * q] - dot), p[4 * q + 1] * (g[4 * q + 1] - dot),
                           p[4 * q + 2] * (g[4 * q + 2] - dot), p[4 * q + 3] * (g[4 * q + 3] - dot));
  }
}

template <bool FIRST>
void lv_sort_pass(const unsigned* kin, const int32_t* iin, unsigned* kout, int32_t* iout, const int32_t* counts,
                  const LvPlan& p, int pass, int32_t* hist, int32_t* totals, hipStream_t st) {
  const int shift = pass * LV_BITS, N = (int)p.N;
  int32_t* tot = totals + (size_t)pass * NC * LV_ND;
  hipLaunchKernelGGL(lovasz_hist_kernel<FIRST>, dim3(p.nblk, NC), dim3(LV_T), 0, st, kin, counts, N, shift, p.nblk, hist, tot);
  hipLaunchKernelGGL(lovasz_scan_kernel<FIRST>, dim3(LV_ND, NC), dim3(LV_T), 0, st, hist, tot, counts, N, p.nblk);
  hipLaunchKernelGGL(lovasz_place_kernel<FIRST>, dim3(p.nblk, NC), dim3(LV_T), 0, st, kin, iin, counts, N, shift, p.nblk, hist,
                     kout, iout);
}

}  // namespace

extern "C" {

int ssbev_lovasz_num_counts(void) { return LV_NCNT; }

size_t ssbev_lovasz_workspace(const ssbev_lovasz_dims* d) { return fine_dims_ok(d) ? lv_plan(d).bytes : 0; }

int ssbev_lovasz_fwd(const float* logits, const uint8_t* label, float* loss, float* dj, int32_t* counts,
                     const ssbev_lovasz_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  if (!fine_dims_ok(d) || !logits || !label || !loss || !dj || !counts || !ws) return SSBEV_EINVAL;
  const LvPlan p = lv_plan(d);
  if (ws_bytes < p.bytes) return SSBEV_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  char* w = static_cast<char*>(ws);
  int32_t* totals = reinterpret_cast<int32_t*>(w + p.totals);
  int32_t* hist = reinterpret_cast<int32_t*>(w + p.hist);
  int32_t* tilefg = reinterpret_cast<int32_t*>(w + p.tilefg);
  double* partial = reinterpret_cast<double*>(w + p.partial);
  double* closs = reinterpret_cast<double*>(w + p.closs);
  unsigned* ka = reinterpret_cast<unsigned*>(w + p.keys_a);
  unsigned* kb = reinterpret_cast<unsigned*>(w + p.keys_b);
  int32_t* ia = reinterpret_cast<int32_t*>(w + p.ids_a);
  int32_t* ib = reinterpret_cast<int32_t*>(w + p.ids_b);
  if (hipMemsetAsync(counts, 0, LV_NCNT * sizeof(int32_t), st) != hipSuccess) return SSBEV_ELAUNCH;
  if (hipMemsetAsync(totals, 0, (size_t)LV_PASSES * NC * LV_ND * sizeof(int32_t), st) != hipSuccess) return SSBEV_ELAUNCH;
  const int N = (int)p.N;
  if (d->upsample)
    hipLaunchKernelGGL(lovasz_key_kernel<true>, dim3(voxel_grid(p.N)), dim3(LV_T), 0, st, logits, label, ka, counts, d->D,
                       d->H, d->W, (long)p.N, d->ignore);
  else
    hipLaunchKernelGGL(lovasz_key_kernel<false>, dim3(voxel_grid(p.N)), dim3(LV_T), 0, st, logits, label, ka, counts, d->D,
                       d->H, d->W, (long)p.N, d->ignore);
  lv_sort_pass<true>(ka, nullptr, kb, ib, counts, p, 0, hist, totals, st);
  lv_sort_pass<false>(kb, ib, ka, ia, counts, p, 1, hist, totals, st);
  lv_sort_pass<false>(ka, ia, kb, ib, counts, p, 2, hist, totals, st);
  lv_sort_pass<false>(kb, ib, ka, ia, counts, p, 3, hist, totals, st);
  hipLaunchKernelGGL(lovasz_tilefg_kernel, dim3(p.nblk, NC), dim3(LV_T), 0, st, ka, counts, N, p.nblk, tilefg);
  hipLaunchKernelGGL(lovasz_dot_kernel, dim3(p.nblk, NC), dim3(LV_T), 0, st, ka, ia, counts, tilefg, N, p.nblk, dj, partial);
  hipLaunchKernelGGL(lovasz_class_kernel, dim3(NC), dim3(LV_T), 0, st, partial, counts, N, p.nblk, closs);
  hipLaunchKernelGGL(lovasz_final_kernel, dim3(1), dim3(64), 0, st, closs, counts, loss);
  return ssbev_launch_status();
}

size_t ssbev_lovasz_bwd_workspace(const ssbev_lovasz_dims* d) {
  if (!fine_dims_ok(d)) return 0;
  return d->upsample ? (size_t)lv_plan(d).N * NC * sizeof(float) : 0;
}

int ssbev_lovasz_bwd(const float* logits, const uint8_t* label, const float* dj, const int32_t* counts,
                     const float* grad_out, float* grad_logits, const ssbev_lovasz_dims* d, void* ws, size_t ws_bytes,
                     ssbev_stream_t stream) {
  if (!fine_dims_ok(d) || !logits || !label || !dj || !counts || !grad_out || !grad_logits) return SSBEV_EINVAL;
  if (d->upsample && !ws) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_lovasz_bwd_workspace(d)) return SSBEV_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const LvPlan p = lv_plan(d);
  float* gfine = d->upsample ? static_cast<float*>(ws) : grad_logits;
  if (!d->upsample)
    hipLaunchKernelGGL(lovasz_bwd_kernel<false>, dim3(voxel_grid(p.N)), dim3(LV_T), 0, st, logits, label, dj, counts, grad_out,
                       gfine, d->D, d->H, d->W, (long)p.N, d->ignore);
  else
    hipLaunchKernelGGL(lovasz_bwd_kernel<true>, dim3(voxel_grid(p.N)), dim3(LV_T), 0, st, logits, label, dj, counts, grad_out,
                       gfine, d->D, d->H, d->W, (long)p.N, d->ignore);
  return finish_fine_grad(gfine, grad_logits, d->B, d->D, d->H, d->W, stream);
}

}  // extern "C"
