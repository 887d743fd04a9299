// OHEM cross-entropy voxel loss (OHEM_CE_ssc_loss, utils/semkitti.py:151-185 of the reference), gfx950.
//
// The reference materialises the up-sampled logit volume (168 MB at the KITTI grid), a [B, N] loss volume, a boolean compaction
// and one torch.topk over up to 2.1 M elements per sample.  A selection needs no sort: cross-entropy losses are >= +0, so their
// fp32 bit patterns order like unsigned integers, and a most-significant-digit-first radix select finds the k-th largest exactly
// in four 8-bit histogram passes.  Here:
//   loss pass   one thread per fine voxel: up-sample (occ_fine.h), log-sum-exp with the ACCURATE expf / logf (the selection
//               depends on l; the fast intrinsics of softmax_inplace are not used here), l = w[t] (lse - z_t) canonicalised to
//               >= +0.0 (a saturated voxel would give -0.0, whose bit pattern sorts above everything; a NaN becomes the one
//               positive quiet NaN, which sorts on top as in torch.topk), written as fp32 bits to [B][N]; ignored voxels write
//               a marker no loss can equal.  M_b and the histogram of the top digit by integer atomics (LDS, then global):
//               exact and order-free.
//   pick        one workgroup per sample: k_b = (long long)((double)M_b * top_k) on the device (Python's int(M * top_k); the
//               host never reads M_b), then the 256 bins from the top: the digit that holds the k-th largest, the new prefix
//               and the count that remains inside the bin.
//   histogram   passes 1..3: the digit counts of the elements that match the prefix found so far.
//               After four picks the threshold T_b and r_b (how many elements equal to T_b belong to the selection) are exact.
//   select      per tile: tie counts, then (exclusive prefix over the tiles in front + in-tile rank by ballot / popcount) the
//               elements equal to T_b are taken lowest flat voxel index first up to r_b; sum of l and of w[t] over the selection
//               in double per tile, one byte per voxel for backward.
//   final       one workgroup folds the tile partials in a fixed order: loss = S / max(Wsum, 1e-4), and 1 / max(Wsum, 1e-4).
//   backward    per fine voxel: selected -> g w[t] (p_j - [j == t]) / max(Wsum, 1e-4), everything else zeros; written once at
//               the fine resolution and pulled back by ssbev_trilinear2x_bwd.  Wsum carries no gradient, as in the reference.
// No float atomics anywhere: every run gives the same bits.
#include "common.h"
#include "occ_fine.h"

namespace {

constexpr int OH_T = 256;                    // threads of a workgroup
constexpr int OH_WAVES = OH_T / 64;
constexpr int OH_ITEMS = 8;                  // rows of OH_T elements per tile
constexpr int OH_TILE = OH_T * OH_ITEMS;
constexpr int OH_ND = 256;                   // bins of an 8-bit digit (== OH_T: one bin per thread)
constexpr int OH_PASSES = 4;
constexpr unsigned OH_MARK = 0xFFFFFFFFu;    // ignored voxel (a canonical loss has bit 31 clear)
constexpr unsigned OH_QNAN = 0x7FC00000u;

struct OhState {                             // per sample
  unsigned prefix;                           // digits fixed so far; after the last pick the bits of T_b (OH_MARK when k_b == 0)
  int M;                                     // labelled voxels
  long long k;                               // still to find inside the prefix; after the last pick r_b
};

struct OhPlan {
  long long N;                               // fine voxels of the batch
  int Ns;                                    // fine voxels of a sample
  int nblk;                                  // tiles per sample
  size_t lbits, hist, state, tiecnt, part_s, part_w, zero_from, zero_bytes, bytes;
};

bool oh_ok(const ssbev_ohem_dims* d) {
  return fine_dims_ok(d) && d->top_k > 0.0 && d->top_k <= 1.0;     // (a NaN fails both)
}

OhPlan oh_plan(const ssbev_ohem_dims* d) {
  OhPlan p;
  p.Ns = d->D * d->H * d->W * (d->upsample ? 8 : 1);
  p.N = (long long)d->B * p.Ns;
  p.nblk = (p.Ns + OH_TILE - 1) / OH_TILE;
  size_t o = 0;
  p.lbits = o;   o += ws_align256((size_t)p.N * sizeof(unsigned));   // first: the per-voxel losses stay readable after the call
  p.zero_from = o;
  p.hist = o;    o += ws_align256((size_t)d->B * OH_PASSES * OH_ND * sizeof(int));
  p.state = o;   o += ws_align256((size_t)d->B * sizeof(OhState));
  p.zero_bytes = o - p.zero_from;
  p.tiecnt = o;  o += ws_align256((size_t)d->B * p.nblk * sizeof(int));
  p.part_s = o;  o += ws_align256((size_t)d->B * p.nblk * sizeof(double));
  p.part_w = o;  o += ws_align256((size_t)d->B * p.nblk * sizeof(double));
  p.bytes = o;
  return p;
}

__device__ __forceinline__ bool oh_labelled(int t, int ignore) { return t != ignore && t < NC; }

// ---------------------------------------------------------------- loss pass (+ histogram of the top digit, + M_b)
template <bool UP>
__global__ void __launch_bounds__(OH_T)
ohem_loss_kernel(const float* __restrict__ x, const uint8_t* __restrict__ label, const float* __restrict__ cw,
                 unsigned* __restrict__ lbits, int32_t* __restrict__ hist, OhState* __restrict__ state, int D, int H, int W,
                 int Ns, int ignore) {
  __shared__ int cnt[OH_ND];
  __shared__ int labelled;
  __shared__ float w[NC];
  const int b = blockIdx.y, tid = threadIdx.x;
  cnt[tid] = 0;
  if (tid == 0) labelled = 0;
  if (tid < NC) w[tid] = cw[tid];
  __syncthreads();
  int mine = 0;
  for (int v = blockIdx.x * OH_T + tid; v < Ns; v += gridDim.x * OH_T) {
    const size_t i = (size_t)b * Ns + v;
    const int t = label[i];
    if (!oh_labelled(t, ignore)) {
      lbits[i] = OH_MARK;
      continue;
    }
    float z[NC];
    fine_logits<UP>(x, b, v, Ns, D, H, W, z);
    float zt = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) zt = (c == t) ? z[c] : zt;
    float m;
    const float s = exp_inplace(z, &m);
    const float l = w[t] * (logf(s) - (zt - m));
    unsigned bits = __float_as_uint(l);
    if (l != l) bits = OH_QNAN;
    else if (bits & 0x80000000u) bits = 0u;      // -0.0 (and a rounding-negative difference) -> +0.0
    lbits[i] = bits;
    atomicAdd(&cnt[bits >> 24], 1);
    ++mine;
  }
  if (mine) atomicAdd(&labelled, mine);
  __syncthreads();
  const int c = cnt[tid];
  if (c) atomicAdd(&hist[(size_t)b * OH_PASSES * OH_ND + tid], c);
  if (tid == 0 && labelled) atomicAdd(&state[b].M, labelled);
}

// ---------------------------------------------------------------- digit counts of the elements inside the prefix, passes 1..3
__global__ void __launch_bounds__(OH_T)
ohem_hist_kernel(const unsigned* __restrict__ lbits, const OhState* __restrict__ state, int32_t* __restrict__ hist, int Ns,
                 int pass) {
  __shared__ int cnt[OH_ND];
  const int b = blockIdx.y, tid = threadIdx.x;
  const unsigned prefix = state[b].prefix;
  if (state[b].k <= 0) return;                   // nothing is selected from this sample
  const int base = blockIdx.x * OH_TILE;
  const int shift = 24 - 8 * pass;
  cnt[tid] = 0;
  __syncthreads();
  const unsigned* seg = lbits + (size_t)b * Ns;
#pragma unroll
  for (int j = 0; j < OH_ITEMS; ++j) {
    const int e = base + j * OH_T + tid;
    const unsigned k = e < Ns ? seg[e] : OH_MARK;
    if (k != OH_MARK && (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&cnt[(k >> shift) & (OH_ND - 1)], 1);
  }
  __syncthreads();
  const int c = cnt[tid];
  if (c) atomicAdd(&hist[((size_t)b * OH_PASSES + pass) * OH_ND + tid], c);
}

// ---------------------------------------------------------------- one workgroup per sample: the digit of the k-th largest
__global__ void __launch_bounds__(OH_T)
ohem_pick_kernel(const int32_t* __restrict__ hist, OhState* __restrict__ state, int pass, double top_k) {
  __shared__ int wsum[OH_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = OH_ND - 1 - tid;                 // thread 0 holds the top bin
  const unsigned prefix = pass == 0 ? 0u : state[b].prefix;
  const long long k = pass == 0 ? (long long)((double)state[b].M * top_k) : state[b].k;
  const int h = hist[((size_t)b * OH_PASSES + pass) * OH_ND + d];
  int incl = wave_incl_scan(h, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();                               // (also: every thread has read the state before one of them writes it)
  for (int w = 0; w < wave; ++w) incl += wsum[w];
  if (k <= 0) {
    if (tid == 0) { state[b].prefix = OH_MARK; state[b].k = 0; }
    return;
  }
  const long long above = (long long)(incl - h); // elements inside the prefix with a larger digit
  if (above < k && k <= (long long)incl) {       // exactly one thread: k <= the number of elements inside the prefix
    state[b].prefix = prefix | ((unsigned)d << (24 - 8 * pass));
    state[b].k = k - above;
  }
}

// ---------------------------------------------------------------- selection
// tiecnt[b * nblk + tile] = elements of the tile equal to T_b
__global__ void __launch_bounds__(OH_T)
ohem_tie_kernel(const unsigned* __restrict__ lbits, const OhState* __restrict__ state, int32_t* __restrict__ tiecnt, int Ns,
                int nblk) {
  __shared__ int wsum[OH_WAVES];
  const int b = blockIdx.y, tid = threadIdx.x;
  const unsigned T = state[b].prefix;
  const int base = blockIdx.x * OH_TILE;
  const unsigned* seg = lbits + (size_t)b * Ns;
  int n = 0;
#pragma unroll
  for (int j = 0; j < OH_ITEMS; ++j) {
    const int e = base + j * OH_T + tid;
    const unsigned k = e < Ns ? seg[e] : OH_MARK;
    n += (k != OH_MARK && k == T) ? 1 : 0;
  }
  n = wave_sum(n);
  if ((tid & 63) == 0) wsum[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) tiecnt[(size_t)b * nblk + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// mask[voxel] = selected;  part_s / part_w [b * nblk + tile] = sum of l / of w[t] over the tile's selected voxels (double)
__global__ void __launch_bounds__(OH_T)
ohem_select_kernel(const unsigned* __restrict__ lbits, const uint8_t* __restrict__ label, const float* __restrict__ cw,
                   const OhState* __restrict__ state, const int32_t* __restrict__ tiecnt, uint8_t* __restrict__ mask,
                   double* __restrict__ part_s, double* __restrict__ part_w, int Ns, int nblk) {
  __shared__ int wsum[OH_WAVES];
  __shared__ int rowcnt[OH_ITEMS * OH_WAVES];    // ties per (row j, wave), then their exclusive prefix in voxel order
  __shared__ double ds[OH_WAVES], dw[OH_WAVES];
  __shared__ float w[NC];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned T = state[b].prefix;
  const long long r = state[b].k;
  if (tid < NC) w[tid] = cw[tid];
  // ties in the tiles in front of this one
  int before = 0;
  for (int t = tid; t < (int)blockIdx.x; t += OH_T) before += tiecnt[(size_t)b * nblk + t];
  before = wave_sum(before);
  if (lane == 0) wsum[wave] = before;
  const int base = blockIdx.x * OH_TILE;
  const size_t seg = (size_t)b * Ns;
  unsigned kk[OH_ITEMS];
  unsigned long long tm[OH_ITEMS];
#pragma unroll
  for (int j = 0; j < OH_ITEMS; ++j) {
    const int e = base + j * OH_T + tid;
    kk[j] = e < Ns ? lbits[seg + e] : OH_MARK;
    tm[j] = __ballot(kk[j] != OH_MARK && kk[j] == T);
    if (lane == 0) rowcnt[j * OH_WAVES + wave] = __popcll(tm[j]);
  }
  __syncthreads();
  before = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  if (wave == 0) {                               // voxel order inside the tile is (row j, wave, lane): 32 counts, one wave
    const int v = lane < OH_ITEMS * OH_WAVES ? rowcnt[lane] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (lane < OH_ITEMS * OH_WAVES) rowcnt[lane] = incl - v;
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  double as = 0.0, aw = 0.0;
#pragma unroll
  for (int j = 0; j < OH_ITEMS; ++j) {
    const int e = base + j * OH_T + tid;
    if (e >= Ns) continue;
    const unsigned k = kk[j];
    bool sel = false;
    if (k != OH_MARK) {
      if (k > T) sel = true;
      else if (k == T) sel = (long long)(before + rowcnt[j * OH_WAVES + wave] + __popcll(tm[j] & below)) < r;
    }
    mask[seg + e] = sel ? 1 : 0;
    if (sel) {
      as += (double)__uint_as_float(k);
      aw += (double)w[label[seg + e]];           // selected => labelled => label < NC
    }
  }
  as = wave_sum(as);
  aw = wave_sum(aw);
  if (lane == 0) { ds[wave] = as; dw[wave] = aw; }
  __syncthreads();
  if (tid == 0) {
    part_s[(size_t)b * nblk + blockIdx.x] = ((ds[0] + ds[1]) + ds[2]) + ds[3];
    part_w[(size_t)b * nblk + blockIdx.x] = ((dw[0] + dw[1]) + dw[2]) + dw[3];
  }
}

// loss = S / max(Wsum, 1e-4), inv = 1 / max(Wsum, 1e-4): the tile partials strided per thread in tile order, then a tree
__global__ void __launch_bounds__(OH_T)
ohem_final_kernel(const double* __restrict__ part_s, const double* __restrict__ part_w, int n, float* __restrict__ loss,
                  float* __restrict__ inv) {
  double s[1], w[1];
  block_fold256(part_s, n, 1, s);
  block_fold256(part_w, n, 1, w);
  if (threadIdx.x == 0) {
    const double den = w[0] > 1e-4 ? w[0] : 1e-4;
    loss[0] = (float)(s[0] / den);
    inv[0] = (float)(1.0 / den);
  }
}

// ---------------------------------------------------------------- backward
template <bool UP>
__global__ void __launch_bounds__(OH_T)
ohem_bwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ label, const float* __restrict__ cw,
                const uint8_t* __restrict__ mask, const float* __restrict__ inv, const float* __restrict__ grad_out,
                float* __restrict__ gdst, int D, int H, int W, int Ns, long N) {
  __shared__ float w[NC];                        // grad_out * w[c] / max(Wsum, 1e-4)
  if (threadIdx.x < NC) w[threadIdx.x] = grad_out[0] * inv[0] * cw[threadIdx.x];
  __syncthreads();
  for (long i = (long)blockIdx.x * OH_T + threadIdx.x; i < N; i += (long)gridDim.x * OH_T) {
    float* dst = gdst + (size_t)i * NC;
    if (!mask[i]) {
      zero20(dst);
      continue;
    }
    const int t = label[i];
    float p[NC];
    fine_logits<UP>(x, (int)(i / Ns), (int)(i % Ns), Ns, D, H, W, p);
    float m;
    const float s = exp_inplace(p, &m);
    const float g = w[t] / s;
    float o[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] = g * p[c] - (c == t ? w[t] : 0.0f);
    store20(dst, o);
  }
}

}  // namespace

extern "C" {

size_t ssbev_ohem_ce_workspace(const ssbev_ohem_dims* d) { return oh_ok(d) ? oh_plan(d).bytes : 0; }

int ssbev_ohem_ce_fwd(const float* logits, const uint8_t* label, const float* class_weight, float* loss, uint8_t* mask,
                      float* inv_wsum, const ssbev_ohem_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  if (!oh_ok(d) || !logits || !label || !class_weight || !loss || !mask || !inv_wsum || !ws) return SSBEV_EINVAL;
  const OhPlan p = oh_plan(d);
  if (ws_bytes < p.bytes) return SSBEV_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  char* w = static_cast<char*>(ws);
  unsigned* lbits = reinterpret_cast<unsigned*>(w + p.lbits);
  int32_t* hist = reinterpret_cast<int32_t*>(w + p.hist);
  OhState* state = reinterpret_cast<OhState*>(w + p.state);
  int32_t* tiecnt = reinterpret_cast<int32_t*>(w + p.tiecnt);
  double* part_s = reinterpret_cast<double*>(w + p.part_s);
  double* part_w = reinterpret_cast<double*>(w + p.part_w);
  if (hipMemsetAsync(w + p.zero_from, 0, p.zero_bytes, st) != hipSuccess) return SSBEV_ELAUNCH;
  const dim3 lgrid(voxel_grid(p.Ns), d->B), tgrid(p.nblk, d->B);
  if (d->upsample)
    hipLaunchKernelGGL(ohem_loss_kernel<true>, lgrid, dim3(OH_T), 0, st, logits, label, class_weight, lbits, hist, state, d->D,
                       d->H, d->W, p.Ns, d->ignore);
  else
    hipLaunchKernelGGL(ohem_loss_kernel<false>, lgrid, dim3(OH_T), 0, st, logits, label, class_weight, lbits, hist, state, d->D,
                       d->H, d->W, p.Ns, d->ignore);
  for (int pass = 0; pass < OH_PASSES; ++pass) {
    if (pass > 0) hipLaunchKernelGGL(ohem_hist_kernel, tgrid, dim3(OH_T), 0, st, lbits, state, hist, p.Ns, pass);
    hipLaunchKernelGGL(ohem_pick_kernel, dim3(d->B), dim3(OH_T), 0, st, hist, state, pass, d->top_k);
  }
  hipLaunchKernelGGL(ohem_tie_kernel, tgrid, dim3(OH_T), 0, st, lbits, state, tiecnt, p.Ns, p.nblk);
  hipLaunchKernelGGL(ohem_select_kernel, tgrid, dim3(OH_T), 0, st, lbits, label, class_weight, state, tiecnt, mask, part_s,
                     part_w, p.Ns, p.nblk);
  hipLaunchKernelGGL(ohem_final_kernel, dim3(1), dim3(OH_T), 0, st, part_s, part_w, d->B * p.nblk, loss, inv_wsum);
  return ssbev_launch_status();
}

size_t ssbev_ohem_ce_bwd_workspace(const ssbev_ohem_dims* d) {
  if (!oh_ok(d)) return 0;
  return d->upsample ? (size_t)oh_plan(d).N * NC * sizeof(float) : 0;
}

int ssbev_ohem_ce_bwd(const float* logits, const uint8_t* label, const float* class_weight, const uint8_t* mask,
                      const float* inv_wsum, const float* grad_out, float* grad_logits, const ssbev_ohem_dims* d, void* ws,
                      size_t ws_bytes, ssbev_stream_t stream) {
  if (!oh_ok(d) || !logits || !label || !class_weight || !mask || !inv_wsum || !grad_out || !grad_logits) return SSBEV_EINVAL;
  if (d->upsample && !ws) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_ohem_ce_bwd_workspace(d)) return SSBEV_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const OhPlan p = oh_plan(d);
  float* gfine = d->upsample ? static_cast<float*>(ws) : grad_logits;
  if (!d->upsample)
    hipLaunchKernelGGL(ohem_bwd_kernel<false>, dim3(voxel_grid(p.N)), dim3(OH_T), 0, st, logits, label, class_weight, mask,
                       inv_wsum, grad_out, gfine, d->D, d->H, d->W, p.Ns, (long)p.N);
  else
    hipLaunchKernelGGL(ohem_bwd_kernel<true>, dim3(voxel_grid(p.N)), dim3(OH_T), 0, st, logits, label, class_weight, mask,
                       inv_wsum, grad_out, gfine, d->D, d->H, d->W, p.Ns, (long)p.N);
  return finish_fine_grad(gfine, grad_logits, d->B, d->D, d->H, d->W, stream);
}

}  // extern "C"
