// 3-D context relation prior (CPMegaVoxels, occupancy/backbones/crp3d.py:173-262 of the reference; its loss
// compute_super_CP_multilabel_loss, resnet3d.py:269-290; its labels CreateRelationLabels._downsample_label / compute_CP_mega_matrix,
// datasets/pipelines/voxel_labels.py:79-174), gfx950, fp32.
//
// Layout.  The four context_prior_logits convolutions run as ONE pointwise layer with R * Mc output channels, and a convolution
// here leaves its result channels-last: P[b][n][r][m] (n = row voxel of the X x Y x Z grid, m = mega voxel of the halved grid),
// which is already the [relation][N][Mc] order the reference reaches by a permute.  The mega context leaves ctx[b][m][c] (c < C2)
// the same way.  Nothing here makes a permuted copy.
//   labels      one wave per coarse voxel: a 256-bin histogram of its ds^3 block (integer LDS atomics), then the reference's
//               rule: more than 0.95 ds^3 empty-or-255 voxels -> 0 if the zeros outnumber the 255s else 255; otherwise the most
//               frequent class 1 .. 254, the lowest id on a tie.
//   loss        y[r][n][m] is a function of the row voxel's label and the eight child labels of mega voxel m: a thread keeps the
//               children of its m in registers and walks CR_ROWS rows; the [4, N, Mc] matrix never exists.  Per relation it sums
//               softplus(-x) over the positives, softplus(x) over the negatives and counts the positives, in double; the
//               workgroup's twelve sums go to its own row of the workspace (wave butterfly, then the four waves in order).  The
//               final kernel folds the rows (block_fold256), forms pw_r = (total - cnt_r) / cnt_r over the whole batch (1 when
//               cnt_r = 0: it multiplies nothing) and loss = sum_r (pw_r S+_r + S-_r) / (4 total), and leaves pw on the device
//               for backward: d loss / d x = y ? -pw_r sigmoid(-x) : sigmoid(x), over 4 total, times the incoming scalar.
//   gather      out[b][n][r C2 + c] = sum_m sigmoid(P[b][n][r][m]) ctx[b][m][c]: an LDS-tiled GEMM per (b, r) on
//               v_mfma_f32_32x32x2_f32 (128 x 128 x 16 tiles, four waves of 64 x 64) whose A loader applies the sigmoid on the way
//               into LDS; the result lands in the channel slice of the concatenated [input, context] tensor (row stride ld_out).
//               Backward: dP = (dOut_r ctx^T) * s (1 - s) with s recomputed from P in the epilogue, and
//               dctx = sum_r sigmoid(P_r)^T dOut_r, the reduction over (r, n) cut into slices whose partial products are folded
//               in a fixed order.  sigmoid(P) is never stored.
// No float atomics, no host read-back; every run gives the same bits.
#include "common.h"
#include "occ_fine.h"

namespace {

constexpr int CR_T = 256;                    // threads of a workgroup
constexpr int CR_R = 4;                      // relations of the loss
constexpr int CR_ROWS = 32;                  // rows a loss workgroup walks
constexpr int CR_NV = 12;                    // S+[4], S-[4], positives[4]
constexpr int CR_NONE = 255;
constexpr int CR_MAX_DS = 32;

bool crp_ok(const ssbev_crp_dims* d) {
  if (!d || d->B <= 0 || d->X <= 0 || d->Y <= 0 || d->Z <= 0) return false;
  if ((d->X | d->Y | d->Z) & 1) return false;
  const long long n = (long long)d->X * d->Y * d->Z;
  return n < (1ll << 24) && (long long)d->B * n * CR_R * (n / 8) < (1ll << 40);
}

struct CrPlan {
  int N, Mc, mblk, nblk, nparts;
  size_t bytes;
};

CrPlan crp_plan(const ssbev_crp_dims* d) {
  CrPlan p;
  p.N = d->X * d->Y * d->Z;
  p.Mc = p.N / 8;
  p.mblk = (p.Mc + CR_T - 1) / CR_T;
  p.nblk = (p.N + CR_ROWS - 1) / CR_ROWS;
  p.nparts = d->B * p.mblk * p.nblk;
  p.bytes = ws_align256((size_t)p.nparts * CR_NV * sizeof(double));
  return p;
}

__device__ __forceinline__ float softplusf(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoidf(float x) {
  const float e = expf(-fabsf(x)), r = 1.0f / (1.0f + e);
  return x >= 0.0f ? r : e * r;
}

// the eight child labels of mega voxel m of a sample's [X, Y, Z] label grid
__device__ __forceinline__ void crp_children(const uint8_t* __restrict__ lab, int m, int Y, int Z, int (&c)[8]) {
  const int Z2 = Z >> 1, Y2 = Y >> 1;
  const int zz = m % Z2, yy = (m / Z2) % Y2, xx = m / (Z2 * Y2);
#pragma unroll
  for (int k = 0; k < 8; ++k)
    c[k] = lab[((size_t)(2 * xx + (k >> 2)) * Y + 2 * yy + ((k >> 1) & 1)) * Z + 2 * zz + (k & 1)];
}

// bit r = y[r] of a row voxel labelled lr against the children (voxel_labels.py:162-169): children labelled 255 are skipped, a
// row labelled 255 has no positive; 0 same non-empty class, 1 two different non-empty classes, 2 both empty, 3 one of them empty
__device__ __forceinline__ unsigned crp_bits(int lr, const int (&c)[8]) {
  unsigned b = 0;
  if (lr == CR_NONE) return b;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int cc = c[k];
    if (cc == CR_NONE) continue;
    if (cc == lr) {
      b |= cc != 0 ? 1u : 4u;
    } else {
      if (cc != 0 && lr != 0) b |= 2u;
      if (cc == 0 || lr == 0) b |= 8u;
    }
  }
  return b;
}

// ---------------------------------------------------------------- loss forward, pass 1
__global__ void __launch_bounds__(CR_T)
crp_loss_accum_kernel(const float* __restrict__ P, const uint8_t* __restrict__ labels, double* __restrict__ part, int N, int Mc,
                      int Y, int Z) {
  __shared__ double red[CR_T / 64][CR_NV];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int m = blockIdx.x * CR_T + tid, n0 = blockIdx.y * CR_ROWS;
  const uint8_t* lab = labels + (size_t)b * N;
  const bool in = m < Mc;
  int c[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = CR_NONE;
  if (in) crp_children(lab, m, Y, Z, c);
  double v[CR_NV];
#pragma unroll
  for (int k = 0; k < CR_NV; ++k) v[k] = 0.0;
  if (in) {
    for (int j = 0; j < CR_ROWS && n0 + j < N; ++j) {
      const int n = n0 + j;
      const unsigned bits = crp_bits(lab[n], c);
      const float* row = P + (((size_t)b * N + n) * CR_R) * Mc + m;
#pragma unroll
      for (int r = 0; r < CR_R; ++r) {
        const float x = row[(size_t)r * Mc];
        if ((bits >> r) & 1u) {
          v[r] += (double)softplusf(-x);
          v[8 + r] += 1.0;
        } else {
          v[4 + r] += (double)softplusf(x);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CR_NV; ++k) {
    const double s = wave_sum(v[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = s;
  }
  __syncthreads();
  if (tid < CR_NV) {
    const size_t blk = ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[blk * CR_NV + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// ---------------------------------------------------------------- loss forward, pass 2: fold, pos_weight, loss
__global__ void __launch_bounds__(CR_T)
crp_loss_final_kernel(const double* __restrict__ part, long nparts, double total, float* __restrict__ loss, float* __restrict__ pw) {
  double s[CR_NV];
  block_fold256<CR_NV>(part, nparts, CR_NV, s);
  if (threadIdx.x == 0) {
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < CR_R; ++r) {
      const double cnt = s[8 + r];
      const double w = cnt > 0.0 ? (total - cnt) / cnt : 1.0;
      pw[r] = (float)w;
      acc += w * s[r] + s[4 + r];
    }
    loss[0] = (float)(acc / ((double)CR_R * total));
  }
}

// ---------------------------------------------------------------- loss backward
__global__ void __launch_bounds__(CR_T)
crp_loss_bwd_kernel(const float* __restrict__ P, const uint8_t* __restrict__ labels, const float* __restrict__ pw,
                    const float* __restrict__ grad_out, float* __restrict__ gP, int N, int Mc, int Y, int Z, float inv_count) {
  const int tid = threadIdx.x, b = blockIdx.z;
  const int m = blockIdx.x * CR_T + tid, n0 = blockIdx.y * CR_ROWS;
  if (m >= Mc) return;
  const uint8_t* lab = labels + (size_t)b * N;
  int c[8];
  crp_children(lab, m, Y, Z, c);
  const float g = grad_out[0] * inv_count;
  float w[CR_R];
#pragma unroll
  for (int r = 0; r < CR_R; ++r) w[r] = pw[r];
  for (int j = 0; j < CR_ROWS && n0 + j < N; ++j) {
    const int n = n0 + j;
    const unsigned bits = crp_bits(lab[n], c);
    const size_t o = (((size_t)b * N + n) * CR_R) * Mc + m;
#pragma unroll
    for (int r = 0; r < CR_R; ++r) {
      const float x = P[o + (size_t)r * Mc];
      gP[o + (size_t)r * Mc] = ((bits >> r) & 1u) ? -g * w[r] * sigmoidf(-x) : g * sigmoidf(x);
    }
  }
}

// ---------------------------------------------------------------- labels: _downsample_label
__global__ void __launch_bounds__(64)
crp_downsample_kernel(const uint8_t* __restrict__ labels, uint8_t* __restrict__ out, int Y, int Z, int ds, double empty_t) {
  __shared__ int hist[256];
  const int lane = threadIdx.x;
  const int Zs = Z / ds, Ys = Y / ds;
  const int o = blockIdx.x;
  const int oz = o % Zs, oy = (o / Zs) % Ys, ox = o / (Zs * Ys);
  for (int i = lane; i < 256; i += 64) hist[i] = 0;
  __syncthreads();
  const int n = ds * ds * ds;
  for (int t = lane; t < n; t += 64) {
    const int dz = t % ds, dy = (t / ds) % ds, dx = t / (ds * ds);
    atomicAdd(&hist[labels[((size_t)(ox * ds + dx) * Y + oy * ds + dy) * Z + oz * ds + dz]], 1);
  }
  __syncthreads();
  // count * 256 + (255 - id) of the best class 1 .. 254: the larger count wins, then the lower id
  int best = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int id = lane * 4 + q;
    if (id >= 1 && id <= 254) {
      const int key = hist[id] * 256 + (255 - id);
      best = key > best ? key : best;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int t = __shfl_xor(best, off, 64);
    best = t > best ? t : best;
  }
  if (lane == 0) {
    const int z0 = hist[0], z255 = hist[255];
    int v;
    if ((double)(z0 + z255) > empty_t)
      v = z0 > z255 ? 0 : 255;
    else
      v = 255 - (best & 255);
    out[o] = (uint8_t)v;
  }
}

// ---------------------------------------------------------------- the GEMM of the gather and its two gradients
constexpr int GB = 128;                      // tile rows = tile columns
constexpr int GK = 16;                       // k per stage
constexpr int GS = GB + 4;                   // LDS row stride (floats): rows stay 16-byte aligned, k and k + 1 fall into other banks

// Two of the 512 float4 of a GB x GK operand tile per thread.  KC: element (x, k) sits at src[x * ld + k] (k contiguous: the tile
// is transposed on its way into LDS), otherwise at src[k * ld + x].  Out-of-range elements are zero AFTER the sigmoid.
template <bool KC, bool SIG>
__device__ __forceinline__ void tile_fetch(const float* __restrict__ src, long ld, int x0, int xmax, int k0, int kmax, int tid,
                                           float4 (&reg)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int f = tid + CR_T * j;
    const int x = KC ? (f >> 2) : ((f & 31) << 2), k = KC ? ((f & 3) << 2) : (f >> 5);
    const float* p = src + (KC ? (long)(x0 + x) * ld + k0 + k : (long)(k0 + k) * ld + x0 + x);
    const bool line = KC ? x0 + x < xmax : k0 + k < kmax;
    const int left = KC ? kmax - (k0 + k) : xmax - (x0 + x);
    const int nv = line ? (left < 0 ? 0 : (left > 4 ? 4 : left)) : 0;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (nv == 4 && (reinterpret_cast<size_t>(p) & 15) == 0) {
      v = *reinterpret_cast<const float4*>(p);
    } else {
      if (nv > 0) v.x = p[0];
      if (nv > 1) v.y = p[1];
      if (nv > 2) v.z = p[2];
      if (nv > 3) v.w = p[3];
    }
    if (SIG) {
      v.x = nv > 0 ? sigmoidf(v.x) : 0.0f;
      v.y = nv > 1 ? sigmoidf(v.y) : 0.0f;
      v.z = nv > 2 ? sigmoidf(v.z) : 0.0f;
      v.w = nv > 3 ? sigmoidf(v.w) : 0.0f;
    }
    reg[j] = v;
  }
}

template <bool KC>
__device__ __forceinline__ void tile_stash(float* __restrict__ tile, int tid, const float4 (&reg)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int f = tid + CR_T * j;
    if (KC) {
      const int x = f >> 2, k = (f & 3) << 2;
      tile[(k + 0) * GS + x] = reg[j].x;
      tile[(k + 1) * GS + x] = reg[j].y;
      tile[(k + 2) * GS + x] = reg[j].z;
      tile[(k + 3) * GS + x] = reg[j].w;
    } else {
      const int x = (f & 31) << 2, k = f >> 5;
      *reinterpret_cast<float4*>(&tile[k * GS + x]) = reg[j];
    }
  }
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GemmArgs {
  const float* A;                            // per-z / per-y strides below, in floats
  const float* Bm;
  float* C;
  const float* E;                            // EPI 1: the logits behind C (same indexing)
  long lda, ldb, ldc;
  long a_z, a_y, b_z, b_y, c_z, c_y;         // blockIdx.z = sample, blockIdx.y = relation (or slice)
  int M, N, K;                               // K: the whole reduction length
  int kchunk;                                // k range of a slice (blockIdx.y selects it when SPLIT): a multiple of GK
  int nslice;                                // SPLIT: slices per relation; y = r * nslice + s
  long a_s, b_s;                             // SPLIT: per-slice advance is kchunk along k
  int tiles_n;
};

// C[i][j] (+ epilogue) = sum_k A(i, k) B(k, j) on one 128 x 128 tile.  EPI 0: store; EPI 1: times s (1 - s), s = sigmoid(E[i][j]).
// SPLIT: blockIdx.y = r * nslice + s walks k in [s kchunk, (s + 1) kchunk) of relation r and stores to its own partial.
template <bool A_KC, bool A_SIG, bool B_KC, int EPI, bool SPLIT>
__global__ void __launch_bounds__(CR_T)
crp_gemm_kernel(const GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float As[GK * GS];
  __shared__ __attribute__((aligned(16))) float Bs[GK * GS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int m0 = (blockIdx.x / g.tiles_n) * GB, n0 = (blockIdx.x % g.tiles_n) * GB;
  const int z = blockIdx.z;
  int r = blockIdx.y, kbeg = 0, kend = g.K;
  if (SPLIT) {
    const int s = r % g.nslice;
    r /= g.nslice;
    kbeg = s * g.kchunk;
    kend = kbeg + g.kchunk < g.K ? kbeg + g.kchunk : g.K;
  }
  const float* A = g.A + z * g.a_z + r * g.a_y;
  const float* Bm = g.Bm + z * g.b_z + r * g.b_y;
  float* C = g.C + z * g.c_z + (long)blockIdx.y * g.c_y;
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.0f;
  float4 ra[2], rb[2];
  if (kbeg < kend) {
    tile_fetch<A_KC, A_SIG>(A, g.lda, m0, g.M, kbeg, kend, tid, ra);
    tile_fetch<B_KC, false>(Bm, g.ldb, n0, g.N, kbeg, kend, tid, rb);
  }
  for (int k0 = kbeg; k0 < kend; k0 += GK) {
    __syncthreads();                             // the previous stage has been read
    tile_stash<A_KC>(As, tid, ra);
    tile_stash<B_KC>(Bs, tid, rb);
    __syncthreads();
    if (k0 + GK < kend) {
      tile_fetch<A_KC, A_SIG>(A, g.lda, m0, g.M, k0 + GK, kend, tid, ra);
      tile_fetch<B_KC, false>(Bm, g.ldb, n0, g.N, k0 + GK, kend, tid, rb);
    }
#pragma unroll
    for (int kk = 0; kk < GK / 2; ++kk) {
      const int k = kk * 2 + (lane >> 5);
      float a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = As[k * GS + wm + t * 32 + (lane & 31)];
        b[t] = Bs[k * GS + wn + t * 32 + (lane & 31)];
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
  }
  const float* E = EPI == 1 ? g.E + z * g.c_z + (long)blockIdx.y * g.c_y : nullptr;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int j = n0 + wn + nt * 32 + (lane & 31);
      if (j >= g.N) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int i = m0 + wm + mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (i >= g.M) continue;
        float v = acc[mt][nt][q];
        if (EPI == 1) {
          const float s = sigmoidf(E[(long)i * g.ldc + j]);
          v *= s * (1.0f - s);
        }
        C[(long)i * g.ldc + j] = v;
      }
    }
}

// dst[i] = part[0][i] + part[1][i] + ... in that order
__global__ void __launch_bounds__(CR_T)
crp_slice_fold_kernel(const float* __restrict__ part, float* __restrict__ dst, long n, long stride, int nparts) {
  for (long i = (long)blockIdx.x * CR_T + threadIdx.x; i < n; i += (long)gridDim.x * CR_T) {
    float a = part[i];
    for (int p = 1; p < nparts; ++p) a += part[(size_t)p * stride + i];
    dst[i] = a;
  }
}

bool gather_ok(const ssbev_crp_gather_dims* d) {
  if (!d || d->B <= 0 || d->N <= 0 || d->Mc <= 0 || d->C2 <= 0 || d->R <= 0 || d->R > 16) return false;
  if (d->N >= (1 << 24) || d->Mc >= (1 << 24) || d->C2 >= (1 << 24) || d->B >= (1 << 16)) return false;
  if (d->ld_out < (long long)d->R * d->C2) return false;
  return (long long)d->B * d->N * (d->ld_out > (long long)d->R * d->Mc ? d->ld_out : (long long)d->R * d->Mc) < (1ll << 40);
}

// slices per relation of the dctx product and their length along n: 512 rows each, which fills the card at the model's shapes
// and keeps every fp32 accumulation chain as short as the forward product's (Mc = 512)
constexpr int GSLICE = 512;
static_assert(GSLICE % GK == 0, "a slice is a whole number of k stages");
void gather_slices(const ssbev_crp_gather_dims* d, int* nslice, int* kchunk) {
  *kchunk = GSLICE;
  *nslice = (d->N + GSLICE - 1) / GSLICE;
}

}  // namespace

extern "C" {

size_t ssbev_crp_loss_workspace(const ssbev_crp_dims* d) { return crp_ok(d) ? crp_plan(d).bytes : 0; }

int ssbev_crp_loss_fwd(const float* logits, const uint8_t* labels, float* loss, float* pos_weight, const ssbev_crp_dims* d, void* ws,
                       size_t ws_bytes, ssbev_stream_t stream) {
  if (!crp_ok(d) || !logits || !labels || !loss || !pos_weight || !ws) return SSBEV_EINVAL;
  const CrPlan p = crp_plan(d);
  if (ws_bytes < p.bytes) return SSBEV_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(crp_loss_accum_kernel, dim3(p.mblk, p.nblk, d->B), dim3(CR_T), 0, st, logits, labels, part, p.N, p.Mc, d->Y,
                     d->Z);
  hipLaunchKernelGGL(crp_loss_final_kernel, dim3(1), dim3(CR_T), 0, st, part, (long)p.nparts, (double)d->B * p.N * p.Mc, loss,
                     pos_weight);
  return ssbev_launch_status();
}

int ssbev_crp_loss_bwd(const float* logits, const uint8_t* labels, const float* pos_weight, const float* grad_out,
                       float* grad_logits, const ssbev_crp_dims* d, ssbev_stream_t stream) {
  if (!crp_ok(d) || !logits || !labels || !pos_weight || !grad_out || !grad_logits) return SSBEV_EINVAL;
  const CrPlan p = crp_plan(d);
  const double count = (double)CR_R * d->B * p.N * p.Mc;
  hipLaunchKernelGGL(crp_loss_bwd_kernel, dim3(p.mblk, p.nblk, d->B), dim3(CR_T), 0, as_stream(stream), logits, labels, pos_weight,
                     grad_out, grad_logits, p.N, p.Mc, d->Y, d->Z, (float)(1.0 / count));
  return ssbev_launch_status();
}

int ssbev_label_downsample(const uint8_t* labels, uint8_t* out, int X, int Y, int Z, int downscale, ssbev_stream_t stream) {
  if (!labels || !out || X <= 0 || Y <= 0 || Z <= 0 || downscale < 1 || downscale > CR_MAX_DS) return SSBEV_EINVAL;
  if (X % downscale || Y % downscale || Z % downscale) return SSBEV_EINVAL;
  if ((long long)X * Y * Z >= (1ll << 31)) return SSBEV_EINVAL;
  const int ds = downscale;
  const double empty_t = 0.95 * ds * ds * ds;        // the reference's expression, in double
  const long long nout = (long long)(X / ds) * (Y / ds) * (Z / ds);
  hipLaunchKernelGGL(crp_downsample_kernel, dim3((unsigned)nout), dim3(64), 0, as_stream(stream), labels, out, Y, Z, ds, empty_t);
  return ssbev_launch_status();
}

int ssbev_crp_gather_fwd(const float* logits, const float* context, float* out, const ssbev_crp_gather_dims* d,
                         ssbev_stream_t stream) {
  if (!gather_ok(d) || !logits || !context || !out) return SSBEV_EINVAL;
  GemmArgs g = {};
  const long ldp = (long)d->R * d->Mc;
  g.A = logits;  g.lda = ldp;      g.a_z = (long)d->N * ldp;          g.a_y = d->Mc;
  g.Bm = context; g.ldb = d->C2;   g.b_z = (long)d->Mc * d->C2;       g.b_y = 0;
  g.C = out;     g.ldc = d->ld_out; g.c_z = (long)d->N * d->ld_out;   g.c_y = d->C2;
  g.M = d->N; g.N = d->C2; g.K = d->Mc;
  g.tiles_n = cdiv(d->C2, GB);
  const dim3 grid(cdiv(d->N, GB) * g.tiles_n, d->R, d->B);
  hipLaunchKernelGGL((crp_gemm_kernel<true, true, false, 0, false>), grid, dim3(CR_T), 0, as_stream(stream), g);
  return ssbev_launch_status();
}

size_t ssbev_crp_gather_bwd_workspace(const ssbev_crp_gather_dims* d) {
  if (!gather_ok(d)) return 0;
  int ns, chunk;
  gather_slices(d, &ns, &chunk);
  return ws_align256((size_t)d->R * ns * d->B * d->Mc * d->C2 * sizeof(float));
}

int ssbev_crp_gather_bwd(const float* logits, const float* context, const float* grad_out, float* grad_logits, float* grad_context,
                         const ssbev_crp_gather_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream) {
  if (!gather_ok(d) || !logits || !context || !grad_out || !grad_logits || !grad_context || !ws) return SSBEV_EINVAL;
  if (ws_bytes < ssbev_crp_gather_bwd_workspace(d)) return SSBEV_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const long ldp = (long)d->R * d->Mc;
  {  // dP[n][r][m] = (sum_c dOut[n][r C2 + c] ctx[m][c]) s (1 - s)
    GemmArgs g = {};
    g.A = grad_out; g.lda = d->ld_out; g.a_z = (long)d->N * d->ld_out; g.a_y = d->C2;
    g.Bm = context; g.ldb = d->C2;     g.b_z = (long)d->Mc * d->C2;    g.b_y = 0;
    g.C = grad_logits; g.E = logits; g.ldc = ldp; g.c_z = (long)d->N * ldp; g.c_y = d->Mc;
    g.M = d->N; g.N = d->Mc; g.K = d->C2;
    g.tiles_n = cdiv(d->Mc, GB);
    const dim3 grid(cdiv(d->N, GB) * g.tiles_n, d->R, d->B);
    hipLaunchKernelGGL((crp_gemm_kernel<true, false, true, 1, false>), grid, dim3(CR_T), 0, st, g);
  }
  {  // dctx[m][c] = sum_r sum_n s[n][r][m] dOut[n][r C2 + c]: slices of (r, n) into the workspace, then one fixed-order fold
    int ns, chunk;
    gather_slices(d, &ns, &chunk);
    float* part = static_cast<float*>(ws);
    const long per = (long)d->B * d->Mc * d->C2;       // one partial: [B][Mc][C2]
    GemmArgs g = {};
    g.A = logits;   g.lda = ldp;       g.a_z = (long)d->N * ldp;       g.a_y = d->Mc;
    g.Bm = grad_out; g.ldb = d->ld_out; g.b_z = (long)d->N * d->ld_out; g.b_y = d->C2;
    g.C = part;     g.ldc = d->C2;     g.c_z = (long)d->Mc * d->C2;    g.c_y = per;
    g.M = d->Mc; g.N = d->C2; g.K = d->N;
    g.kchunk = chunk; g.nslice = ns;
    g.tiles_n = cdiv(d->C2, GB);
    const dim3 grid(cdiv(d->Mc, GB) * g.tiles_n, d->R * ns, d->B);
    hipLaunchKernelGGL((crp_gemm_kernel<false, true, false, 0, true>), grid, dim3(CR_T), 0, st, g);
    hipLaunchKernelGGL(crp_slice_fold_kernel, dim3(voxel_grid(per)), dim3(CR_T), 0, st, part, grad_context, per, per, d->R * ns);
  }
  return ssbev_launch_status();
}

}  // extern "C"
