/* ssbev.h -- C ABI of libssbev_hip.so: MI355X (gfx950) kernels for the StereoScene hot path.
 *
 * Drop-in boundary.  Every entry point is what a maintainer of the
 * reference would bind (ctypes stub in INTEGRATION.md) in place of the third-party CUDA op or
 * the torch op sequence cited next to it.  Citations are relative to the reference checkout:
 *   VT  = projects/mmdet3d_plugin/occupancy/image2bev/ViewTransformerLSSVoxel.py
 *   BD  = projects/mmdet3d_plugin/occupancy/image2bev/ViewTransformerLSSBEVDepth.py
 *   ATT = projects/mmdet3d_plugin/occupancy/image2bev/attention.py
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - all data pointers are DEVICE pointers owned by the caller; the library never allocates or frees
 *     device memory, never synchronises and keeps no state that changes a result; work is enqueued
 *     on `stream` (a hipStream_t).  The one thing it remembers is host-side memoisation of launch
 *     PLANS (chunking searches of a few 10k iterations keyed by the problem shape: a mutex-guarded
 *     std::map in csrc/conv_mfma.hip, plan_wgrad_lds): same inputs -> same plan -> same bits, with
 *     or without the cache.
 *   - return 0 on success, <0 on error (no exceptions cross the boundary):
 *       SSBEV_EINVAL      bad dims / null pointer / unsupported configuration
 *       SSBEV_EWORKSPACE  workspace smaller than ssbev_*_workspace() says
 *       SSBEV_ELAUNCH     hipGetLastError() != hipSuccess after a launch
 *   - re-entrant and thread-safe (autograd backward threads call in concurrently).
 *   - "channels-last" below means the channel index is the fastest-moving one.
 */
#ifndef SSBEV_H
#define SSBEV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSBEV_OK 0
#define SSBEV_EINVAL (-1)
#define SSBEV_EWORKSPACE (-2)
#define SSBEV_ELAUNCH (-3)

typedef void* ssbev_stream_t; /* hipStream_t */

/* library / device identification */
int ssbev_version(void);                 /* 10000*major + 100*minor + patch */
const char* ssbev_build_arch(void);      /* "gfx950" */
/* The library reads its SSBEV_* environment switches once per process (first use) and answers from a table afterwards: no
 * getenv on the launch path.  A host that changes a switch later (tests do) calls this to have it read again; not to be called
 * while other threads are inside the library. */
void ssbev_env_refresh(void);

/* ------------------------------------------------------------------------------------------
 * Frustum -> voxel scatter  (replaces VT:432-476 `voxel_pooling` + mmdet3d.ops.bev_pool, VT:473)
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int B;            /* batch                                                        */
  int P;            /* points per batch element (= N*D*fH*fW)                        */
  int C;            /* channels                                                      */
  int nx, ny, nz;   /* voxel grid of the LSS volume (e.g. 128,128,16)                */
  float origin[3];  /* fp32( bx - dx/2 ), computed by the caller in fp32 (VT:441)    */
  float dx[3];      /* voxel size                                                    */
} ssbev_pool_dims;

/* VT:441-451.  geom[B*P,3] fp32 -> vox[B*P] int32: linear voxel ((b*nx+ix)*ny+iy)*nz+iz, or -1
 * if the point is dropped.  idx3 (int32 [B*P,3], may be NULL) receives (ix,iy,iz) =
 * trunc_toward_zero((geom - origin)/dx) saturated to int32.  Bit-exact w.r.t. the fp32
 * subtract / IEEE divide / truncate sequence of the reference. */
int ssbev_voxel_index(const float* geom, int32_t* vox, int32_t* idx3, const ssbev_pool_dims* d,
                      ssbev_stream_t stream);

/* mmdet3d.ops.bev_pool's coords[n,4] = (ix,iy,iz,b) (int32) -> vox[n] (same linearisation). */
int ssbev_coords_to_vox(const int32_t* coords, int n, int32_t* vox, const ssbev_pool_dims* d,
                        ssbev_stream_t stream);

/* Frustum points -> ego frame: the per-point part of get_geometry (ViewTransformerLSSBEVDepth.py:123-156) in one kernel,
 *   p = frustum[d,h,w,:] - t0[b,n];  p = m1[b,n] p;  p = (p.x p.z, p.y p.z, p.z);  p -= t2[b,n] (if given);
 *   p = m2[b,n] p + tr[b,n];  p = m3[b] p (+ t3[b] if given)
 * with m1 = inv(post_rots), t0 = post_trans, m2 = rots inv(intrins), t2 = intrins[:3,3] (4-column intrinsics), tr = trans,
 * m3 / t3 = the BEV augmentation; all row-major fp32.  Separately rounded multiplies and adds in the reference's order: the
 * points (and the voxel indices of ssbev_voxel_index) are bit-identical to the tensor expression.  geom[B,N,D,H,W,3]. */
typedef struct { int B, N, D, H, W; } ssbev_geom_dims;
int ssbev_frustum_geometry(const float* frustum, const float* m1, const float* t0, const float* m2, const float* t2,
                           const float* tr, const float* m3, const float* t3, float* geom, const ssbev_geom_dims* d,
                           ssbev_stream_t stream);

/* CSR build: starts[NV+1], order[n] with NV = B*nx*ny*nz.  Points of voxel v are
 * order[starts[v] .. starts[v+1]) in ASCENDING point index (the canonical summation order,
 * = stable argsort by rank in the upstream op).  Entries with vox<0 (or >= NV) are skipped: order[] holds starts[NV] ids,
 * its tail is left untouched.  Own two-level counting sort (csrc/voxel_pool.hip, "CSR build"): a stable partition by the
 * high digit of the voxel id, then one wavefront per 2^lo-voxel bucket that counts, scans (= starts) and places; five
 * launches for NV <= 2^22, no device-wide library sort.  SSBEV_POOL_MAX_DIGIT_BITS (2..11) narrows the digit (tests). */
size_t ssbev_pool_prepare_workspace(int n_points, const ssbev_pool_dims* d);
/* ... 2: additionally long_list[ssbev_pool_long_list_elems(n)] (nullable): long_list[0] = number of voxels with more than 32
 * points, long_list[1 ..] their ids in no particular order -- the work list of ssbev_lift_splat_fwd2's long-list waves. */
size_t ssbev_pool_long_list_elems(int n_points);
int ssbev_pool_prepare2(const int32_t* vox, int n_points, int32_t* starts, int32_t* order, int32_t* long_list,
                        const ssbev_pool_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);
int ssbev_pool_prepare(const int32_t* vox, int n_points, int32_t* starts, int32_t* order,
                       const ssbev_pool_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);

/* Drop-in for mmdet3d.ops.bev_pool forward/backward (VT:473).  feats[n,C] fp32 ->
 * out[B,nx,ny,nz,C] (channels-last; the reference's [B,C,nz,nx,ny].permute(0,1,3,4,2) is a
 * stride view of it).  Sequential fp32 sums in canonical order -> bit-reproducible. */
int ssbev_bev_pool_fwd(const float* feats, const int32_t* starts, const int32_t* order, float* out,
                       const ssbev_pool_dims* d, ssbev_stream_t stream);
int ssbev_bev_pool_bwd(const float* grad_out, const int32_t* vox, int n_points, float* grad_feats,
                       const ssbev_pool_dims* d, ssbev_stream_t stream);

/* Fused Lift (VT:517-519) + Splat (VT:523): the [B,N,D,H,W,C] product is never materialised.
 * depth[B*P] fp32 (= depth_prob [B*N,D,fH,fW] contiguous), feat[B*N*HW, C] channels-last,
 * point p of batch b uses feature row  b*(P/D) + (p/(D*HW))*HW + p%HW.
 * out[B,nx,ny,nz,C].  Each product is rounded to fp32 before the sequential add, exactly as the
 * reference's materialised `volume` would be. */
typedef struct { int N, D, HW; } ssbev_lift_dims;
int ssbev_lift_splat_fwd(const float* depth, const float* feat, const int32_t* starts,
                         const int32_t* order, float* out, const ssbev_pool_dims* d,
                         const ssbev_lift_dims* l, ssbev_stream_t stream);
/* ... 2: with the long-voxel list of ssbev_pool_prepare2 (nullable = ssbev_lift_splat_fwd): the lists of more than 32 points are
 * summed by dedicated whole-wave workgroups, the short ones four voxels per wave; same sums in the same order. */
int ssbev_lift_splat_fwd2(const float* depth, const float* feat, const int32_t* starts, const int32_t* order,
                          const int32_t* long_list, float* out, const ssbev_pool_dims* d, const ssbev_lift_dims* l,
                          ssbev_stream_t stream);
int ssbev_lift_splat_bwd(const float* grad_out, const float* depth, const float* feat,
                         const int32_t* vox, float* grad_depth, float* grad_feat,
                         const ssbev_pool_dims* d, const ssbev_lift_dims* l, ssbev_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Stereo plane-sweep cost volume: group-wise correlation fused with the disparity->depth
 * resample (replaces VT:104-114 `build_gwc_volume` + VT:128-156 `warp`).
 * left/right [B,H,W,C] channels-last fp32, calib[B] fp32 (= fx * baseline),
 * vol [B,D,H,W,G] channels-last (logical [B,G,D,H,W]).  align_corners selects the grid_sample
 * convention of VT:151-154 (0 = as-trained under torch 1.10.1, 1 = torch >= 1.3 literal).
 * ------------------------------------------------------------------------------------------ */
typedef struct { int B, C, G, D, H, W; float down; int align_corners; } ssbev_gwc_dims;
int ssbev_gwc_warp_fwd(const float* left, const float* right, const float* calib, float* vol,
                       const ssbev_gwc_dims* d, ssbev_stream_t stream);
int ssbev_gwc_warp_bwd(const float* grad_vol, const float* left, const float* right,
                       const float* calib, float* grad_left, float* grad_right,
                       const ssbev_gwc_dims* d, ssbev_stream_t stream);
/* Same gradients from ONE read of grad_vol (both views in one launch; plane chunks write partial rows into the
 * caller-owned workspace and are summed in chunk order: deterministic, no atomics).  Falls back to the two-launch
 * kernels above for shapes it does not cover (G % 4 != 0, 64 % G != 0, rows wider than its register plan). */
size_t ssbev_gwc_warp_bwd_workspace(const ssbev_gwc_dims* d);
int ssbev_gwc_warp_bwd_fused(const float* grad_vol, const float* left, const float* right,
                             const float* calib, float* grad_left, float* grad_right,
                             const ssbev_gwc_dims* d, void* workspace, size_t ws_bytes, ssbev_stream_t stream);
/* Host-side plan query (since ssbev_version() 116; no device work): the kernel, block, plane chunks and dynamic LDS a launch of
 * these dims uses, from the plan functions the launchers and ssbev_gwc_warp_bwd_workspace themselves read.  SSBEV_EINVAL for a
 * NULL argument and for dims every entry point refuses (C % G, C % 4, a group width outside 1 / 2 / 4 / 8, down != 1); otherwise
 * SSBEV_OK, and *_rc is what the entry point answers for these dims before anything is launched (SSBEV_OK, or SSBEV_EINVAL
 * when no kernel fits the row into 160 KB of LDS: the other fields of that group are 0 then).
 *   fwd_kernel: 1 = gwc_warp_fwd_kernel (a row per workgroup, 16-plane blocks: fwd_start holds multiples of 16 and is filled
 *               for up to SSBEV_GWC_MAX_CHUNKS blocks), 4 = gwc_warp_fwd4_kernel, 5 = gwc_warp_fwd5_kernel.  fwd_px = pixels
 *               of a tile (5) / of a pass over the row (4) / the row (1); fwd_tiles = tiles per row (1 for kernels 1 and 4).
 *   bwd_kernel (ssbev_gwc_warp_bwd_fused): 1 = the two launches of gwc_warp_bwd_kernel (no plane chunks: one chunk [0, D);
 *               bwd_threads is the block of each, 32-pixel tiles), 2 = gwc_warp_bwd2_kernel, 3 = gwc_warp_bwd3_kernel.
 *   direct_* : ssbev_gwc_warp_bwd, always the two launches.
 * Chunk c covers the planes [start[c], start[c + 1]). */
#define SSBEV_GWC_MAX_CHUNKS 48
typedef struct {
  int fwd_rc, fwd_kernel, fwd_threads, fwd_px, fwd_tiles, fwd_nchunks;
  int fwd_start[SSBEV_GWC_MAX_CHUNKS + 1];
  size_t fwd_lds;
  int bwd_rc, bwd_kernel, bwd_threads, bwd_nchunks;
  int bwd_start[SSBEV_GWC_MAX_CHUNKS + 1];
  size_t bwd_lds;
  size_t bwd_workspace;          /* bytes, what ssbev_gwc_warp_bwd_workspace returns: 2 nchunks B H W C floats, 0 for one chunk */
  int direct_rc, direct_threads;
  size_t direct_lds;
} ssbev_gwc_plan;
int ssbev_gwc_plan_query(const ssbev_gwc_dims* d, ssbev_gwc_plan* out);

/* ------------------------------------------------------------------------------------------
 * Dense N-d convolution family on MFMA (implicit GEMM, no im2col), channels-last fp32.
 * Replaces the ATen/cuDNN conv3d / conv_transpose3d / conv2d calls behind VT:66-88,167-187,
 * VT:239-241, ATT:94-110, resnet3d.py:18-32, second_fpn_3d.py:53-69, occhead.py:100-107.
 *   x   [B, Di, Hi, Wi, Cin]     (2-D convs: Di = 1, kd = 1)
 *   y   [B, Do, Ho, Wo, Cout]
 *   w   packed by ssbev_conv_pack_weight (layout private to the library)
 * transposed = 0: y[o] = sum_k w[k] x[o*stride - pad + k*dil]
 * transposed = 1: y[o] = sum_k w[k] x[(o + pad - k)/stride]  (taps where divisible)
 * The MFMA used is v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int B, Cin, Cout;
  int Di, Hi, Wi;
  int Do, Ho, Wo;
  int kd, kh, kw;
  int sd, sh, sw;
  int pd, ph, pw;
  int dd, dh, dw;      /* dilation */
  int transposed;
  int relu;            /* fused epilogue: y = max(y,0) after bias                        */
  int accumulate;      /* y += result (used for residual / split accumulations)          */
  int tile_hint;       /* 0 = library heuristic; MT*100+NT*10+QU forces a register tiling  */
  int precision;       /* 0 = fp32 MFMA (exact fp32 products, the parity contract);
                        * 1 = forward / data gradient round their operands to bf16 in registers (nearest even) and use
                        *     v_mfma_f32_32x32x16_bf16 with fp32 accumulation (BASELINE configs[3]); tensors in memory
                        *     stay fp32, the weight gradient kernels stay on the fp32 MFMA;
                        * 2 = bf16 STORAGE (round 4; the configs[3] path proper, csrc/conv_bf16.hip): the source tensor (x in
                        *     ssbev_conv_fwd_bf16, gy in ssbev_conv_bwd_data_bf16; both in ssbev_conv_bwd_weight_bf16) AND the
                        *     result (y / gx) are bf16 channels-last tensors (uint16_t bit patterns), the packed
                        *     weights hold bf16 operands, accumulation is fp32, gw is fp32.  Needs Cin % 8 == 0 (and
                        *     Cout % 8 == 0 wherever the Cout-channel tensor is a source); bias stays fp32.  Round 5: modes 2 / 3
                        *     are served by the typed *_bf16 entry points ONLY; ssbev_conv_fwd / _bwd_data / _bwd_weight
                        *     answer SSBEV_EINVAL for them (and the *_bf16 ones for precision 0 / 1): a precision value that
                        *     does not match the tensors cannot be passed silently any more;
                        * 3 = as 2 with an fp32 RESULT (the layer in front of an fp32 island, e.g. the logits conv)
                        *     ssbev_conv_kernel_class answers, for these modes: 16 generic gather (conv_gather16_kernel), 17
                        *     LDS-ring tap kernel (<= 32 channels, conv_tap16_kernel), 19 LDS-ring implicit GEMM for the wide
                        *     stride-1 3x3x3 layers (conv_wide16_kernel); mode 2: 18 generic weight gradient (wgrad16_kernel),
                        *     20 LDS-ring weight gradient (wgrad_ring16_kernel)                                       */
} ssbev_conv_dims;

/* weight packing: src is the torch layout  conv: [Cout,Cin,kd,kh,kw]  deconv: [Cin,Cout,kd,kh,kw]
 * mode 0: forward operand;  mode 1: operand of the data-gradient (channels swapped, taps flipped) */
size_t ssbev_conv_packed_weight_elems(const ssbev_conv_dims* d);
/* which kernel family ssbev_conv_fwd (mode 0) / ssbev_conv_bwd_data (mode 1) dispatches this problem to -- for FLOP
 * accounting in profilers (bench.py): 0 = generic gather kernels, 1 = conv_tap_kernel, 2 = conv_taph_kernel (Winograd
 * F(2,3) along h inside the kernel: executes 2/3 of the operator's multiply-adds), 3 = conv_thin_kernel, 4 =
 * conv_thinin_kernel (1 / 2 / 4 -> 32 channels: the K-role tensor is taken UNPADDED, Cin % 4 is not required),
 * 5 = a 32 -> 1 / 2 / 4 channel problem for which the two-pass ssbev_conv_thin_* entry points below are available
 * (ssbev_conv_fwd / _bwd_data themselves run such a problem on class 3 or 0); mode 2 asks about ssbev_conv_bwd_weight:
 * 6 = wgrad_thinside_kernel (32 <-> 1 / 2 / 4 channels; x and gy are taken UNPADDED), 0 = the other weight-gradient
 * kernels; 7 / 8 = the stride-2 "down" / "up" gathers on conv_tap2_kernel / conv_tap2up_kernel; 9 = conv_tapdh_kernel
 * (round 4: Winograd F(2,3) along d AND h inside the kernel, even D and H: executes 4/9 of the operator's multiply-adds;
 * SSBEV_TAPDH=0 or tile_hint 4 keeps class 2); < 0 = error.  The weight gradient of a class-9 problem runs on
 * wgrad_tapdh_kernel (same transform domain; SSBEV_WGRAD_DH=0 or tile_hint 4 / 5 / 6 / 7 keep wgrad_lds_kernel);
 * 10 = conv_pw32_kernel (1x1x1 stride-1 layers with <= 32 channels on both sides: an HBM stream through per-wave LDS tiles;
 * SSBEV_PW32=0 or tile_hint 8 keep the generic gather kernel); 11 = conv_igemm_kernel (round 5: LDS-staged implicit GEMM for the
 * strided / transposed / dilated layers whose gather source has a multiple of 32 channels and whose destination has >= 64;
 * SSBEV_IGEMM=0 or tile_hint >= 10 keep class 0); bf16 storage: 21 = conv_igemm16_kernel (SSBEV_IGEMM16=0 keeps 16). */
int ssbev_conv_kernel_class(const ssbev_conv_dims* d, int mode);
/* Host-side plan query (since ssbev_version() 105; no device work): the row-walking kernels give every workgroup a CHUNK of
 * consecutive row groups of one w-segment and walk them through an LDS ring.  Modes 0 / 1: the chunk length (row groups per
 * workgroup) the launch of this problem will use when ssbev_conv_kernel_class reports class 1, 2, 3, 7, 8, 9 or 17; a row
 * group is one row (classes 1, 3, 17), a row pair (2; 7: of the destination, 8: of the coarse grid) or a 2 x 2 (plane, row)
 * block (9).  Mode 2: the chunk length of wgrad_tapdh_kernel (2 x 2 blocks) when ssbev_conv_bwd_weight takes that kernel.
 * 0 in every other case.  The launchers call the same plan functions, so the answer is the launch's own. */
int ssbev_conv_chunk_groups(const ssbev_conv_dims* d, int mode);
/* Host-side plan query of the bf16 storage family (since ssbev_version() 113; no device work; csrc/conv_bf16.hip): the kernel,
 * template instance and launch geometry ssbev_conv_fwd_bf16 (mode 0), ssbev_conv_bwd_data_bf16 (mode 1) and
 * ssbev_conv_bwd_weight_bf16 (mode 2) use for these dims, from the plan functions the launchers themselves read.  Only the group
 * of the reported kernel class is filled in, every other field is 0.  SSBEV_EINVAL for a NULL argument, a mode outside 0 .. 2
 * and dims the entry point of that mode refuses (precision 0 / 1, channel counts, precision 3 in mode 2). */
typedef struct {
  int kernel;                     /* 16 .. 21, what ssbev_conv_kernel_class answers */
  int mt, nt;                     /* 16: conv_gather16_kernel<MT, NT>, 32-voxel x 32-channel tiles per wave */
  int bm, bn, bkc;                /* 21: conv_igemm16_kernel, workgroup tile (rows x columns) and source channels per stage */
  int ntl, nth, ntw, ntn;         /* 19: conv_wide16_kernel<NTL>; tiles along h (16 rows), w (16 voxels), the output channels */
  int nseg, gpc;                  /* 17: conv_tap16_kernel; 32-voxel w segments, rows per workgroup chunk */
  int mq, mp, th, tw;             /* 18: wgrad16_kernel<MQ, MP, TH, TW> */
  int chunk, nchunks;             /* 18: voxels per wave chunk, chunks (four per workgroup); 20: nchunks = tile chunks */
  int narrow, tpc, ncqt;          /* 20: wgrad_ring16_kernel<NARROW>, 8 x 16 tiles per chunk, 32-channel Q tiles */
  int64_t grid;                   /* workgroups of the main launch */
  size_t workspace;               /* mode 2: bytes, what ssbev_conv_bwd_weight_workspace returns; else 0 */
} ssbev_conv_bf16_plan;
int ssbev_conv_bf16_plan_query(const ssbev_conv_dims* d, int mode, ssbev_conv_bf16_plan* out);

/* 32 -> 1 / 2 / 4 channel 3x3x3 stride-1 "same" layers (the 32 -> 1 classifiers of the cost-volume stack,
 * ViewTransformerLSSVoxel.py:185-187, 239-241; mode 1: the data gradient of a 1 / 2 / 4 -> 32 layer) as one pass over the
 * wide tensor on the matrix pipe + one pass over 9 N partial planes in a caller-owned workspace
 * (ssbev_conv_thin_workspace bytes; 0 = not applicable).  Weights: torch layout -> ssbev_conv_thin_pack
 * (ssbev_conv_thin_packed_elems floats).  Tensors channels-last as for ssbev_conv_fwd; mode 0 applies bias / ReLU. */
size_t ssbev_conv_thin_workspace(const ssbev_conv_dims* d, int mode);
size_t ssbev_conv_thin_packed_elems(const ssbev_conv_dims* d, int mode);
int ssbev_conv_thin_pack(const float* w_src, float* w_packed, const ssbev_conv_dims* d, int mode, ssbev_stream_t stream);
int ssbev_conv_thin_run(const float* x, const float* w_packed, const float* bias, float* y, const ssbev_conv_dims* d,
                        int mode, void* workspace, size_t ws_bytes, ssbev_stream_t stream);
int ssbev_conv_pack_weight(const float* w_src, float* w_packed, const ssbev_conv_dims* d, int mode,
                           ssbev_stream_t stream);
int ssbev_conv_fwd(const float* x, const float* w_packed, const float* bias, float* y,
                   const ssbev_conv_dims* d, ssbev_stream_t stream);
/* bf16 storage (precision 2: y / gx are uint16_t bf16 tensors; 3: fp32 results, forward / data gradient only); pack the
 * weights with ssbev_conv_pack_weight under the same dims; workspace of the weight gradient from
 * ssbev_conv_bwd_weight_workspace under the same dims */
int ssbev_conv_fwd_bf16(const uint16_t* x, const float* w_packed, const float* bias, void* y,
                        const ssbev_conv_dims* d, ssbev_stream_t stream);
int ssbev_conv_bwd_data_bf16(const uint16_t* gy, const float* w_packed_t, void* gx,
                             const ssbev_conv_dims* d, ssbev_stream_t stream);
int ssbev_conv_bwd_weight_bf16(const uint16_t* x, const uint16_t* gy, float* gw, const ssbev_conv_dims* d,
                               void* ws, size_t ws_bytes, ssbev_stream_t stream);
/* data gradient: gx from gy with weights packed in mode 1 (d describes the FORWARD problem) */
int ssbev_conv_bwd_data(const float* gy, const float* w_packed_t, float* gx,
                        const ssbev_conv_dims* d, ssbev_stream_t stream);
/* weight gradient in the torch layout of w_src; ws from ssbev_conv_bwd_weight_workspace */
size_t ssbev_conv_bwd_weight_workspace(const ssbev_conv_dims* d);
int ssbev_conv_bwd_weight(const float* x, const float* gy, float* gw, const ssbev_conv_dims* d,
                          void* ws, size_t ws_bytes, ssbev_stream_t stream);
/* Host-side plan query of the weight gradient (since ssbev_version() 123; no device work): the kind ssbev_conv_bwd_weight takes for these dims, the partial
 * slabs [nchunks][taps][Cq][Cp] it leaves at the start of the workspace, how they are folded, and the launch numbers of that kind,
 * all from the functions the launch itself reads.  Only the group of the reported kind is filled in, every other field is 0
 * (kind 0, bf16 storage: `kind` and `workspace` only; ssbev_conv_bf16_plan_query describes that launch).  SSBEV_EINVAL for a
 * NULL argument or dims no entry point takes. */
typedef struct {
  int kind;                       /* 0 bf16 storage, 1 thin side (wgrad_thinside_kernel), 2 thin (wgrad_thin_kernel), 3 pointwise
                                   * (wgrad_1x1_kernel), 4 F(2,3) x F(2,3) ring walk (wgrad_tapdh_kernel), 5 LDS-staged
                                   * (wgrad_lds_kernel), 6 channels-first (wgrad_cf_kernel), 7 direct (wgrad_kernel) */
  int nchunks, taps, Cq, Cp;      /* slabs handed to the fold (5: workgroup chunks x ksplit), taps per slab (4: the 48 of the
                                   * transform domain), Q (tap side) and P (coarse-grid side) channels */
  int two_stage, nsl, per;        /* kinds 2 .. 7: wgrad_reduce_stage_kernel runs first, over nsl slices of `per` slabs (the last
                                   * slice may be shorter); 0 0 0 when it does not */
  int final;                      /* kinds 2 .. 7: 0 = wgrad_reduce_kernel, 1 = wgrad_reduce_tiled_kernel (1: its own fold, 0) */
  int cfg, Wseg, RG, nseg, gpc, nranges, ksplit;   /* 5: <MQB, MPB, KDB, KSPLIT, S> number, w-segment, P rows per step, segments,
                                   * row groups per chunk, chunk ranges, k split; 2 and 4: nseg and gpc of their row walks */
  int instance;                   /* 5: 0 plain, 1 F(2,3) along h, 2 the same with the unrolled NKS = 4 k-step count */
  int MQ, MP, TH, TW, chunk;      /* 3: wgrad_1x1_kernel<MQ, MP>, voxels per wave chunk; 6, 7: <MQ, MP, TH, TW>, voxels per chunk */
  int rows_per_wave, nt;          /* 1: rows per wave chunk, thin-side channel count */
  size_t workspace;               /* bytes, what ssbev_conv_bwd_weight_workspace returns */
} ssbev_conv_wgrad_plan;
int ssbev_conv_wgrad_plan_query(const ssbev_conv_dims* d, ssbev_conv_wgrad_plan* out);

/* Batched plain products of the bf16 storage mode (round 5): C[b][m][n] = sum_k A[b][m][k] B[b][k][n], A and (out_fp32 = 0) C
 * bf16 bit patterns, fp32 accumulation on v_mfma_f32_32x32x16_bf16 -- the Winograd frequency products (functional._WinoConv:
 * torch.bmm / rocBLAS in round 4).  B is fp32 [batch][K][N] (the transformed weights) and is packed once per call by
 * ssbev_gemm16_pack into ssbev_gemm16_packed_elems 16-bit elements (layout private to the library).  K % 32 == 0, N % 8 == 0. */
typedef struct { int M, N, K, batch; int out_fp32; } ssbev_gemm16_dims;
size_t ssbev_gemm16_packed_elems(const ssbev_gemm16_dims* d);
int ssbev_gemm16_pack(const float* B, uint16_t* packed, const ssbev_gemm16_dims* d, ssbev_stream_t stream);
int ssbev_gemm16_nn(const uint16_t* A, const uint16_t* packed, void* C, const ssbev_gemm16_dims* d, ssbev_stream_t stream);
/* C[b] = A[b]^T x B[b] over the row axis: A [batch][M][K], B [batch][M][N] (bf16, row-major) -> C [batch][K][N] fp32 -- the weight-
 * gradient frequency products (reference: the F.conv2d / F.conv3d weight gradients of the same layers).  K % 8 == 0, N % 8 == 0.
 * workspace: ssbev_gemm16_tn_workspace(d) floats, caller-owned (0 when the output tiles alone fill the chip; fixed-order sums). */
size_t ssbev_gemm16_tn_workspace(const ssbev_gemm16_dims* d);
int ssbev_gemm16_tn(const uint16_t* A, const uint16_t* B, float* C, const ssbev_gemm16_dims* d, float* workspace,
                    size_t workspace_elems, ssbev_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm / BatchNorm(train) over channels-last volumes with fused residual add + ReLU.
 * Replaces the ATen group_norm / batch_norm calls behind build_norm_layer (VT:31,45,69,83,86;
 * ATT:96,111; resnet3d.py:42-45; second_fpn_3d.py:68; occhead.py:104).
 *   x, y, residual [B, S, C] channels-last fp32; group g = channels [g*C/G, (g+1)*C/G)
 *   y = relu?( (x - mean[b,g]) * rstd[b,g] * gamma[c] + beta[c] + residual? )
 *   stats_given = 1: mean/rstd are inputs (eval-mode BatchNorm), otherwise outputs.
 * BatchNorm3d in training mode = the same call with G = C on the tensor viewed as [1, B*S, C].
 *   pre_act = 1: the normalised quantity is gelu(x) (exact erf form) -- the Conv3d -> GELU -> GroupNorm triples of CA3D
 *   (attention.py:94-111) without the two elementwise passes of the activation; backward returns the gradient w.r.t. x.
 * ------------------------------------------------------------------------------------------ */
/* ld_y / ld_gy (0 = dense, C floats): row stride of y in _fwd and of gy in _bwd when the operator writes / reads a channel slice
 * of a wider channels-last tensor -- the branches of a concatenation (SECONDFPN3D, second_fpn3d.py:113-116; ASPP) normalise
 * straight into their slice of the concatenated tensor and read their slice of its gradient, no torch.cat / slice copies.
 * Pass y / gy already offset to the first channel of the slice; multiples of 4, >= C.  A strided y/gy of a B > 1 per-sample
 * GroupNorm is addressed as [(b * S + s) * ld + c]. */
/* io_dtype (round 4, BASELINE configs[3]): 0 = the activation tensors x / residual / y (and gy / gx / gresidual) are fp32, 1 = they
 * hold bf16 bit patterns (pass the pointers cast to float*; ld_y / ld_gy then count bf16 elements).  Statistics, gamma / beta and their
 * gradients, and all arithmetic stay fp32.  ABI note: ld_y / ld_gy (round 3) and io_dtype (round 4) were appended to the struct; a
 * binding built against an older, shorter struct must be rebuilt -- the library reads all fields. */
typedef struct { int B, C, G; int64_t S; float eps; int relu; int stats_given; int pre_act; int64_t ld_y, ld_gy; int io_dtype; } ssbev_norm_dims;
size_t ssbev_groupnorm_workspace(const ssbev_norm_dims* d);
int ssbev_groupnorm_fwd(const float* x, const float* gamma, const float* beta, const float* residual,
                        float* y, float* mean, float* rstd, const ssbev_norm_dims* d, void* ws,
                        size_t ws_bytes, ssbev_stream_t stream);
/* gx (and gresidual = relu-masked gy, may be NULL), ggamma[C], gbeta[C]; y only needed when relu=1 */
int ssbev_groupnorm_bwd(const float* gy, const float* x, const float* y, const float* gamma,
                        const float* mean, const float* rstd, float* gx, float* gresidual,
                        float* ggamma, float* gbeta, const ssbev_norm_dims* d, void* ws,
                        size_t ws_bytes, ssbev_stream_t stream);
/* Variants that carry the fused ReLU's sign pattern as a bit mask instead of re-reading y in backward (2 of the 8 tensor
 * passes of a normalisation with ReLU): relu_mask has ssbev_groupnorm_mask_words(d) 64-bit words; with T = float4 index of
 * an element quadruple, word (T / 64) * 4 + k, bit T % 64 = [component k of y is > 0].  Written by _fwd_mask when
 * d->relu = 1 (ignored otherwise), read by _bwd_mask. */
size_t ssbev_groupnorm_mask_words(const ssbev_norm_dims* d);
int ssbev_groupnorm_fwd_mask(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                             float* mean, float* rstd, uint64_t* relu_mask, const ssbev_norm_dims* d, void* ws,
                             size_t ws_bytes, ssbev_stream_t stream);
int ssbev_groupnorm_bwd_mask(const float* gy, const float* x, const uint64_t* relu_mask, const float* gamma,
                             const float* mean, const float* rstd, float* gx, float* gresidual, float* ggamma, float* gbeta,
                             const ssbev_norm_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);

/* BatchNorm running statistics inside the statistics finalize (round 5).
 *   running_mean / running_var (BatchNorm, G == C with the batch folded into S; NULL = none): the momentum update
 *                 r = (1 - momentum) r + momentum {mean, var * n / (n - 1)} of nn.BatchNorm in training mode, done by the
 *                 finalize kernel (ssbev_bn_update_running as a launch of its own otherwise); n = samples per channel.
 * _fwd_ext / _bwd_ext are ssbev_groupnorm_fwd_mask / _bwd_mask (relu_mask may be NULL when relu = 0; _bwd_ext takes y OR
 * relu_mask for a fused ReLU) with `ext` (may be NULL).
 * (Round 5 also carried a `sync` word here for a finalize-in-the-statistics-tail variant; measured slower, removed in round 6.) */
typedef struct { float* running_mean; float* running_var; float momentum; int64_t n; } ssbev_norm_ext;
int ssbev_groupnorm_fwd_ext(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                            float* mean, float* rstd, uint64_t* relu_mask, const ssbev_norm_dims* d,
                            const ssbev_norm_ext* ext, void* ws, size_t ws_bytes, ssbev_stream_t stream);
int ssbev_groupnorm_bwd_ext(const float* gy, const float* x, const float* y, const uint64_t* relu_mask, const float* gamma,
                            const float* mean, const float* rstd, float* gx, float* gresidual, float* ggamma, float* gbeta,
                            const ssbev_norm_dims* d, const ssbev_norm_ext* ext, void* ws, size_t ws_bytes,
                            ssbev_stream_t stream);

/* Two normalisations and their sum in one operator: y = relu?( N_a(xa) + N_b(xb) ), the tail of every hourglass level of
 * the cost-volume aggregation (ViewTransformerLSSVoxel.py:92-95: relu(BatchNorm3d(deconv) + GN(redir conv))).  Each side is a
 * per-sample GroupNorm (x_batch = 0: statistics [B][G]) or a normalisation over the batch (x_batch = 1: statistics [G], BatchNorm
 * when G == C).  The apply pass reads the two raw tensors once and writes the sum once; backward reads (gy, mask, xa, xb) twice
 * instead of eleven tensor passes for the two separate operators.  C % 4 == 0, C <= 1024; relu_mask as in ssbev_groupnorm_*_mask
 * (required when relu = 1).  Statistics are outputs of _fwd and inputs of _bwd. */
typedef struct { int B, C, Ga, Gb; int64_t S; float eps_a, eps_b; int relu; int a_batch, b_batch; int io_dtype; /* as in ssbev_norm_dims */ } ssbev_norm2_dims;
size_t ssbev_groupnorm2_workspace(const ssbev_norm2_dims* d);
int ssbev_groupnorm2_fwd(const float* xa, const float* gamma_a, const float* beta_a, float* mean_a, float* rstd_a,
                         const float* xb, const float* gamma_b, const float* beta_b, float* mean_b, float* rstd_b, float* y,
                         uint64_t* relu_mask, const ssbev_norm2_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);
int ssbev_groupnorm2_bwd(const float* gy, const uint64_t* relu_mask, const float* xa, const float* gamma_a, const float* mean_a,
                         const float* rstd_a, const float* xb, const float* gamma_b, const float* mean_b, const float* rstd_b,
                         float* gxa, float* gxb, float* ggamma_a, float* gbeta_a, float* ggamma_b, float* gbeta_b,
                         const ssbev_norm2_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);

/* as ssbev_norm_ext for the two-norm operator (running statistics per side, n = B * S) */
typedef struct { float* running_mean_a; float* running_var_a; float momentum_a;
                 float* running_mean_b; float* running_var_b; float momentum_b; } ssbev_norm2_ext;
int ssbev_groupnorm2_fwd_ext(const float* xa, const float* gamma_a, const float* beta_a, float* mean_a, float* rstd_a,
                             const float* xb, const float* gamma_b, const float* beta_b, float* mean_b, float* rstd_b, float* y,
                             uint64_t* relu_mask, const ssbev_norm2_dims* d, const ssbev_norm2_ext* ext, void* ws, size_t ws_bytes,
                             ssbev_stream_t stream);
int ssbev_groupnorm2_bwd_ext(const float* gy, const uint64_t* relu_mask, const float* xa, const float* gamma_a, const float* mean_a,
                             const float* rstd_a, const float* xb, const float* gamma_b, const float* mean_b, const float* rstd_b,
                             float* gxa, float* gxb, float* ggamma_a, float* gbeta_a, float* ggamma_b, float* gbeta_b,
                             const ssbev_norm2_dims* d, const ssbev_norm2_ext* ext, void* ws, size_t ws_bytes,
                             ssbev_stream_t stream);

/* Host-side plan query (since ssbev_version() 107; no device work): the geometry a launch of these dims runs with, from the
 * functions the launchers and the *_workspace queries themselves call.  Exactly one of `d` (ssbev_groupnorm_*) and `d2`
 * (ssbev_groupnorm2_*) is given.  16-byte bf16 lanes need 16-byte aligned tensors; the entry points look at their pointers,
 * the query takes `aligned16` (non-zero: every tensor pointer of the call is 16-byte aligned) in their place.  SSBEV_EINVAL for
 * dims the entry points refuse.
 * The statistics kernels run a grid of chunks x B x slabs workgroups of 256 threads: a workgroup covers `chunk_len` voxels (the
 * last chunk of a sample what is left) and a slab of `slab_q` lanes of `vw` channels (the last slab what is left), 256 / lanes
 * voxels per trip.  The apply kernels run `blocks` workgroups of 256 threads, one lane of 4 channels per thread and trip. */
typedef struct {
  int vw;              /* channels per lane of the statistics passes: 4, or 8 (bf16, C % 8 == 0, aligned rows) */
  int slab_q;          /* lanes per channel slab */
  int slabs;           /* channel slabs */
  int chunks;          /* voxel chunks per sample (a batch-statistics side of the two-norm operator: of the folded B * S voxels) */
  int64_t chunk_len;   /* voxels per chunk */
  int64_t blocks;      /* workgroups of the apply passes */
  int fixed;           /* 1: blocks * 256 is a multiple of C / 4, so a thread keeps its channels over its grid-stride trips */
  int chunks_b;        /* two-norm operator: chunks / chunk_len above are side a's forward statistics, these are side b's */
  int64_t chunk_len_b;
  int chunks2;         /* two-norm operator: chunks per sample and voxels per chunk of the backward partial sums (one slab) */
  int64_t chunk_len2;
} ssbev_groupnorm_plan;
int ssbev_groupnorm_plan_query(const ssbev_norm_dims* d, const ssbev_norm2_dims* d2, int aligned16, ssbev_groupnorm_plan* out);

/* ------------------------------------------------------------------------------------------
 * Trilinear x2 upsample (align_corners=False) of channels-last volumes, forward and gather-form
 * backward.  Replaces F.interpolate(..., mode='trilinear') at occhead.py:293-294 and
 * bevdepth_occupancy.py:293 (logits [B,20,128,128,16] -> [B,20,256,256,32]).
 *   x [B, D, H, W, C] -> y [B, 2D, 2H, 2W, C];  C % 4 == 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct { int B, D, H, W, C; } ssbev_upsample_dims;
int ssbev_trilinear2x_fwd(const float* x, float* y, const ssbev_upsample_dims* d, ssbev_stream_t stream);
int ssbev_trilinear2x_bwd(const float* gy, float* gx, const ssbev_upsample_dims* d, ssbev_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimiser step over one flat fp32 parameter buffer: global gradient L2 norm + fused AdamW with
 * clip-by-global-norm (the reference recipe, stereoscene.py:203-209: AdamW lr 1e-4 wd 0.01,
 * grad_clip max_norm 5).  torch.optim.AdamW semantics (decoupled decay, bias correction).
 * ------------------------------------------------------------------------------------------ */
typedef struct { float lr, beta1, beta2, eps, weight_decay, max_grad_norm; int step; } ssbev_adamw_cfg;
size_t ssbev_grad_norm_workspace(void);
int ssbev_grad_norm(const float* g, int64_t n, float* norm_out, void* ws, size_t ws_bytes,
                    ssbev_stream_t stream);
/* grad_norm: device pointer to the norm (may be NULL or max_grad_norm <= 0 to disable clipping) */
int ssbev_adamw_step(float* p, const float* g, float* m, float* v, int64_t n,
                     const ssbev_adamw_cfg* c, const float* grad_norm, ssbev_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused occupancy-head epilogue: x2 trilinear upsample + softmax + every reduction the SemanticKITTI
 * losses (CE_ssc / sem_scal / geo_scal, utils/semkitti.py:67-149) and the train-time metric
 * (occhead.py:345-359) need, in one pass over the coarse logits; nothing of the fine grid is stored.
 *   logits [B, D, H, W, 20] channels-last;  label [B, 2D, 2H, 2W] uint8 (255 = ignore);  class_weight[20]
 *   sums[ssbev_occ_loss_num_sums()] (double): ce_num, ce_den, M, sum_p[20], nom[20], cnt[20], conf[20][20]
 *   backward: coef[41] = dL/d{ce_num, sum_p[20], nom[20]}  ->  grad_logits [B, D, H, W, 20]
 * ------------------------------------------------------------------------------------------ */
typedef struct { int B, D, H, W, C; } ssbev_occloss_dims;
int ssbev_occ_loss_num_sums(void);
size_t ssbev_occ_loss_workspace(const ssbev_occloss_dims* d);
int ssbev_occ_loss_fwd(const float* logits, const uint8_t* label, const float* class_weight, double* sums,
                       const ssbev_occloss_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);
/* The elementwise shell of a BRI attention block (attention.py:45-86) around its six products, operands [B, D, T] with the token
 * axis contiguous; every scalar parameter is a DEVICE pointer to one float (the 1x1x1 single-channel convolutions' weight / bias,
 * gamma).  Forward: Q = q wq + bq, K = kv wk + bk, Vc = (kv wv + bv) conf[b, t]  (pre);  y = gamma out + kv  (post).
 * Backward: post_bwd writes gout = gy gamma, per-chunk partial column sums delta_part[chunks][B*T] of gout * out (their sum over
 * the chunk axis is the softmax-backward row term) and partial sums of gy * out (-> d gamma); pre_bwd writes gq, gkv (gres = the
 * residual branch's gradient, added in), gconf_part[chunks][B*T] and part[..][6] = partial sums for d(wq, bq, wk, bk, wv, bv).
 * chunks = ssbev_bri_shell_chunks(); part arrays have chunks * ceil(B*T / 256) rows (doubles), summed by the caller. */
int ssbev_bri_shell_chunks(void);
int ssbev_bri_shell_pre_fwd(const float* q, const float* kv, const float* conf, const float* wq, const float* bq,
                            const float* wk, const float* bk, const float* wv, const float* bv, float* Q, float* K, float* Vc,
                            int B, int D, int T, ssbev_stream_t stream);
int ssbev_bri_shell_post_fwd(const float* out, const float* kv, const float* gamma, float* y, int B, int D, int T,
                             ssbev_stream_t stream);
int ssbev_bri_shell_post_bwd(const float* gy, const float* out, const float* gamma, float* gout, float* delta_part, double* part,
                             int B, int D, int T, ssbev_stream_t stream);
int ssbev_bri_shell_pre_bwd(const float* gQ, const float* gK, const float* gVc, const float* q, const float* kv, const float* conf,
                            const float* gres, const float* wq, const float* wk, const float* wv, const float* bv, float* gq,
                            float* gkv, float* gconf_part, double* part, int B, int D, int T, ssbev_stream_t stream);

/* The scalar algebra behind the sums in one launch: out5 (float) = w_ce * CE, w_sem * sem_scal, w_geo * geo_scal (occhead.py:
 * 291-361, semkitti.py:67-149), completion IoU, mean IoU over classes 1..19; jac[3][41] (double) = the Jacobian of the three
 * weighted losses w.r.t. (ce_num, sum_p[20], nom[20]) -- backward is jac^T times the three incoming scalars, which is the
 * `coef` of ssbev_occ_loss_bwd. */
int ssbev_occ_loss_tail(const double* sums, float w_ce, float w_sem, float w_geo, float* out5, double* jac,
                        ssbev_stream_t stream);
size_t ssbev_occ_loss_bwd_workspace(const ssbev_occloss_dims* d);
int ssbev_occ_loss_bwd(const float* logits, const uint8_t* label, const float* class_weight,
                       const float* coef, float* grad_logits, const ssbev_occloss_dims* d, void* ws,
                       size_t ws_bytes, ssbev_stream_t stream);

/* Soft-Dice and LGA-weighted voxel losses of the head (since version 114; occhead.py:331-343, utils/dice_loss.py:36-66,
 * utils/pal_loss.py).
 *
 * ssbev_occ_dice_tail: SoftDiceLossWithProb(p = 1) of the occupied probability 1 - p_0 against [t > 0] over the labelled voxels is
 * a function of four sums of ssbev_occ_loss_fwd:  inter = (M - cnt[0]) - (sum_p[0] - nom[0]),
 *   dice = 1 - (2 inter + smooth) / ((M - sum_p[0]) + (M - cnt[0]) + smooth).
 * One small launch: out1 (float, device) = dice, jac41 (double, device) = its Jacobian row over (ce_num, sum_p[20], nom[20]) (only
 * sum_p[0] and nom[0] are non-zero), which scaled by the incoming gradient is (part of) the `coef` of ssbev_occ_loss_bwd.
 * SSBEV_EINVAL on a NULL pointer.
 *
 * ssbev_lga_weights: lga2 [B, X, Y, Z] uint8 = twice PositionAwareLoss.get_lga(label) (the sum over the 20 class masks of the
 * 1-norm of torch.gradient), exact: per axis, with is(t) = [t < 20], an interior voxel adds is(t-) + is(t+) if its two neighbours
 * differ (its own label does not enter), the first and the last voxel add 2 (is(a) + is(b)) [a != b] of the end pair (the
 * one-sided difference); 0..12.  An ignored voxel (255) is in no class mask but is a neighbour that differs.  Neighbours never
 * cross a sample or a row.  SSBEV_EINVAL: NULL pointers, B < 1, an axis shorter than 2 (torch.gradient raises there too),
 * B X Y Z >= 2^31.
 *
 * ssbev_occ_lga_*: sum over the labelled voxels of w[t] (alpha + beta lga) (-log softmax(up(logits))[t]) over the sum of w[t], with
 * the tensors of ssbev_occ_loss_fwd plus lga2 on the label grid.  One grid-stride pass over the fine voxels, per-wave float sums
 * folded in wave order into per-workgroup double partials, a fixed-order fold: no float atomics, nothing read back, the same bits
 * on every run.  numden (2 doubles, device) = numerator, denominator; loss (float, device) = num / den, and 0 when den == 0 (the
 * reference divides 0 / 0).  Backward writes grad_out[0] / den * w[t] (alpha + beta lga) (p - onehot) per fine voxel (0 where
 * ignored or den == 0) into the workspace and pulls it back to the coarse grid with ssbev_trilinear2x_bwd.
 * SSBEV_EINVAL: NULL pointers, non-positive dims, C != 20, 20 x fine voxels >= 2^31;  SSBEV_EWORKSPACE: ws_bytes below the query.
 * The queries answer 0 for refused dims. */
int ssbev_occ_dice_tail(const double* sums, float smooth, float* out1, double* jac41, ssbev_stream_t stream);
int ssbev_lga_weights(const uint8_t* label, uint8_t* lga2, int B, int X, int Y, int Z, ssbev_stream_t stream);
size_t ssbev_occ_lga_workspace(const ssbev_occloss_dims* d);
int ssbev_occ_lga_fwd(const float* logits, const uint8_t* label, const uint8_t* lga2, const float* class_weight, float alpha,
                      float beta, double* numden, float* loss, const ssbev_occloss_dims* d, void* ws, size_t ws_bytes,
                      ssbev_stream_t stream);
size_t ssbev_occ_lga_bwd_workspace(const ssbev_occloss_dims* d);
int ssbev_occ_lga_bwd(const float* logits, const uint8_t* label, const uint8_t* lga2, const float* class_weight, float alpha,
                      float beta, const double* numden, const float* grad_out, float* grad_logits,
                      const ssbev_occloss_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);

/* ssbev_occ_predict (since version 103): the INFERENCE epilogue of the head in one pass over the coarse logits -- what the
 * reference does with F.interpolate (bevdepth_occupancy.py:293), torch.argmax + SSCMetrics (semantic_kitti_lss_dataset.py:
 * 231-287; apis/test.py:141-224) and the submission writer's argmax + learning_map_inv (apis/test.py:49-64), without the 168 MB
 * of up-sampled logits.
 *   logits    [B, D, H, W, 20] fp32 channels-last, 16-byte aligned (d->C must be 20)
 *   label     [B, 2D, 2H, 2W] uint8, 255 (any value >= 20) = ignore; optional, required by conf / n_ignored
 *   remap     HOST pointer to 20 uint16 (training id -> raw id, e.g. SemanticKITTI learning_map_inv), copied by the call;
 *             optional, required by raw
 *   pred      [B, 2D, 2H, 2W] uint8: argmax over the classes of the x2 trilinear up-sampled logits (align_corners=False); the
 *             interpolated values are those of ssbev_trilinear2x_fwd bit for bit (same taps, weight product and accumulation
 *             order) and ties go to the lowest class index, so pred == argmax(ssbev_trilinear2x_fwd(logits)) exactly
 *   raw       [B, 2D, 2H, 2W] uint16 = remap[pred] (the bytes of a SemanticKITTI .label file)
 *   conf      [B, 20, 20] int64, [gt][pred], PER SAMPLE, over the voxels whose label is not ignored
 *   n_ignored [B] int64: ignored voxels per sample
 * Every output is optional (NULL), at least one must be given.  Counts are integer sums (LDS atomics, per-block partials, one
 * reduce): exact and identical from run to run.  Non-finite logits: the result is unspecified.
 * SSBEV_EINVAL, before any pointer is touched: d NULL / non-positive dims / C != 20 / 8 D H W >= 2^31 / B > 65535, logits NULL,
 * all outputs NULL, conf or n_ignored without label (or without ws), raw without remap.  The workspace (needed for conf /
 * n_ignored only) is 0 for refused dims and grows with B. */
size_t ssbev_occ_predict_workspace(const ssbev_upsample_dims* d);
int ssbev_occ_predict(const float* logits, const uint8_t* label, const uint16_t* remap, uint8_t* pred, uint16_t* raw,
                      int64_t* conf, int64_t* n_ignored, const ssbev_upsample_dims* d, void* ws, size_t ws_bytes,
                      ssbev_stream_t stream);

/* Lovasz-softmax voxel loss (since version 104): lovasz_softmax(softmax(up(logits)), label, classes='present', per_image=False,
 * ignore) of the reference head (lovasz_softmax.py:21-33, 156-225), UNWEIGHTED, on a fused key / segmented-radix-sort / scan
 * path; the up-sampled logits and the probabilities are never written.
 *   dims      B, D, H, W: the LOGITS' grid; C == 20; ignore: label value that is skipped (255); upsample 1: the label grid is
 *             exactly [2D, 2H, 2W] and the logits are up-sampled trilinearly (align_corners=False), 0: labels on [D, H, W]
 *   logits    [B, D, H, W, 20] channels-last fp32;  label [B, D', H', W'] uint8
 *   loss      one float (device): mean over the classes present among the labelled voxels; 0 when no voxel is labelled
 *   dj        [B D' H' W'][20] float (device), kept by the caller for backward: dJ at the rank of voxel v in the descending
 *             sort of class c's errors; written for labelled voxels and present classes only, never read elsewhere
 *   counts    [ssbev_lovasz_num_counts()] int32 (device), kept for backward: labelled voxels per class [20], M, n_present
 *   backward  grad_logits [B, D, H, W, 20] = grad_out[0] * d loss / d logits (grad_out: one float on the device)
 * Nothing is read back to the host.  Ties in the errors keep voxel order (stable LSD sort, ballot ranking): every run gives
 * the same bits.  SSBEV_EINVAL before any device work: NULL pointers, non-positive dims, C != 20, upsample not 0 / 1,
 * 20 x voxels >= 2^31;  SSBEV_EWORKSPACE: ws_bytes below the query.  The queries answer 0 for refused dims. */
typedef struct { int B, D, H, W, C, ignore, upsample; } ssbev_lovasz_dims;
int ssbev_lovasz_num_counts(void);
size_t ssbev_lovasz_workspace(const ssbev_lovasz_dims* d);
int ssbev_lovasz_fwd(const float* logits, const uint8_t* label, float* loss, float* dj, int32_t* counts,
                     const ssbev_lovasz_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);
size_t ssbev_lovasz_bwd_workspace(const ssbev_lovasz_dims* d);
int ssbev_lovasz_bwd(const float* logits, const uint8_t* label, const float* dj, const int32_t* counts,
                     const float* grad_out, float* grad_logits, const ssbev_lovasz_dims* d, void* ws, size_t ws_bytes,
                     ssbev_stream_t stream);

/* OHEM cross-entropy voxel loss (since version 110): OHEM_CE_ssc_loss(up(logits), label, class_weight, top_k) of the reference
 * (utils/semkitti.py:151-185): l_v = w[t_v] * CE_v per labelled voxel; per sample the k_b = int(M_b * top_k) largest of its M_b
 * losses are kept; loss = sum(kept l) / max(sum of w[t] over the kept voxels, 1e-4), both sums over the batch.  No sort: the
 * losses are >= +0, so their fp32 bit patterns order like unsigned integers and a most-significant-digit-first radix select
 * finds the k_b-th largest exactly in four 8-bit histogram passes.  The up-sampled logits are never written.
 *   dims          ssbev_lovasz_dims' fields (B, D, H, W: the LOGITS' grid; C == 20; ignore; upsample 0 / 1) + top_k in (0, 1]
 *   logits        [B, D, H, W, 20] channels-last fp32;  label [B, D', H', W'] uint8 (a value >= 20 counts as ignored)
 *   class_weight  [20] float (device)
 *   loss          one float (device); 0 when no voxel is labelled or every k_b is 0
 *   mask          [B D' H' W'] one byte per voxel (device), kept by the caller for backward: 1 = in the selection
 *   inv_wsum      one float (device), kept for backward: 1 / max(sum of w[t] over the selection, 1e-4)
 *   backward      grad_logits [B, D, H, W, 20] = grad_out[0] * d loss / d logits (grad_out: one float on the device); the
 *                 divisor carries no gradient, as in the reference
 * k_b = (long long)((double)M_b * top_k) is computed on the device; nothing is read back to the host.  Losses equal to the
 * threshold are taken lowest flat voxel index first; integer atomics and fixed-order double sums only: every run gives the
 * same bits.  After ssbev_ohem_ce_fwd the first B D' H' W' words of ws hold the per-voxel losses as fp32 (0xFFFFFFFF for an
 * ignored voxel).  SSBEV_EINVAL before any device work: NULL pointers, non-positive dims, C != 20, upsample not 0 / 1, top_k
 * outside (0, 1], 20 x voxels >= 2^31;  SSBEV_EWORKSPACE: ws_bytes below the query.  The queries answer 0 for refused dims. */
typedef struct { int B, D, H, W, C, ignore, upsample; double top_k; } ssbev_ohem_dims;
size_t ssbev_ohem_ce_workspace(const ssbev_ohem_dims* d);
int ssbev_ohem_ce_fwd(const float* logits, const uint8_t* label, const float* class_weight, float* loss, uint8_t* mask,
                      float* inv_wsum, const ssbev_ohem_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);
size_t ssbev_ohem_ce_bwd_workspace(const ssbev_ohem_dims* d);
int ssbev_ohem_ce_bwd(const float* logits, const uint8_t* label, const float* class_weight, const uint8_t* mask,
                      const float* inv_wsum, const float* grad_out, float* grad_logits, const ssbev_ohem_dims* d, void* ws,
                      size_t ws_bytes, ssbev_stream_t stream);

/* Frustum-proportion voxel loss (since version 112): compute_frustum_dist_loss(up(logits), masks, dists) of the reference
 * (utils/semkitti.py:218-244) with the 64 disjoint bool masks of a sample held as ONE byte per voxel (the frustum id, 255 = none).
 * p = softmax over the classes; cum[f][c] = sum over the batch and the voxels with id f of p[c]; cnt[f][c] = sum over the batch of
 * dists[b][f][c]; a frustum counts if sum_c cum > 0 and sum_c cnt > 0; its term is sum over the classes with t_c != 0 of
 * t_c (log t_c - log q_c), t = cnt[f] / sum, q = cum[f] / sum; loss = sum of the terms / number of counted frusta, and 0 (the
 * reference divides 0 / 0) when no frustum counts.  The up-sampled logits are never written.
 *   dims      B, D, H, W: the LOGITS' grid; C == 20; F in 1..64 frusta; upsample 0 / 1 as in ssbev_ohem_dims
 *   logits    [B, D, H, W, 20] channels-last fp32;  ids [B, D', H', W'] uint8 (a value >= F names no frustum)
 *   dists     [B, F, 20] float (device)
 *   loss      one float (device)
 *   g         [F, 20] float (device), kept by the caller for backward: d loss / d cum
 *   backward  grad_logits [B, D, H, W, 20] = grad_out[0] * d loss / d logits (grad_out: one float on the device); dists carry no
 *             gradient
 * One pass over the fine voxels with per-wave row tables in LDS (a cross-lane sum per distinct id of the wave), per-workgroup
 * partial tables in double, fixed-order sums: no float atomics, nothing read back, every run gives the same bits.
 * SSBEV_EINVAL before any device work: NULL pointers, non-positive dims, C != 20, F outside 1..64, upsample not 0 / 1,
 * 20 x voxels >= 2^31;  SSBEV_EWORKSPACE: ws_bytes below the query.  The queries answer 0 for refused dims. */
typedef struct { int B, D, H, W, C, F, upsample; } ssbev_frustum_dims;
size_t ssbev_frustum_dist_workspace(const ssbev_frustum_dims* d);
int ssbev_frustum_dist_fwd(const float* logits, const uint8_t* ids, const float* dists, float* loss, float* g,
                           const ssbev_frustum_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);
size_t ssbev_frustum_dist_bwd_workspace(const ssbev_frustum_dims* d);
int ssbev_frustum_dist_bwd(const float* logits, const uint8_t* ids, const float* g, const float* grad_out, float* grad_logits,
                           const ssbev_frustum_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);
/* The loader step CreateRelationLabels (datasets/pipelines/voxel_labels.py:201-265 of the reference) on the device: the frustum id
 * of every voxel of a label grid and the class counts of every frustum.
 *   labels   [X, Y, Z] uint8 (device; a value >= 20 counts as unlabelled);  ids [X, Y, Z] uint8 (device): py * frustum_size + px,
 *            255 when the centre lies in no patch, at depth <= 0 or the voxel is unlabelled;  counts [frustum_size^2][20] int32
 *            (device; zeroed here, integer atomics: exact)
 *   params   24 floats on the HOST: centre of voxel (0, 0, 0) [3], voxel size [3], the row-major 3x4 matrix that takes a centre to
 *            (x d, y d, d) [12], the 2x2 post-rotation [4], the post-translation [2]
 *   patch i along an axis is [i / frustum_size * size, (i + 1) / frustum_size * size), the products in double rounded to fp32
 * SSBEV_EINVAL: NULL pointers, non-positive dims or image size, frustum_size outside 1..8, X Y Z >= 2^31. */
int ssbev_frustum_labels(const uint8_t* labels, uint8_t* ids, int32_t* counts, int X, int Y, int Z, const float* params,
                         int img_h, int img_w, int frustum_size, ssbev_stream_t stream);

/* 3-D context relation prior (since version 117): the operators of CPMegaVoxels (occupancy/backbones/crp3d.py:217-262 of the
 * reference), its loss compute_super_CP_multilabel_loss (resnet3d.py:269-290) and its label step (voxel_labels.py:79-174).
 * The relation grid is [X, Y, Z] with N = X Y Z row voxels; its 2 x 2 x 2 blocks are the Mc = N / 8 mega voxels, numbered
 * (x / 2) (Y / 2) (Z / 2) + (y / 2) (Z / 2) + z / 2.  The four relations of a (row voxel, mega voxel) pair: 0 a child of the mega
 * voxel has the row's non-empty class, 1 a child has another non-empty class and the row is non-empty, 2 row and a child are both
 * empty (0), 3 exactly one of row and child is empty; children labelled 255 are skipped and a row labelled 255 has no positive.
 *   logits    [B, N, 4, Mc] fp32: the channels-last result of the four context_prior_logits convolutions run as one layer
 *   labels    [B, X, Y, Z] uint8: the down-sampled label grid (ssbev_label_downsample); the [4, N, Mc] matrix is never built
 *   loss      one float (device): mean over all 4 B N Mc elements of -[pw_r y log s(x) + (1 - y) log(1 - s(x))], s = sigmoid, in
 *             the softplus form (finite for any x); pw_r = (B N Mc - cnt_r) / cnt_r with cnt_r the positives of relation r over
 *             the whole batch, and 1 when cnt_r = 0 (it then multiplies nothing; the reference divides by zero and returns NaN)
 *   pos_weight  [4] float (device), kept by the caller for backward
 *   backward  grad_logits [B, N, 4, Mc] = grad_out[0] * d loss / d logits (grad_out: one float on the device)
 * Per-workgroup sums in double, folded in a fixed order: no float atomics, nothing read back, every run gives the same bits.
 * SSBEV_EINVAL before any device work: NULL pointers, non-positive or odd X / Y / Z, N >= 2^24;  SSBEV_EWORKSPACE: ws_bytes below
 * the query, which answers 0 for refused dims. */
typedef struct { int B, X, Y, Z; } ssbev_crp_dims;
size_t ssbev_crp_loss_workspace(const ssbev_crp_dims* d);
int ssbev_crp_loss_fwd(const float* logits, const uint8_t* labels, float* loss, float* pos_weight, const ssbev_crp_dims* d, void* ws,
                       size_t ws_bytes, ssbev_stream_t stream);
int ssbev_crp_loss_bwd(const float* logits, const uint8_t* labels, const float* pos_weight, const float* grad_out,
                       float* grad_logits, const ssbev_crp_dims* d, ssbev_stream_t stream);
/* CreateRelationLabels._downsample_label on the device, byte-exact: labels [X, Y, Z] uint8 -> out [X / ds, Y / ds, Z / ds].  A
 * block with more than 0.95 ds^3 (in double, compared with >) voxels labelled 0 or 255 becomes 0 when the zeros outnumber the
 * 255s and 255 otherwise (also on a tie); any other block takes its most frequent class 1 .. 254, the lowest id on a tie.
 * SSBEV_EINVAL: NULL pointers, non-positive dims, downscale outside 1..32 or not a divisor of X, Y and Z, X Y Z >= 2^31. */
int ssbev_label_downsample(const uint8_t* labels, uint8_t* out, int X, int Y, int Z, int downscale, ssbev_stream_t stream);
/* Relation gather: out[b][n][r C2 + c] = sum_m sigmoid(logits[b][n][r][m]) context[b][m][c], one fp32 MFMA GEMM per (b, r) with
 * the sigmoid applied while the A operand is staged; sigmoid(logits) is never written.
 *   logits    [B, N, R, Mc];  context [B, Mc, C2] (the channels-last mega-context volume)
 *   out       row n of sample b starts at out + (b N + n) ld_out: pass the address of the first context channel of the
 *             concatenated [input, context] tensor and its channel count as ld_out (>= R C2)
 *   backward  grad_out laid out as out;  grad_logits [B, N, R, Mc] = (grad_out_r context^T) s (1 - s);
 *             grad_context [B, Mc, C2] = sum_r s_r^T grad_out_r, the reduction cut into slices folded in a fixed order (ws)
 * SSBEV_EINVAL: NULL pointers, non-positive dims, R > 16, ld_out < R C2;  SSBEV_EWORKSPACE: ws_bytes below the query. */
typedef struct { int B, N, Mc, C2, R; int64_t ld_out; } ssbev_crp_gather_dims;
int ssbev_crp_gather_fwd(const float* logits, const float* context, float* out, const ssbev_crp_gather_dims* d,
                         ssbev_stream_t stream);
size_t ssbev_crp_gather_bwd_workspace(const ssbev_crp_gather_dims* d);
int ssbev_crp_gather_bwd(const float* logits, const float* context, const float* grad_out, float* grad_logits, float* grad_context,
                         const ssbev_crp_gather_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);

/* Lifted-point position encoder (since version 118): point_xyz_channel of the reference's voxel_pooling
 * (ViewTransformerLSSVoxel.py:432-476) without a tensor that has a row per point.  A kept point p (vox[p] >= 0) at ego position
 * g has the unit position u = ((g - lo) / (hi - lo) - 0.5) * 2, each step rounded to fp32 as the tensor expression rounds it.
 *   geom      [B, P, 3] fp32;  vox [B P] int32;  starts / order / long_list: the tables of ssbev_pool_prepare2 for these points
 *             (long_list may be NULL in _fwd: every list is then summed by the lanes of its voxel)
 *   moments   [10] double (device): count, sum u (x, y, z), sum u u^T (xx, xy, xz, yy, yz, zz) over the kept points;
 *             per-workgroup double sums folded in a fixed order: no atomics, every run gives the same bits
 *   coef      [6, M] fp32 (device), per channel m: w_m / s_m (3 rows), (b1_m - mu_m) / s_m, gamma_m, beta_m, where
 *             h = W1 u + b1 is the first Linear, mu / s the mean and standard deviation BatchNorm1d normalises with
 *   _fwd      S [B, nx, ny, nz, M] fp32 (channels-last, 16-byte stores): S[v] = sum over the points of v, in ascending point
 *             order and sequentially in fp32, of relu(gamma hhat + beta), hhat = fma(c0, ux, fma(c1, uy, fma(c2, uz, c3)));
 *             zeros for empty voxels.  Lists of more than 32 points: 64 / (M / 4) strided slices folded in slice order
 *   _bwd      sums [5, M] double (device): sum gz, sum gz hhat, sum gz ux, sum gz uy, sum gz uz over all kept points, with
 *             gz = gS[v(p)] [z_p > 0] and z recomputed by the expression of _fwd (the masks agree bit for bit); gS is laid
 *             out as S and read once per voxel.  Per-workgroup double sums over fixed voxel ranges, folded in workgroup order
 * SSBEV_EINVAL before any device work: NULL pointers (d included), non-positive dims, M outside 4 .. 256 or no multiple of
 * 4, hi <= lo or a non-finite bound, B P >= 2^31, B nx ny nz >= 2^31;  SSBEV_EWORKSPACE: ws_bytes below the query (one query
 * serves _moments and _bwd), which answers 0 for refused dims. */
typedef struct { int B, P, nx, ny, nz, M; float lo[3], hi[3]; } ssbev_point_xyz_dims;
size_t ssbev_point_xyz_workspace(const ssbev_point_xyz_dims* d);
int ssbev_point_xyz_moments(const float* geom, const int32_t* vox, double* moments, const ssbev_point_xyz_dims* d, void* ws,
                            size_t ws_bytes, ssbev_stream_t stream);
int ssbev_point_xyz_fwd(const float* geom, const int32_t* starts, const int32_t* order, const int32_t* long_list,
                        const float* coef, float* S, const ssbev_point_xyz_dims* d, ssbev_stream_t stream);
int ssbev_point_xyz_bwd(const float* geom, const int32_t* starts, const int32_t* order, const float* coef, const float* gS,
                        double* sums, const ssbev_point_xyz_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);

/* Point-level branch of the occupancy head (since version 119; occhead.py:171-236 sample_point_feats + feature_sampling): every
 * point of the batch samples the voxel feature maps trilinearly and the image features bilinearly, as F.grid_sample with zero
 * padding and align_corners=False does (source index ((g + 1) S - 1) / 2 in fp32, ATen's corner weights and corner order;
 * corners outside the map are skipped, never clamped).  csrc/point_head.hip.
 *   points    [N, 3] fp32: the normalised coordinates g of all samples' points, sample after sample
 *   offsets   [B + 1] int32 (device): first point of every sample, offsets[B] = N
 *   f0 .. f3  the L <= 4 levels, channels-last [B, X_l, Y_l, Z_l, C] fp32 (the unused ones NULL)
 *   axis_xyz  0: g = (x, y, z) is handed to the sampler as the reference hands it, so that x walks the Z axis and z the X axis;
 *             1: x walks X, y walks Y, z walks Z
 *   rows      per_level = 1: [L, N, C];  per_level = 0: [N, C], the levels added in level order
 *   ws        kept for _bwd: int32 keys | fp32 weights, one pair per (level, point, corner) in that order; a key is the cell
 *             of the concatenated level grids the corner read, -1 for a skipped corner.  The keys sit at the start of ws
 *   _bwd      starts / order: the CSR table ssbev_pool_prepare2 makes of the keys with dims (1, sum_l B X_l Y_l Z_l, 1, 1);
 *             g0 .. g3 laid out as f0 .. f3: every cell = sum of weight * grad_rows over its list in list order, zeros for an
 *             empty list.  Every element is written exactly once: no float atomics, the same bits on every run
 * The image form: img [B, cams, H, W, C], uv [N, cams, 3] = (u, v, depth); a pair contributes when depth > 1e-5 and u, v lie
 * strictly inside (-1, 1); rows [N, C] = sum over the cameras; keys over B cams H W pixels, 4 per (point, camera).  Masked
 * pairs are never read (NaN features behind them are not scrubbed).
 * SSBEV_EINVAL before any device work: NULL pointers (d included), non-positive dims, C no multiple of 4, L > 4, flags other
 * than 0 / 1, 2^31 or more keys or cells;  SSBEV_EWORKSPACE: ws_bytes below the query, which answers 0 for refused dims. */
typedef struct { int B, N, C, L; int X[4], Y[4], Z[4]; int axis_xyz, per_level; } ssbev_point_head_dims;
typedef struct { int B, N, cams, C, H, W; } ssbev_point_img_dims;
size_t ssbev_point_sample_workspace(const ssbev_point_head_dims* d);
int ssbev_point_sample_fwd(const float* points, const int32_t* offsets, const float* f0, const float* f1, const float* f2,
                           const float* f3, float* rows, const ssbev_point_head_dims* d, void* ws, size_t ws_bytes,
                           ssbev_stream_t stream);
int ssbev_point_sample_bwd(const float* grad_rows, const int32_t* starts, const int32_t* order, const void* ws, float* g0,
                           float* g1, float* g2, float* g3, const ssbev_point_head_dims* d, ssbev_stream_t stream);
size_t ssbev_point_img_workspace(const ssbev_point_img_dims* d);
int ssbev_point_img_fwd(const float* img, const float* uv, const int32_t* offsets, float* rows, const ssbev_point_img_dims* d,
                        void* ws, size_t ws_bytes, ssbev_stream_t stream);
int ssbev_point_img_bwd(const float* grad_rows, const int32_t* starts, const int32_t* order, const void* ws, float* grad_img,
                        const ssbev_point_img_dims* d, ssbev_stream_t stream);

/* Running statistics of a training-mode BatchNorm from the (mean, rstd) ssbev_groupnorm_fwd returned with G == C over the
 * batch: running_mean <- (1-m) running_mean + m mean; running_var <- (1-m) running_var + m var n/(n-1)
 * (torch.nn.BatchNorm3d as built at ViewTransformerLSSVoxel.py:83-88; n = elements per channel). */
int ssbev_bn_update_running(const float* mean, const float* rstd, float* running_mean, float* running_var, int C,
                            float momentum, float eps, int64_t n, ssbev_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Softmax along a strided axis: x = [outer][C][inner] (inner contiguous), y = softmax over C.
 * Replaces F.softmax(dim=1) on the depth-major matching distribution (ViewTransformerLSSVoxel.py:255-259)
 * and F.softmax(q, dim=2) of the BRI confidence (attention.py:66-68); bwd: gx = y * (gy - sum_c y * gy).
 * ------------------------------------------------------------------------------------------ */
int ssbev_softmax_axis_fwd(const float* x, float* y, int64_t outer, int C, int64_t inner, ssbev_stream_t stream);
int ssbev_softmax_axis_bwd(const float* y, const float* gy, float* gx, int64_t outer, int C, int64_t inner,
                           ssbev_stream_t stream);
/* Host-side query (since ssbev_version() 121; no device work): the kernel instance both launchers pick for this geometry, as the
 * number of slices a column's axis is cut into across the threads of a workgroup: 8 (32 columns per workgroup) or 1 (256
 * columns per workgroup); 0 for C <= 0 or inner <= 0. */
int ssbev_softmax_axis_slices(int C, int64_t inner);
/* Softmax along the innermost axis of `rows` rows of C contiguous floats (C % 4 == 0, C <= 8192): the BRI attention
 * matrix softmax(energy, -1) of attention.py:66-68 (T = 7680).  One read + one write of the matrix forward, two reads +
 * one write backward (gx = y * (gy - sum_c y * gy)); y may alias x and gx may alias gy. */
int ssbev_softmax_rows_fwd(const float* x, float* y, int64_t rows, int C, ssbev_stream_t stream);
int ssbev_softmax_rows_bwd(const float* y, const float* gy, float* gx, int64_t rows, int C, ssbev_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Deformable convolution v1, sampling stages (mmcv DeformConv2dPack as built by DepthNet, bevdepth.py:490-498;
 * mmcv/ops/csrc deform_conv: deformable_im2col / deformable_col2im / deformable_col2im_coord).  stride 1,
 * deform_groups 1.  x [B,H,W,C], offset [B,H,W,2*k*k] (channel 2t = dy, 2t+1 = dx of tap t),
 * cols / gcols [G][B*H*W][k*k*(C/G)]: slab g is a channels-last [B, k*k*C/G, H, W] tensor, so the grouped
 * contraction is ssbev_conv_fwd with a 1x1 kernel per group.  col2im overwrites gx and goffset; both are run-to-run identical
 * (round 6: the x gradient is a gather over the samples sorted by target pixel with ssbev_pool_prepare, summed in ascending
 * (pixel, tap, corner) order -- mmcv's col2im scatters with atomics).  ws: ssbev_dcn_col2im_workspace bytes.
 * ------------------------------------------------------------------------------------------ */
typedef struct { int B, C, H, W, G, k, pad, dil; } ssbev_dcn_dims;
int ssbev_dcn_im2col(const float* x, const float* offset, float* cols, const ssbev_dcn_dims* d, ssbev_stream_t stream);
size_t ssbev_dcn_col2im_workspace(const ssbev_dcn_dims* d);
int ssbev_dcn_col2im(const float* x, const float* offset, const float* gcols, float* gx, float* goffset,
                     const ssbev_dcn_dims* d, void* ws, size_t ws_bytes, ssbev_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Data side: CreateDepthFromLiDAR (datasets/pipelines/occ_to_depth.py:216-303), the producer of the
 * gt_depths slot of img_inputs.  points [N][3] fp32 (lidar frame), cam = 34 floats (host or device memory):
 * inv(rots) 3x3 row major | trans 3 | intrins 4x4 row major | post_rots[:2,:2] | post_trans[:2].
 * Writes uvd [N][3] (augmented pixel u, v and depth of every point), valid [N] (inside the image, depth > 0), the
 * depth map [H][W] = depth of the NEAREST valid point per pixel (pixel = round-half-even(u, v)), 0 where none, and --
 * when labels [N] and seg are given -- seg [H][W] = label of that nearest point.  Same operation order as the
 * reference's torch expressions; ties on depth resolve to the lowest point index.  ws: ssbev_lidar_depth_workspace bytes.
 * The 34 camera floats are copied synchronously (one implicit stream sync: this is a data-loading operator).
 * ------------------------------------------------------------------------------------------ */
/* Image loading (loading_semkitti.py:101-131, 176-232: `img.resize(resize_dims)`, `img.crop(crop)`, flip, mmcv
 * `imnormalize`, HWC -> CHW).  ssbev_resize_pil_u8 is byte-exact with Pillow's antialiased resize of 8-bit images: the
 * caller passes libImaging's fixed-point coefficient tables (kk [out][ksize] int32 with 22 fractional bits, bounds
 * [out][2] = first source index, tap count) for the horizontal and the vertical pass; tmp [Hs][Wd][C] is the 8-bit
 * intermediate.  ssbev_crop_normalize_u8: dst [3][h][w] = (src[y0+y][x0+x'][c'] - mean[c]) * stdinv[c], x' mirrored when
 * flip, c' = 2-c when swap_rb; pixels outside the source read 0 (PIL crop semantics); mean / stdinv are HOST pointers. */
int ssbev_resize_pil_u8(const uint8_t* src, int Hs, int Ws, int C, const int32_t* kk_h, const int32_t* bounds_h, int ksize_h,
                        const int32_t* kk_v, const int32_t* bounds_v, int ksize_v, uint8_t* tmp, uint8_t* dst, int Hd, int Wd,
                        ssbev_stream_t stream);
int ssbev_crop_normalize_u8(const uint8_t* src, int Hs, int Ws, float* dst, int x0, int y0, int w, int h, int flip,
                            const float* mean, const float* stdinv, int swap_rb, ssbev_stream_t stream);
/* ssbev_crop_rotate_normalize_u8 (since version 101): the same crop + flip + normalise followed by Pillow's `img.rotate(rotate)`
 * (loading_semkitti.py:128-135: nearest neighbour, expand=False, centre (w/2, h/2) of the cropped image, black fill), byte-exact
 * with Pillow in its 16.16 fixed-point range.  affine6 = libImaging's fixed-point inverse map a0..a5 (HOST pointer, 6 int32;
 * pipelines.pil_rotate_fixed): output (x, y) takes intermediate pixel xi = (a2 + y*a1 + x*a0) >> 16, yi = (a5 + y*a4 + x*a3) >> 16
 * (floor), 0 when (xi, yi) lies outside [0,w) x [0,h); otherwise it reads src[y0+yi][x0+xi'] with xi' = w-1-xi when flip, 0
 * outside the source, and normalises as ssbev_crop_normalize_u8. */
int ssbev_crop_rotate_normalize_u8(const uint8_t* src, int Hs, int Ws, float* dst, int x0, int y0, int w, int h, int flip,
                                   const int32_t* affine6, const float* mean, const float* stdinv, int swap_rb,
                                   ssbev_stream_t stream);
/* ssbev_crop_rotate_jitter_normalize_u8 (since version 102): ssbev_crop_rotate_normalize_u8 with the train-time colour jitter
 * (loading_semkitti.py:213, 273: PhotoMetricDistortionMultiViewImage, loading_bevdet.py:532-620) between the rotate and the
 * normalise; affine6 = pil_rotate_fixed(w, h, 0) is the identity map for an unrotated view.  The pixel as the normalise reads it
 * (RGB) is the upstream's image in BGR order b = c2, g = c1, r = c0, in fp32, and the drawn values (HOST pointer) apply as:
 *   1. flags & BRIGHTNESS: x += delta                     2. mode == 1 and flags & CONTRAST: x *= alpha
 *   3. BGR -> HSV as OpenCV's scalar float path (RGB2HSV_f, h in degrees)
 *   4. flags & SATURATION: s *= saturation                 5. flags & HUE: h += hue; h > 360: h -= 360; then h < 0: h += 360
 *   6. HSV -> BGR (HSV2RGB_f)                              7. mode == 0 and flags & CONTRAST: x *= alpha
 *   8. flags & SWAP: x = x[perm] (perm indexes BGR)        9. uint8 without clipping: truncate toward zero, keep the low 8 bits
 * every product and sum rounded on its own (no FMA), IEEE division; then the normalise as ssbev_crop_normalize_u8.
 * SSBEV_EINVAL when perm is not a permutation of {0, 1, 2}, mode is not 0 / 1, flags has unknown bits, or a value is not
 * finite or outside |delta| <= 255, 0 <= alpha, saturation <= 8, |hue| <= 360 (upstream draws +-32, 0.5..1.5, +-18). */
#define SSBEV_JITTER_BRIGHTNESS 1
#define SSBEV_JITTER_CONTRAST 2
#define SSBEV_JITTER_SATURATION 4
#define SSBEV_JITTER_HUE 8
#define SSBEV_JITTER_SWAP 16
typedef struct { int flags, mode; float delta, alpha, saturation, hue; int perm[3]; } ssbev_jitter_params;
int ssbev_crop_rotate_jitter_normalize_u8(const uint8_t* src, int Hs, int Ws, float* dst, int x0, int y0, int w, int h, int flip,
                                          const int32_t* affine6, const ssbev_jitter_params* jitter, const float* mean,
                                          const float* stdinv, int swap_rb, ssbev_stream_t stream);
/* BEV augmentation of the voxel labels (since ssbev_version() 120; loading_semkitti.py:304-356 bev_transform; csrc/bev_augment.hip):
 * src uint8 [X,Y,Z] -> dst [X,Y,Z] (int64, or uint8 for the _u8 form): scipy.ndimage.rotate(order=0, mode='constant', cval=fill,
 * axes=(0,1), reshape=False), then the flip of axis 1 (flip_dy), then the flip of axis 0 (flip_dx).
 * coeffs6 = {m00, m01, m10, m11, off0, off1} (HOST pointer, doubles; scipy's own matrix [[c, s], [-s, c]] and offset, composed by
 * the caller): output (i, j) of a plane samples ci = (m00*i + m01*j) + off0, cj = (m10*i + m11*j) + off1 -- IEEE double, every
 * product and sum rounded on its own, no FMA -- and takes source voxel (floor(ci + 0.5), floor(cj + 0.5)) iff 0 <= ci <= X-1
 * and 0 <= cj <= Y-1, else `fill`.  coeffs6 == NULL: no rotation (flips and widening alone; no workspace).
 * inplace != 0 reproduces the upstream's rotate(lab, output=lab): scipy writes a plane in raster order p = i*Y + j over the array
 * it reads, so an output whose source index is BELOW p takes the value already written there, out[p] = out[m[p]].  These chains
 * are collapsed by pointer jumping in ceil(log2(X*Y)) rounds on a table of X*Y int32 (a count fixed by the dims: no read-back,
 * the same bits every run).  inplace == 0 is the out-of-place rotation.  src and dst must not overlap in either form.
 * ws: ssbev_bev_label_workspace bytes (rotate = whether coeffs6 is given), caller-owned.
 * SSBEV_EINVAL before any device work: NULL src / dst (or ws with coeffs6), X, Y or Z < 1, X*Y > 2^31 - 3 (the int32 table),
 * more than 2^31 - 1 blocks of 256 voxels, a non-finite coefficient, fill outside 0 .. 255, overlapping src and dst;
 * SSBEV_EWORKSPACE: ws_bytes below the query. */
size_t ssbev_bev_label_workspace(int X, int Y, int rotate, int inplace);
int ssbev_bev_label_transform(const uint8_t* src, int64_t* dst, int X, int Y, int Z, const double* coeffs6, int inplace,
                              int flip_dx, int flip_dy, int fill, void* ws, size_t ws_bytes, ssbev_stream_t stream);
int ssbev_bev_label_transform_u8(const uint8_t* src, uint8_t* dst, int X, int Y, int Z, const double* coeffs6, int inplace,
                                 int flip_dx, int flip_dy, int fill, void* ws, size_t ws_bytes, ssbev_stream_t stream);
/* Depth BCE loss (ViewTransformerLSSVoxel.py:349-416: get_downsampled_gt_depth + get_depth_loss): gt_depths [BN, fH*ds, fW*ds]
 * (0 = no LiDAR return), depth_pred [BN, D, fH, fW] (a probability distribution over the D bins per pixel).  out2[0] = weight *
 * sum of the binary cross entropies over the pixels that have a return / max(their number, 1), out2[1] = that divisor.  The
 * bin of a pixel is (min over its ds x ds block - c0) / dd in fp32, truncated, with c0 = d0 - dd / 2 computed by the caller as
 * the reference does (in double, rounded to fp32 once).  The workspace keeps the per-pixel labels for _bwd, which writes
 * grad_pred = grad_loss[0] * d out2[0] / d depth_pred. */
size_t ssbev_depth_bce_workspace(int BN, int fH, int fW);
int ssbev_depth_bce_fwd(const float* gt_depths, const float* depth_pred, float* out2, int BN, int D, int fH, int fW, int ds,
                        float c0, float dd, float weight, void* ws, size_t ws_bytes, ssbev_stream_t stream);
int ssbev_depth_bce_bwd(const float* depth_pred, const float* grad_loss, const float* out2, float* grad_pred, int BN, int D, int fH,
                        int fW, int ds, float c0, float dd, float weight, const void* ws, ssbev_stream_t stream);

/* Depth KL loss (since ssbev_version() 109; ViewTransformerLSSVoxel.py:390-416 get_klv_depth_loss with
 * utils/gaussian.py:90-130 generate_guassian_depth_target, constant_std): same tensors as the BCE form; dbound = (d0, d1, dd) as
 * the config gives it, in double.  Per feature pixel m = the smallest non-zero depth of its ds x ds block (0 when it has none);
 * the row is foreground when (float)d0 <= m <= (float)(d1 - dd); its target over the D bins is
 *   t_d = cdf(x_{d+1}) - cdf(x_d),  x_i = (d0 - dd / 2) + i dd (i = 0..D, rounded to fp32 once),
 *   cdf(x) = 0.5 (1 + erf(((x * edge_scale - m / dd) / (sigma / dd)) / sqrt 2)),  all in fp32,
 * sigma = the standard deviation in metres (the reference's constant_std = 0.5).  edge_scale = 1 is the reference as executed
 * (the mean is in bin units, the edges are in metres); edge_scale = 1 / dd puts both in bin units.
 * out2[0] = weight * sum over foreground rows and bins of (xlogy(t, t) - t log(p + 1e-4)) / max(foreground rows, 1), out2[1] =
 * that divisor; the sum is taken in double in a fixed order (no atomics: the same bits every run).  With no foreground row
 * out2[0] = 0 and the gradient is all zero (the reference divides 0 by 0).  A t that rounds below zero counts as 0.
 * The workspace keeps m and the foreground flag per pixel for _bwd, which recomputes t and writes
 * grad_pred = -(grad_loss[0] * weight / out2[1]) * t / (p + 1e-4) on foreground rows and exactly 0 elsewhere.
 * SSBEV_EINVAL (before any device work) for a NULL pointer, a non-positive dim, sigma <= 0, dd <= 0, edge_scale <= 0, a non-finite
 * value, or when ceil((d1 - (d0 - dd / 2)) / dd), the length of torch.arange(d0 - dd / 2, d1, dd), is not D + 1;
 * SSBEV_EWORKSPACE when ws_bytes is below the query, which answers 0 for refused dims. */
size_t ssbev_depth_kld_workspace(int BN, int fH, int fW);
int ssbev_depth_kld_fwd(const float* gt_depths, const float* depth_pred, float* out2, int BN, int D, int fH, int fW, int ds,
                        double d0, double d1, double dd, float sigma, float edge_scale, float weight, void* ws, size_t ws_bytes,
                        ssbev_stream_t stream);
int ssbev_depth_kld_bwd(const float* depth_pred, const float* grad_loss, const float* out2, float* grad_pred, int BN, int D, int fH,
                        int fW, int ds, double d0, double d1, double dd, float sigma, float edge_scale, float weight, const void* ws,
                        size_t ws_bytes, ssbev_stream_t stream);

/* Image-view segmentation loss (since ssbev_version() 115; ViewTransformerLSSVoxel.py:418-430 get_seg_loss: F.interpolate of the
 * head's logits to the label map (nearest) + CrossEntropyLoss(weight, ignore_index=0)), without the up-sampled tensor.
 *   logits   [BN, K, h, w] fp32, contiguous (2 <= K <= 32);  labels [BN, H, W] fp32 (h <= H, w <= W);  class_w [K] fp32
 * Image pixel (y, x) reads the logits of cell (min(floor(y * s_h), h - 1), min(floor(x * s_w), w - 1)), s_h = (float)h / H and
 * s_w = (float)w / W in fp32: torch's `nearest` rule.  The pixels of a cell form a rectangle; the rectangles tile the image.
 * A pixel is valid when its label, truncated towards zero (the reference's .long()), lies in [1, K).  0 is the reference's
 * ignore_index; a NaN and every value outside [0, K) are ignored as well and never index memory (the reference raises on them).
 *   num = sum over valid pixels p of class_w[l_p] (lse(logits[:, cell(p)]) - logits[l_p, cell(p)]),  den = sum of class_w[l_p]
 *   loss_out[0] = weight * (num / den); without a valid pixel loss_out[0] = 0 and the gradient is all zero (the reference: NaN).
 * _fwd: one wavefront per cell counts the labels of its rectangle into K bins held in registers (lane c keeps bin c), takes one
 * max-subtracted log-sum-exp and writes the cell's (num, den) in double; a second launch folds the cells in a fixed order (no
 * atomics: the same bits every run).  The workspace keeps (num, den), the partials and the K counts of every cell; _bwd takes
 * the SAME workspace (it reads the counts and den, not the labels) and writes every element of grad_logits exactly once:
 *   grad_logits[c, cell] = grad_loss[0] * weight / den * (softmax_c * den_cell - n_c class_w[c]),  exactly 0 for a cell without
 * a valid pixel.  SSBEV_EINVAL (before any device work) for a NULL pointer, K outside 2 .. 32, a non-positive dim, h > H, w > W,
 * BN h w >= 2^24, and in _fwd for ws_bytes below the query, which answers 0 for refused dims. */
size_t ssbev_imgseg_ce_workspace(int BN, int h, int w);
int ssbev_imgseg_ce_fwd(const float* logits, const float* labels, const float* class_w, int BN, int K, int h, int w, int H, int W,
                        float weight, float* loss_out, void* ws, size_t ws_bytes, ssbev_stream_t stream);
int ssbev_imgseg_ce_bwd(const float* logits, const float* labels, const float* class_w, const float* grad_loss, int BN, int K,
                        int h, int w, int H, int W, float weight, float* grad_logits, const void* ws, ssbev_stream_t stream);

size_t ssbev_lidar_depth_workspace(int H, int W);
int ssbev_lidar_depth_map(const float* points, int n_points, const float* cam, const float* labels, float* uvd,
                          unsigned char* valid, float* depth, float* seg, int H, int W, void* ws, size_t ws_bytes,
                          ssbev_stream_t stream);

/* CreateDepthFromOccupancy (since ssbev_version() 122; datasets/pipelines/occ_to_depth.py:15-153; csrc/occ_depth.hip): the depth
 * map and the image-view label map of one view from the voxel labels alone.  labels uint8 [X][Y][Z] (device); xs [X], ys [Y],
 * zs [Z] = the voxel centres per axis (device, fp32; the caller makes them with the reference's torch.arange, :36-38); cam46 = 46
 * floats in HOST memory (copied into the launch: no synchronisation):
 *   inv(bda)[:3] as 3x4 row major (column 3 ignored when bda_cols == 3) | inv(rots) 3x3 | trans 3 | intrins 4x4 | post_rots[:2,:2] |
 *   post_trans[:2];  bda_cols = 3 or 4, the size of the BEV matrix (4: the centre is taken as [p; 1]).
 * Every centre is projected with project_points' fp32 operation order (:43-65: inv_bda @ p, - trans, inv_rots @, intrins @ [p; 1],
 * / depth, post_rots[:2,:2] @, + post_trans[:2]; every product and sum rounded on its own), is in view when 0 <= u <= W-1,
 * 0 <= v <= H-1 and depth > 0 (:112-116), and lands on pixel (round-half-even(v), round-half-even(u)).
 *   depth [H][W] = depth of the NEAREST in-view voxel labelled 1..254 per pixel, 0 where none (:121-127);
 *   seg   [H][W] = label of the nearest in-view voxel per pixel, 255 where none (:132-140).  seg_occupied == 0 is the reference:
 *                  EVERY in-view voxel competes, empty (0) and ignored (255) ones included, so an empty voxel in front of a
 *                  surface takes the pixel; seg_occupied != 0 lets only labels 1..254 compete (the depth map's own voxels).
 * Among voxels of a pixel with exactly equal fp32 depth the lowest flat index x*Y*Z + y*Z + z wins (the reference's argsort
 * leaves it open); the result is the same bits every run.  ws: ssbev_occ_depth_workspace bytes, caller-owned (two key buffers).
 * SSBEV_EINVAL before any device work: a NULL pointer (a table included), X, Y, Z, H or W < 1, more than 2^32 voxels, H*W above
 * 2^31 - 257, bda_cols not 3 / 4; SSBEV_EWORKSPACE: ws_bytes below the query, which answers 0 for refused dims.
 * ssbev_label_map_downsample: _downsample_label (:67-93) of a label map seg [H][W] (fp32 holding 0..255; anything else counts as
 * 255) -> out [H/ds][W/ds] (trailing rows / columns dropped): a patch with more than empty_t (the caller's (float)(0.95*ds*ds))
 * pixels 0 or 255 becomes 0 when the zeros outnumber the 255s, else 255; any other patch its most frequent label in 1..254, the
 * LOWEST on a tie (torch.mode's choice).  1 <= ds <= 256. */
size_t ssbev_occ_depth_workspace(int H, int W);
int ssbev_occ_depth_map(const uint8_t* labels, int X, int Y, int Z, const float* xs, const float* ys, const float* zs,
                        const float* cam46, int bda_cols, int seg_occupied, float* depth, float* seg, int H, int W, void* ws,
                        size_t ws_bytes, ssbev_stream_t stream);
int ssbev_label_map_downsample(const float* seg, float* out, int H, int W, int ds, float empty_t, ssbev_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Image branch (the step before a1/a5): operators of CustomEfficientNet (backbones/efficientnet.py:112-229,
 * 275-519: InvertedResidual = expand 1x1 -> depthwise k x k -> SE -> linear 1x1) that are not dense contractions.
 * Channels-last fp32, C % 4 == 0.
 *   dwconv2d: depthwise k x k (k = 3 | 5, stride 1 | 2), y[b,ho,wo,c] = sum_ij x[b, ho*s - pad_t + i, wo*s - pad_l + j, c]
 *             * w[i*k + j][c]; out-of-range taps read zero.  pad_t / pad_l and Ho / Wo are explicit, so mmcv's
 *             Conv2dAdaptivePadding ("same": Ho = ceil(Hi/s), odd padding row/column at the bottom/right) is
 *             pad_t = pad_total_h / 2, pad_l = pad_total_w / 2.  w / gw layout: [k*k][C] (torch [C,1,k,k] transposed).
 *   swish:    y = x * sigmoid(x) (mmcv Swish) and its gradient.
 *   chan_sum: out[b][c] = scale * sum_s a[b][s][c] * (bmul ? bmul[b][s][c] : 1) -- AdaptiveAvgPool2d(1) of mmdet's
 *             SELayer (scale = 1/S) and the gate gradient of its rescale.
 *   chan_scale: y[b][s][c] = x[b][s][c] * gate[b][c]; x = NULL: y = gate[b][c] * scale (gradient of the pool).
 * ------------------------------------------------------------------------------------------ */
typedef struct { int B, C, Hi, Wi, Ho, Wo, k, stride, pad_t, pad_l; } ssbev_dw_dims;
int ssbev_dwconv2d_fwd(const float* x, const float* w, float* y, const ssbev_dw_dims* d, ssbev_stream_t stream);
int ssbev_dwconv2d_bwd_data(const float* gy, const float* w, float* gx, const ssbev_dw_dims* d, ssbev_stream_t stream);
size_t ssbev_dwconv2d_bwd_weight_workspace(const ssbev_dw_dims* d);                      /* floats */
int ssbev_dwconv2d_bwd_weight(const float* x, const float* gy, float* gw, const ssbev_dw_dims* d, float* ws,
                              size_t ws_elems, ssbev_stream_t stream);
int ssbev_swish_fwd(const float* x, float* y, int64_t n, ssbev_stream_t stream);        /* n % 4 == 0 */
int ssbev_swish_bwd(const float* x, const float* gy, float* gx, int64_t n, ssbev_stream_t stream);
size_t ssbev_chan_sum_workspace(int B, int64_t S, int C);                                 /* floats */
int ssbev_chan_sum(const float* a, const float* bmul, float* out, int B, int64_t S, int C, float scale, float* ws,
                   size_t ws_elems, ssbev_stream_t stream);
int ssbev_chan_scale(const float* x, const float* gate, float* y, int B, int64_t S, int C, float scale,
                     ssbev_stream_t stream);
/* Host-side queries (since ssbev_version() 121; no device work), from the functions the launchers themselves read:
 *   bwd_weight_layout: a workgroup of ssbev_dwconv2d_bwd_weight is Q channel quads x L pixel lanes (Q * L <= 256), the channels
 *                      take qblocks such workgroups per pixel chunk (the pixel chunks follow from the workspace query).
 *   stream_blocks:     workgroups of the grid-stride passes (swish, chan_scale) over n4 float4 elements; 0 for n4 <= 0. */
int ssbev_dwconv2d_bwd_weight_layout(const ssbev_dw_dims* d, int* Q, int* L, int* qblocks);
int64_t ssbev_stream_blocks(int64_t n4);

/* ---------------------------------------------------------------------------------------------
 * Winograd F(2x2x2, 3x3x3) transforms for stride-1 3x3x3 "same" convolutions (even D, H, W; channels-last).
 * T = B * D/2 * H/2 * W/2 tiles, 64 frequencies.  The element-wise stage between them is 64 plain GEMMs
 * [T x Cin] x [Cin x Cout] (forward / data gradient) or [Cin x T] x [T x Cout] (weight gradient).
 *   input_transform:   x  [B,D,H,W,C] -> V [64][T][C]   (B^T d B; also used on gy for the data gradient)
 *   output_transform:  M  [64][T][C]  -> y [B,D,H,W,C]  (A^T M A)
 *   output_adjoint:    gy [B,D,H,W,C] -> Z [64][T][C]   (A gy A^T, weight gradient)
 * Replaces nn.Conv3d at resnet3d.py:18-32, second_fpn_3d.py:53-69 (3x3x3 convs), occhead.py:100-107.
 * ------------------------------------------------------------------------------------------ */
typedef struct { int B, D, H, W, C; int dil; } ssbev_wino_dims;   /* dil: 0 / 1 = undilated; > 1: see ssbev_wino2d_* below */
int ssbev_wino_input_transform(const float* x, float* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino_output_transform(const float* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino_output_adjoint(const float* gy, float* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
/* 2-D variant F(2x2, 3x3) for the 3x3 conv2d layers of DepthNet (ViewTransformerLSSBEVDepth.py:461-504): 16 frequencies,
 * T = B * D * H/2 * W/2 (D is a batch axis), buffers [16][T][C].
 * ssbev_wino_dims.dil > 1 (these three fp32 functions and ssbev_wino2d_output_transform_acc only; every other ssbev_wino*
 * function answers SSBEV_EINVAL): the 3x3 layer with dilation = padding = dil.  Every residue class modulo dil is tiled on
 * its own with its rows / columns dil apart, so H and W may be odd and nothing is padded or copied: T = B * D * TH * TW with
 * TH = ssbev_wino2d_axis_tiles(H, dil, ...), TW likewise (each at most SSBEV_WINO2D_MAX_AXIS_TILES, H and W at most 65535).
 * Weight functions and frequency products are those of the undilated layer. */
#define SSBEV_WINO2D_MAX_AXIS_TILES 128
/* Host only: tiles along an axis of `extent` positions = sum over ph < min(dil, extent) of ceil(ceil((extent - ph) / dil) / 2),
 * numbered phase-major; first[i] (i < cap; first may be NULL) = first output coordinate ph + 2 t dil of tile i, whose second
 * output is dil further (outside the axis for the half-empty last tile of a class).  0 for extent or dil <= 0. */
int ssbev_wino2d_axis_tiles(int extent, int dil, uint16_t* first, int cap);
int ssbev_wino2d_input_transform(const float* x, float* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino2d_output_transform(const float* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino2d_output_adjoint(const float* gy, float* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
/* bf16 variants (BASELINE configs[3], "bf16 mixed precision, MFMA 3D-conv path"): identical transforms, but the
 * transformed-domain tensor (V, M, Z) is stored as bf16 (uint16_t bit patterns, round-to-nearest-even) so that the
 * frequency GEMMs run on the bf16 matrix pipe with fp32 accumulation and the streaming passes move half the bytes.
 * Activations, gradients and weights on the caller's side stay fp32. */
int ssbev_wino_input_transform_bf16(const float* x, uint16_t* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino_output_transform_bf16(const uint16_t* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino_output_adjoint_bf16(const float* gy, uint16_t* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino2d_input_transform_bf16(const float* x, uint16_t* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino2d_output_transform_bf16(const uint16_t* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino2d_output_adjoint_bf16(const float* gy, uint16_t* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
/* `_bf16a` (round 4, bf16 STORAGE mode): the activation side (x, gy, y) is a bf16 channels-last tensor too -- every pass of the
 * F(2,3) pipeline then moves 16-bit elements only. */
int ssbev_wino_input_transform_bf16a(const uint16_t* x, uint16_t* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino_output_transform_bf16a(const uint16_t* M, uint16_t* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino_output_adjoint_bf16a(const uint16_t* gy, uint16_t* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino2d_input_transform_bf16a(const uint16_t* x, uint16_t* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino2d_output_transform_bf16a(const uint16_t* M, uint16_t* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino2d_output_adjoint_bf16a(const uint16_t* gy, uint16_t* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
/* F(2x4x4, 3x3x3) / F(4x4, 3x3): 4-wide tiles along h and w (Lavin & Gray's F(4,3)), 2-deep along d.  144 (2-D: 36)
 * frequencies, xi = (a*6 + e)*6 + f; T = B * D/2 * H/4 * W/4 (2-D: B * D * H/4 * W/4); needs H % 4 == W % 4 == 0
 * (3-D: D % 2 == 0).  Transformed domain 4.5x (2.25x) the activation instead of 8x (4x), GEMM stage 6x (4x) fewer
 * multiply-adds than the direct convolution.  Same roles as the ssbev_wino_* functions above; `_bf16` = bf16 storage of
 * the transformed-domain tensor. */
int ssbev_wino43_input_transform(const float* x, float* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_output_transform(const float* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_output_adjoint(const float* gy, float* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_2d_input_transform(const float* x, float* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_2d_output_transform(const float* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
/* y += transform(M): the data gradient of a second consumer of an activation is added to the first consumer's in the output
 * transform itself (functional.fork / GradSlot) instead of by a separate elementwise pass */
int ssbev_wino43_2d_output_transform_acc(const float* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino2d_output_transform_acc(const float* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_2d_output_adjoint(const float* gy, float* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_input_transform_bf16(const float* x, uint16_t* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_output_transform_bf16(const uint16_t* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_output_adjoint_bf16(const float* gy, uint16_t* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_2d_input_transform_bf16(const float* x, uint16_t* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_2d_output_transform_bf16(const uint16_t* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_2d_output_adjoint_bf16(const float* gy, uint16_t* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
/* F(4x4x4, 3x3x3): F(4,3) along d as well (D % 4 == 0): 216 frequencies per 64 outputs, T = B * D/4 * H/4 * W/4, 8x fewer
 * multiply-adds, 3.375x transformed domain.  Weight functions below: ndim = 4 selects this variant (3 = F(2x4x4), 2 = 2-D). */
int ssbev_wino444_input_transform(const float* x, float* V, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino444_output_transform(const float* M, float* y, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino444_output_adjoint(const float* gy, float* Z, const ssbev_wino_dims* d, ssbev_stream_t stream);
int ssbev_wino43_weight_transform(const float* w, float* U, int Cout, int Cin, int ndim, int mode, ssbev_stream_t stream);
int ssbev_wino43_weight_grad(const float* gU, float* gw, int Cout, int Cin, int ndim, ssbev_stream_t stream);
/* Weight side: U = G w G^T (mode 0: U [NF][Cin][Cout] from torch-layout w [Cout][Cin][taps]; mode 1: the data-gradient
 * operand [NF][Cout][Cin] from the mirrored taps), and gw = G^T gU G for the weight gradient.  ndim = 3 (27 taps, NF = 64)
 * or 2 (9 taps, NF = 16). */
int ssbev_wino_weight_transform(const float* w, float* U, int Cout, int Cin, int ndim, int mode, ssbev_stream_t stream);
int ssbev_wino_weight_grad(const float* gU, float* gw, int Cout, int Cin, int ndim, ssbev_stream_t stream);
/* Depth-fused frequency GEMM of the 3-D path: P = ssbev_wino2d_input_transform(x) [16][B*D*Thw][K] -> Mo [16][B*D*Thw][N]
 * (-> ssbev_wino2d_output_transform); the depth axis of F(2,3) is applied in registers (d->C = K input channels of this
 * product; mode 0 forward: K = Cin, N = Cout; mode 1 data gradient: K = Cout, N = Cin). */
size_t ssbev_wino_dgemm_packed_elems(int Cout, int Cin);
int ssbev_wino_dgemm_pack(const float* w, float* Wp, int Cout, int Cin, int mode, ssbev_stream_t stream);
int ssbev_wino_dgemm(const float* P, const float* Wp, float* Mo, const ssbev_wino_dims* d, int N, ssbev_stream_t stream);
/* Batched frequency GEMM of the plain 3-D pipeline: Cm[xi][T][N] = A[xi][T][K] x U[xi][K][N] for the 64 frequencies, A
 * streamed through LDS once, U in the ssbev_wino_dgemm_pack layout. */
int ssbev_wino_bgemm(const float* A, const float* Wp, float* Cm, int64_t T, int K, int N, ssbev_stream_t stream);
/* Host-side plan query (since ssbev_version() 124; no device work): the launch geometry of ssbev_wino_bgemm(T, K, N) (b_ group,
 * filled when T > 0) and of ssbev_wino_dgemm(d, N) (d_ group, filled when d is not NULL), from the plan functions the two
 * launchers themselves read; the group that is not asked for is zero.  SSBEV_EINVAL for a NULL `out`, when neither group is
 * asked for, and for arguments the launcher of a requested group refuses. */
typedef struct {
  int b_nt;                 /* wino_bgemm_kernel<NT>: 32-column tiles per wave */
  int b_ycols;              /* grid y: column groups of 4 NT 32 columns */
  int b_gx;                 /* grid x: persistent workgroups per (frequency, column group) */
  int b_nstage;             /* 64-column k-stages per row block */
  int64_t b_nrb, b_rb_per;  /* 64-row blocks, and row blocks per workgroup (workgroup x owns [x rb_per, (x + 1) rb_per)) */
  int d_mt, d_nt;           /* wino_dgemm_kernel<MT, NT> */
  int d_tgroups;            /* groups of 32 MT (h, w)-tiles per plane; a workgroup's four waves take four consecutive groups */
  int d_grid_x, d_grid_y, d_grid_z;
  int d_Q;                  /* k-steps of 8 channels */
  int d_CoutPad;            /* N rounded up to 32: the column stride of the packed weights */
} ssbev_wino_gemm_plan;
int ssbev_wino_gemm_plan_query(int64_t T, int K, int N, const ssbev_wino_dims* d, ssbev_wino_gemm_plan* out);

/* ------------------------------------------------------------------------------------------
 * Plain fp32 GEMMs on the matrix cores (csrc/gemm.hip): the layers that are matrix products in the channels-last layout
 * -- kernel == stride transposed convolutions of SECONDFPN3D (second_fpn_3d.py:50-69), wide pointwise convolutions
 * (ASPP 3200 -> 640), the DCN group contractions (BD:490-498), the six products of a BRI block (attention.py:72-81), the
 * batched frequency products of the 2-D Winograd layers.  Replaces the rocBLAS calls behind torch.mm / torch.bmm.
 *   nn: C[b][m][n] = sum_k A[b][m][k] B[b][k][n]      nt: ... W[b][n][k]      tn: C[b][k][n] = sum_r A[b][r][k] B[b][r][n]
 * Leading dimensions / batch strides in floats; K, N, lda, ldb multiples of 4.  d2s_*: depth-to-space index map of a k == s
 * transposed convolution (d2s_kd = 0: off): row m = coarse voxel (bb, d, h, w), wide index tap * Co + co <-> fine voxel
 * (d kd + a, h kh + b, w kw + c), channel co.  nn scatters C, nt gathers A, tn gathers B through it.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int M, N, K, batch;
  int64_t lda, ldb, ldc, sa, sb, sc;
  int relu;
  int d2s_D, d2s_H, d2s_W, d2s_kd, d2s_kh, d2s_kw, d2s_Co;
  const int64_t* d2s_rowoff;      /* device table of M row offsets (ssbev_gemm_d2s_rowoff), required when d2s_kd > 0 */
  /* ssbev_gemm_tn only, both or neither: C[b][k][n] = ep_mul[b][k][n] * ((A^T B)[b][k][n] - ep_rowsub[b][k]), ep_mul laid out
   * like C.  With A = grad_out, B = V conf, ep_mul = att, ep_rowsub[i] = <grad_out[:, i], out[:, i]> this is the softmax
   * backward gE = att (.) (gatt - rowsum(gatt (.) att)) of the BRI attention (attention.py:63-81) inside the product that
   * forms gatt: neither gatt nor a separate softmax-backward pass over the T x T matrices exists. */
  const float* ep_mul;
  const float* ep_rowsub;
} ssbev_gemm_dims;
int ssbev_gemm_d2s_rowoff(int64_t* rowoff, int M, int D, int H, int W, int kd, int kh, int kw, int Co, ssbev_stream_t stream);
size_t ssbev_gemm_nn_workspace(const ssbev_gemm_dims* d);      /* split-K partials (0 when the output tiles fill the chip) */
size_t ssbev_gemm_nt_workspace(const ssbev_gemm_dims* d);
int ssbev_gemm_nn(const float* A, const float* B, const float* bias, float* C, const ssbev_gemm_dims* d, void* workspace,
                  size_t ws_bytes, ssbev_stream_t stream);
int ssbev_gemm_nt(const float* A, const float* W, const float* bias, float* C, const ssbev_gemm_dims* d, void* workspace,
                  size_t ws_bytes, ssbev_stream_t stream);
size_t ssbev_gemm_tn_workspace(const ssbev_gemm_dims* d);
int ssbev_gemm_tn(const float* A, const float* B, float* C, const ssbev_gemm_dims* d, void* workspace, size_t ws_bytes,
                  ssbev_stream_t stream);
/* Host-side plan query (since ssbev_version() 106; no device work): the kernel, tile and chunking a launch of these dims uses,
 * from the plan function the launchers and the *_workspace queries themselves read.  form: 0 NN, 1 NT, 2 TN.  SSBEV_EINVAL for
 * dims the matching entry point refuses (d2s dims are answered like any other).
 * kernel codes --
 *   NN / NT: the tile configuration of gemm_nn_kernel: 0 = 128 x 128, 1 = 128 x 64, 2 = 192 x 128 (96-row wave tiles),
 *            3 = 128 x 160 (four waves stacked along M), 4 = 128 x 128 with 16-deep k stages (tuning builds only);
 *   TN:      10 = gemm_tn_kernel<1> (128 k x 64 n), 11 = gemm_tn_kernel<2> (128 x 128), 12 = gemm_tn_kernel<5, 1, 1> (128 x 160);
 *   skinny TN (gemm_tn_skinny_kernel<KT, NT, QUAD> + gemm_sum_wide_kernel): 20 = <1, 1>, 21 = <1, 2>, 22 = <2, 1>, 23 = <2, 2>,
 *            24 = <2, 2, quad>. */
typedef struct {
  int kernel;      /* see above */
  int bm, bn, bk;  /* workgroup tile (TN: k rows x n columns x 32 reduction rows; skinny: the tile a workgroup holds x 16 rows per step) */
  int nchunk;      /* split-K chunks (NN / NT), row chunks (TN), workgroups per batch element (skinny TN) */
  int per_chunk;   /* k stages per chunk (NN / NT), rows per chunk (TN), rows per run of a wave (skinny: 4 nchunk runs, quad: nchunk) */
  int64_t grid;    /* workgroups of the main launch */
  size_t workspace;/* bytes, what the form's *_workspace function returns */
} ssbev_gemm_plan;
int ssbev_gemm_plan_query(const ssbev_gemm_dims* d, int form, ssbev_gemm_plan* out);

/* Depth-fused Winograd contraction (csrc/winograd_fused.hip): F(4,3) x F(4,3) over (h, w) in memory (P / Mo / Z are
 * [36][B*D*(H/4)*(W/4)][C], the 2-D transforms above with D as a batch axis), F(2,3) along d in registers around the MFMAs.
 * The default realisation of the wide stride-1 3x3x3 layers (resnet3d.py:18-32, second_fpn_3d.py:53-69, occhead.py:100-107):
 * forward / data gradient = ssbev_wino43_2d_input_transform -> ssbev_wino43_df_gemm -> ssbev_wino43_2d_output_transform,
 * weight gradient = ssbev_wino43_2d_output_adjoint(gy) + ssbev_wino43_df_wgrad(P saved by the forward).
 * d = (B, D, H, W, C = K).  Supported when H % 4 == W % 4 == 0, D even, K % 32 == 0. */
int ssbev_wino43_df_supported(const ssbev_wino_dims* d, int N);
/* template instance of the contraction kernel a problem runs on: MT * 10 + NW of wino_df_kernel<MT, NW> (0: unsupported dims) --
 * lets a profiler attribute launches to kernel symbols (bench.py picks its roofline kernel by summed time per SYMBOL) */
int ssbev_wino43_df_instance(const ssbev_wino_dims* d, int N);
size_t ssbev_wino43_df_packed_elems(int Cout, int Cin);
int ssbev_wino43_df_pack(const float* w, float* Wp, int Cout, int Cin, int mode, ssbev_stream_t stream);
int ssbev_wino43_df_gemm(const float* P, const float* Wp, float* Mo, const ssbev_wino_dims* d, int N, ssbev_stream_t stream);
size_t ssbev_wino43_df_wgrad_workspace(const ssbev_wino_dims* d, int N);
int ssbev_wino43_df_wgrad(const float* P, const float* Z, float* gw, const ssbev_wino_dims* d, int N, void* workspace,
                          size_t ws_bytes, ssbev_stream_t stream);
/* Host-side plan query (since ssbev_version() 108; no device work): the kernel instance and launch geometry of
 * ssbev_wino43_df_gemm (first group) and ssbev_wino43_df_wgrad (w_ group) for these dims, from the plan functions the launchers,
 * ssbev_wino43_df_instance and ssbev_wino43_df_wgrad_workspace themselves read.  SSBEV_EINVAL for a NULL argument and for dims
 * ssbev_wino43_df_supported refuses.  (ssbev_wino43_df_wgrad additionally refuses B D (H/4) (W/4) max(K, N) >= 2^31.) */
typedef struct {
  int mt, nw;               /* wino_df_kernel<MT, NW>: 32-row tiles per wave, waves per workgroup (instance = 10 mt + nw) */
  int ncolgrp, nrowgrp;     /* column groups of 32 nw columns, row groups of 32 mt hw-tiles per (b, depth tile) */
  int nst;                  /* k-stages of 32 channels */
  int64_t grid;             /* workgroups = 36 B (D/2) nrowgrp ncolgrp */
  size_t lds_bytes;         /* dynamic LDS per workgroup */
  int w_kw, w_nt, w_br;     /* wino_dfw_kernel<KW, NT, BR>: k-waves, 32-column tiles per wave, rows per stage */
  int w_nkb, w_nnb;         /* blocks of 32 kw channels / (4 / kw) nt 32 columns */
  int w_nchunk;             /* row chunks (partial sums; > 1: wino_dfw_sum_kernel runs) */
  int w_stages_per_chunk;   /* stages of a chunk (the last chunk may be shorter) */
  int w_total_stages;       /* B (D/2) ceil((H/4)(W/4) / br) */
  int64_t w_grid;           /* workgroups = 36 nchunk nkb nnb */
  size_t w_lds_bytes;       /* dynamic LDS per workgroup */
  size_t w_workspace;       /* bytes, what ssbev_wino43_df_wgrad_workspace returns */
} ssbev_wino43_df_plan;
int ssbev_wino43_df_plan_query(const ssbev_wino_dims* d, int N, ssbev_wino43_df_plan* out);

#ifdef __cplusplus
}
#endif
#endif /* SSBEV_H */
