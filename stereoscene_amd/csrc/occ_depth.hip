// Occupancy -> dense depth map / image-view segmentation (CreateDepthFromOccupancy, datasets/pipelines/occ_to_depth.py:15-153:
// the second producer of the `gt_depths` slot of img_inputs and of `img_seg`, from nothing but the voxel labels `gt_occ`).
// Upstream projects all X Y Z voxel centres on the CPU (five broadcast matmuls), sorts the visible ones by depth (descending,
// twice) and lets an index_put with "last write wins" keep the nearest voxel per pixel; with downsample=True a Python double loop
// pools the label map per 16 x 16 patch.  Here, following lidar_depth.hip: one thread per voxel projects its centre with the same
// fp32 operation order (built with -ffp-contract=off), and the nearest voxel per pixel is a 64-bit atomicMin on
// (depth bits << 32 | flat voxel index) -- for positive floats the IEEE bit pattern is monotone, so the minimum is the nearest
// voxel.  DEFINITION: among voxels of one pixel with exactly equal fp32 depth the LOWEST flat index (x Y Z + y Z + z) wins;
// upstream's unstable argsort leaves such ties unspecified.  Two key buffers: the depth map takes voxels labelled 1..254
// (:122), the segmentation map every in-view voxel, empty (0) and ignored (255) ones included (:133: they occlude), or -- with
// seg_occupied -- the depth map's own voxels, and then one buffer serves both.  Integer / bit-pattern work: 2 M label bytes read,
// at most 2 x 2 M atomics into 2 x 0.5 M keys that stay in L2.
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"

namespace {

struct OccCam {
  float inv_bda[12];    // bda^-1, first three rows of 3 x 4 row major (fourth column unused for a 3 x 3 bda)
  float inv_rot[9];     // rots^-1, row major
  float trans[3];
  float K[16];          // intrins, 4 x 4 row major
  float post_rot[4];    // post_rots[:2, :2]
  float post_trans[2];
};
static_assert(sizeof(OccCam) == 46 * sizeof(float), "the 46 camera floats of ssbev_occ_depth_map");

constexpr unsigned long long OCC_NONE = ~0ull;

__global__ void __launch_bounds__(256)
occ_project_kernel(const unsigned char* __restrict__ labels, const float* __restrict__ xs, const float* __restrict__ ys,
                   const float* __restrict__ zs, OccCam c, int bda4, int seg_occupied, unsigned long long* __restrict__ zdepth,
                   unsigned long long* __restrict__ zseg, unsigned Y, unsigned Z, unsigned long long N, int H, int W) {
  const unsigned long long stride = (unsigned long long)gridDim.x * 256;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
    const unsigned lab = labels[i];
    const bool occupied = lab != 0 && lab != 255;
    if (seg_occupied && !occupied) continue;
    const unsigned long long xy = i / Z;
    const float px = xs[xy / Y], py = ys[xy % Y], pz = zs[i % Z];
    // augmented lidar -> lidar: bda^-1 p                   (project_points, occ_to_depth.py:45-46)
    float lx = (c.inv_bda[0] * px + c.inv_bda[1] * py) + c.inv_bda[2] * pz;
    float ly = (c.inv_bda[4] * px + c.inv_bda[5] * py) + c.inv_bda[6] * pz;
    float lz = (c.inv_bda[8] * px + c.inv_bda[9] * py) + c.inv_bda[10] * pz;
    if (bda4) { lx += c.inv_bda[3]; ly += c.inv_bda[7]; lz += c.inv_bda[11]; }     // a 4 x 4 bda: [p; 1]
    // lidar -> camera: R^-1 (p - t)                         (:49-52)
    const float x = lx - c.trans[0], y = ly - c.trans[1], z = lz - c.trans[2];
    const float cx = (c.inv_rot[0] * x + c.inv_rot[1] * y) + c.inv_rot[2] * z;
    const float cy = (c.inv_rot[3] * x + c.inv_rot[4] * y) + c.inv_rot[5] * z;
    const float cz = (c.inv_rot[6] * x + c.inv_rot[7] * y) + c.inv_rot[8] * z;
    // camera -> raw pixel: K [p; 1]                         (:55-58)
    const float qx = ((c.K[0] * cx + c.K[1] * cy) + c.K[2] * cz) + c.K[3];
    const float qy = ((c.K[4] * cx + c.K[5] * cy) + c.K[6] * cz) + c.K[7];
    const float d = ((c.K[8] * cx + c.K[9] * cy) + c.K[10] * cz) + c.K[11];
    const float u0 = qx / d, v0 = qy / d;
    // raw pixel -> augmented pixel                          (:61-62)
    const float u = (c.post_rot[0] * u0 + c.post_rot[1] * v0) + c.post_trans[0];
    const float v = (c.post_rot[2] * u0 + c.post_rot[3] * v0) + c.post_trans[1];
    const bool ok = u >= 0.0f && v >= 0.0f && u <= (float)(W - 1) && v <= (float)(H - 1) && d > 0.0f;    // :112-116 (a NaN fails)
    if (!ok) continue;
    const int col = (int)rintf(u), row = (int)rintf(v);            // torch.round: half to even; 0 <= col <= W-1, 0 <= row <= H-1
    const size_t pix = (size_t)row * W + col;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
    if (occupied) atomicMin(&zdepth[pix], key);                    // :122
    if (!seg_occupied) atomicMin(&zseg[pix], key);                 // :133
  }
}

__global__ void __launch_bounds__(256)
occ_resolve_kernel(const unsigned long long* __restrict__ zdepth, const unsigned long long* __restrict__ zseg,
                   const unsigned char* __restrict__ labels, float* __restrict__ depth, float* __restrict__ seg, int HW) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const unsigned long long kd = zdepth[i], ks = zseg[i];
  depth[i] = kd != OCC_NONE ? __uint_as_float((unsigned)(kd >> 32)) : 0.0f;                  // :121, :127
  seg[i] = ks != OCC_NONE ? (float)labels[(unsigned)(ks & 0xffffffffu)] : 255.0f;            // :132, :140
}

// _downsample_label (:67-93): one workgroup per ds x ds patch, a 256-bin histogram in LDS, then the fold of (count, lowest id)
// over the classes 1..254.  A map value outside 0..255 (or NaN) counts as 255.
__global__ void __launch_bounds__(256)
label_map_pool_kernel(const float* __restrict__ seg, float* __restrict__ out, int W, int ow, int ds, float empty_t) {
  __shared__ unsigned hist[256];
  __shared__ unsigned best[256];
  const int tid = threadIdx.x;
  const int pi = blockIdx.x / ow, pj = blockIdx.x - pi * ow;
  hist[tid] = 0;
  __syncthreads();
  for (int t = tid; t < ds * ds; t += 256) {
    const int r = t / ds, q = t - r * ds;
    const float v = seg[(size_t)(pi * ds + r) * W + pj * ds + q];
    const int l = (v >= 0.0f && v <= 255.0f) ? (int)v : 255;
    atomicAdd(&hist[l], 1u);
  }
  __syncthreads();
  // count in the high bits, 255 - id below: the maximum is the larger count, then the LOWER id (torch.mode's choice on a tie)
  best[tid] = (tid >= 1 && tid <= 254) ? (hist[tid] << 8) | (unsigned)(255 - tid) : 0u;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) best[tid] = max(best[tid], best[tid + off]);
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned z0 = hist[0], z255 = hist[255];
    float r;
    if ((float)(z0 + z255) > empty_t) r = z0 > z255 ? 0.0f : 255.0f;              // :87-88
    else r = (float)(255 - (int)(best[0] & 0xffu));                               // :90-91
    out[blockIdx.x] = r;
  }
}

}  // namespace

extern "C" {

size_t ssbev_occ_depth_workspace(int H, int W) {
  if (H <= 0 || W <= 0 || (size_t)H * W > (size_t)INT_MAX - 256) return 0;
  return 2 * (size_t)H * W * sizeof(unsigned long long);
}

/* see include/ssbev.h */
int ssbev_occ_depth_map(const uint8_t* labels, int X, int Y, int Z, const float* xs, const float* ys, const float* zs,
                        const float* cam46, int bda_cols, int seg_occupied, float* depth, float* seg, int H, int W, void* ws,
                        size_t ws_bytes, ssbev_stream_t stream) {
  if (!labels || !xs || !ys || !zs || !cam46 || !depth || !seg || !ws) return SSBEV_EINVAL;
  if (X <= 0 || Y <= 0 || Z <= 0 || H <= 0 || W <= 0 || (bda_cols != 3 && bda_cols != 4)) return SSBEV_EINVAL;
  if ((size_t)H * W > (size_t)INT_MAX - 256) return SSBEV_EINVAL;
  const unsigned long long XY = (unsigned long long)X * Y;
  if (XY > (1ull << 32) || XY * Z > (1ull << 32)) return SSBEV_EINVAL;       // the key's low word holds the flat voxel index
  const unsigned long long N = XY * Z;
  if (ws_bytes < ssbev_occ_depth_workspace(H, W)) return SSBEV_EWORKSPACE;
  OccCam c;
  std::memcpy(&c, cam46, sizeof(OccCam));                      // HOST pointer: no copy on the stream, no synchronisation
  hipStream_t st = as_stream(stream);
  const size_t HW = (size_t)H * W;
  unsigned long long* zdepth = static_cast<unsigned long long*>(ws);
  unsigned long long* zseg = seg_occupied ? zdepth : zdepth + HW;
  if (hipMemsetAsync(zdepth, 0xff, (seg_occupied ? 1 : 2) * HW * sizeof(unsigned long long), st) != hipSuccess) return SSBEV_ELAUNCH;
  const unsigned long long nb = (N + 255) / 256;
  const unsigned grid = (unsigned)(nb < 16384 ? nb : 16384);   // grid-stride above 4 M voxels
  hipLaunchKernelGGL(occ_project_kernel, dim3(grid), dim3(256), 0, st, labels, xs, ys, zs, c, bda_cols == 4 ? 1 : 0,
                     seg_occupied ? 1 : 0, zdepth, zseg, (unsigned)Y, (unsigned)Z, N, H, W);
  hipLaunchKernelGGL(occ_resolve_kernel, dim3(cdiv(HW, 256)), dim3(256), 0, st, zdepth, zseg, labels, depth, seg, (int)HW);
  return ssbev_launch_status();
}

int ssbev_label_map_downsample(const float* seg, float* out, int H, int W, int ds, float empty_t, ssbev_stream_t stream) {
  if (!seg || H <= 0 || W <= 0 || ds <= 0 || ds > 256 || (size_t)H * W > (size_t)INT_MAX - 256 || !(empty_t == empty_t))
    return SSBEV_EINVAL;
  const int oh = H / ds, ow = W / ds;
  if (oh == 0 || ow == 0) return SSBEV_OK;                     // an empty result: nothing to write
  if (!out) return SSBEV_EINVAL;
  hipLaunchKernelGGL(label_map_pool_kernel, dim3((unsigned)(oh * ow)), dim3(256), 0, as_stream(stream), seg, out, W, ow, ds, empty_t);
  return ssbev_launch_status();
}

}  // extern "C"
