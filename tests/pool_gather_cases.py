"""Case tables of the pool-gather parity tests (test_pool_gather_cases.py on the CPU, test_gpu_pool_gather.py on the GPU).

``launch_gather`` and ``ssbev_lift_splat_bwd`` (csrc/voxel_pool.hip) choose among eight forward gather instantiations and four
backward kernels by the channel count C and by whether the long-voxel work list of ``ssbev_pool_prepare2`` was passed.  The
frustum geometry of the other tests reaches only C = 128 and C = 12, one camera, D a multiple of 4, and whatever list lengths
the geometry happens to produce.  The tables here are HANDCRAFTED voxel tables instead: a case is a set of dims
(B, N, D, H, W, grid) and a seeded ``vox[B * P]`` (P = N * D * H * W) built from per-voxel target list lengths, so that every
chunk edge of every kernel (4, 16, 32 | 33, 64, ...), the stride loops over the work list and the depth-plane split of the
backward are hit on purpose.  ``F.lift_splat(..., tables=(vox, starts, order))`` takes such tables directly.

Point p = ((b * N + n) * D + d) * HW + pix reads feature row (b * N + n) * HW + pix and depth[p].

References (plain numpy):
  * ``pool_seq32``: per voxel, ascending point id, the product rounded to fp32 and then added in fp32 -- the arithmetic of
    ``oracle.path_ref.bev_pool``, which the kernels reproduce bit for bit;
  * ``pool_f64`` / ``grads_f64``: float64 values of the output and of both gradients."""
import collections
import functools

import numpy as np
import torch

from stereoscene_amd import synthetic as S

POOL_LONG = 32          # lists longer than this take the whole-wave / work-list paths (csrc/voxel_pool.hip)

Table = collections.namedtuple("Table", "name B N D H W grid vox lengths")

# channel counts -> kernel family (read from launch_gather / ssbev_lift_splat_bwd):
#   forward, work list passed (F.GATHER_SPLIT):  128 pool_gather7<true>;  64 / 256 pool_gather_long + pool_gather_short<true, 1 | 4>
#   forward, no work list (GATHER_SPLIT off, ssbev_lift_splat_fwd, bev_pool):  64 / 128 / 256 pool_gather5<*, 1 | 2 | 4>
#   forward, any other C:  pool_gather2, VEC 4 (C % 256 == 0: 512, two channel passes), VEC 2 (even: 20, 72, 132 -- 132 with a
#                          second pass of two live lanes, 16 for bev_pool), VEC 1 (odd: 7, 67 -- 67 with a second pass)
#   backward:  64 / 128 / 256 lift_splat_bwd2<16 | 32 | 64>;  20, 72, 132, 512 lift_splat_bwd (1, 2, 3, 8 slabs of 64 channels)
CHANNELS = {"fused": (20, 64, 72, 128, 132, 256, 512), "forward_only": (7, 67), "bev_pool": (7, 16, 64, 128, 256)}

RAGGED_REQUIRED = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 96, 97, 129)
DEPTH_PLANES = (1, 2, 3, 7, 13, 64, 260, 263)
KEPT_PATTERNS = ("all", "none", "quarter")
BWD_DEPTH_CHANNELS = (64, 128, 256, 72)


def vox_per_batch(t):
    return t.grid[0] * t.grid[1] * t.grid[2]


def points_per_batch(t):
    return t.N * t.D * t.H * t.W


def _perm(name, n):
    """Seeded permutation of range(n): the ranks of a hashed uniform (no RNG state, the same on every machine)."""
    return np.argsort(S.hash_uniform(name, (n,)).numpy(), kind="stable")


def _hash_int(name, n, lo, hi):
    """n hashed integers in [lo, hi]."""
    u = S.hash_uniform(name, (n,), 0.0, 1.0).numpy().astype(np.float64)
    return np.minimum(lo + (u * (hi - lo + 1)).astype(np.int64), hi)


def build_table(name, B, N, D, H, W, grid, lengths):
    """``lengths[b][i]`` = target list length of voxel i of batch element b.  The points of a voxel are drawn through a seeded
    permutation of the batch element's own points (scattered and interleaved in point order, never contiguous, and inside the
    batch element's voxel range as the fused kernels assume); what is left over is dropped (-1)."""
    P, vpb = N * D * H * W, grid[0] * grid[1] * grid[2]
    vox = np.full(B * P, -1, dtype=np.int32)
    for b in range(B):
        ln = np.asarray(lengths[b], dtype=np.int64)
        assert ln.shape == (vpb,) and ln.min() >= 0 and ln.sum() <= P, (name, b, ln.shape, int(ln.sum()), P)
        ids = np.repeat(np.arange(vpb, dtype=np.int64), ln)
        vox[b * P + _perm(f"{name}/perm{b}", P)[:len(ids)]] = b * vpb + ids
    return Table(name, B, N, D, H, W, tuple(grid), vox, tuple(tuple(int(x) for x in l) for l in lengths))


# ------------------------------------------------------------------------------------------------- RAGGED
# Two cameras, D = 5 (not a multiple of 4: ragged planes per wave in the backward), 5 x 7 x 3 = 105 cells per batch element
# (a wave's four voxels straddle the batch boundary, nv = 210 is no multiple of 4).  Batch 0: voxel 0 empty, voxels 4..7 = one
# wave's four voxels, all long (the `todo` ballot loop of pool_gather5 walks four), every chunk edge of the short role (4, 16),
# of gather7's LDS chunks (16), of the whole-wave path (32, 64) and the POOL_LONG boundary (32 | 33).  Batch 1: the same lists in
# reverse order (the four long neighbours then straddle two waves) and a long last voxel.
_FILL = (0, 2, 7, 0, 12, 1, 0, 20, 6, 0, 9, 32)


def _ragged():
    l0 = [0, 1, 3, 4, 33, 129, 34, 65, 5, 15, 16, 17, 31, 32, 47, 48, 49, 63, 64, 96, 97]
    l0 += [_FILL[i % len(_FILL)] for i in range(105 - len(l0))]
    l1 = l0[:0:-1] + [40]
    return build_table("RAGGED", 2, 2, 5, 11, 17, (5, 7, 3), [l0, l1])


def _many_long(name, D, H, W, grid, n_long, n_short, long_len):
    """Per batch element: ``n_long`` voxels at hashed positions with lengths from ``long_len``, ``n_short`` with 1..32, rest empty."""
    vpb = grid[0] * grid[1] * grid[2]
    lengths = []
    for b in range(2):
        rank = _perm(f"{name}/sel{b}", vpb)
        ln = np.zeros(vpb, dtype=np.int64)
        ln[rank[:n_long]] = long_len(f"{name}/len{b}", n_long)
        ln[rank[n_long:n_long + n_short]] = _hash_int(f"{name}/short{b}", n_short, 1, POOL_LONG)
        lengths.append(ln)
    return build_table(name, 2, 2, D, H, W, grid, lengths)


def _len_128(name, n):
    return _hash_int(name, n, 33, 80)       # 3..5 LDS chunks of 16: the chunk count differs between a workgroup's two voxels


def _len_split(name, n):
    ln = _hash_int(name, n, 33, 46)
    ln[::16] = _hash_int(name + "/far", len(ln[::16]), 64, 80)      # some lists with a second 64-point block
    return ln


@functools.lru_cache(maxsize=None)
def table(name):
    if name == "RAGGED":
        return _ragged()
    if name == "MANY_LONG_128":       # 2 x 576 long voxels > pool_gather7's 1024 long-role workgroups: 128 of them take a second voxel
        return _many_long(name, 16, 31, 40, (16, 16, 8), 576, 128, _len_128)
    if name == "MANY_LONG_SPLIT":     # 2 x 1032 long voxels > pool_gather_long's 2048 waves
        return _many_long(name, 16, 31, 50, (16, 16, 10), 1032, 64, _len_split)
    raise KeyError(name)


TABLES = ("RAGGED", "MANY_LONG_128", "MANY_LONG_SPLIT")
MIN_LONG = {"MANY_LONG_128": 1025, "MANY_LONG_SPLIT": 2049}


@functools.lru_cache(maxsize=None)
def depth_table(D, kept):
    """Backward cases: one camera, one batch element, 2 x 3 pixels, D planes; every point kept / none / about a quarter (the
    frustum's ratio).  lift_splat_bwd2 gives each of its four waves (D + 3) >> 2 planes and walks them 64 at a time."""
    H, W, grid = 2, 3, (3, 3, 2)
    n = D * H * W
    name = f"DEPTHS/{D}/{kept}"
    vox = _hash_int(name + "/vox", n, 0, 17).astype(np.int32)
    if kept == "none":
        vox[:] = -1
    elif kept == "quarter":
        vox[S.hash_uniform(name + "/keep", (n,), 0.0, 1.0).numpy() >= 0.25] = -1
    else:
        assert kept == "all"
    return Table(name, 1, 1, D, H, W, grid, vox, None)


# ------------------------------------------------------------------------------------------------- inputs
def depth_input(t, tag="depth"):
    """softmax over D of a hashed normal: [B * N, D, H, W] fp32."""
    return torch.softmax(S.hash_normal(f"{t.name}/{tag}", (t.B * t.N, t.D, t.H, t.W), 2.0), 1)


def feat_rows(t, C):
    """feature rows [B * N * H * W, C] fp32 (the channels-last buffer of the [B * N, C, H, W] feature map)."""
    return S.hash_normal(f"{t.name}/feat{C}", (t.B * t.N * t.H * t.W, C))


def gout_rows(t, C):
    """grad_out rows [nv, C] fp32 (the channels-last buffer of the [B, C, X, Y, Z] output gradient)."""
    return S.hash_normal(f"{t.name}/go{C}", (t.B * vox_per_batch(t), C))


def feat_nchw(t, rows):
    C = rows.shape[1]
    return rows.view(t.B * t.N, t.H, t.W, C).permute(0, 3, 1, 2)


def out_rows(t, out):
    """[B, C, X, Y, Z] (logical) -> rows [nv, C]."""
    return out.permute(0, 2, 3, 4, 1).reshape(t.B * vox_per_batch(t), -1)


def gout_logical(t, rows):
    return rows.view(t.B, *t.grid, rows.shape[1]).permute(0, 4, 1, 2, 3)


def coords_of(t):
    """(ix, iy, iz, b) int64 [B * P, 4] of every point; dropped points get ix = -1."""
    nx, ny, nz = t.grid
    v = t.vox.astype(np.int64)
    c = np.stack([v // (ny * nz) % nx, v // nz % ny, v % nz, v // (nx * ny * nz)], 1)
    c[v < 0] = (-1, 0, 0, 0)
    return torch.from_numpy(c)


# ------------------------------------------------------------------------------------------------- references
def point_rows(t):
    """feature row of every point."""
    P, HW = points_per_batch(t), t.H * t.W
    p = np.arange(t.B * P, dtype=np.int64)
    b, q = p // P, p % P
    return (b * t.N + q // (t.D * HW)) * HW + q % HW


def csr(t):
    """(counts [nv], starts [nv], order [kept]): the voxel -> ascending point id lists."""
    nv = t.B * vox_per_batch(t)
    v = t.vox.astype(np.int64)
    ids = np.flatnonzero(v >= 0)
    order = ids[np.argsort(v[ids], kind="stable")]
    counts = np.bincount(v[ids], minlength=nv)
    return counts, np.concatenate([[0], np.cumsum(counts)])[:-1], order


def _walk(t, depth, rows, dtype, absolute=False):
    """Sum of depth[p] * feat[row(p)] per voxel, sequentially over the list position (a loop over positions, vectorised over
    voxels): in ``dtype`` arithmetic -- for float32 every product is rounded, then added."""
    counts, starts, order = csr(t)
    w = depth.numpy().reshape(-1).astype(dtype)
    f = rows.numpy().astype(dtype)
    prow = point_rows(t)
    acc = np.zeros((len(counts), f.shape[1]), dtype=dtype)
    for j in range(int(counts.max()) if len(order) else 0):
        live = np.flatnonzero(counts > j)
        p = order[starts[live] + j]
        term = w[p][:, None] * f[prow[p]]
        acc[live] = acc[live] + (np.abs(term) if absolute else term)
    assert acc.dtype == dtype
    return acc


def pool_seq32(t, depth, rows):
    """fp32 sequential sums [nv, C]: what the gather kernels must reproduce bit for bit."""
    return torch.from_numpy(_walk(t, depth, rows, np.float32))


def pool_f64(t, depth, rows):
    """(float64 sums, float64 sums of |depth * feat|) [nv, C]."""
    return _walk(t, depth, rows, np.float64), _walk(t, depth, rows, np.float64, absolute=True)


def grads_f64(t, depth, rows, gout):
    """float64 (grad_depth [B * P], grad_feat [rows, C]): grad_depth[p] = <gout[vox[p]], feat[row(p)]>,
    grad_feat[row] = sum over the row's planes of depth[p] * gout[vox[p]]; dropped points contribute 0."""
    v = t.vox.astype(np.int64)
    kept = v >= 0
    g = gout.numpy().astype(np.float64)[np.where(kept, v, 0)] * kept[:, None]
    f = rows.numpy().astype(np.float64)
    prow = point_rows(t)
    gd = (g * f[prow]).sum(1)
    gf = np.zeros_like(f)
    np.add.at(gf, prow, depth.numpy().reshape(-1).astype(np.float64)[:, None] * g)
    return gd, gf


@functools.lru_cache(maxsize=None)
def forward_case(name, C, depth_tag="depth"):
    """(table, depth, feature rows, fp32 sequential reference) of a table at C channels: computed once, shared, never changed."""
    t = table(name)
    depth, rows = depth_input(t, depth_tag), feat_rows(t, C)
    return t, depth, rows, pool_seq32(t, depth, rows)


# ------------------------------------------------------------------------------------------------- CSR tables of the sort test
def csr_tables():
    """(vox int32, B, nx, ny, nz): the tables of test_pool_prepare_csr_is_a_stable_sort's kind -- random with dropped points,
    clustered like a frustum (long lists on few voxels), one voxel taking everything, everything dropped."""
    g = torch.Generator().manual_seed(7)
    out = []
    for (n, B, nx, ny, nz) in [(100000, 2, 32, 32, 8), (5000, 1, 7, 5, 3), (37, 1, 4, 4, 2), (70000, 1, 128, 128, 16), (1, 1, 1, 1, 1)]:
        nv = B * nx * ny * nz
        vox = torch.randint(-nv // 4 - 1, nv, (n,), generator=g, dtype=torch.int64).clamp_(min=-1).to(torch.int32)
        out.append((vox, B, nx, ny, nz))
    hot = torch.randint(0, 64, (200000,), generator=g) * 517 + 11
    out.append((hot.to(torch.int32), 1, 128, 128, 16))
    out.append((torch.full((3000,), 4242, dtype=torch.int32), 1, 32, 32, 8))
    out.append((torch.full((3000,), -1, dtype=torch.int32), 1, 32, 32, 8))
    return out


def all_32_table():
    """64 voxels of exactly POOL_LONG points each (no long voxel), and the same table with one point moved from voxel 5 to
    voxel 9 (one long voxel: 9)."""
    vox = (_perm("ALL32/perm", 64 * POOL_LONG) % 64).astype(np.int32)
    moved = vox.copy()
    moved[np.flatnonzero(vox == 5)[0]] = 9
    return torch.from_numpy(vox), torch.from_numpy(moved), (1, 4, 4, 4)
