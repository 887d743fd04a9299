"""Float64 reference of the Winograd transforms and frequency GEMMs of csrc/winograd.hip, written from the matrices.

Nothing here is shared with the kernels' add chains: every transform is the textbook  Y = A^T [ (G g G^T) (.) (B^T d B) ] A,
applied separably with one einsum over explicit matrices (torch float64 on the CPU).  test_wino_ref.py proves the reference
against torch's float64 convolutions before test_gpu_wino_transforms.py measures a kernel against it.

Axis families.  An axis is tiled by F(2,3) ("23": 2 outputs, 4 inputs per tile), by F(4,3) ("43", Lavin & Gray: 4 outputs, 6
inputs) or not at all (None: a batch axis, every plane its own "tile", 1 x 1 identity matrices, one tap).  A tile of m outputs
starts at output m t and reads the inputs m t - 1 .. m t + m (offset -1, zeros outside the map).

Tilings (TILINGS): families along (d, h, w).
  w3d     ("23", "23", "23")   F(2x2x2, 3x3x3), 64 frequencies              ssbev_wino_*
  w2d     (None, "23", "23")   F(2x2, 3x3), 16 frequencies, D a batch axis  ssbev_wino2d_*   (dil <= 1)
  w43_2d  (None, "43", "43")   F(4x4, 3x3), 36 frequencies, DA = 0          ssbev_wino43_2d_*
  w43     ("23", "43", "43")   F(2x4x4, 3x3x3), 144 frequencies, DA = 2     ssbev_wino43_*
  w444    ("43", "43", "43")   F(4x4x4, 3x3x3), 216 frequencies, DA = 4     ssbev_wino444_*

Layouts.  Activations are channels-last [B][D][H][W][C].  Transformed tensors are [NF][T][C] with the frequency index
xi = (a na_h + e) na_w + f  (a: d axis, e: h, f: w; 4 or 6 or 1 entries per axis) and the tile index T ordered (b, td, th, tw);
in the 2-D tilings td runs over all D planes.  Weights are torch's [Cout][Cin][taps]; U is [NF][K][N].

Magnitude companions.  Every transform takes ``absolute=True``: the same transform with |coefficients| applied to |input|.
It bounds every intermediate of any evaluation order, so  n 2^-24 magnitude  bounds the fp32 error of a kernel whose longest
chain of roundings has length n (``chain`` below computes n from the matrices)."""
import torch

F64 = torch.float64


def _m(rows):
    return torch.tensor(rows, dtype=F64)


class Family:
    """One axis: m outputs and n = m + r - 1 inputs per tile, r taps, halo `pad`; Bt [n][n], G [n][r], At [m][n]."""

    def __init__(self, name, Bt, G, At, pad):
        self.name, self.Bt, self.G, self.At, self.pad = name, _m(Bt), _m(G), _m(At), pad
        self.m, self.n = self.At.shape
        self.r = self.G.shape[1]
        assert self.Bt.shape == (self.n, self.n) and self.G.shape[0] == self.n and self.n == self.m + self.r - 1


F23 = Family("23",
             Bt=[[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
             G=[[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]],
             At=[[1, 1, 1, 0], [0, 1, -1, -1]], pad=1)
F43 = Family("43",
             Bt=[[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                 [0, 4, 0, -5, 0, 1]],
             G=[[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                [0, 0, 1]],
             At=[[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], pad=1)
BATCH = Family(None, Bt=[[1]], G=[[1]], At=[[1]], pad=0)
FAMILIES = {"23": F23, "43": F43, None: BATCH}

TILINGS = {"w3d": ("23", "23", "23"), "w2d": (None, "23", "23"), "w43_2d": (None, "43", "43"), "w43": ("23", "43", "43"),
           "w444": ("43", "43", "43")}


def families(tiling):
    return tuple(FAMILIES[f] for f in TILINGS[tiling])


def nfreq(tiling):
    fd, fh, fw = families(tiling)
    return fd.n * fh.n * fw.n


def tile_counts(tiling, D, H, W):
    """(Td, Th, Tw); the extents must be multiples of the outputs per tile."""
    out = []
    for fam, n in zip(families(tiling), (D, H, W)):
        assert n % fam.m == 0, (tiling, D, H, W)
        out.append(n // fam.m)
    return tuple(out)


def ntiles(tiling, B, D, H, W):
    td, th, tw = tile_counts(tiling, D, H, W)
    return B * td * th * tw


def _mats(tiling, which, absolute, negate=None):
    """The three matrices `which` ("Bt" / "G" / "At") of a tiling.  negate = (axis, row, col): that one coefficient with the
    opposite sign -- the deliberately wrong reference of the negative controls."""
    ms = [getattr(f, which).clone() for f in families(tiling)]
    if negate is not None:
        ax, i, j = negate
        assert ms[ax][i, j] != 0
        ms[ax][i, j] = -ms[ax][i, j]
    return [m.abs() for m in ms] if absolute else ms


def _prep(t, absolute):
    t = torch.as_tensor(t).detach().to("cpu", F64)
    return t.abs() if absolute else t


# ------------------------------------------------------------------------------------------------------------- activations
def input_transform(x, tiling, absolute=False, negate=None):
    """x [B][D][H][W][C] -> V [NF][T][C] = B^T d B per axis, d the tile with its halo (zeros outside the map)."""
    x = _prep(x, absolute)
    fams = families(tiling)
    B, D, H, W, C = x.shape
    tile_counts(tiling, D, H, W)
    pd, ph, pw = (f.pad for f in fams)
    t = torch.nn.functional.pad(x, (0, 0, pw, pw, ph, ph, pd, pd))
    for ax, f in zip((1, 2, 3), fams):
        t = t.unfold(ax, f.n, f.m)                    # [B][Td][Th][Tw][C] + one trailing axis of n inputs per tiled axis
    bd, bh, bw = _mats(tiling, "Bt", absolute, negate)
    V = torch.einsum("ai,ej,fk,btuvcijk->aefbtuvc", bd, bh, bw, t)
    return V.reshape(nfreq(tiling), -1, C)


def _to_tiles(M, tiling, dims):
    B, D, H, W = dims
    fd, fh, fw = families(tiling)
    td, th, tw = tile_counts(tiling, D, H, W)
    return M.reshape(fd.n, fh.n, fw.n, B, td, th, tw, M.shape[-1])


def output_transform(M, tiling, dims, absolute=False, negate=None):
    """M [NF][T][C] -> y [B][D][H][W][C] = A^T M A per axis; dims = (B, D, H, W)."""
    M = _prep(M, absolute)
    ad, ah, aw = _mats(tiling, "At", absolute, negate)
    y = torch.einsum("ia,je,kf,aefbtuvc->btiujvkc", ad, ah, aw, _to_tiles(M, tiling, dims))
    B, D, H, W = dims
    return y.reshape(B, D, H, W, M.shape[-1])


def output_adjoint(g, tiling, absolute=False, negate=None):
    """g [B][D][H][W][C] -> Z [NF][T][C] = A g A^T per axis (the adjoint of output_transform)."""
    g = _prep(g, absolute)
    fd, fh, fw = families(tiling)
    B, D, H, W, C = g.shape
    td, th, tw = tile_counts(tiling, D, H, W)
    ad, ah, aw = _mats(tiling, "At", absolute, negate)
    Z = torch.einsum("ia,je,kf,btiujvkc->aefbtuvc", ad, ah, aw, g.reshape(B, td, fd.m, th, fh.m, tw, fw.m, C))
    return Z.reshape(nfreq(tiling), -1, C)


# ----------------------------------------------------------------------------------------------------------------- weights
def _w5(w, tiling):
    fd = families(tiling)[0]
    w = torch.as_tensor(w).detach().to("cpu", F64)
    if w.dim() == 4:
        w = w.unsqueeze(2)
    assert tuple(w.shape[2:]) == (fd.r, 3, 3), (tuple(w.shape), tiling)
    return w


def weight_transform(w, tiling, mode=0, absolute=False, negate=None):
    """w [Cout][Cin][taps] -> U [NF][K][N] = G g G^T per axis.  mode 0 (forward): g[n][k] = w[n][k], K = Cin, N = Cout.
    mode 1 (data gradient): the taps mirrored and the channel roles swapped, g[n][k] = flip(w[k][n]), K = Cout, N = Cin."""
    w = _w5(w, tiling)
    g = w if mode == 0 else w.flip(2, 3, 4).transpose(0, 1)
    if absolute:
        g = g.abs()
    gd, gh, gw = _mats(tiling, "G", absolute, negate)
    U = torch.einsum("ad,be,cf,nkdef->abckn", gd, gh, gw, g)
    return U.reshape(nfreq(tiling), g.shape[1], g.shape[0])


def weight_grad(gU, tiling, two_d=False, absolute=False, negate=None):
    """gU [NF][Cin][Cout] -> gw [Cout][Cin][taps] = G^T gU G per axis (the adjoint of weight_transform mode 0)."""
    gU = _prep(gU, absolute)
    fd, fh, fw = families(tiling)
    gd, gh, gw_ = _mats(tiling, "G", absolute, negate)
    out = torch.einsum("ad,be,cf,abckn->nkdef", gd, gh, gw_, gU.reshape(fd.n, fh.n, fw.n, gU.shape[1], gU.shape[2]))
    return out.squeeze(2) if two_d else out


def dgemm_pack_layout(U):
    """U [64][K][N] -> Wp [64][Q][2][NPad][4] of ssbev_wino_dgemm_pack: Wp[xi][q][kh][n][t] = U[xi][8 q + 4 kh + t][n], zero for
    k >= K and n >= N (K padded to 8, N to 32)."""
    nf, K, N = U.shape
    KPad, NPad = -(-K // 8) * 8, -(-N // 32) * 32
    full = torch.zeros(nf, KPad, NPad, dtype=F64)
    full[:, :K, :N] = U
    return full.reshape(nf, KPad // 8, 2, 4, NPad).permute(0, 1, 2, 4, 3).contiguous()


# ------------------------------------------------------------------------------------------------------------- GEMM stages
def bgemm(A, U, absolute=False):
    """Cm[xi][T][N] = A[xi][T][K] U[xi][K][N]."""
    return torch.einsum("xtk,xkn->xtn", _prep(A, absolute), _prep(U, absolute))


def dgemm(P, U, B, D, absolute=False, negate=None):
    """The depth-fused product: P [16][B D Thw][K] ((h, w)-transformed planes), U [64][K][N] with xi = xi_d 16 + xi_hw ->
    Mo [16][B D Thw][N]: depth B^T over the planes 2i-1 .. 2i+2 (zeros outside [0, D)), the 4 products, depth A^T.
    negate: one coefficient of the depth B^T with the opposite sign (row, col)."""
    P, U = _prep(P, absolute), _prep(U, absolute)
    K, N = U.shape[1:]
    Thw = P.shape[1] // (B * D)
    bt = F23.Bt.clone()
    if negate is not None:
        bt[negate] = -bt[negate]
    at = F23.At
    if absolute:
        bt, at = bt.abs(), at.abs()
    planes = torch.nn.functional.pad(P.reshape(16, B, D, Thw, K), (0, 0, 0, 0, 1, 1)).unfold(2, 4, 2)      # [16][B][D/2][Thw][K][4]
    V = torch.einsum("ai,xbdtki->axbdtk", bt, planes)
    M = torch.einsum("axbdtk,axkn->axbdtn", V, U.reshape(4, 16, K, N))
    return torch.einsum("ia,axbdtn->xbditn", at, M).reshape(16, B * D * Thw, N)


# ------------------------------------------------------------------------------------------------------------------ chains
def chain_axis(mat):
    """Longest chain of roundings of one application of `mat`: over its rows, the non-zeros minus one (the additions) plus one
    per non-zero coefficient that is not +-1 (its multiplication)."""
    best = 0
    for row in mat:
        nz = row[row != 0]
        if len(nz):
            best = max(best, int(len(nz) - 1 + (nz.abs() != 1).sum()))
    return best


def chain(tiling, which, transposed=False):
    """n of a whole transform: chain_axis summed over the three axes.  which = "Bt" (input), "At" (output), "G" (weights);
    transposed = the adjoint (A g A^T: the matrix At^T; G^T gU G: the matrix G^T)."""
    return sum(chain_axis(m.t() if transposed else m) for m in _mats(tiling, which, False))


N_DEPTH_DGEMM = chain_axis(F23.Bt) + chain_axis(F23.At)       # the depth B^T and A^T of wino_dgemm_kernel, in registers


def to_bf16_exact(t):
    """fp32 values that bf16 holds exactly (round to nearest even), as fp32."""
    return torch.as_tensor(t).to(torch.bfloat16).to(torch.float32)
