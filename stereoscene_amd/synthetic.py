"""Deterministic synthetic tensors: weights-by-key and SemanticKITTI-shaped inputs.

Everything is generated from integer hashes (no torch RNG), so the same tensors are reproduced
bit-for-bit in the build container (fixture generation against the imported reference), in the
CPU test-suite and on the GPU box, independent of torch version or module construction order.
SURVEY.md section 8(c) "fill-by-key" and section 8(d) "synthetic inputs".
"""
import math
import zlib

import numpy as np
import torch


def hash_uniform(name, shape, lo=-0.5, hi=0.5):
    """float32 tensor u[i] in [lo, hi): ((i * 2654435761 + crc32(name)) mod 2^32) / 2^32."""
    n = int(np.prod(shape)) if len(shape) else 1
    seed = zlib.crc32(name.encode())
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(seed)) & np.uint64(0xFFFFFFFF)
    # second mixing round so that consecutive indices are not a plain lattice
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(13))) * np.uint64(3266489917) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    u = h.astype(np.float64) / 4294967296.0
    out = (lo + (hi - lo) * u).astype(np.float32)
    return torch.from_numpy(out.reshape(shape))


def hash_normal(name, shape, std=1.0):
    """Approximately N(0, std^2): sum of four hashed uniforms (Irwin-Hall), exactly reproducible."""
    acc = sum(hash_uniform(f"{name}#{j}", shape) for j in range(4))
    return (acc * (std * math.sqrt(3.0))).float()


# Cases of the Lovasz-softmax tests (tools/make_golden_lovasz.py records the reference on them): name -> (logits shape, label
# grid).  A / B are up-sampled x2, C is A at the label resolution, D all-zero logits (two big tie groups per class), E nothing
# labelled, F two labelled voxels of two classes, G fewer voxels than one wave.
LOVASZ_CASES = {"A": ((2, 20, 8, 6, 4), (2, 16, 12, 8)), "B": ((1, 20, 16, 16, 8), (1, 32, 32, 16)),
                "C": ((2, 20, 16, 12, 8), (2, 16, 12, 8)), "D": ((2, 20, 8, 6, 4), (2, 16, 12, 8)),
                "E": ((2, 20, 8, 6, 4), (2, 16, 12, 8)), "F": ((2, 20, 8, 6, 4), (2, 16, 12, 8)),
                "G": ((1, 20, 3, 2, 2), (1, 6, 4, 4))}
LOVASZ_SEED = {"A": 0, "B": 0, "C": 0, "G": 0}      # bumped when a fixture's fp32-vs-float64 gradient spread is above 2.5e-5


def lovasz_labels(tag, shape):
    """uint8 labels: ~10 % ignored (255), a skewed distribution over the classes (0 dominant), 2, 3 and 8 absent."""
    classes = torch.tensor([c for c in range(20) if c not in (2, 3, 8)], dtype=torch.uint8)
    u = hash_uniform(f"{tag}_cls", shape, 0.0, 1.0).double()
    lab = classes[(u ** 2.5 * len(classes)).long().clamp_(max=len(classes) - 1)]
    lab[hash_uniform(f"{tag}_ign", shape, 0.0, 1.0) < 0.1] = 255
    return lab


def lovasz_case(name):
    """(logits fp32 [B,20,d,h,w] ~ N(0, 2^2), labels uint8 [B,D,H,W]) of LOVASZ_CASES[name]."""
    coarse, fine = LOVASZ_CASES[name]
    base = "A" if name in "CDEF" else name
    lab = lovasz_labels(f"lovasz_{base}{LOVASZ_SEED[base]}", fine)
    if base == "A":
        lab[0][lab[0] == 19] = 0                       # class 19 occurs in sample 1 only: the batch is ONE set of voxels
    src = name if name in LOVASZ_SEED else "A"
    logits = hash_normal(f"lovasz_{src}{LOVASZ_SEED[src]}_x", coarse, 2.0)
    if name == "D":
        logits = torch.zeros(coarse)
    if name == "E":
        lab = torch.full(fine, 255, dtype=torch.uint8)
    if name == "F":
        lab = torch.full(fine, 255, dtype=torch.uint8)
        lab.view(-1)[5] = 4
        lab.view(-1)[1999] = 9
    return logits, lab


# Cases of the OHEM cross-entropy tests (tools/make_golden_ohem.py records the reference on them): name -> (logits shape, label
# grid, top_k).  The labels are the Lovasz cases' (A: two samples with different M_b and k_b; B: 14 716 labelled voxels = many
# tiles; C: A's labels with the logits on the label grid; D: all-zero logits, every loss is w_t * log 20 and the threshold falls
# inside one class's tie group; E: nothing labelled; F: two labelled voxels, k = 0; G: fewer voxels than a wave); H is C with +40
# on the target logit of a hashed ~20 % of the voxels: exactly zero fp32 losses inside the selection.
OHEM_CASES = {"A": ((2, 20, 8, 6, 4), (2, 16, 12, 8), 0.25), "B": ((1, 20, 16, 16, 8), (1, 32, 32, 16), 0.25),
              "C": ((2, 20, 16, 12, 8), (2, 16, 12, 8), 0.9), "D": ((2, 20, 8, 6, 4), (2, 16, 12, 8), 0.25),
              "E": ((2, 20, 8, 6, 4), (2, 16, 12, 8), 0.25), "F": ((2, 20, 8, 6, 4), (2, 16, 12, 8), 0.25),
              "G": ((1, 20, 3, 2, 2), (1, 6, 4, 4), 0.25), "H": ((2, 20, 16, 12, 8), (2, 16, 12, 8), 0.9)}
# 0: the Lovasz case's tensors; bumped (logits "ohem_<case><seed>_x"; for A also the labels, which C D F H share) when a sample's
# float64 gap between the k-th and the (k+1)-th loss is below 64 x the largest fp32 per-voxel loss error, or when A's two samples
# would keep the same number of voxels (the generator refuses the fixture)
OHEM_SEED = {"A": 1, "B": 1, "C": 0, "G": 0}


def ohem_case(name):
    """(logits fp32 [B,20,d,h,w] ~ N(0, 2^2), labels uint8 [B,D,H,W], top_k) of OHEM_CASES[name]."""
    coarse, fine, top_k = OHEM_CASES[name]
    src = {"D": "A", "E": "A", "F": "A", "H": "C"}.get(name, name)
    _, lab = lovasz_case("C" if name == "H" else name)
    if name in "ACDH" and OHEM_SEED["A"]:
        lab = lovasz_labels(f"ohem_A{OHEM_SEED['A']}", fine)
    seed = OHEM_SEED[src]
    logits = hash_normal(f"ohem_{src}{seed}_x" if seed else f"lovasz_{src}{LOVASZ_SEED[src]}_x", coarse, 2.0)
    if name == "D":
        logits = torch.zeros(coarse)
    if name == "H":
        plant = (hash_uniform("ohem_H_plant", fine, 0.0, 1.0) < 0.2) & (lab != 255)
        t = lab.long().clamp(max=19).unsqueeze(1)
        logits = logits + 40.0 * torch.zeros_like(logits).scatter_(1, t, plant.unsqueeze(1).float())
    return logits, lab, top_k


# Cases of the soft-Dice / LGA-weighted loss tests (tools/make_golden_dice_lga.py records the reference on them): name -> (logits
# shape, label grid).  A B C G: the Lovasz cases' tensors (A two samples; B many workgroups; C the logits already on the label grid
# = the tensor-form route; G fewer voxels than a wave).  K: blocky labels, a hashed 3-class 8x6x4 volume repeated 2x2x2 (9 % of the
# voxels have lga = 0), sample 0's first two planes ignored, and the last plane of sample 0 differs from the first plane of sample 1 (a
# kernel that reads across the sample boundary gets other weights).  L: coarse 1x1x1 -> 2x2x2, every voxel is first-or-last on
# every axis.  E: nothing labelled.  N: A without a voxel of class 0 (cnt0 = 0).  Z: A's labels, all-zero logits.
DICE_LGA_CASES = {"A": LOVASZ_CASES["A"], "B": LOVASZ_CASES["B"], "C": LOVASZ_CASES["C"], "G": LOVASZ_CASES["G"],
                  "K": ((2, 20, 8, 6, 4), (2, 16, 12, 8)), "L": ((1, 20, 1, 1, 1), (1, 2, 2, 2)),
                  "E": LOVASZ_CASES["E"], "N": LOVASZ_CASES["A"], "Z": LOVASZ_CASES["A"]}


def dice_lga_case(name):
    """(logits fp32 [B,20,d,h,w] ~ N(0, 2^2), labels uint8 [B,D,H,W]) of DICE_LGA_CASES[name]."""
    coarse, fine = DICE_LGA_CASES[name]
    if name in "ABCGE":
        return lovasz_case(name)
    if name in "NZ":
        logits, lab = lovasz_case("A")
        if name == "N":
            lab = torch.where(lab == 0, torch.full_like(lab, 9), lab)
        return (torch.zeros(coarse) if name == "Z" else logits), lab
    logits = hash_normal(f"dice_lga_{name}_x", coarse, 2.0)
    if name == "L":
        lab = torch.tensor([0, 5, 5, 255, 9, 9, 0, 13], dtype=torch.uint8).view(fine)
        return logits, lab
    classes = torch.tensor([0, 9, 15], dtype=torch.uint8)                     # K
    small = classes[(hash_uniform("dice_lga_K_cls", (2, 8, 6, 4), 0.0, 1.0) * 3).long().clamp_(max=2)]
    lab = small.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3).contiguous()
    lab[0, :2] = 255
    return logits, lab


# Cases of the Gaussian KL depth-loss tests (tools/make_golden_depth_kld.py records the reference on them): name -> (gt_depths
# shape [B, N, H, W], ds, dbound, units, density of LiDAR returns, their value range).  A: the reference grid (D = 112), 30 feature
# pixels, blocks with 0 / 1 / many returns and the planted edge depths of DEPTH_KLD_PLANTS; B: D = 13 (no multiple of the
# kernel's chunk count), 552 pixels = three thread blocks with a ragged last one, ds = 4, returns on both sides of the range;
# C: B without any return; D: B in bin units; E: the kitti_d192 depth range (D = 192) on a 2 x 3 feature map.
DEPTH_KLD_CASES = {"A": ((1, 2, 48, 80), 16, (2.0, 58.0, 0.5), "reference", 0.004, (2.2, 28.0)),
                   "B": ((2, 1, 48, 92), 4, (2.0, 8.5, 0.5), "reference", 0.08, (1.5, 9.5)),
                   "C": ((2, 1, 48, 92), 4, (2.0, 8.5, 0.5), "reference", 0.0, (1.5, 9.5)),
                   "D": ((2, 1, 48, 92), 4, (2.0, 8.5, 0.5), "bins", 0.08, (1.5, 9.5)),
                   "E": ((1, 1, 16, 24), 8, (2.0, 98.0, 0.5), "reference", 0.03, (1.0, 60.0))}
# Case A, camera 0, feature row 0: feature column -> ((row, column) inside the 16 x 16 block, depth), the rest of the block empty.
# d0 exactly (foreground); d1 - dd exactly (foreground); the next fp32 above it (background); 1.9 next to a deeper return (the
# minimum decides: background); 33.6 (foreground, its Gaussian is centred at bin 67.2 = 33.6 / dd, beyond the last edge 57.75: an
# all-zero target row that still counts in the divisor).
DEPTH_KLD_PLANTS = {0: (((3, 7), 2.0),), 1: (((15, 15), 57.5),), 2: (((0, 0), float(np.nextafter(np.float32(57.5), np.float32(100.0)))),),
                    3: (((8, 1), 1.9), ((2, 12), 7.0)), 4: (((11, 4), 33.6),)}


def depth_kld_case(name):
    """(gt_depths fp32 [B,N,H,W], depth_pred fp32 [B*N,D,H/ds,W/ds] with rows that sum to 1, ds, dbound, units) of
    DEPTH_KLD_CASES[name]."""
    shape, ds, dbound, units, density, (lo, hi) = DEPTH_KLD_CASES[name]
    assert name != "E" or list(dbound) == grid_config(CFG_K192)["dbound"]
    src = "B" if name in "CD" else name
    u = hash_uniform(f"depth_kld_{src}/mask", shape, 0.0, 1.0)
    d = hash_uniform(f"depth_kld_{src}/val", shape, lo, hi)
    gt = torch.where(u < density, d, torch.zeros_like(d))
    if name == "A":
        for col, plants in DEPTH_KLD_PLANTS.items():
            gt[0, 0, :ds, col * ds:(col + 1) * ds] = 0.0
            for (i, j), v in plants:
                gt[0, 0, i, col * ds + j] = v
    B, N, H, W = shape
    D = int(round((dbound[1] - dbound[0]) / dbound[2]))
    w = hash_uniform(f"depth_kld_{src}/pred", (B * N, D, H // ds, W // ds), 0.02, 1.0).double()
    w = w * w * w                                    # products and one division in float64, rounded once: exactly reproducible
    return gt, (w / w.sum(dim=1, keepdim=True)).float(), ds, dbound, units


# Cases of the image-view segmentation loss tests (tools/make_golden_imgseg.py records the reference on them): name -> (BN,
# (h, w) of the logits, (H, W) of the label map, fraction of labelled pixels).  A: exact 16 x 16 blocks, sparse labels of classes
# 1 .. 19, two samples, one cell cleared; B: ratios 7.4 and 14.43 (rectangles of unequal size, the min(.., n - 1) clamp, cells of
# up to 8 x 15 = 120 pixels: two passes of a wavefront), every pixel labelled with 0 .. 19; C: A's first sample with nothing
# labelled; D: logits in +-80, cell (0, 0) with a single labelled pixel, cell (0, 1) with none; E: the model's own sizes.
IMGSEG_CASES = {"A": (2, (3, 5), (48, 80), 0.05), "B": (2, (5, 7), (37, 101), 1.0), "C": (1, (3, 5), (48, 80), 0.0),
                "D": (1, (2, 3), (32, 48), 0.3), "E": (1, (24, 80), (384, 1280), 0.05)}
IMGSEG_CLASSES = 20


def imgseg_case(name):
    """(seg_logits fp32 [BN,20,h,w], seg_labels fp32 [BN,H,W] with integer values 0 .. 19, 0 = unlabelled) of IMGSEG_CASES[name]."""
    BN, (h, w), (H, W), density = IMGSEG_CASES[name]
    K = IMGSEG_CLASSES
    if name == "D":
        logits = hash_uniform("imgseg_D/logits", (BN, K, h, w), -80.0, 80.0)
    else:
        logits = hash_normal(f"imgseg_{name}/logits", (BN, K, h, w), std=2.0)
    if name == "B":                                   # every pixel carries a class, 0 among them
        lab = hash_uniform("imgseg_B/cls", (BN, H, W), 0.0, float(K)).floor().clamp_(0, K - 1)
    else:
        cls = hash_uniform(f"imgseg_{name}/cls", (BN, H, W), 1.0, float(K)).floor().clamp_(1, K - 1)
        u = hash_uniform(f"imgseg_{name}/mask", (BN, H, W), 0.0, 1.0)
        lab = torch.where(u < density, cls, torch.zeros_like(cls))
    if name == "A":
        lab[1, 32:48, 64:80] = 0.0                    # cell (2, 4) of the second sample: no valid pixel
    if name == "D":
        lab[0, :16, :32] = 0.0
        lab[0, 5, 9] = 7.0                            # cell (0, 0): one labelled pixel; cell (0, 1): none
    return logits, lab


_NORM_TOKENS = (".bn", ".gn", "norm")


def fill_value_for(key, t):
    """Deterministic content for state-dict entry ``key`` with the shape/dtype of ``t``."""
    leaf = key.rsplit(".", 1)[-1]
    if key.endswith(("frustum", ".dx", ".bx", ".nx")) or key in ("dx", "bx", "nx", "frustum"):
        return None  # geometry buffers stay as constructed
    if leaf == "num_batches_tracked":
        return torch.zeros_like(t)
    if leaf in ("gamma", "alpha"):
        return torch.full_like(t, 0.5)
    if leaf == "running_mean":
        return hash_uniform(key, t.shape, -0.1, 0.1)
    if leaf == "running_var":
        return 1.0 + hash_uniform(key, t.shape, 0.0, 0.5)
    if t.dim() <= 1:
        if leaf == "weight":  # norm scale (1-D weights only belong to norms)
            return 1.0 + hash_uniform(key, t.shape, -0.25, 0.25)
        return hash_uniform(key, t.shape, -0.1, 0.1)  # biases
    if t.numel() == 1:  # BRI 1x1x1 single-channel convs
        return hash_uniform(key, t.shape, 0.5, 1.5)
    fan_in = int(np.prod(t.shape[1:]))
    if "conv_offset" in key:
        return hash_uniform(key, t.shape, -0.5, 0.5) * (0.5 / math.sqrt(fan_in))
    return hash_uniform(key, t.shape, -1.0, 1.0) * math.sqrt(3.0 / fan_in)


@torch.no_grad()
def fill_state_dict_(module_or_sd, prefix=""):
    """In-place deterministic fill of every tensor of a module / state dict, keyed by its name."""
    sd = module_or_sd.state_dict() if hasattr(module_or_sd, "state_dict") else module_or_sd
    for k, t in sd.items():
        v = fill_value_for(prefix + k, t)
        if v is not None:
            t.copy_(v.to(t.dtype))
    return module_or_sd


# ---------------------------------------------------------------------------------------------
# SemanticKITTI-shaped synthetic sample
# ---------------------------------------------------------------------------------------------

CFG_K112 = dict(name="kitti_d112", input_size=(384, 1280), downsample=8, occ_size=(256, 256, 32),
                pc_range=(0.0, -25.6, -2.0, 51.2, 25.6, 4.4), dbound=(2.0, 58.0, 0.5))
CFG_K192 = dict(name="kitti_d192", input_size=(384, 1280), downsample=8, occ_size=(256, 256, 32),
                pc_range=(0.0, -25.6, -2.0, 51.2, 25.6, 4.4), dbound=(2.0, 98.0, 0.5))
CFG_S = dict(name="small_d48", input_size=(96, 320), downsample=8, occ_size=(64, 64, 16),
             pc_range=(0.0, -12.8, -2.0, 25.6, 12.8, 4.4), dbound=(2.0, 26.0, 0.5))
CFG_T = dict(name="tiny_d16", input_size=(64, 160), downsample=8, occ_size=(32, 32, 8),
             pc_range=(0.0, -6.4, -2.0, 12.8, 6.4, 4.4), dbound=(2.0, 10.0, 0.5))
CONFIGS = {c["name"]: c for c in (CFG_K112, CFG_K192, CFG_S, CFG_T)}


def grid_config(cfg, lss_downsample=(2, 2, 2)):
    """xbound/ybound/zbound/dbound exactly as the reference config computes them (CFG:23-49)."""
    r, o = cfg["pc_range"], cfg["occ_size"]
    vox = [(r[3 + i] - r[i]) / o[i] for i in range(3)]
    return {
        "xbound": [r[0], r[3], vox[0] * lss_downsample[0]],
        "ybound": [r[1], r[4], vox[1] * lss_downsample[1]],
        "zbound": [r[2], r[5], vox[2] * lss_downsample[2]],
        "dbound": list(cfg["dbound"]),
    }


def kitti_calibration(B, img_w, right=False):
    """KITTI-like camera (scaled to ``img_w`` pixels) -> rots, trans, intrins(4x4), post_rots,
    post_trans, bda, calib  for B samples and N=1 camera."""
    s = img_w / 1241.0
    fx = 707.0912 * s
    cx, cy = 601.8873 * s, 183.1104 * s
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = fx
    K[0, 2], K[1, 2] = cx, cy
    K[0, 3] = -0.54 * fx if right else 0.0
    R = torch.tensor([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])  # cam -> ego (inverse of velo->cam)
    t_velo = torch.tensor([0.0, -0.08, -0.27])
    t = -(R @ t_velo)
    rots = R.view(1, 1, 3, 3).repeat(B, 1, 1, 1)
    trans = t.view(1, 1, 3).repeat(B, 1, 1)
    intr = K.view(1, 1, 4, 4).repeat(B, 1, 1, 1)
    post_rots = torch.eye(3).view(1, 1, 3, 3).repeat(B, 1, 1, 1)
    post_trans = torch.zeros(B, 1, 3)
    bda = torch.eye(3).view(1, 3, 3).repeat(B, 1, 1)
    calib = torch.full((B,), fx * 0.54)
    return rots, trans, intr, post_rots, post_trans, bda, calib


def frustum_view(cfg, B=1, post=None, bda=None):
    """The left view of ``kitti_calibration`` in the ``img_inputs`` layout with a (stride-0, all-zero) image of the config's
    input size in slot 0: (imgs [B,1,3,H,W], rots, trans, intrins, post_rots, post_trans, bda).  ``post`` = (2x2, 2-vector)
    and ``bda`` (3x3 or 4x4) replace the identity post transform / BEV matrix."""
    H, W = cfg["input_size"]
    rots, trans, intr, post_rots, post_trans, bda0, _ = kitti_calibration(B, W)
    if post is not None:
        post_rots, post_trans = post_rots.clone(), post_trans.clone()
        post_rots[..., :2, :2] = torch.as_tensor(post[0], dtype=torch.float32)
        post_trans[..., :2] = torch.as_tensor(post[1], dtype=torch.float32)
    if bda is not None:
        bda0 = torch.as_tensor(bda, dtype=torch.float32).unsqueeze(0).repeat(B, 1, 1)
    return (torch.zeros(1).expand(B, 1, 3, H, W), rots, trans, intr, post_rots, post_trans, bda0)


# Cases of the loader-step tests (tools/make_golden_frustum.py records the reference on them), all on CFG_T's grid (32, 32, 8)
# and image size.  P: identity post transform, 3x3 identity BEV matrix, every voxel labelled.  Q: resize + crop + flip post
# transform, a 4x4 BEV matrix (rotation about the centre of the range and a flip of y), ~10 % of the labels 255.  R: a yaw of the
# BEV matrix that puts a good third of the grid behind the camera or outside the image.
FRUSTUM_LABEL_CASES = ("P", "Q", "R")
FRUSTUM_LABEL_SEED = {"P": 0, "Q": 0, "R": 0}     # bumped when the generator refuses a fixture (see its comparison rule)


def frustum_label_case(name):
    """(labels uint8 [32,32,8], the left view of ``frustum_view``, point-cloud range) of a loader case."""
    cfg = CFG_T
    shape = tuple(cfg["occ_size"])
    tag = f"frustum_{name}{FRUSTUM_LABEL_SEED[name]}"
    lab = hash_uniform(f"{tag}_lab", shape, 0.0, 20.0).long().clamp_(0, 19).to(torch.uint8)
    r = torch.tensor(cfg["pc_range"], dtype=torch.float64)
    centre = (r[:3] + r[3:]) / 2
    post = bda = None
    if name == "Q":
        lab[hash_uniform(f"{tag}_ign", shape, 0.0, 1.0) < 0.1] = 255
        s, W = 0.9375, cfg["input_size"][1]
        post = ([[-s, 0.0], [0.0, s]], [W - 3.0 * s, -2.0 * s])          # resize by s, crop at (-8 s .. ), mirror about the width
        ang = math.radians(7.0)
        rot = torch.tensor([[math.cos(ang), -math.sin(ang), 0, 0], [math.sin(ang), math.cos(ang), 0, 0], [0, 0, 1, 0],
                            [0, 0, 0, 1]], dtype=torch.float64)
        norm, denorm = torch.eye(4, dtype=torch.float64), torch.eye(4, dtype=torch.float64)
        norm[:3, 3], denorm[:3, 3] = -centre, centre
        bda = denorm @ torch.diag(torch.tensor([1.0, -1.0, 1.0, 1.0], dtype=torch.float64)) @ rot @ norm
    if name == "R":
        ang = math.radians(75.0)
        bda = torch.tensor([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1]], dtype=torch.float64)
    return lab, frustum_view(cfg, 1, post, bda), cfg["pc_range"]


# Cases of the frustum-proportion loss tests (tools/make_golden_frustum.py records the reference on them): name -> (logits shape,
# id grid, frusta).  A: x2, the ids of the loader rule on a 16 x 12 x 8 grid under two yawed cameras (most frusta empty: the skip
# rule); B: same grid; C: ids drawn per voxel from 0..63 and 255 (every wave sees many ids), classes without a count that receive
# probability, frustum 5 with voxels and an all-zero count row, frustum 9 with counts and no voxel; D: every id 255 (loss 0,
# gradient 0; the reference raises ZeroDivisionError); E: A with the first frustum both samples see kept in sample 0 only and the
# counts of the second taken from sample 1 only; F: x2, 16 frusta in slabs of whole frusta ALONG THE LAST AXIS, so every frustum
# has voxels in each of the eight 8192-voxel workgroup tiles (eight partial rows per frustum); G: F's shape with two samples,
# sixteen partial tables (more than the eight strided slices of the fold, whose loop runs twice); only G's scalars are recorded.
FRUSTUM_CASES = {"A": ((2, 20, 8, 6, 4), (2, 16, 12, 8), 64), "B": ((1, 20, 16, 16, 8), (1, 16, 16, 8), 64),
                 "C": ((1, 20, 16, 12, 8), (1, 16, 12, 8), 64), "D": ((2, 20, 8, 6, 4), (2, 16, 12, 8), 64),
                 "E": ((2, 20, 8, 6, 4), (2, 16, 12, 8), 64), "F": ((1, 20, 16, 32, 16), (1, 32, 64, 32), 16),
                 "G": ((2, 20, 16, 32, 16), (2, 32, 64, 32), 16)}


def _frustum_counts(ids, lab, F):
    """float [B, F, 20]: labelled voxels per sample, frustum and class."""
    B = ids.shape[0]
    out = torch.zeros(B, F * 20)
    for b in range(B):
        ok = (ids[b] != 255) & (lab[b] != 255)
        out[b].index_add_(0, (ids[b].long() * 20 + lab[b].long())[ok], torch.ones(int(ok.sum())))
    return out.view(B, F, 20)


def frustum_case(name):
    """(logits fp32 [B,20,d,h,w] ~ N(0, 2^2), ids uint8 [B,D,H,W], counts fp32 [B,F,20]) of FRUSTUM_CASES[name].  The counts are
    those of hashed labels inside the ids' frusta (so the labelled mix differs from the predicted one), edited as the case says."""
    coarse, fine, F = FRUSTUM_CASES[name]
    src = "A" if name in "DE" else name
    logits = hash_normal(f"frustum_{src}_x", coarse, 2.0)
    lab = lovasz_labels(f"frustum_{src}", fine)
    B = fine[0]
    if src == "A":
        from . import functional as Fn
        ids = torch.stack([Fn.frustum_labels(torch.zeros(fine[1:], dtype=torch.uint8), frustum_view(CFG_T, 1, bda=torch.tensor(
            [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])), CFG_T["pc_range"])[0]
            for a in (math.radians(100.0), math.radians(95.0))])
    elif name == "B":
        i = torch.arange(fine[1]).view(-1, 1, 1) // 2
        j = torch.arange(fine[2]).view(1, -1, 1) // 2
        ids = (i * 8 + j).expand(fine[1:]).clone().to(torch.uint8).unsqueeze(0)       # 2 x 2 columns of voxels, all 64 frusta
        ids[hash_uniform("frustum_B_none", fine, 0.0, 1.0) < 0.2] = 255
    elif name == "C":
        ids = hash_uniform("frustum_C_ids", fine, 0.0, 65.0).long().clamp_(0, 64)
        ids[ids == 9] = 10                                                            # frustum 9 holds no voxel
        ids = torch.where(ids == 64, torch.full_like(ids, 255), ids).to(torch.uint8)
    else:                                                                             # F, G: slabs of whole frusta along the last axis
        ids = (torch.arange(fine[3]) // 2).view(1, 1, 1, -1).expand(fine).clone().to(torch.uint8)
        ids[hash_uniform(f"frustum_{name}_none", fine, 0.0, 1.0) < 0.1] = 255
    if name == "D":
        ids = torch.full(fine, 255, dtype=torch.uint8)
    if name == "E":
        both = [f for f in range(F) if all(bool((ids[b] == f).any()) for b in range(B))]     # frusta both samples see
        ids[1][ids[1] == both[0]] = 255
    dists = _frustum_counts(ids, lab, F)
    if name == "C":
        dists[0, 5] = 0.0                                                             # voxels, no counts: skipped
        dists[0, 9, 0], dists[0, 9, 4] = 7.0, 2.0                                     # counts, no voxel: skipped
    if name == "E":
        dists[0, both[1]] = 0.0
    return logits, ids, dists


# Cases of the context-relation-prior tests (tools/make_golden_crp.py records the reference on them).
# Down-sampling: name -> (label grid, downscale).  Hashed labels 0..19 and 255 with planted blocks (block index in the coarse
# grid's flat order -> (value, count) pairs, the rest of the block stays hashed only where the counts do not fill it):
#   D8 (threshold 486.4): 0 exactly 486 empty-or-255 voxels (a class wins), 1 exactly 487 with more zeros (0), 2 exactly 487 with
#   more 255s (255), 3 a 0 / 255 tie (255), 4 classes 7 and 3 tie (3), 5 all 255, 6 all 0;
#   D2 (threshold 7.6): 0 seven empty voxels and one of class 4 (4), 1 a 4 / 4 tie of 0 and 255 (255), 2 five zeros and three
#   255s (0), 3 classes 9 and 2 tie with four voxels each (2), 4 all 255.
CRP_DOWNSAMPLE_CASES = {"D8": ((32, 16, 16), 8), "D2": ((8, 6, 4), 2), "D4": ((32, 32, 8), 4)}
CRP_DOWNSAMPLE_PLANTS = {
    "D8": {0: ((0, 300), (255, 186), (11, 20), (6, 6)), 1: ((0, 300), (255, 187), (11, 25)), 2: ((0, 200), (255, 287), (11, 25)),
           3: ((0, 250), (255, 250), (5, 12)), 4: ((7, 100), (3, 100), (0, 312)), 5: ((255, 512),), 6: ((0, 512),)},
    "D2": {0: ((0, 4), (255, 3), (4, 1)), 1: ((0, 4), (255, 4)), 2: ((0, 5), (255, 3)), 3: ((9, 4), (2, 4)), 4: ((255, 8),)},
    "D4": {}}


def crp_downsample_case(name):
    """(labels uint8 [X,Y,Z], downscale) of CRP_DOWNSAMPLE_CASES[name]."""
    grid, ds = CRP_DOWNSAMPLE_CASES[name]
    lab = hash_uniform(f"crp_{name}_lab", grid, 0.0, 20.0).long().clamp_(0, 19).to(torch.uint8)
    lab[hash_uniform(f"crp_{name}_ign", grid, 0.0, 1.0) < 0.15] = 255
    lab[hash_uniform(f"crp_{name}_empty", grid, 0.0, 1.0) < 0.5] = 0
    Ys, Zs = grid[1] // ds, grid[2] // ds
    for blk, plants in CRP_DOWNSAMPLE_PLANTS[name].items():
        vals = torch.cat([torch.full((n,), v, dtype=torch.uint8) for v, n in plants])
        assert vals.numel() == ds ** 3
        perm = torch.argsort(hash_uniform(f"crp_{name}_perm{blk}", (ds ** 3,), 0.0, 1.0))
        x, y, z = blk // (Ys * Zs), (blk // Zs) % Ys, blk % Zs
        lab[x * ds:(x + 1) * ds, y * ds:(y + 1) * ds, z * ds:(z + 1) * ds] = vals[perm].view(ds, ds, ds)
    return lab, ds


# Relation loss: name -> (B, relation grid).  A: all four relations have positives; B: labels 0 and 5 only, relation 1 (two
# different non-empty classes) has no positive (the reference returns NaN, here pos_weight 1); C: ~20 % of the voxels 255 (rows
# without a positive, skipped children) and logits of +-90 planted on ~2 % of the elements; D: two samples, the second all empty
# but one voxel, counts pooled over the batch; E: Mc = 288 > one 256-wide workgroup and 72 row chunks (only scalars recorded).
CRP_LOSS_CASES = {"A": (1, (4, 4, 2)), "B": (1, (6, 4, 2)), "C": (1, (4, 4, 4)), "D": (2, (4, 4, 2)), "E": (1, (18, 16, 8))}


def crp_loss_case(name):
    """(P_logits fp32 [B,4,Mc,N] ~ N(0, 2^2), labels uint8 [B,X,Y,Z]: the down-sampled grid) of CRP_LOSS_CASES[name]."""
    B, grid = CRP_LOSS_CASES[name]
    N = grid[0] * grid[1] * grid[2]
    classes = torch.tensor([0, 0, 0, 5, 9, 13] if name != "B" else [0, 0, 5, 5], dtype=torch.uint8)
    u = hash_uniform(f"crp_loss_{name}_cls", (B,) + grid, 0.0, float(len(classes))).long().clamp_(0, len(classes) - 1)
    lab = classes[u]
    if name in "CE":
        lab[hash_uniform(f"crp_loss_{name}_ign", (B,) + grid, 0.0, 1.0) < 0.2] = 255
    if name == "D":
        lab[1] = 0
        lab[1, 2, 1, 1] = 9
    P = hash_normal(f"crp_loss_{name}_x", (B, 4, N // 8, N), 2.0)
    if name == "C":
        big = hash_uniform("crp_loss_C_big", tuple(P.shape), 0.0, 1.0)
        P = torch.where(big < 0.01, torch.full_like(P, 90.0), torch.where(big > 0.99, torch.full_like(P, -90.0), P))
    return P, lab


# Relation gather: name -> (B, R, N, Mc, C2, Cin).  The kernel's tiles are 128 rows x 128 columns x 16 along the reduction; the
# three products put N, Mc and C2 on each of those axes in turn.  T: the module's own tiny shape, every size below one tile; U: Mc
# = 3 and C2 = 10 (rows that are not 16-byte aligned), Cin = 2; V: two samples, two relations, no size a multiple of its tile; W:
# every size spans several tiles, Cin = 6 puts the context slice off the 16-byte grid; X: the true depth Mc = 512 and N = 4096
# (eight slices of the context gradient's reduction) with a small C2.
CRP_GATHER_CASES = {"T": (1, 4, 32, 4, 16, 8), "U": (1, 2, 24, 3, 10, 2), "V": (2, 2, 200, 20, 36, 0), "W": (1, 4, 384, 144, 272, 6),
                    "X": (1, 4, 4096, 512, 16, 0)}


def crp_gather_case(name):
    """(P_logits [B,R,Mc,N] ~ N(0, 2^2), context [B,Mc,C2], x [B,Cin,N] or None, upstream gradient [B,Cin + R C2,N]), fp32."""
    B, R, N, Mc, C2, Cin = CRP_GATHER_CASES[name]
    P = hash_normal(f"crp_gather_{name}_p", (B, R, Mc, N), 2.0)
    ctx = hash_normal(f"crp_gather_{name}_c", (B, Mc, C2))
    x = hash_normal(f"crp_gather_{name}_x", (B, Cin, N)) if Cin else None
    g = hash_normal(f"crp_gather_{name}_g", (B, Cin + R * C2, N))
    return P, ctx, x, g


CRP_BLOCK = dict(feature=8, size=(4, 4, 2), batch=2)


def crp_block_case():
    """(input fp32 [2,8,4,4,2], weights of sum(x * wx) + sum(P_logits * wp): the scalar whose input gradient is recorded)."""
    f, size, B = CRP_BLOCK["feature"], CRP_BLOCK["size"], CRP_BLOCK["batch"]
    N = size[0] * size[1] * size[2]
    return (hash_normal("crp_block_x", (B, f) + size), hash_normal("crp_block_wx", (B, f) + size),
            hash_normal("crp_block_wp", (B, 4, N // 8, N)))


# Cases of the position-encoder tests (tools/make_golden_point_xyz.py records the reference on them), on CFG_T's frustum (D = 16,
# 8 x 20 feature map: 2 560 points per sample): name -> (B, Cxyz, mode, training, pc_range or None = CFG_T's, occ_size or None).
# E: a shrunk range with large voxels (most points outside, the rest crowded into a few voxels: lists of more than 32 and more
# than 256 points next to empty voxels); F: eval mode with hashed running statistics; G: a range no point falls into.
POINT_XYZ_CASES = {"A": (1, 16, "cat", True, None, None), "B": (2, 16, "add", True, None, None),
                   "C": (1, 128, "cat", True, None, None), "D": (1, 8, "cat", True, None, None),
                   "E": (1, 24, "cat", True, (0.0, -3.2, -2.0, 6.0, 3.2, 4.4), (4, 4, 4)),
                   "F": (1, 16, "cat", False, None, None),
                   "G": (1, 16, "cat", True, (100.0, 100.0, 100.0, 112.8, 112.8, 106.4), None)}
POINT_XYZ_SEED = {n: 0 for n in POINT_XYZ_CASES}    # bumped when the generator refuses a case (a pre-activation or a point too close to a decision)
POINT_XYZ_PARAMS = ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias")


def point_xyz_case(name):
    """dict of a POINT_XYZ_CASES entry: cfg (CFG_T with the case's range / grid), B, Cxyz, mode, training, calib (the six tensors
    of get_geometry; B: a yaw + translation in the second sample's 4x4 BEV matrix), geom fp32 [B,1,16,8,20,3] (the tensor form
    of get_geometry on the CPU), grid_host = (origin, dx, n), state (the encoder's state dict, reference names), G fp32
    [B,Cxyz,X,Y,Z]: the weights of the recorded scalar sum(P * G)."""
    from types import SimpleNamespace
    from .plugin.view_transformer import ViewTransformerLiftSplatShootVoxel as VT, gen_dx_bx
    B, Cx, mode, training, rng, occ = POINT_XYZ_CASES[name]
    cfg = dict(CFG_T, pc_range=rng or CFG_T["pc_range"], occ_size=occ or CFG_T["occ_size"])
    tag = f"point_xyz/{name}/{POINT_XYZ_SEED[name]}"
    grid = grid_config(cfg)
    view = frustum_view(cfg, B=B, bda=torch.eye(4) if name == "B" else None)
    calib = [t.clone() for t in view[1:]]
    if name == "B":
        a = 0.2
        calib[5][1] = torch.tensor([[math.cos(a), -math.sin(a), 0.0, 0.3], [math.sin(a), math.cos(a), 0.0, -0.2],
                                    [0.0, 0.0, 1.0, 0.1], [0.0, 0.0, 0.0, 1.0]])
    ns = SimpleNamespace(data_config=dict(input_size=tuple(cfg["input_size"])), grid_config=grid, downsample=cfg["downsample"],
                         _apply3x3=VT._apply3x3)
    ns.frustum = VT.create_frustum(ns)
    geom = VT.get_geometry(ns, *calib)
    dx, bx, nx = gen_dx_bx(grid["xbound"], grid["ybound"], grid["zbound"])
    grid_host = ((bx - dx / 2.0).tolist(), dx.tolist(), [int(v) for v in nx.tolist()])
    M = Cx // 2
    state = {"0.weight": hash_uniform(f"{tag}/w1", (M, 3), -1.0, 1.0), "0.bias": hash_uniform(f"{tag}/b1", (M,), -0.5, 0.5),
             "1.weight": hash_uniform(f"{tag}/gamma", (M,), 0.5, 1.5), "1.bias": hash_uniform(f"{tag}/beta", (M,), -0.5, 0.5),
             "1.running_mean": hash_uniform(f"{tag}/rm", (M,), -0.3, 0.3) if not training else torch.zeros(M),
             "1.running_var": hash_uniform(f"{tag}/rv", (M,), 0.2, 0.8) if not training else torch.ones(M),
             "1.num_batches_tracked": torch.tensor(0 if training else 7),
             "3.weight": hash_uniform(f"{tag}/w2", (Cx, M), -0.3, 0.3), "3.bias": hash_uniform(f"{tag}/b2", (Cx,), -0.1, 0.1)}
    # The ReLU's kink must not sit on a point: with thousands of points per channel a hashed beta puts some pre-activation within
    # rounding of 0, and the fp32 evaluations would disagree on its mask.  beta_m is therefore moved (in float64, from the inputs
    # alone) to the middle of the widest gap between consecutive sorted values of gamma_m hhat_m whose middle is within half of the
    # channel's largest magnitude -- the normalised values themselves do not depend on beta.
    from . import functional as F
    kept = F.voxel_index_tensor(geom, *grid_host) >= 0
    if int(kept.sum()) >= 2:
        r = torch.tensor(cfg["pc_range"], dtype=torch.float32).double()
        u = ((geom.reshape(-1, 3)[kept].double() - r[:3]) / (r[3:] - r[:3]) - 0.5) * 2
        h = u @ state["0.weight"].double().t() + state["0.bias"].double()
        mu, var = (h.mean(0), h.var(0, unbiased=False)) if training else (state["1.running_mean"].double(), state["1.running_var"].double())
        y = (state["1.weight"].double() * (h - mu) / torch.sqrt(var + 1e-5)).sort(0).values          # [n_kept, M]
        mid, gap = (y[1:] + y[:-1]) / 2, y[1:] - y[:-1]
        gap = torch.where(mid.abs() <= 0.5 * y.abs().max(0).values, gap, torch.zeros_like(gap))
        state["1.bias"] = (-mid.gather(0, gap.argmax(0, keepdim=True))[0]).float()
    n = grid_host[2]
    return dict(cfg=cfg, B=B, Cxyz=Cx, mode=mode, training=training, calib=calib, geom=geom, grid_host=grid_host, state=state,
                G=hash_uniform(f"{tag}/G", (B, Cx, n[0], n[1], n[2]), -1.0, 1.0))


# Cases of the point-level branch (tools/make_golden_point_head.py records the float64 result on them): name -> dict(counts = points
# per sample, C = level width, grids = the levels' (X, Y, Z), soft = soft_weights, cams = cameras of the image branch (0: none),
# axis = point_axis_order, kind = how the points are drawn).  A: all inside; B: unequal axes, points up to 0.6 of the range outside
# on every side (1.5 cells and more), exactly on the range's faces and on cell centres; C1 / C2: two levels, soft weights, image
# features [cams, 12, 3, 5] with uv exactly +-1, depth at and below 1e-5 and uv outside; D: 600 points in one cell of 256;
# E: an empty and a single-point sample; F: B sampled in xyz order; G: C1 with every label 0.
POINT_HEAD_RANGE = (0.0, -4.0, -1.0, 8.0, 4.0, 3.0)
POINT_HEAD_CLASSES = 20
POINT_HEAD_IMG = (12, 3, 5)
POINT_HEAD_CASES = {
    "A": dict(counts=(37,), C=8, grids=((4, 4, 2),), soft=False, cams=0, axis="reference", kind="inside"),
    "B": dict(counts=(5, 130), C=40, grids=((6, 5, 3),), soft=False, cams=0, axis="reference", kind="edges"),
    "C1": dict(counts=(40, 23), C=16, grids=((8, 8, 4), (4, 4, 2)), soft=True, cams=1, axis="reference", kind="edges"),
    "C2": dict(counts=(40, 23), C=16, grids=((8, 8, 4), (4, 4, 2)), soft=True, cams=2, axis="reference", kind="edges"),
    "D": dict(counts=(600,), C=8, grids=((8, 8, 4),), soft=False, cams=0, axis="reference", kind="one_cell"),
    "E": dict(counts=(0, 1), C=8, grids=((4, 4, 2),), soft=False, cams=0, axis="reference", kind="inside"),
    "F": dict(counts=(5, 130), C=40, grids=((6, 5, 3),), soft=False, cams=0, axis="xyz", kind="edges"),
    "G": dict(counts=(40, 23), C=16, grids=((8, 8, 4), (4, 4, 2)), soft=True, cams=1, axis="reference", kind="edges", labels="zero"),
}
POINT_HEAD_ORDER = ("A", "B", "C1", "C2", "D", "E", "F", "G")


def point_head_case(name):
    """dict of a POINT_HEAD_CASES entry: spec, head_kwargs (for ``OccHead``; parameters: ``fill_state_dict_``), feats (list of
    fp32 [B, C, X, Y, Z]), points (list of fp32 [N_b, 4] = x, y, z, label), img_feats (fp32 [B, cams, 12, 3, 5] or None) and
    points_uv (list of fp32 [N_b, cams, 3] or None), all hash-generated."""
    spec = POINT_HEAD_CASES[name]
    src = {"F": "B", "G": "C1"}.get(name, name)                     # F and G reuse the inputs of B and C1
    tag = f"point_head/{src}"
    counts, C_, B = spec["counts"], spec["C"], len(spec["counts"])
    lo = torch.tensor(POINT_HEAD_RANGE[:3])
    rng = torch.tensor(POINT_HEAD_RANGE[3:]) - lo
    X, Y, Z = spec["grids"][0]
    points, uvs = [], []
    for b, n in enumerate(counts):
        if spec["kind"] == "inside":
            g = hash_uniform(f"{tag}/g{b}", (n, 3), -0.999, 0.999)
        elif spec["kind"] == "edges":
            g = hash_uniform(f"{tag}/g{b}", (n, 3), -1.6, 1.6)
            for i in range(min(n, 24)):                            # the first rows: faces of the range and cell centres
                if i % 4 == 0:
                    g[i, i // 4 % 3] = 1.0 if i % 8 else -1.0
                elif i % 4 == 1:
                    cell = torch.tensor([i % X, i % Y, i % Z], dtype=torch.float32)
                    g[i] = (2 * cell + 1) / torch.tensor([X, Y, Z], dtype=torch.float32) - 1
        else:                                                       # every point within 0.4 cells of one grid corner: eight long lists
            g = torch.tensor([0.375, -0.125, 0.375]) + hash_uniform(f"{tag}/g{b}", (n, 3), -0.1, 0.1)
        p = lo + (g + 1) / 2 * rng
        hit = torch.isclose(g, torch.ones(())) | torch.isclose(g, -torch.ones(()))
        p = torch.where(hit & (g > 0), lo + rng, torch.where(hit, lo.expand_as(p), p))      # exactly on the faces: g = +-1 exactly
        lab = (hash_uniform(f"{tag}/lab{b}", (n,), 0.0, 1.0) * POINT_HEAD_CLASSES).floor().clamp_(0, POINT_HEAD_CLASSES - 1)
        if spec.get("labels") == "zero":
            lab = torch.zeros(n)
        points.append(torch.cat((p, lab[:, None]), 1))
        if spec["cams"]:
            uv = torch.cat((hash_uniform(f"{tag}/uv{b}", (n, spec["cams"], 2), -1.3, 1.3),
                            hash_uniform(f"{tag}/d{b}", (n, spec["cams"], 1), 0.5, 20.0)), -1)
            special = [(1.0, 0.2, 5.0), (-1.0, 0.2, 5.0), (0.3, 1.0, 5.0), (0.3, -1.0, 5.0), (0.3, 0.2, 1e-5), (0.3, 0.2, 0.0),
                       (0.3, 0.2, -2.0), (0.9999, -0.9999, 2e-5), (-0.95, 0.95, 5.0)]
            for i, s in enumerate(special[:n]):
                uv[i, i % spec["cams"]] = torch.tensor(s)
            uvs.append(uv)
    feats = [hash_normal(f"{tag}/feat{l}", (B, C_) + tuple(gr)) for l, gr in enumerate(spec["grids"])]
    img = hash_normal(f"{tag}/img", (B, spec["cams"]) + POINT_HEAD_IMG) if spec["cams"] else None
    head_kwargs = dict(in_channels=[C_] * len(spec["grids"]), out_channel=POINT_HEAD_CLASSES, semantic_kitti=True,
                       num_level=len(spec["grids"]), supervise_points=True, soft_weights=spec["soft"],
                       sampling_img_feats=bool(spec["cams"]), in_img_channels=POINT_HEAD_IMG[0],
                       point_cloud_range=list(POINT_HEAD_RANGE), point_axis_order=spec["axis"],
                       norm_cfg=dict(type="GN", num_groups=2, requires_grad=True))
    return dict(spec=spec, head_kwargs=head_kwargs, feats=feats, points=points, img_feats=img, points_uv=uvs if spec["cams"] else None)


def synthetic_sample(cfg, B=1, C_in=640, tag="s0", with_targets=True):
    """Image-neck outputs for both views + geometry + targets, all hash-generated.

    Returns a dict: x_l, x_r [B,1,C,fH,fW]; geo_l, geo_r (6-tuples); calib [B];
    gt_depths [B,1,H,W]; gt_occ [B,X,Y,Z] int64 in {0..19, 255}; img_seg [B,H,W] float in {0..19}, 0 = unlabelled.
    """
    H, W = cfg["input_size"]
    fH, fW = H // cfg["downsample"], W // cfg["downsample"]
    x_l = hash_normal(f"{tag}/x_l", (B, 1, C_in, fH, fW))
    # right view = left view shifted by a few feature pixels + noise: keeps the correlation volume informative
    shift = 3
    x_r = torch.roll(x_l, -shift, dims=-1) * 0.8 + 0.2 * hash_normal(f"{tag}/x_r", (B, 1, C_in, fH, fW))
    gl = kitti_calibration(B, W, right=False)
    gr = kitti_calibration(B, W, right=True)
    out = dict(x_l=x_l, x_r=x_r, geo_l=gl[:6], geo_r=gr[:6], calib=gl[6])
    if with_targets:
        u = hash_uniform(f"{tag}/gt_depth_mask", (B, 1, H, W), 0.0, 1.0)
        d = hash_uniform(f"{tag}/gt_depth_val", (B, 1, H, W), cfg["dbound"][0], cfg["dbound"][1] - 6.0)
        out["gt_depths"] = torch.where(u < 0.05, d, torch.zeros_like(d))
        X, Y, Z = cfg["occ_size"]
        c = (hash_uniform(f"{tag}/gt_occ", (B, X, Y, Z), 0.0, 20.0)).long().clamp_(0, 19)
        ig = hash_uniform(f"{tag}/gt_occ_ignore", (B, X, Y, Z), 0.0, 1.0) < 0.10
        out["gt_occ"] = torch.where(ig, torch.full_like(c, 255), c)
        # image-view segmentation labels (CreateDepthFromLiDAR's img_seg): a class 1 .. 19 where the view has a LiDAR return
        seg = hash_uniform(f"{tag}/img_seg", (B, H, W), 1.0, 20.0).floor().clamp_(1, 19)
        out["img_seg"] = torch.where(u[:, 0] < 0.05, seg, torch.zeros_like(seg))
    return out
