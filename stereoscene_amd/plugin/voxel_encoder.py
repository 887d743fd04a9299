"""Dense 3-D encoder, neck and occupancy head over the voxel grid: host-side mirrors of
``CustomResNet3D`` (resnet3d.py:106-246), ``SECONDFPN3D`` (second_fpn_3d.py:14-117) and
``OccHead`` (occhead.py:28-426) with identical registry names, kwargs and state-dict keys.
All convolutions run on the MFMA implicit-GEMM kernels (stereoscene_amd.layers)."""
import numpy as np
import torch
import torch.nn as nn

from .. import functional as F
from ..layers import Conv3d, GroupNorm, build_conv_layer, build_norm_layer, build_upsample_layer, fuse_relu_, norm_pair
from ..registry import BACKBONES, HEADS, NECKS
from . import losses as L
from .crp3d import CPMegaVoxels


class BasicBlock3d(nn.Module):
    """conv3-GN-ReLU-conv3-GN, projected shortcut when the shape changes, ReLU (resnet3d.py:35-65)."""
    expansion = 1

    def __init__(self, in_planes, planes, stride=1, downsample=None, norm_cfg=None):
        super().__init__()
        self.conv1 = Conv3d(in_planes, planes, 3, stride, 1, bias=False)
        self.bn1 = build_norm_layer(norm_cfg, planes)[1]
        self.conv2 = Conv3d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = build_norm_layer(norm_cfg, planes)[1]
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        xa, xb = F.fork(x)                                   # two consumers: conv1 and the shortcut
        out = self.bn1(self.conv1(xa), relu=True)
        if self.downsample is None:
            return self.bn2(self.conv2(out), residual=xb, relu=True)   # relu(GN(conv2) + shortcut) in one pass
        # projected shortcut: relu(GN(conv2(out)) + GN(conv1x1(x))) as one two-norm operator
        return norm_pair(self.bn2, self.conv2(out), self.downsample[1], self.downsample[0](xb), relu=True)


@BACKBONES.register_module()
class CustomResNet3D(nn.Module):
    def __init__(self, depth, block_inplanes=(64, 128, 256, 512), block_strides=(1, 2, 2, 2), out_indices=(0, 1, 2, 3),
                 num_stage=4, n_input_channels=3, shortcut_type="B", norm_cfg=dict(type="BN3d", requires_grad=True),
                 crp3d=False, crp_level=2, widen_factor=1.0, crp_size=(32, 32, 4)):
        """``crp3d=True`` builds the context relation prior ``CP_mega_voxels`` (crp3d.py:173-262) behind stage ``crp_level``
        (resnet3d.py:158-165, 238-241).  ``crp_size``: the grid of that stage's output, which the reference hard-codes as
        (32, 32, 4); a keyword here so that small grids can run."""
        super().__init__()
        if depth not in (10, 18, 34) or shortcut_type != "B":
            raise NotImplementedError("only the BasicBlock / shortcut-B variants used by the config are built")
        nblocks = {10: [1, 1, 1, 1], 18: [2, 2, 2, 2], 34: [3, 4, 6, 3]}[depth]
        planes = [int(c * widen_factor) for c in block_inplanes]
        self.in_planes = planes[0]
        self.out_indices, self.num_stage, self.crp3d = out_indices, num_stage, bool(crp3d)
        self.input_proj = nn.Sequential(Conv3d(n_input_channels, self.in_planes, 1, 1, 0, bias=False),
                                        build_norm_layer(norm_cfg, self.in_planes)[1], nn.ReLU(inplace=True))
        self.layers = nn.ModuleList()
        for i, c in enumerate(planes[:num_stage]):
            self.layers.append(self._make_layer(c, nblocks[i], block_strides[i], norm_cfg))
        if self.crp3d:
            if F.storage_bf16():
                raise NotImplementedError("crp3d=True runs in fp32 only: the relation kernels have no bf16 storage form")
            if not 0 <= crp_level < len(self.layers):
                raise ValueError(f"crp_level {crp_level} names no built stage (num_stage={len(self.layers)})")
            self.crp_level = crp_level
            self.CP_mega_voxels = CPMegaVoxels(planes[crp_level], tuple(crp_size), bn_momentum=0.1)
        self.forward_dic = {}
        fuse_relu_(self)
        for m in self.modules():
            if isinstance(m, Conv3d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make_layer(self, planes, blocks, stride, norm_cfg):
        down = None
        if stride != 1 or self.in_planes != planes:
            down = nn.Sequential(Conv3d(self.in_planes, planes, 1, stride, 0, bias=False),
                                 build_norm_layer(norm_cfg, planes)[1])
        layers = [BasicBlock3d(self.in_planes, planes, stride, down, norm_cfg)]
        self.in_planes = planes
        layers += [BasicBlock3d(planes, planes, norm_cfg=norm_cfg) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def crp_loss(self, CP_mega_matrices=None, CP_mega_labels=None):
        """The relation loss of the last forward's ``P_logits`` (resnet3d.py:213-217).  ``CP_mega_labels``: the loader's
        down-sampled label grid uint8 [B, X, Y, Z] (``CreateRelationLabels(relations=True)``), from which the fused kernel derives
        the relation bits; ``CP_mega_matrices``: the reference's dense [B, 4, N, Mc] matrices, which take precedence and run the
        tensor form.  A relation without a positive in the batch has pos_weight 1 (the reference returns NaN)."""
        if not self.crp3d or "crp_logits" not in self.forward_dic:
            raise RuntimeError("crp_loss needs crp3d=True and a forward pass")
        return F.relation_loss(self.forward_dic["crp_logits"], CP_mega_labels, CP_mega_matrices)

    def forward(self, x):
        x = self.input_proj(x)
        res = []
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if self.crp3d and self.crp_level == i:
                outputs = self.CP_mega_voxels(x)
                self.forward_dic["crp_logits"] = outputs["P_logits"]
                x = outputs["x"]
            if i in self.out_indices:
                if i + 1 < len(self.layers):
                    x, out = F.fork(x)                       # next stage + neck
                    res.append(out)
                else:
                    res.append(x)
        return res


@NECKS.register_module()
class SECONDFPN3D(nn.Module):
    def __init__(self, in_channels=(128, 128, 256), out_channels=(256, 256, 256), upsample_strides=(1, 2, 4),
                 norm_cfg=dict(type="GN", num_groups=32, requires_grad=True),
                 upsample_cfg=dict(type="deconv3d", bias=False), conv_cfg=dict(type="Conv3d", bias=False),
                 use_conv_for_no_stride=False, use_output_upsample=False, with_cp=False, init_cfg=None):
        super().__init__()
        assert len(out_channels) == len(upsample_strides) == len(in_channels) and not use_output_upsample
        self.in_channels, self.out_channels = list(in_channels), list(out_channels)
        blocks = []
        for cin, cout, s in zip(in_channels, out_channels, upsample_strides):
            if s >= 1 and not (s == 1 and use_conv_for_no_stride):
                up = build_upsample_layer(upsample_cfg, in_channels=cin, out_channels=cout, kernel_size=s, stride=s)
            else:
                k = int(np.round(1 / s))
                up = build_conv_layer(conv_cfg, in_channels=cin, out_channels=cout, kernel_size=k, stride=k)
            blocks.append(nn.Sequential(up, build_norm_layer(norm_cfg, cout)[1], nn.ReLU(inplace=True)))
        self.deblocks = nn.ModuleList(blocks)
        fuse_relu_(self)

    def forward(self, x):
        assert len(x) == len(self.in_channels)
        norms = [blk[1] for blk in self.deblocks]
        if (len(x) > 1 and all(isinstance(n, GroupNorm) and n.fused_relu for n in norms)
                and all(isinstance(blk[2], nn.Identity) for blk in self.deblocks)):
            raw = [blk[0](f) for blk, f in zip(self.deblocks, x)]
            if F.norm_cat_supported(raw):
                # every branch's GroupNorm + ReLU writes its channel slice of the concatenated tensor (FPN:113-116 without
                # the torch.cat pass and, backward, without the three slice copies)
                return [F.norm_cat(raw, [(n.weight, n.bias, n.num_groups, n.eps, False) for n in norms], relu=True)[0]]
            ups = [blk[2](blk[1](r)) for blk, r in zip(self.deblocks, raw)]
        else:
            ups = [blk(f) for blk, f in zip(self.deblocks, x)]
        return [torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]]


class Mlp(nn.Module):
    """``fc1 -> GELU (exact, erf) -> fc2`` (dense_heads/mlp.py; dropout 0): the reference's keys ``fc1.*`` / ``fc2.*``, both
    products on the own GEMM kernels (``functional.small_linear``)."""

    def __init__(self, in_features, hidden_features=None, out_features=None):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

    def forward(self, x):
        h = torch.nn.functional.gelu(F.small_linear(x, self.fc1.weight, self.fc1.bias))
        return F.small_linear(h, self.fc2.weight, self.fc2.bias)


@HEADS.register_module()
class OccHead(nn.Module):
    """``supervise_points=True`` builds the point-level branch (occhead.py:110-133, 171-236, 363-398): every labelled LiDAR
    point samples the first ``num_level`` voxel feature maps trilinearly and, with ``sampling_img_feats``, the left view's image
    features bilinearly at its projection; ``soft_weights`` mixes the row sets with a learned softmax, ``point_occ_mlp`` gives
    the logits, and ``loss`` adds ``loss_point_ce_`` and ``loss_point_lovasz_`` (weights ``loss_weight_cfg.loss_point_ce_weight``
    / ``.loss_point_lovasz_weight``, both 1 by default).  ``point_axis_order``: "reference" hands (x, y, z) to the sampler as the
    reference does, so that a point's x walks the Z axis and its z the X axis (``functional.point_sample_tensor``); "xyz" samples
    X with x, Y with y and Z with z.  Without a labelled point both losses are exactly 0 (the reference's CE is NaN); samples
    of one point work (the reference's ``.squeeze().t()`` breaks on them).  fp32 only."""

    def __init__(self, in_channels, out_channel, out_point_channel=None, semantic_kitti=False, supervise_voxel=True,
                 num_level=1, num_img_level=1, in_img_channels=512, sampling_img_feats=False, soft_weights=False,
                 supervise_points=False, loss_weight_cfg=None, semkitti_loss_weight_cfg=None,
                 loss_voxel_prototype="cylinder3d", use_ohem_loss=False, use_sc_ohem_loss=False, ohem_topk=0.25,
                 conv_cfg=dict(type="Conv3d", bias=False), norm_cfg=dict(type="GN", num_groups=32, requires_grad=True),
                 point_cloud_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0), with_cp=False, train_cfg=None, test_cfg=None,
                 use_frustum_loss=False, use_dice_loss=False, use_lga_loss=False, point_axis_order="reference"):
        super().__init__()
        if not semantic_kitti or not supervise_voxel:
            raise NotImplementedError("only the voxel-supervised SemanticKITTI head used by the config is built")
        self.in_channels = list(in_channels) if isinstance(in_channels, (list, tuple)) else [in_channels]
        self.out_channel, self.num_level = out_channel, num_level
        self.semantic_kitti, self.supervise_voxel, self.supervise_points = True, True, bool(supervise_points)
        self.point_cloud_range = torch.tensor(np.array(point_cloud_range))
        if self.supervise_points:
            if point_axis_order not in F.POINT_AXIS_ORDERS:
                raise ValueError(f"point_axis_order must be one of {F.POINT_AXIS_ORDERS}, got {point_axis_order!r}")
            if F.storage_bf16():
                raise NotImplementedError("supervise_points=True runs in fp32 only: the point kernels have no bf16 storage form")
            if len(set(self.in_channels[:num_level])) != 1:
                raise NotImplementedError("the point-level branch adds the levels' rows: they must have one width")
            self.point_axis_order = point_axis_order
            self.soft_weights, self.sampling_img_feats = bool(soft_weights), bool(sampling_img_feats)
            self.num_img_level, self.in_img_channels = num_img_level, in_img_channels
            c0 = self.in_channels[0]
            if self.sampling_img_feats:
                self.img_feat_reduce = nn.Linear(in_img_channels, c0)
            self.num_point_sampling_feat = num_level + int(self.sampling_img_feats) * num_img_level
            if self.soft_weights:
                self.point_soft_weights = nn.Sequential(nn.Linear(c0, c0 // 2), nn.ReLU(inplace=True),
                                                        nn.Linear(c0 // 2, self.num_point_sampling_feat))
            self.point_occ_mlp = Mlp(self.in_channels[-1], self.in_channels[-1], out_point_channel or out_channel)
            lw = loss_weight_cfg or {}
            self.loss_point_ce_weight = float(lw.get("loss_point_ce_weight", 1.0))
            self.loss_point_lovasz_weight = float(lw.get("loss_point_lovasz_weight", 1.0))
        self.occ_convs = nn.ModuleList()
        for i in range(num_level):
            mid = self.in_channels[i] // 2
            self.occ_convs.append(nn.Sequential(
                build_conv_layer(conv_cfg, in_channels=self.in_channels[i], out_channels=mid, kernel_size=3, stride=1,
                                 padding=1),
                build_norm_layer(norm_cfg, mid)[1], nn.ReLU(inplace=True),
                build_conv_layer(conv_cfg, in_channels=mid, out_channels=out_channel, kernel_size=1, stride=1,
                                 padding=0)))
        fuse_relu_(self)
        self.class_names = L.KITTI_CLASS_NAMES
        assert out_channel == len(self.class_names)
        # non-persistent buffer: follows the module to the device (a per-step .to(device) of a host tensor is a blocking copy =
        # a stream synchronisation right before the losses) without adding a state-dict key the reference does not have
        self.register_buffer("class_weights", L.semkitti_class_weights(), persistent=False)
        self.semkitti_loss_weight_cfg = semkitti_loss_weight_cfg or {}
        # the soft-Dice and the LGA-weighted losses run behind constructor flags of this head (the reference has none): the weight
        # alone does not switch them on; alpha = beta = 1 as in the reference's PositionAwareLoss(num_class=out_channel)
        self.use_dice_loss, self.use_lga_loss = bool(use_dice_loss), bool(use_lga_loss)
        for k, flag, on in (("voxel_dice", "use_dice_loss", self.use_dice_loss), ("voxel_lga", "use_lga_loss", self.use_lga_loss)):
            if self.semkitti_loss_weight_cfg.get(k, 0.0) > 0 and not on:
                raise NotImplementedError(f"loss '{k}' is disabled in the reference config: pass {flag}=True to OccHead to "
                                          "compute it")
        # the frustum-proportion loss runs behind a constructor flag of this head (the reference has none): the weight alone
        # does not switch it on, because it needs the loader's frustums_ids / frustums_class_dists in the call of loss()
        self.use_frustum_loss = bool(use_frustum_loss)
        if self.semkitti_loss_weight_cfg.get("frustum_dist", 0.0) > 0 and not self.use_frustum_loss:
            raise NotImplementedError("loss 'frustum_dist' is disabled in the reference config: pass use_frustum_loss=True to "
                                      "OccHead (and CreateRelationLabels' outputs to loss()) to compute it")
        # the OHEM cross entropy runs behind the reference's constructor flag: the weight alone does not switch it on
        self.use_ohem_loss, self.ohem_topk = bool(use_ohem_loss), float(ohem_topk)
        if not 0.0 < self.ohem_topk <= 1.0:
            raise ValueError(f"ohem_topk must be in (0, 1], got {ohem_topk}")
        if self.semkitti_loss_weight_cfg.get("voxel_ohem", 0.0) > 0 and not self.use_ohem_loss:
            raise NotImplementedError("loss 'voxel_ohem' is disabled in the reference config: pass use_ohem_loss=True to "
                                      "OccHead to compute it")

    def forward_voxel(self, voxel_feats):
        return [conv(f) for f, conv in zip(voxel_feats, self.occ_convs)]

    def sample_point_feats(self, points, voxel_feats, img_feats=None, points_uv=None):
        """occhead.py:171-236 for the whole batch at once: ``points`` list of [N_b, >= 3], ``points_uv`` list of [N_b, cams, 3],
        ``img_feats`` [B, cams, C_img, fH, fW] -> rows [sum N_b, C].  The row-wise layers run on the concatenation (same
        arithmetic per row); the second soft-weight Linear has ``num_point_sampling_feat`` (2 in the config) output rows, which
        are zero-padded to a multiple of 4 so that this product stays on the own GEMM kernels too."""
        counts = [int(p.shape[0]) for p in points]
        g = F.point_unit(torch.cat([p[:, :3].float() for p in points], 0), self.point_cloud_range.tolist())
        feats = list(voxel_feats[:self.num_level])
        g = g.to(feats[0].device)
        sets = list(F.point_sample(feats, g, counts, self.point_axis_order, per_level=self.soft_weights).unbind(0)) \
            if self.soft_weights else [F.point_sample(feats, g, counts, self.point_axis_order)]
        if self.sampling_img_feats:
            uv = torch.cat([u.float() for u in points_uv], 0).to(g.device)
            rows = F.point_img_sample(img_feats, uv, counts)
            sets.append(F.small_linear(rows, self.img_feat_reduce.weight, self.img_feat_reduce.bias))
        if not self.soft_weights:
            return sum(sets[1:], sets[0])
        fc1, fc2 = self.point_soft_weights[0], self.point_soft_weights[2]
        nl = fc2.out_features
        pad = -nl % 4
        h = torch.relu(F.small_linear(sets[0], fc1.weight, fc1.bias))
        w = F.small_linear(h, torch.nn.functional.pad(fc2.weight, (0, 0, 0, pad)), torch.nn.functional.pad(fc2.bias, (0, pad)))
        w = torch.softmax(w[:, :nl], dim=1)
        out = 0
        for rows, wl in zip(sets, torch.unbind(w, dim=1)):
            out = out + rows * wl.unsqueeze(1)
        return out

    def forward_points(self, points, voxel_feats, img_feats=None, points_uv=None):
        counts = [int(p.shape[0]) for p in points]
        K = self.point_occ_mlp.fc2.out_features
        if sum(counts) == 0:
            zero = sum((p * 0).sum() for p in self.parameters())
            return [voxel_feats[0].new_zeros(0, K) + zero for _ in counts]
        logits = self.point_occ_mlp(self.sample_point_feats(points, voxel_feats, img_feats, points_uv))
        return list(torch.split(logits, counts, 0))

    def forward(self, voxel_feats, points=None, img_metas=None, img_feats=None, points_uv=None, **kwargs):
        assert type(voxel_feats) is list and len(voxel_feats) == self.num_level
        output_points = None
        if self.supervise_points:
            missing = [n for n, v in (("points_occ", points), ("points_uv", points_uv if self.sampling_img_feats else 0))
                       if v is None]
            if missing and (self.training or points is not None):
                raise KeyError(f"supervise_points=True needs the kwargs {missing} (pipelines.CreateDepthFromLiDAR + "
                               "OccDefaultFormatBundle3D provide them)")
            if self.sampling_img_feats and points is not None and img_feats is None:
                raise KeyError("sampling_img_feats=True needs 'img_feats' (the detector passes the left view's neck output)")
            if points is not None:
                output_points = self.forward_points(points, voxel_feats, img_feats, points_uv)
        return {"output_voxels": self.forward_voxel(voxel_feats), "output_points": output_points}

    def loss_point_single(self, output_points, target_points, tag=""):
        """occhead.py:363-398 with ``semantic_kitti=True`` (no ``point_mean_iou``): labels = ``target_points[:, -1]``, class 0
        ignored; both losses exactly 0 with zero gradients when no point is labelled."""
        labels = target_points[:, -1].to(output_points.device)
        out = {}
        if self.loss_point_ce_weight > 0:
            out[f"loss_point_ce_{tag}"] = F.point_ce_loss(output_points, labels) * self.loss_point_ce_weight
        if self.loss_point_lovasz_weight > 0:
            out[f"loss_point_lovasz_{tag}"] = F.point_lovasz_loss(output_points, labels) * self.loss_point_lovasz_weight
        return out

    def loss_voxel_single_semkitti(self, output_voxels, target_voxels, tag, compute_metric=False, **kwargs):
        w = self.semkitti_loss_weight_cfg
        return L.occ_losses(output_voxels, target_voxels, self.class_weights.to(output_voxels), tag,
                            w.get("voxel_ce", 0.0), w.get("voxel_sem_scal", 0.0), w.get("voxel_geo_scal", 0.0),
                            compute_metric, w.get("voxel_lovasz", 0.0),
                            w.get("voxel_ohem", 0.0) if self.use_ohem_loss else 0.0, self.ohem_topk,
                            w.get("frustum_dist", 0.0) if self.use_frustum_loss else 0.0, kwargs,
                            w.get("voxel_dice", 0.0) if self.use_dice_loss else 0.0,
                            w.get("voxel_lga", 0.0) if self.use_lga_loss else 0.0)

    def loss(self, output_voxels=None, target_voxels=None, output_points=None, target_points=None, img_metas=None,
             **kwargs):
        targets = target_voxels[:self.num_level] if type(target_voxels) is list else [target_voxels] * self.num_level
        out = {}
        for i, o in enumerate(output_voxels):
            out.update(self.loss_voxel_single_semkitti(o, targets[i], tag=str(i), compute_metric=(i == 0), **kwargs))
        if self.supervise_points:
            if output_points is None or target_points is None:
                raise KeyError("supervise_points=True needs 'points_occ' (output_points / target_points) in loss()")
            out.update(self.loss_point_single(torch.cat(output_points, 0), torch.cat(list(target_points), 0), tag=""))
        return out
