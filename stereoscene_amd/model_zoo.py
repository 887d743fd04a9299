"""Model construction helpers for the benchmark / smoke / tests: the reference's model dict
(projects/configs/occupancy/semantickitti/stereoscene.py:57-126) re-derived for a given grid."""
import torch

from . import synthetic as S


def image_branch_cfg(arch="b7"):
    """``img_backbone`` / ``img_neck`` of the reference config (stereoscene.py:59-74), minus the checkpoint init."""
    return dict(
        img_backbone=dict(type="CustomEfficientNet", arch=arch, drop_path_rate=0.2, frozen_stages=0, norm_eval=False,
                          out_indices=(2, 3, 4, 5, 6), with_cp=True),
        img_neck=dict(type="SECONDFPN", in_channels=[48, 80, 224, 640, 2560], upsample_strides=[0.5, 1, 2, 4, 4],
                      out_channels=[128, 128, 128, 128, 128]))


def model_cfg(cfg, numC_Trans=128, warp_align_corners=True, image_branch=False, loss_depth_type="bce", voxel_ohem=0.0,
              ohem_topk=0.25, frustum_dist=0.0, voxel_dice=0.0, voxel_lga=0.0, imgseg=False, loss_seg_weight=1.0,
              lift_with_imgseg=False, imgseg_labels="img_seg", crp3d=False, crp_level=2, point_xyz_channel=0, point_xyz_mode="cat",
              supervise_points=False, sampling_img_feats=True, soft_weights=True, point_axis_order="reference"):
    """Same structure and hyper-parameters as the reference config's ``model`` dict for the sizes in ``cfg`` (a
    synthetic.CFG_*).  ``image_branch=False`` (default, the benchmarked hot path a1-a16) leaves the 2-D
    image backbone/neck out: the detector then takes the image-neck features in place of raw images.  ``loss_depth_type``:
    "bce" (the reference config's value) or "kld".  ``voxel_ohem`` > 0 switches the head's OHEM cross entropy on with that
    weight (``semkitti_loss_weight_cfg.voxel_ohem``, ``use_ohem_loss=True``) and ``ohem_topk`` as the kept fraction.
    ``frustum_dist`` > 0 switches the head's frustum-proportion loss on with that weight
    (``semkitti_loss_weight_cfg.frustum_dist``, ``use_frustum_loss=True``); the training call then needs ``frustums_ids`` / ``frustums_class_dists`` (pipelines.CreateRelationLabels).
    ``voxel_dice`` / ``voxel_lga`` > 0 switch the head's soft-Dice / LGA-weighted losses on with that weight
    (``semkitti_loss_weight_cfg.voxel_dice`` / ``.voxel_lga``, ``use_dice_loss=True`` / ``use_lga_loss=True``).
    ``imgseg=True`` builds the view transformer's image-view segmentation head and adds ``loss_imgseg`` (weight
    ``loss_seg_weight``); the training call then needs the label map named by ``imgseg_labels`` ("img_seg", the reference's
    right-view map, or "img_seg_left").  ``lift_with_imgseg=True`` lifts the 20 class probabilities with the features: the 3-D
    encoder then takes ``numC_Trans + 20`` channels.  ``crp3d=True`` builds the 3-D encoder's context relation prior behind stage
    ``crp_level`` (on that stage's grid: ``crp_size``) and adds ``loss_rel_ce``; the training call then needs ``CP_mega_labels``
    (pipelines.CreateRelationLabels(relations=True)) or a dense ``CP_mega_matrix``.  ``point_xyz_channel`` > 0 (a multiple of 8)
    pools a learned encoding of every lifted point's position next to the features (``point_xyz_mode`` "cat": the 3-D encoder
    takes that many more channels; "add": the width is ``numC_Trans`` and the encoding is added), fp32 only.
    ``supervise_points=True`` builds the head's point-level branch (``sampling_img_feats`` / ``soft_weights``: the reference
    config's values by default; ``point_axis_order`` "reference" or "xyz", see ``OccHead``) and adds ``loss_point_ce_`` /
    ``loss_point_lovasz_``; the training call then needs ``points_occ`` and ``points_uv`` (pipelines.CreateDepthFromLiDAR)."""
    seg = dict(imgseg=True, imgseg_class=20, loss_seg_weight=float(loss_seg_weight), lift_with_imgseg=bool(lift_with_imgseg)) \
        if imgseg else {}
    bev_in = numC_Trans + (20 if imgseg and lift_with_imgseg else 0)
    xyz = {}
    if point_xyz_channel:
        xyz = dict(point_xyz_channel=int(point_xyz_channel), point_xyz_mode=point_xyz_mode, point_cloud_range=list(cfg["pc_range"]))
        bev_in += int(point_xyz_channel) if point_xyz_mode == "cat" else 0
    norm_cfg = dict(type="GN", num_groups=32, requires_grad=True)
    channels = [128, 256, 512]
    crp = {}
    if crp3d:
        if not 0 <= crp_level < len(channels):
            raise ValueError(f"crp_level must name one of the {len(channels)} encoder stages, got {crp_level}")
        # the encoder works on the lifted grid (occ_size / 2); stage i halves it i times
        crp = dict(crp3d=True, crp_level=int(crp_level), crp_size=tuple(int(v) // (2 << crp_level) for v in cfg["occ_size"]))
    return dict(
        type="BEVDepthOccupancy", **(image_branch_cfg() if image_branch else {}),
        img_view_transformer=dict(
            type="ViewTransformerLiftSplatShootVoxel", downsample=cfg["downsample"], numC_input=640,
            cam_channels=30, semkitti=False, loss_depth_weight=1.0, grid_config=S.grid_config(cfg),
            data_config=dict(input_size=tuple(cfg["input_size"])), numC_Trans=numC_Trans, vp_megvii=False,
            warp_align_corners=warp_align_corners, loss_depth_type=loss_depth_type, **seg, **xyz),
        img_bev_encoder_backbone=dict(type="CustomResNet3D", depth=18, num_stage=3, n_input_channels=bev_in,
                                      block_inplanes=channels, out_indices=(0, 1, 2), norm_cfg=norm_cfg, **crp),
        img_bev_encoder_neck=dict(type="SECONDFPN3D", norm_cfg=norm_cfg, in_channels=channels,
                                  upsample_strides=[1, 2, 4], out_channels=[128, 128, 128]),
        pts_bbox_head=dict(type="OccHead", num_level=1, in_channels=[384], out_channel=20, semantic_kitti=True,
                           point_cloud_range=list(cfg["pc_range"]), supervise_points=bool(supervise_points),
                           sampling_img_feats=bool(sampling_img_feats), in_img_channels=640, soft_weights=bool(soft_weights),
                           **(dict(point_axis_order=point_axis_order) if supervise_points else {}),
                           **(dict(use_ohem_loss=True, ohem_topk=ohem_topk) if voxel_ohem > 0 else {}),
                           **(dict(use_frustum_loss=True) if frustum_dist > 0 else {}),
                           **(dict(use_dice_loss=True) if voxel_dice > 0 else {}),
                           **(dict(use_lga_loss=True) if voxel_lga > 0 else {}),
                           semkitti_loss_weight_cfg={"voxel_ce": 1.0, "voxel_sem_scal": 1.0, "voxel_geo_scal": 1.0,
                                                     "voxel_ohem": float(voxel_ohem), "voxel_lovasz": 0.0,
                                                     "frustum_dist": float(frustum_dist),
                                                     **({"voxel_dice": float(voxel_dice)} if voxel_dice > 0 else {}),
                                                     **({"voxel_lga": float(voxel_lga)} if voxel_lga > 0 else {})}),
        **(dict(imgseg_labels=imgseg_labels) if imgseg else {}),
        train_cfg=dict(pts=None), test_cfg=dict(pts=None))


def build_detector(cfg, device="cuda", fill=True, **kw):
    from . import plugin  # noqa: F401  (fills the registries)
    from .registry import DETECTORS
    m = DETECTORS.build(model_cfg(cfg, **kw))
    if fill:
        S.fill_state_dict_(m)
    return m.to(device)


def img_inputs_from_sample(smp, device="cuda"):
    """(left10, right10) tuples in the reference's ``img_inputs`` layout; slot 0 carries
    the image-neck features instead of raw images."""
    def side(x, geo, gt_depths, calib):
        rots, trans, intr, post_rots, post_trans, bda = (t.to(device) for t in geo)
        if torch.device(device).type == "cuda":      # what the data layer does (pipelines.collate): see attach_host_inverses
            from .plugin.view_transformer import attach_host_inverses
            attach_host_inverses(post_rots, intr, geo[3], geo[2])
        B = x.shape[0]
        s2s = intr.new_zeros(B, 1, 4, 4)
        return (x.to(device), rots, trans, intr, post_rots, post_trans, bda, gt_depths.to(device), s2s,
                calib.to(device))
    gd = smp["gt_depths"]
    return (side(smp["x_l"], smp["geo_l"], gd, smp["calib"]), side(smp["x_r"], smp["geo_r"], gd, smp["calib"]))
