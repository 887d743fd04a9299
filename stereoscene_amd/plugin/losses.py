"""SemanticKITTI occupancy losses and SSC metric of the hot path (device-side torch ops).

Mirrors utils/semkitti.py:67-149 (CE_ssc_loss / sem_scal_loss / geo_scal_loss), the loss assembly
of occhead.py:291-361 and SSCMetrics (utils/ssc_metric.py:40-169).  The per-class Python loop of
the reference's sem_scal_loss is replaced by one pass of class-indexed reductions (same sums)."""
import numpy as np
import torch
import torch.nn.functional as TF

KITTI_CLASS_NAMES = ["empty", "car", "bicycle", "motorcycle", "truck", "other-vehicle", "person", "bicyclist",
                     "motorcyclist", "road", "parking", "sidewalk", "other-ground", "building", "fence",
                     "vegetation", "trunk", "terrain", "pole", "traffic-sign"]

# SemanticKITTI per-class voxel counts (dataset statistics, utils/semkitti.py:8-31)
CLASS_FREQUENCIES = np.array([
    5.41773033e09, 1.57835390e07, 1.25136000e05, 1.18809000e05, 6.46799000e05, 8.21951000e05, 2.62978000e05,
    2.83696000e05, 2.04750000e05, 6.16887030e07, 4.50296100e06, 4.48836500e07, 2.26992300e06, 5.68402180e07,
    1.57196520e07, 1.58442623e08, 2.06162300e06, 3.69705220e07, 1.15198800e06, 3.34146000e05])


def semkitti_class_weights():
    return torch.from_numpy(1 / np.log(CLASS_FREQUENCIES + 0.001)).float()


def _nll_to_one(v):
    """BCE(v, 1) with torch's log clamp at -100."""
    return -torch.clamp(torch.log(v), min=-100.0)


def ce_ssc_loss(logits, target, class_weights):
    return TF.cross_entropy(logits, target.long(), weight=class_weights, ignore_index=255, reduction="mean")


def scal_losses(logits, target):
    """(sem_scal, geo_scal): all class-wise sums in one sweep over the softmax volume."""
    n_cls = logits.shape[1]
    prob = torch.softmax(logits, dim=1)
    valid = target != 255
    p = prob.permute(0, 2, 3, 4, 1)[valid]                    # [M, C]
    t = target[valid].long()                                   # [M]
    onehot = TF.one_hot(t, n_cls).to(p.dtype)                  # [M, C]
    M = p.shape[0]
    sum_p = p.sum(0)                                           # sum of p_c
    cnt = onehot.sum(0)                                        # |{t == c}|
    nom = (p * onehot).sum(0)                                  # sum p_c [t == c]
    spec_num = (M - cnt) - (sum_p - nom)                       # sum (1-p_c)(1-[t==c])
    present = cnt > 0
    loss_c = torch.zeros_like(sum_p)
    loss_c = loss_c + torch.where(sum_p > 0, _nll_to_one(nom / sum_p.clamp_min(1e-30)), torch.zeros_like(sum_p))
    loss_c = loss_c + _nll_to_one(nom / cnt.clamp_min(1.0))
    neg = M - cnt
    loss_c = loss_c + torch.where(neg > 0, _nll_to_one(spec_num / neg.clamp_min(1.0)), torch.zeros_like(sum_p))
    sem = (loss_c * present).sum() / present.sum()
    # geometric: occupied vs empty
    occ_t = (t != 0).to(p.dtype)
    occ_p = 1 - p[:, 0]
    inter = (occ_t * occ_p).sum()
    geo = (_nll_to_one(inter / occ_p.sum()) + _nll_to_one(inter / occ_t.sum())
           + _nll_to_one(((1 - occ_t) * p[:, 0]).sum() / (1 - occ_t).sum()))
    return sem, geo


def ssc_counts(pred, gt, n_classes=20, recompute_mask=False):
    """Integer tp/fp/fn for completion and per class (SSCMetrics semantics, see oracle docstring)."""
    valid = gt != 255
    p = torch.where(valid, pred, torch.zeros_like(pred)).reshape(-1)
    g = torch.where(valid, gt, torch.zeros_like(gt)).reshape(-1)
    v = valid.reshape(-1)
    po, go = (p > 0) & v, (g > 0) & v
    tp = (po & go).sum()
    fp = (po & ~go & v).sum()
    fn = (~po & go & v).sum()
    sel = torch.ones_like(v) if recompute_mask else v
    conf = torch.bincount((g[sel] * n_classes + p[sel]).long(), minlength=n_classes * n_classes)
    conf = conf.view(n_classes, n_classes)                       # [gt, pred]
    tpc = conf.diagonal()
    fpc = conf.sum(0) - tpc
    fnc = conf.sum(1) - tpc
    return tp, fp, fn, tpc, fpc, fnc


def confusion_counts(pred, gt, n_classes=20):
    """Per-sample confusion of a label volume: (conf int64 [B,n,n] indexed [gt][pred] over the voxels with gt != 255, n_ignored
    int64 [B]) -- what the fused inference epilogue (``functional.occ_predict``) returns, from tensor ops."""
    B = gt.shape[0]
    p, g = pred.reshape(B, -1).long(), gt.reshape(B, -1).long()
    valid = g != 255
    key = torch.where(valid, g * n_classes + p, torch.full_like(g, n_classes * n_classes))
    key = key + torch.arange(B, device=key.device).view(B, 1) * (n_classes * n_classes + 1)
    cnt = torch.bincount(key.reshape(-1), minlength=B * (n_classes * n_classes + 1)).view(B, -1)
    return cnt[:, :-1].reshape(B, n_classes, n_classes), cnt[:, -1]


def ssc_counts_from_confusion(conf, n_ignored):
    """``ssc_counts(pred, gt, 20, recompute_mask=True)`` from the confusion counts ``conf`` [20,20] or [B,20,20] ([gt][pred] over
    the labelled voxels; a batch is summed) and the number of ignored voxels.  SSCMetrics counts an ignored voxel as a
    (gt 0, pred 0) pair in the per-class statistics (utils/ssc_metric.py:123-169 re-derives the mask from the zeroed target), so
    ``tpc[0]`` includes them; the completion counts see labelled voxels only.  Integer algebra on 400 numbers, any device."""
    n = conf.shape[-1]
    conf = conf.reshape(-1, n, n).sum(0).long()
    tp = conf[1:, 1:].sum()
    fp = conf[0, 1:].sum()
    fn = conf[1:, 0].sum()
    full = conf.clone()
    full[0, 0] += torch.as_tensor(n_ignored, device=conf.device).long().sum()
    tpc = full.diagonal()
    fpc = full.sum(0) - tpc
    fnc = full.sum(1) - tpc
    return tp, fp, fn, tpc, fpc, fnc


def _nll1(v):
    return -torch.clamp(torch.log(v), min=-100.0)


def lovasz_softmax_tensor(logits, target, ignore=255):
    """Lovasz-softmax (lovasz_softmax.py:21-33, 156-225 with classes='present', per_image=False) of logits that already sit on
    the label grid, from tensor ops on any device and in the logits' dtype: ignored voxels dropped, one descending sort per class
    present in the labels, mean over those classes; a zero with a zero gradient when no voxel is labelled."""
    n_cls = logits.shape[1]
    valid = target != ignore
    p = torch.softmax(logits, dim=1).permute(0, 2, 3, 4, 1)[valid]   # [M, C]
    t = target[valid].long()                                          # [M]
    if t.numel() == 0:
        return logits.sum() * 0.0
    cnt = torch.bincount(t, minlength=n_cls)[:n_cls]
    losses = []
    for c in torch.nonzero(cnt).flatten().tolist():
        fg = (t == c).to(p.dtype)
        err, perm = torch.sort((fg - p[:, c]).abs(), 0, descending=True)
        fg_sorted = fg[perm]
        total = fg_sorted.sum()
        jac = 1.0 - (total - fg_sorted.cumsum(0)) / (total + (1.0 - fg_sorted).cumsum(0))
        losses.append(torch.dot(err, torch.cat((jac[:1], jac[1:] - jac[:-1]))))
    if not losses:                                                    # labelled voxels, but none of a known class
        return logits.sum() * 0.0
    return torch.stack(losses).mean()


def lovasz_softmax_loss(logits, gt_occ, ignore=255):
    """Unweighted Lovasz-softmax voxel loss of the head (occhead.py:284-287, 321-324): logits [B,C,d,h,w] are up-sampled
    trilinearly to the grid of ``gt_occ`` [B,D,H,W].  The fused HIP path serves what ``functional.lovasz_supported`` accepts;
    everything else (other devices, dtypes, class counts or ratios, ``SSBEV_LOVASZ=0``) runs ``lovasz_softmax_tensor``."""
    from .. import functional as F
    if F.LOVASZ and F.lovasz_supported(logits, gt_occ):
        return F.lovasz_softmax(logits, gt_occ, ignore)
    if logits.shape[-3:] != gt_occ.shape[-3:]:
        if logits.is_cuda:
            logits = F.upsample_trilinear(logits, gt_occ.shape[-3:])
        else:                                                         # (the HIP up-sampling has no CPU form)
            logits = TF.interpolate(logits, size=tuple(gt_occ.shape[-3:]), mode="trilinear", align_corners=False)
    return lovasz_softmax_tensor(logits, gt_occ, ignore)


def ohem_k(n_labelled, top_k):
    """Voxels a sample keeps: the reference's ``int(flatten_loss_i.shape[0] * top_k)`` (a double product, truncated)."""
    return int(n_labelled * top_k)


def ohem_ce_tensor(logits, target, class_weights, top_k=0.25):
    """OHEM_CE_ssc_loss (utils/semkitti.py:151-185) of logits that already sit on the label grid, from tensor ops on any device
    and in the logits' dtype: class-weighted cross entropy per voxel; per sample the ``int(M_b * top_k)`` largest losses of its
    M_b labelled voxels; sum of the kept losses over the sum of the kept voxels' class weights (clamped at 1e-4), both over the
    batch.  The selection is a STABLE descending sort, so equal losses go to the lowest voxel index -- the rule of the fused
    kernel (``torch.topk`` leaves the choice among ties open).  The losses are canonicalised to +0.0 first (a saturated voxel
    gives -0.0).  A zero with a zero gradient when nothing is selected."""
    loss = TF.cross_entropy(logits, target.long(), weight=class_weights, ignore_index=255, reduction="none").flatten(1)
    loss = loss + 0.0                                                 # -0.0 -> +0.0
    flat = target.flatten(1)
    top, norm = logits.sum() * 0.0, class_weights.sum() * 0.0
    for b in range(loss.shape[0]):
        valid = flat[b] != 255
        li = loss[b, valid]
        k = ohem_k(li.shape[0], top_k)
        if k == 0:
            continue
        keep = torch.argsort(li.detach(), descending=True, stable=True)[:k]
        top = top + li[keep].sum()
        norm = norm + class_weights[flat[b, valid].long()][keep].sum()
    return top / torch.clamp_min(norm.detach(), 1e-4)


def ohem_ce_loss(logits, gt_occ, class_weights, top_k=0.25):
    """OHEM cross-entropy voxel loss of the head (occhead.py:315-319): logits [B,C,d,h,w] are up-sampled trilinearly to the grid
    of ``gt_occ`` [B,D,H,W].  The fused HIP path serves what ``functional.ohem_supported`` accepts; everything else (other
    devices, dtypes, class counts or ratios, ``SSBEV_OHEM=0``) runs ``ohem_ce_tensor``."""
    from .. import functional as F
    if F.OHEM and F.ohem_supported(logits, gt_occ):
        return F.ohem_ce_loss(logits, gt_occ, class_weights, top_k)
    if logits.shape[-3:] != gt_occ.shape[-3:]:
        if logits.is_cuda:
            logits = F.upsample_trilinear(logits, gt_occ.shape[-3:])
        else:                                                         # (the HIP up-sampling has no CPU form)
            logits = TF.interpolate(logits, size=tuple(gt_occ.shape[-3:]), mode="trilinear", align_corners=False)
    return ohem_ce_tensor(logits, gt_occ, class_weights.to(logits), top_k)


def frustum_dist_tensor(logits, ids_or_masks, dists):
    """compute_frustum_dist_loss (utils/semkitti.py:218-244) of logits that already sit on the frustum grid, from tensor ops on any
    device and in the logits' dtype, without a read-back.  ``ids_or_masks``: the id volume [B,X,Y,Z] (integer; 255 = in no frustum)
    or the reference's dense bool masks [B,F,X,Y,Z] (which may overlap); ``dists`` [B,F,C] class counts.  Per frustum, pooled
    over the batch: cum = sum of the softmax over its voxels, t = counts / their sum, q = cum / its sum, the term
    sum over t_c != 0 of t_c (log t_c - log q_c) (``KL_sep``); the mean over the frusta whose two sums are both > 0.  With no such
    frustum the reference divides 0 / 0 (ZeroDivisionError); here the loss is 0 with a zero gradient."""
    p = torch.softmax(logits, dim=1)
    B, Cn = p.shape[:2]
    F = dists.shape[1]
    if ids_or_masks.dim() == 5:
        cum = torch.einsum("bfn,bcn->fc", ids_or_masks.flatten(2).to(p.dtype), p.flatten(2))
    else:
        ids = ids_or_masks.flatten(1).long()
        ids = torch.where(ids < F, ids, torch.full_like(ids, F))                   # row F collects the voxels of no frustum
        cum = p.new_zeros(F + 1, Cn).index_add_(0, ids.reshape(-1), p.flatten(2).transpose(1, 2).reshape(-1, Cn))[:F]
    cnt = dists.to(p.dtype).sum(0)
    total_prob, total_cnt = cum.sum(1, keepdim=True), cnt.sum(1, keepdim=True)
    counted = (total_prob > 0) & (total_cnt > 0)                                  # [F, 1]
    one = torch.ones_like(total_prob)
    t = cnt / torch.where(counted, total_cnt, one)
    q = cum / torch.where(counted, total_prob, one)
    use = counted & (t != 0)
    term = torch.where(use, t * (torch.log(torch.where(use, t, one)) - torch.log(torch.where(use, q, one))), torch.zeros_like(t))
    n = counted.sum().to(p.dtype)
    return term.sum() / torch.where(n > 0, n, torch.ones_like(n))


def frustum_dist_loss(logits, ids_or_masks, dists):
    """Frustum-proportion voxel loss of the head (occhead.py:326-329): logits [B,C,d,h,w] are up-sampled trilinearly to the grid of
    the ids [B,D,H,W] (or of the reference's dense masks [B,F,D,H,W], which are turned into ids when they are disjoint).  The fused
    HIP path serves what ``functional.frustum_dist_supported`` accepts; everything else (other devices, dtypes, class counts or
    ratios, overlapping masks, ``SSBEV_FRUSTUM_DIST=0``) runs ``frustum_dist_tensor``."""
    from .. import functional as F
    ids_or_masks = ids_or_masks.to(logits.device)                     # (the loader step's output may still live on the host)
    if ids_or_masks.dim() == 5 and F.FRUSTUM_DIST and logits.is_cuda:
        ids = F.frustum_ids_from_masks(ids_or_masks)
        ids_or_masks = ids_or_masks if ids is None else ids
    if ids_or_masks.dim() == 4 and F.FRUSTUM_DIST and F.frustum_dist_supported(logits, ids_or_masks.to(torch.uint8), dists):
        return F.frustum_dist_loss(logits, ids_or_masks, dists)
    grid = tuple(ids_or_masks.shape[-3:])
    if tuple(logits.shape[-3:]) != grid:
        if logits.is_cuda:
            logits = F.upsample_trilinear(logits, grid)
        else:                                                         # (the HIP up-sampling has no CPU form)
            logits = TF.interpolate(logits, size=grid, mode="trilinear", align_corners=False)
    return frustum_dist_tensor(logits, ids_or_masks, dists.detach().to(logits))


def _frustum_term(logits, gt_occ, frustums):
    """The frustum-proportion loss from the head's keyword arguments: ``frustums_ids`` (preferred) or ``frustums_masks``, and
    ``frustums_class_dists``."""
    if frustums is None or "frustums_class_dists" not in frustums:
        raise KeyError("frustums_class_dists")
    if frustums.get("frustums_ids") is not None:
        vol = frustums["frustums_ids"]
    elif frustums.get("frustums_masks") is not None:
        vol = frustums["frustums_masks"]
    else:
        raise KeyError("frustums_ids")
    if tuple(vol.shape[-3:]) != tuple(gt_occ.shape[-3:]):
        raise ValueError(f"frustum_dist: the frustum grid {tuple(vol.shape[-3:])} is not the label grid {tuple(gt_occ.shape[-3:])}")
    return frustum_dist_loss(logits, vol, frustums["frustums_class_dists"])


def dice_tensor(logits, target, smooth=1.0):
    """Soft-Dice voxel loss of the head (occhead.py:331-336, SoftDiceLossWithProb of utils/dice_loss.py:36-66 with p = 1) of logits
    that already sit on the label grid, from tensor ops on any device and in the logits' dtype: the occupied probability
    ``softmax(logits)[:, 1:].sum(1)`` against ``target > 0`` over the labelled voxels,
    1 - (2 sum(p t) + smooth) / (sum(p) + sum(t) + smooth).  Nothing labelled gives 1 - smooth / smooth = 0 with a zero gradient."""
    p = torch.softmax(logits, dim=1)[:, 1:].sum(dim=1)
    valid = target != 255
    p = p[valid]
    t = (target[valid] > 0).to(p.dtype)
    return 1.0 - (2.0 * (p * t).sum() + smooth) / ((p + t).sum() + smooth)


def dice_from_sums(diff, aux, smooth=1.0):
    """``dice_tensor`` from the sums of the fused epilogue (``functional.occ_loss_sums``), in their dtype (float64): with
    p_occ = 1 - p_0, sum(p_occ [t > 0]) = (M - cnt0) - (sum_p0 - nom0) (the ``inter`` of geo_scal), sum(p_occ) = M - sum_p0 and
    sum([t > 0]) = M - cnt0.  The torch algebra behind ``SSBEV_OCC_TAIL=0``; ``functional.occ_dice_tail`` is the one-launch form."""
    nc = (diff.numel() - 1) // 2
    sum_p0, nom0 = diff[1], diff[1 + nc]
    M, cnt0 = aux[1], aux[2]
    occ_t = M - cnt0
    inter = occ_t - (sum_p0 - nom0)
    return 1.0 - (2.0 * inter + smooth) / ((M - sum_p0) + occ_t + smooth)


def lga_weights_tensor(target):
    """TWICE the local geometric anisotropy of ``PositionAwareLoss.get_lga`` (utils/pal_loss.py: the sum over the 20 class masks of
    the 1-norm of ``torch.gradient``) for labels [B,X,Y,Z], uint8 in 0..12 and exact, from tensor ops on any device.  Per axis, with
    is(t) = [t < 20]: an interior voxel adds is(t-) + is(t+) when its two neighbours differ (its own label does not enter); the
    first and the last voxel add 2 (is(a) + is(b)) [a != b] of the end pair (the one-sided difference).  An ignored voxel (255) is
    in no class mask but is a neighbour that differs.  An axis shorter than 2 is a ``ValueError`` (``torch.gradient`` raises too)."""
    if target.dim() != 4 or min(target.shape[1:]) < 2:
        raise ValueError(f"lga_weights_tensor: labels [B,X,Y,Z] with every axis >= 2 expected, got {tuple(target.shape)}")
    t = target.to(torch.int16)
    isc = (t < 20).to(torch.int16)
    out = torch.zeros_like(t)

    def pair(a, b, ia, ib):
        return (a != b).to(torch.int16) * (ia + ib)
    for dim in (1, 2, 3):
        n = t.shape[dim]
        first = 2 * pair(t.narrow(dim, 0, 1), t.narrow(dim, 1, 1), isc.narrow(dim, 0, 1), isc.narrow(dim, 1, 1))
        last = 2 * pair(t.narrow(dim, n - 2, 1), t.narrow(dim, n - 1, 1), isc.narrow(dim, n - 2, 1), isc.narrow(dim, n - 1, 1))
        parts = [first]
        if n > 2:
            parts.append(pair(t.narrow(dim, 0, n - 2), t.narrow(dim, 2, n - 2), isc.narrow(dim, 0, n - 2), isc.narrow(dim, 2, n - 2)))
        parts.append(last)
        out = out + torch.cat(parts, dim=dim)
    return out.to(torch.uint8)


def pal_tensor(logits, target, class_weights, alpha=1.0, beta=1.0):
    """PositionAwareLoss (utils/pal_loss.py) of logits that already sit on the label grid, from tensor ops on any device and in the
    logits' dtype, without a read-back: the class-weighted cross entropy per voxel times alpha + beta lga, summed over the labelled
    voxels, over the sum of their class weights.  With nothing labelled the reference divides 0 / 0; here the loss is 0 with a
    zero gradient."""
    loss = TF.cross_entropy(logits, target.long(), weight=class_weights, ignore_index=255, reduction="none")
    fac = alpha + beta * (0.5 * lga_weights_tensor(target).to(loss.dtype))
    valid = target != 255
    num = (loss * fac * valid.to(loss.dtype)).sum()
    den = (class_weights[target.long().clamp(max=class_weights.numel() - 1)] * valid.to(class_weights.dtype)).sum().detach()
    return num / torch.where(den > 0, den, torch.ones_like(den))


def occ_lga_loss(logits, gt_occ, class_weights, alpha=1.0, beta=1.0):
    """LGA-weighted voxel loss of the head (occhead.py:338-343): logits [B,C,d,h,w] are up-sampled trilinearly to the grid of
    ``gt_occ`` [B,D,H,W].  The fused HIP path serves what ``functional.occ_lga_supported`` accepts; everything else (other devices,
    dtypes, class counts or ratios, ``SSBEV_LGA=0``) runs ``pal_tensor``."""
    from .. import functional as F
    if F.LGA and F.occ_lga_supported(logits, gt_occ):
        return F.occ_lga_loss(logits, gt_occ, class_weights, alpha, beta)
    if logits.shape[-3:] != gt_occ.shape[-3:]:
        if logits.is_cuda:
            logits = F.upsample_trilinear(logits, gt_occ.shape[-3:])
        else:                                                         # (the HIP up-sampling has no CPU form)
            logits = TF.interpolate(logits, size=tuple(gt_occ.shape[-3:]), mode="trilinear", align_corners=False)
    return pal_tensor(logits, gt_occ, class_weights.to(logits), alpha, beta)


def _dice_term(logits, gt_occ):
    """The soft-Dice loss outside the fused epilogue: up-sample, then ``dice_tensor``."""
    if logits.shape[-3:] != gt_occ.shape[-3:]:
        if logits.is_cuda:
            from ..functional import upsample_trilinear
            logits = upsample_trilinear(logits, gt_occ.shape[-3:])
        else:
            logits = TF.interpolate(logits, size=tuple(gt_occ.shape[-3:]), mode="trilinear", align_corners=False)
    return dice_tensor(logits, gt_occ)


def occ_losses_fused(logits, gt_occ, class_weights, tag="0", w_ce=1.0, w_sem=1.0, w_geo=1.0, compute_metric=False,
                     w_lovasz=0.0, w_ohem=0.0, ohem_topk=0.25, w_fp=0.0, frustums=None, w_dice=0.0, w_lga=0.0):
    """Same losses / metric as ``occ_losses`` from the sums of the fused HIP epilogue (one pass over the coarse
    logits; the up-sampled logits, probabilities and one-hot volumes are never materialised)."""
    from .. import functional as F
    from ..functional import occ_loss_sums
    nc = logits.shape[1]
    label = gt_occ.to(torch.uint8)                      # classes 0..19, 255 = ignore
    diff, aux = occ_loss_sums(logits, label, class_weights)
    if F.OCC_TAIL:                                      # the algebra below in one launch (+ its Jacobian for backward)
        ce, sem, geo, iou, miou = F.occ_loss_tail(diff, aux, w_ce, w_sem, w_geo)
        out = {}
        if w_ce > 0:
            out[f"loss_voxel_ce_{tag}"] = ce
        if w_sem > 0:
            out[f"loss_voxel_sem_scal_{tag}"] = sem
        if w_geo > 0:
            out[f"loss_voxel_geo_scal_{tag}"] = geo
        if w_ohem > 0:
            out[f"loss_voxel_sem_ohem_{tag}"] = ohem_ce_loss(logits, gt_occ, class_weights, ohem_topk) * w_ohem
        if w_lovasz > 0:
            out[f"loss_voxel_lovasz_{tag}"] = lovasz_softmax_loss(logits, gt_occ) * w_lovasz
        if w_fp > 0:
            out[f"loss_voxel_fp_{tag}"] = _frustum_term(logits, gt_occ, frustums) * w_fp
        if w_dice > 0:
            out[f"loss_voxel_dice_{tag}"] = F.occ_dice_tail(diff, aux) * w_dice
        if w_lga > 0:
            out[f"loss_voxel_lga_{tag}"] = occ_lga_loss(logits, gt_occ, class_weights) * w_lga
        if compute_metric:
            out[f"sc_iou_{tag}"], out[f"ssc_miou_{tag}"] = iou.detach(), miou.detach()
        return out
    ce_num, sum_p, nom = diff[0], diff[1:1 + nc], diff[1 + nc:1 + 2 * nc]
    ce_den, M, cnt, conf = aux[0], aux[1], aux[2:2 + nc], aux[2 + nc:].view(nc, nc)
    out = {}
    if w_ce > 0:
        out[f"loss_voxel_ce_{tag}"] = (ce_num / ce_den).float() * w_ce
    if w_sem > 0:
        present = cnt > 0
        neg = M - cnt
        spec_num = neg - (sum_p - nom)
        one = torch.ones_like(sum_p)
        loss_c = torch.where(sum_p > 0, _nll1(nom / torch.where(sum_p > 0, sum_p, one)), torch.zeros_like(sum_p))
        loss_c = loss_c + _nll1(nom / cnt.clamp_min(1.0))
        loss_c = loss_c + torch.where(neg > 0, _nll1(spec_num / neg.clamp_min(1.0)), torch.zeros_like(sum_p))
        out[f"loss_voxel_sem_scal_{tag}"] = ((loss_c * present).sum() / present.sum()).float() * w_sem
    if w_geo > 0:
        occ_t = M - cnt[0]
        inter = occ_t - (sum_p[0] - nom[0])
        geo = _nll1(inter / (M - sum_p[0])) + _nll1(inter / occ_t) + _nll1(nom[0] / cnt[0])
        out[f"loss_voxel_geo_scal_{tag}"] = geo.float() * w_geo
    if w_ohem > 0:
        out[f"loss_voxel_sem_ohem_{tag}"] = ohem_ce_loss(logits, gt_occ, class_weights, ohem_topk) * w_ohem
    if w_lovasz > 0:
        out[f"loss_voxel_lovasz_{tag}"] = lovasz_softmax_loss(logits, gt_occ) * w_lovasz
    if w_fp > 0:
        out[f"loss_voxel_fp_{tag}"] = _frustum_term(logits, gt_occ, frustums) * w_fp
    if w_dice > 0:
        out[f"loss_voxel_dice_{tag}"] = dice_from_sums(diff, aux).float() * w_dice
    if w_lga > 0:
        out[f"loss_voxel_lga_{tag}"] = occ_lga_loss(logits, gt_occ, class_weights) * w_lga
    if compute_metric:
        with torch.no_grad():
            tp = conf[1:, 1:].sum()
            fp = conf[0, 1:].sum()
            fn = conf[1:, 0].sum()
            tpc = conf.diagonal()
            fpc = conf.sum(0) - tpc
            fnc = conf.sum(1) - tpc
            out[f"sc_iou_{tag}"] = (tp / (tp + fp + fn)).float()
            out[f"ssc_miou_{tag}"] = (tpc / (tpc + fpc + fnc + 1e-5))[1:].mean().float()
    return out


def occ_losses(logits, gt_occ, class_weights, tag="0", w_ce=1.0, w_sem=1.0, w_geo=1.0, compute_metric=False, w_lovasz=0.0,
               w_ohem=0.0, ohem_topk=0.25, w_fp=0.0, frustums=None, w_dice=0.0, w_lga=0.0):
    """occhead.py:291-361: trilinear upsample to the label grid, CE + sem_scal + geo_scal (+ OHEM CE, + Lovasz-softmax, + the
    frustum-proportion loss from ``frustums`` = the head's keyword arguments, + soft Dice, + the LGA-weighted CE, + metric)."""
    if (logits.is_cuda and logits.shape[1] == 20 and all(o == 2 * i for o, i in zip(gt_occ.shape[-3:], logits.shape[-3:]))):
        return occ_losses_fused(logits, gt_occ, class_weights, tag, w_ce, w_sem, w_geo, compute_metric, w_lovasz, w_ohem,
                                ohem_topk, w_fp, frustums, w_dice, w_lga)
    if logits.shape[-3:] != gt_occ.shape[-3:]:
        from ..functional import upsample_trilinear
        logits = upsample_trilinear(logits, gt_occ.shape[-3:])
    t = gt_occ.long()
    out = {}
    if w_ce > 0:
        out[f"loss_voxel_ce_{tag}"] = ce_ssc_loss(logits, t, class_weights) * w_ce
    if w_sem > 0 or w_geo > 0:
        sem, geo = scal_losses(logits, t)
        if w_sem > 0:
            out[f"loss_voxel_sem_scal_{tag}"] = sem * w_sem
        if w_geo > 0:
            out[f"loss_voxel_geo_scal_{tag}"] = geo * w_geo
    if w_ohem > 0:
        out[f"loss_voxel_sem_ohem_{tag}"] = ohem_ce_loss(logits, gt_occ, class_weights, ohem_topk) * w_ohem
    if w_lovasz > 0:
        out[f"loss_voxel_lovasz_{tag}"] = lovasz_softmax_loss(logits, gt_occ) * w_lovasz
    if w_fp > 0:
        out[f"loss_voxel_fp_{tag}"] = _frustum_term(logits, gt_occ, frustums) * w_fp
    if w_dice > 0:
        out[f"loss_voxel_dice_{tag}"] = _dice_term(logits, gt_occ) * w_dice
    if w_lga > 0:
        out[f"loss_voxel_lga_{tag}"] = occ_lga_loss(logits, gt_occ, class_weights) * w_lga
    if compute_metric:
        with torch.no_grad():
            tp, fp, fn, tpc, fpc, fnc = ssc_counts(logits.argmax(1), t)
            out[f"sc_iou_{tag}"] = tp / (tp + fp + fn)
            out[f"ssc_miou_{tag}"] = (tpc / (tpc + fpc + fnc + 1e-5))[1:].mean()
    return out


class SSCMetrics(torch.nn.Module):
    """Accumulating SC-IoU / SSC-mIoU metric with the reference's interface
    (utils/ssc_metric.py:14-103): ``compute_single`` -> 6-tuple of numpy counts, ``update``,
    ``compute``.  State lives in non-persistent buffers (torchmetrics' default), reduced over
    ranks by summation."""

    def __init__(self, class_names=None):
        super().__init__()
        self.class_names = class_names or KITTI_CLASS_NAMES
        self.n_classes = len(self.class_names)
        for n in ("tps", "fps", "fns"):
            self.register_buffer(n, torch.zeros(self.n_classes), persistent=False)
        for n in ("completion_tp", "completion_fp", "completion_fn"):
            self.register_buffer(n, torch.zeros(1), persistent=False)

    def compute_single(self, y_pred, y_true):
        c = ssc_counts(y_pred, y_true, self.n_classes, recompute_mask=True)
        return tuple(v.cpu().numpy() for v in c)

    def update(self, y_pred, y_true):
        tp, fp, fn, tpc, fpc, fnc = ssc_counts(y_pred, y_true, self.n_classes, recompute_mask=True)
        self.completion_tp += tp
        self.completion_fp += fp
        self.completion_fn += fn
        self.tps += tpc
        self.fps += fpc
        self.fns += fnc

    def sync(self):
        """Sum the state over ranks (dist_reduce_fx='sum')."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            for b in (self.tps, self.fps, self.fns, self.completion_tp, self.completion_fp, self.completion_fn):
                dist.all_reduce(b)

    def compute(self):
        iou = self.completion_tp / (self.completion_tp + self.completion_fp + self.completion_fn)
        iou_ssc = self.tps / (self.tps + self.fps + self.fns + 1e-5)
        return {"precision": self.completion_tp / (self.completion_tp + self.completion_fp),
                "recall": self.completion_tp / (self.completion_tp + self.completion_fn),
                "iou": iou.item(), "iou_ssc": iou_ssc, "iou_ssc_mean": iou_ssc[1:].mean().item()}
