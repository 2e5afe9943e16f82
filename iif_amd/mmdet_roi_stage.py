"""The RoI head's training front end on the gfx950 kernels (csrc/roi_stage.hip): targets for a whole batch in one launch from
PADDED proposals, and the cascade's ``refine_bboxes`` with a padded result.

Mirror of instance_segmentation/mmdet/models/roi_heads/standard_roi_head.py:85-100 (assign and sample per image) with
bbox_heads/bbox_head.py:188-261 (``get_targets``), and of bbox_head.py:380-496 (``refine_bboxes`` / ``regress_by_class``).

  * ``roi_stage_targets_padded``: ``iif_roi_stage_targets``.  ``MaxIoUAssigner.assign``, ``add_gt_``, ``RandomSampler.sample``
    and ``bbox_targets`` for every image of the batch in ONE launch; the number of valid proposals of each image is read on the
    device, so ``rpn_proposals_padded``' ``(dets, counts)`` - or ``refine_bboxes_padded``' - go in as they are and nothing
    synchronises the host.  Its rows are bit for bit those of the per-image chain (``assign`` on ``proposals[b, :n_b]``,
    ``sample_padded``, ``bbox_targets``) fed the same keys.
  * ``refine_bboxes_padded``: ``iif_refine_bboxes``, one launch, ``(proposals [B, num, 4], counts [B])`` on the device.
  * ``refine_bboxes``: the reference's signature and list result, at the cost of ONE host read (the counts).

Limits of the single launch: 1 .. 16 images, at most 4096 proposals and 1024 ground-truth boxes per image, ``sampler.num`` at
most 1024.  Larger shapes go through the per-image chain (mmdet_assigner / mmdet_targets), which has no such limits.

Deliberately not offered: ``gt_bboxes_ignore`` at the RoI stage, samplers other than ``RandomSampler``, OHEM, and the
``argmax`` that resolves background labels between cascade stages (cascade_roi_head.py:279-281: torch operations of the caller's,
which do not synchronise).
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from .mmdet_targets import _coder_norm

__all__ = ["RoIStageTargets", "roi_stage_targets_padded", "refine_bboxes_padded", "refine_bboxes", "MAX_IMAGES", "MAX_PROPOSALS",
           "MAX_GTS", "MAX_NUM"]

MAX_IMAGES, MAX_PROPOSALS, MAX_GTS, MAX_NUM = 16, 4096, 1024, 1024

# The first six fields are ``bbox_targets``' padded tuple, in its order.  ``counts [B, 2]`` int64: positives and negatives kept
# per image; ``pos_is_gt [B num]`` uint8; ``pos_rois [B num_expected_pos, 5]``, ``pos_gt_inds``, ``pos_labels``: the positives
# alone (for the mask branch), unused rows with image index -1, gt index -1, label ``num_classes``.
RoIStageTargets = collections.namedtuple("RoIStageTargets", [
    "labels", "label_weights", "bbox_targets", "bbox_weights", "rois", "pos_assigned_gt_inds", "counts", "pos_is_gt", "pos_rois",
    "pos_gt_inds", "pos_labels"])


def _chain_hint(what):
    return ValueError("%s; the single launch takes 1 .. %d images, <= %d proposals and <= %d ground-truth boxes per image and "
                      "num <= %d - larger shapes go through the per-image chain (MaxIoUAssigner.assign, "
                      "RandomSampler.sample_padded, bbox_targets)" % (what, MAX_IMAGES, MAX_PROPOSALS, MAX_GTS, MAX_NUM))


def _pack(proposals):
    """A list of ``[n, 4|5]`` tensors as ``([B, P, w], counts [B])``; the counts come from the shapes (no read)."""
    B = len(proposals)
    for p in proposals:
        if p.dim() != 2 or (p.size(0) and p.size(1) not in (4, 5)):
            raise ValueError("proposals: a list of [n, 4] or [n, 5] tensors expected (got %s)" % (tuple(p.shape),))
    width = max([p.size(1) for p in proposals if p.size(0)] + [4])
    if any(p.size(0) and p.size(1) != width for p in proposals):
        raise ValueError("proposals: the tensors of a list must have the same number of columns")
    ns = [int(p.size(0)) for p in proposals]
    P = max(ns + [0])
    if P > MAX_PROPOSALS:
        raise _chain_hint("%d proposals in one image" % P)
    _lib.require_gpu(*proposals)
    dev = proposals[0].device
    packed = torch.zeros((B, P, width), dtype=torch.float32, device=dev)
    for b, p in enumerate(proposals):
        if ns[b]:
            packed[b, :ns[b]] = p
    counts = torch.tensor(ns, dtype=torch.int64).to(dev, non_blocking=True)
    return packed, counts


def roi_stage_targets_padded(proposals, proposal_counts, gt_bboxes_list, gt_labels_list, assigner, sampler, coder, num_classes,
                             pos_weight=-1, reg_decoded_bbox=False, keys=None, gt_bboxes_ignore=None):
    """Assign, add the ground truth, sample and build the bbox targets of all images in one launch: a ``RoIStageTargets``.

    ``proposals`` ``[B, P, 4|5]`` float32 with ``proposal_counts [B]`` int64 on the device (None: all ``P`` rows are valid) -
    rows at or beyond an image's count are never read -, or a list of ``[n, 4|5]`` tensors (packed from their shapes;
    ``proposal_counts`` must be None).  ``gt_bboxes_list[b]`` ``[G_b, 4]`` float32, ``gt_labels_list[b]`` ``[G_b]`` int64.
    ``assigner`` a ``MaxIoUAssigner`` (its thresholds; ``ignore_iof_thr`` has no effect without ignore boxes), ``sampler`` a
    ``RandomSampler`` (``num``, ``pos_fraction``, ``neg_pos_ub``, ``add_gt_as_proposals``), ``coder`` a ``DeltaXYWHBBoxCoder``.
    ``keys`` int32 ``[B, Gmax + P]`` (``Gmax`` the largest ``G_b`` under ``add_gt_as_proposals``, else 0): the key of candidate
    ``c`` of image ``b`` - ground truth first, as in ``sample_padded`` - is ``keys[b, c]``; None draws them in one call from
    the device generator.  Image ``b`` fills rows ``[b num, (b + 1) num)``: positives, negatives, padding.  Nothing
    synchronises the host."""
    if gt_bboxes_ignore is not None:
        raise NotImplementedError("roi_stage_targets_padded: gt_bboxes_ignore is not offered at the RoI stage")
    if isinstance(proposals, (list, tuple)):
        if proposal_counts is not None:
            raise ValueError("roi_stage_targets_padded: a list of proposals carries its own counts; pass proposal_counts=None")
        if len(proposals) != len(gt_bboxes_list):
            raise ValueError("roi_stage_targets_padded: %d proposal tensors for %d images" % (len(proposals), len(gt_bboxes_list)))
        if not 1 <= len(proposals) <= MAX_IMAGES:
            raise _chain_hint("%d images" % len(proposals))
        proposals, proposal_counts = _pack(list(proposals))
    if proposals.dim() != 3 or proposals.size(2) not in (4, 5):
        raise ValueError("roi_stage_targets_padded: proposals [B, P, 4] or [B, P, 5] expected (got %s)" % (tuple(proposals.shape),))
    if proposals.dtype != torch.float32:
        raise NotImplementedError("roi_stage_targets_padded: float32 proposals only (got %s)" % proposals.dtype)
    B, P = int(proposals.size(0)), int(proposals.size(1))
    if len(gt_bboxes_list) != B or len(gt_labels_list) != B:
        raise ValueError("roi_stage_targets_padded: %d images, %d gt box tensors, %d gt label tensors"
                         % (B, len(gt_bboxes_list), len(gt_labels_list)))
    num = int(sampler.num)
    nep = int(sampler.num * sampler.pos_fraction)
    Gs = [int(g.shape[0]) for g in gt_bboxes_list]
    if not 1 <= B <= MAX_IMAGES:
        raise _chain_hint("%d images" % B)
    if P > MAX_PROPOSALS:
        raise _chain_hint("%d proposals per image" % P)
    if max(Gs) > MAX_GTS:
        raise _chain_hint("%d ground-truth boxes in one image" % max(Gs))
    if num > MAX_NUM:
        raise _chain_hint("sampler.num = %d" % num)
    if not 0 <= nep <= num:
        raise ValueError("roi_stage_targets_padded: 0 <= num_expected_pos <= num expected (got %d, %d)" % (nep, num))
    for g, l in zip(gt_bboxes_list, gt_labels_list):
        if g.dim() != 2 or (g.size(0) and g.size(1) != 4) or g.dtype != torch.float32:
            raise ValueError("roi_stage_targets_padded: float32 [G, 4] ground-truth boxes expected (got %s %s)" % (g.dtype, tuple(g.shape)))
        if l is None or l.numel() != g.size(0):
            raise ValueError("roi_stage_targets_padded: one label per ground-truth box expected")
    add_gt = bool(sampler.add_gt_as_proposals)
    gmax = max(Gs) if add_gt else 0
    if proposal_counts is not None and (proposal_counts.dtype != torch.int64 or proposal_counts.numel() != B):
        raise ValueError("roi_stage_targets_padded: proposal_counts int64 [B] expected (got %s %s)"
                         % (proposal_counts.dtype, tuple(proposal_counts.shape)))
    if keys is not None and (keys.dtype != torch.int32 or tuple(keys.shape) != (B, gmax + P)):
        raise ValueError("roi_stage_targets_padded: keys int32 [%d, %d] expected - one per candidate, ground truth first (got %s %s)"
                         % (B, gmax + P, keys.dtype, tuple(keys.shape)))
    _lib.require_gpu(proposals, proposal_counts, keys, *gt_bboxes_list, *gt_labels_list)
    dev = proposals.device
    proposals = proposals.detach()
    if P and (proposals.stride(2) != 1 or proposals.stride(1) < 4 or (B > 1 and proposals.stride(0) < 4)):
        proposals = proposals.contiguous()
    ld_row = proposals.stride(1) if P > 1 else proposals.size(2)
    ld_img = proposals.stride(0) if (B > 1 and P) else P * proposals.size(2)
    if proposal_counts is not None:
        proposal_counts = proposal_counts.reshape(-1).contiguous()
    if keys is None:
        keys = torch.randint(0, 2 ** 31, (B, gmax + P), dtype=torch.int32, device=dev)
    else:
        keys = keys.contiguous()
    images, held = _lib.roi_images(gt_bboxes_list, gt_labels_list)
    neg_lo, neg_hi = assigner._neg_range()
    means, stds = _coder_norm(coder)
    f32, i64 = torch.float32, torch.int64
    rois = torch.empty((B * num, 5), dtype=f32, device=dev)
    labels = torch.empty((B * num,), dtype=i64, device=dev)
    label_weights = torch.empty((B * num,), dtype=f32, device=dev)
    bbox_targets = torch.empty((B * num, 4), dtype=f32, device=dev)
    bbox_weights = torch.empty((B * num, 4), dtype=f32, device=dev)
    pos_gt = torch.empty((B * num,), dtype=i64, device=dev)
    counts = torch.empty((B, 2), dtype=i64, device=dev)
    pos_is_gt = torch.empty((B * num,), dtype=torch.uint8, device=dev)
    pos_rois = torch.empty((B * nep, 5), dtype=f32, device=dev)
    pos_gt_inds = torch.empty((B * nep,), dtype=i64, device=dev)
    pos_labels = torch.empty((B * nep,), dtype=i64, device=dev)
    rc = _lib.lib().iif_roi_stage_targets(
        images, B, _lib.ptr(proposals), ld_row, ld_img, P, _lib.ptr(proposal_counts), _lib.ptr(keys), gmax + P,
        float(assigner.pos_iou_thr), neg_lo, neg_hi, float(assigner.min_pos_iou), int(bool(assigner.gt_max_assign_all)),
        int(bool(assigner.match_low_quality)), int(add_gt), nep, num, float(sampler.neg_pos_ub), int(num_classes), float(pos_weight),
        int(bool(reg_decoded_bbox)), means, stds, _lib.ptr(rois), _lib.ptr(labels), _lib.ptr(label_weights), _lib.ptr(bbox_targets),
        _lib.ptr(bbox_weights), _lib.ptr(pos_gt), _lib.ptr(counts), _lib.ptr(pos_is_gt), _lib.ptr(pos_rois), _lib.ptr(pos_gt_inds),
        _lib.ptr(pos_labels), _lib.stream_ptr())
    _lib.check(rc, "iif_roi_stage_targets")
    del held
    return RoIStageTargets(labels, label_weights, bbox_targets, bbox_weights, rois, pos_gt, counts, pos_is_gt, pos_rois, pos_gt_inds,
                           pos_labels)


def refine_bboxes_padded(rois, labels, bbox_preds, pos_is_gt, counts, img_shapes, coder, reg_class_agnostic=False,
                         wh_ratio_clip=16 / 1000):
    """bbox_head.py:380-496 on the padded rows of one stage, in one launch: ``(proposals [B, num, 4], counts [B])`` on the device,
    which ``roi_stage_targets_padded`` takes as they are.

    ``rois [B num, 5]``, ``labels [B num]`` int64, ``pos_is_gt [B num]`` uint8 and ``counts [B, 2]`` as ``RoIStageTargets``
    holds them; ``bbox_preds [B num, 4 C]`` float32, or ``[B num, 4]`` with ``reg_class_agnostic``; ``img_shapes`` one
    ``(H, W[, C])`` per image.  Of each image the rows below ``counts[b].sum()`` are decoded at their label with the coder's
    means, stds and clamps, clipped to the image under ``clip_border``; the rows that are ground truth are dropped, the rest
    kept in order, zero rows behind them.  LABELS MUST BE IN RANGE ``[0, C)``: the reference raises on a background label, this
    call decodes such a row with zero deltas (cascade heads replace background labels by the ``argmax`` of the scores first).
    Nothing synchronises the host."""
    B = len(img_shapes)
    if not 1 <= B <= MAX_IMAGES:
        raise _chain_hint("%d images" % B)
    if isinstance(img_shapes, torch.Tensor) or any(isinstance(x, torch.Tensor) for x in img_shapes):
        raise NotImplementedError("refine_bboxes_padded: a tensor img_shape is not offered; pass (H, W) per image")
    if rois.dim() != 2 or rois.size(1) != 5 or rois.size(0) % B:
        raise ValueError("refine_bboxes_padded: rois [B num, 5] expected (got %s for %d images)" % (tuple(rois.shape), B))
    rows = int(rois.size(0))
    num = rows // B
    if num > MAX_NUM:
        raise _chain_hint("%d rows per image" % num)
    if rois.dtype != torch.float32 or bbox_preds.dtype != torch.float32:
        raise NotImplementedError("refine_bboxes_padded: float32 only (got %s, %s)" % (rois.dtype, bbox_preds.dtype))
    if bbox_preds.dim() != 2 or bbox_preds.size(0) != rows or bbox_preds.size(1) % 4 or bbox_preds.size(1) < 4:
        raise ValueError("refine_bboxes_padded: bbox_preds [%d, 4 C] expected (got %s)" % (rows, tuple(bbox_preds.shape)))
    C = bbox_preds.size(1) // 4
    if reg_class_agnostic and C != 1:
        raise ValueError("refine_bboxes_padded: reg_class_agnostic takes bbox_preds [.., 4] (got %s)" % (tuple(bbox_preds.shape),))
    if labels.numel() != rows or pos_is_gt.numel() != rows or pos_is_gt.dtype != torch.uint8:
        raise ValueError("refine_bboxes_padded: labels [B num] and uint8 pos_is_gt [B num] expected")
    if counts.dtype != torch.int64 or tuple(counts.shape) != (B, 2):
        raise ValueError("refine_bboxes_padded: counts int64 [B, 2] expected (got %s %s)" % (counts.dtype, tuple(counts.shape)))
    _lib.require_gpu(rois, labels, bbox_preds, pos_is_gt, counts)
    dev = rois.device
    rois, bbox_preds = rois.detach().contiguous(), bbox_preds.detach().contiguous()
    labels = labels.reshape(-1).to(torch.int64).contiguous()
    pos_is_gt, counts = pos_is_gt.reshape(-1).contiguous(), counts.contiguous()
    clip = bool(coder.clip_border)
    hw = (ctypes.c_float * (2 * B))(*[float(v) for s in img_shapes for v in (s[0], s[1])])
    means, stds = _coder_norm(coder)
    out = torch.empty((B, num, 4), dtype=torch.float32, device=dev)
    out_counts = torch.empty((B,), dtype=torch.int64, device=dev)
    max_ratio = float(np.abs(np.log(wh_ratio_clip)))
    rc = _lib.lib().iif_refine_bboxes(_lib.ptr(rois), 5, _lib.ptr(labels), _lib.ptr(bbox_preds), 4 * C, C, int(bool(reg_class_agnostic)),
                                      _lib.ptr(pos_is_gt), _lib.ptr(counts), B, num, hw, means, stds, max_ratio,
                                      int(bool(coder.add_ctr_clamp)), float(coder.ctr_clamp), int(clip), _lib.ptr(out),
                                      _lib.ptr(out_counts), _lib.stream_ptr())
    _lib.check(rc, "iif_refine_bboxes")
    return out, out_counts


def refine_bboxes(rois, labels, bbox_preds, pos_is_gts, img_metas, coder, reg_class_agnostic=False):
    """bbox_head.py:380-456 with the reference's arguments (``coder`` and ``reg_class_agnostic`` are the head's attributes there)
    and its result, a list of ``[k_i, 4]`` tensors - for the rows of EXACT sizes that the reference works on: image ``i`` owns
    the consecutive rows whose first column is ``i``, ``pos_is_gts[i]`` covers its leading positives.  ONE host read: the rows
    of each image and how many of them are ground truth, from which the kept counts follow."""
    B = len(img_metas)
    if len(pos_is_gts) != B:
        raise ValueError("refine_bboxes: %d pos_is_gts for %d images" % (len(pos_is_gts), B))
    _lib.require_gpu(rois, labels, bbox_preds, *pos_is_gts)
    dev = rois.device
    gts = torch.stack([p.sum(dtype=torch.int64) for p in pos_is_gts])
    read = torch.cat([torch.bincount(rois[:, 0].long(), minlength=B)[:B], gts]).tolist()          # the one read
    ns, dropped = read[:B], read[B:]
    if sum(ns) != rois.size(0):
        raise ValueError("refine_bboxes: every row must carry an image index below len(img_metas)")
    num = max(ns + [1])
    C4 = bbox_preds.size(1)
    p_rois = rois.new_zeros((B, num, 5))
    p_labels = labels.new_zeros((B, num))
    p_preds = bbox_preds.new_zeros((B, num, C4))
    p_gt = torch.zeros((B, num), dtype=torch.uint8, device=dev)
    at = 0
    for i, n in enumerate(ns):
        p_rois[i, :n], p_labels[i, :n], p_preds[i, :n] = rois[at:at + n], labels[at:at + n], bbox_preds[at:at + n]
        k = len(pos_is_gts[i])
        p_gt[i, :k] = pos_is_gts[i].to(torch.uint8)
        at += n
    counts = torch.tensor([[n, 0] for n in ns], dtype=torch.int64).to(dev)
    shapes = [m["img_shape"] for m in img_metas]
    out, _ = refine_bboxes_padded(p_rois.view(B * num, 5), p_labels.view(-1), p_preds.view(B * num, C4), p_gt.view(-1), counts,
                                  shapes, coder, reg_class_agnostic)
    return [out[i, :ns[i] - dropped[i]] for i in range(B)]
