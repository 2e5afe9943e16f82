"""The RPN head's training side on the gfx950 kernels (csrc/rpn_stage.hip): targets for a whole batch without stored anchors and
without a host synchronisation, and the loss at the sampled anchors only.

Mirror of instance_segmentation/mmdet/models/dense_heads/anchor_head.py:142-170 (``get_anchors``), :172-371
(``_get_targets_single`` / ``get_targets``) and :373-491 (``loss_single`` / ``loss``) with rpn_head.py's ``loss``.

  * ``rpn_stage_targets``: ``iif_rpn_stage_targets``.  ``MaxIoUAssigner.assign`` on the anchors that are valid for each image,
    ``RandomSampler.sample`` and the encode of the sampled positives for all B images.  The kernels generate every anchor from its
    flat index (``mmdet_anchor.AnchorGenerator``'s formula); no anchor tensor is read.  A candidate takes part only if it is
    valid for image ``b`` - ``valid_flags`` on ``pad_shapes[b]`` and, for ``allowed_border >= 0``, ``anchor_inside_flags`` on
    ``img_shapes[b]``; every other candidate is in no gt's arg-max, is no negative and is not sampled: the semantics of the
    reference's compaction (compaction is monotone, so "lowest index wins" is the same rule in both index spaces).  SIX enqueued
    operations whatever B, the number of levels, G and the data: the key draw (none when ``keys`` are given), the clear of the
    workspace's head, two assignment passes, the selection (with the encode), the total.  The rows are bit for bit those of the
    per-image chain (``anchor_inside_flags``, ``assign(anchors[inside])``, ``sample_padded(keys=keys[b][inside])``, ``encode``).
  * ``rpn_stage_dense``: the four per-level lists ``get_targets`` returns after ``images_to_levels``, one launch, for callers
    with another loss.
  * ``rpn_loss``: one autograd function.  Forward ONE launch (one workgroup per level, fixed summation order), reading the
    NCHW or ``channels_last`` maps in place at ``(level, y, x, a)``; backward one clear of one arena that holds every level's
    gradient in the input's memory format and ONE launch of plain stores.  ``num_total_samples`` never leaves the device.
  * ``rpn_head_loss``: layers 1 to 3 strung together with ``RPNHead.loss``'s arguments.

Limits of the batch call (beyond them a ``ValueError`` that names the per-image chain): 1 .. 16 images, at most 8 levels and 16
base anchors per level, fewer than 2^31 anchors, ``sampler.num <= 1024``; any number of ground-truth boxes.

Deliberately not offered: ``reg_decoded_bbox``; samplers other than ``RandomSampler`` (``add_gt_as_proposals`` must be False);
labels from ``gt_labels`` (the non-RPN anchor heads); ignore boxes with ``assigner.ignore_iof_thr > 0`` (``NotImplementedError``;
with a threshold <= 0 they have no effect, the reference's own rule); and the reference's ``None`` result for a batch that holds
an image without a valid anchor: such an image simply has counts ``(0, 0)`` and adds 2 to ``num_total_samples``.
"""
import collections
import ctypes

import torch

from . import _lib
from .mmdet_targets import _coder_norm

__all__ = ["RPNStageTargets", "rpn_stage_targets", "rpn_stage_dense", "rpn_loss", "rpn_head_loss", "MAX_IMAGES", "MAX_NUM"]

MAX_IMAGES, MAX_NUM = 16, 1024

# ``pos_inds [B, nep]`` / ``neg_inds [B, num]`` int64: flat indices over the concatenated levels, ascending, tails -1;
# ``counts [B, 2]`` int64; ``pos_assigned_gt_inds [B, nep]`` int64 (tail -1); ``pos_bbox_targets [B, nep, 4]`` float32 (tail 0);
# ``num_total_samples``: float32 scalar on the device; ``num_level_anchors`` / ``featmap_sizes``: host integers; ``grid``: the
# launch's description of the anchor grid; ``pos_weight``: the call's, for ``rpn_stage_dense``.
RPNStageTargets = collections.namedtuple("RPNStageTargets", [
    "pos_inds", "neg_inds", "counts", "pos_assigned_gt_inds", "pos_bbox_targets", "num_total_samples", "num_level_anchors",
    "featmap_sizes", "grid", "pos_weight"])


def _chain_hint(what):
    return ValueError("%s; the batch call takes 1 .. %d images, <= 8 levels, <= 16 base anchors per level, fewer than 2^31 "
                      "anchors and sampler.num <= %d - other shapes go through the per-image chain (AnchorGenerator, "
                      "anchor_inside_flags, anchor_targets_single)" % (what, MAX_IMAGES, MAX_NUM))


def rpn_stage_targets(featmap_sizes, anchor_generator, pad_shapes, img_shapes, gt_bboxes_list, assigner, sampler, coder,
                      allowed_border=-1, pos_weight=-1, keys=None, gt_bboxes_ignore_list=None):
    """Assign, sample and encode for all images at once: an ``RPNStageTargets``.  ``featmap_sizes`` one ``(H, W)`` per level;
    ``pad_shapes`` / ``img_shapes`` one ``(H, W[, C])`` per image; ``gt_bboxes_list[b]`` float32 ``[G_b, 4]`` on the device;
    ``keys`` int32 ``[B, A]``, one per flat anchor (None draws them in one ``torch.randint`` call).  ``pos_weight`` is kept
    for ``rpn_stage_dense``'s label weights (``rpn_loss`` takes its own).  Nothing synchronises the host."""
    B = len(gt_bboxes_list)
    if not 1 <= B <= MAX_IMAGES:
        raise _chain_hint("%d images" % B)
    if len(pad_shapes) != B or len(img_shapes) != B:
        raise ValueError("rpn_stage_targets: %d images, %d pad_shapes, %d img_shapes" % (B, len(pad_shapes), len(img_shapes)))
    if type(sampler).__name__ != "RandomSampler":
        raise NotImplementedError("rpn_stage_targets: RandomSampler only (got %s)" % type(sampler).__name__)
    if sampler.add_gt_as_proposals:
        raise ValueError("rpn_stage_targets: the sampler must have add_gt_as_proposals=False")
    if gt_bboxes_ignore_list is not None and float(assigner.ignore_iof_thr) > 0 and any(
            g is not None and g.numel() for g in gt_bboxes_ignore_list):
        raise NotImplementedError("rpn_stage_targets: ignore boxes with ignore_iof_thr > 0 are not offered")
    num = int(sampler.num)
    nep = int(sampler.num * sampler.pos_fraction)
    if num > MAX_NUM:
        raise _chain_hint("sampler.num = %d" % num)
    if not 0 <= nep <= num:
        raise ValueError("rpn_stage_targets: 0 <= num_expected_pos <= num expected (got %d, %d)" % (nep, num))
    try:
        grid, level_counts = anchor_generator._grid(featmap_sizes, "rpn_stage_targets")
    except ValueError as e:
        raise _chain_hint(str(e))
    A = sum(level_counts)
    if A == 0:
        raise ValueError("rpn_stage_targets: no anchors")
    L = len(level_counts)
    for g in gt_bboxes_list:
        if g.dim() != 2 or (g.size(0) and g.size(1) != 4) or g.dtype != torch.float32:
            raise ValueError("rpn_stage_targets: float32 [G, 4] ground-truth boxes expected (got %s %s)" % (g.dtype, tuple(g.shape)))
    if keys is not None and (keys.dtype != torch.int32 or tuple(keys.shape) != (B, A)):
        raise ValueError("rpn_stage_targets: keys int32 [%d, %d] expected - one per flat anchor (got %s %s)"
                         % (B, A, keys.dtype, tuple(keys.shape)))
    _lib.require_gpu(keys, *gt_bboxes_list)
    dev = gt_bboxes_list[0].device
    valid = (ctypes.c_int32 * (2 * B * L))()
    for b in range(B):
        for l, (vw, vh) in enumerate(anchor_generator._valid_sizes(featmap_sizes, pad_shapes[b])):
            valid[(b * L + l) * 2], valid[(b * L + l) * 2 + 1] = max(vw, 0), max(vh, 0)
    use_border = allowed_border >= 0
    hi = (ctypes.c_float * (2 * B))()
    if use_border:
        for b in range(B):
            img_h, img_w = img_shapes[b][:2]
            hi[2 * b], hi[2 * b + 1] = float(img_w + allowed_border), float(img_h + allowed_border)
    images, held = _lib.roi_images(gt_bboxes_list)
    Gs = [int(g.shape[0]) for g in gt_bboxes_list]
    if keys is None:
        keys = torch.randint(0, 2 ** 31, (B, A), dtype=torch.int32, device=dev)
    else:
        keys = keys.contiguous()
    neg_lo, neg_hi = assigner._neg_range()
    means, stds = _coder_norm(coder)
    i64, f32 = torch.int64, torch.float32
    pos_inds = torch.empty((B, nep), dtype=i64, device=dev)
    neg_inds = torch.empty((B, num), dtype=i64, device=dev)
    counts = torch.empty((B, 2), dtype=i64, device=dev)
    pos_gt = torch.empty((B, nep), dtype=i64, device=dev)
    pos_bt = torch.empty((B, nep, 4), dtype=f32, device=dev)
    nts = torch.empty((), dtype=f32, device=dev)
    L_ = _lib.lib()
    ws_bytes = int(L_.iif_rpn_stage_workspace_bytes(B, A, sum(Gs)))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)                          # this call's own
    with torch.cuda.device(dev):
        rc = L_.iif_rpn_stage_targets(
            ctypes.byref(grid), images, B, valid, int(use_border), float(-allowed_border), hi, _lib.ptr(keys),
            float(assigner.pos_iou_thr), neg_lo, neg_hi, float(assigner.min_pos_iou), int(bool(assigner.gt_max_assign_all)),
            int(bool(assigner.match_low_quality)), nep, num, float(sampler.neg_pos_ub), means, stds, _lib.ptr(pos_inds),
            _lib.ptr(neg_inds), _lib.ptr(counts), _lib.ptr(pos_gt), _lib.ptr(pos_bt), _lib.ptr(nts), _lib.ptr(ws), ws_bytes,
            _lib.stream_ptr())
    _lib.check(rc, "iif_rpn_stage_targets")
    del held
    return RPNStageTargets(pos_inds, neg_inds, counts, pos_gt, pos_bt, nts, list(level_counts),
                           [(int(s[0]), int(s[1])) for s in featmap_sizes], grid, float(pos_weight))


def rpn_stage_dense(targets, num_classes=1):
    """``(labels_list, label_weights_list, bbox_targets_list, bbox_weights_list)``: per-level ``[B, A_l(, 4)]`` tensors with the
    values ``AnchorHead.get_targets`` returns after ``images_to_levels``.  One launch, every element written once, nothing
    cleared first; the lists are views of four buffers."""
    t = targets
    B, nep = t.pos_inds.shape
    num = t.neg_inds.size(1)
    A = sum(t.num_level_anchors)
    dev = t.pos_inds.device
    labels = torch.empty((B * A,), dtype=torch.int64, device=dev)
    lw = torch.empty((B * A,), dtype=torch.float32, device=dev)
    bt = torch.empty((B * A, 4), dtype=torch.float32, device=dev)
    bw = torch.empty((B * A, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().iif_rpn_stage_dense(ctypes.byref(t.grid), B, _lib.ptr(t.pos_inds), _lib.ptr(t.neg_inds), _lib.ptr(t.counts),
                                            _lib.ptr(t.pos_bbox_targets), nep, num, int(num_classes), float(t.pos_weight),
                                            _lib.ptr(labels), _lib.ptr(lw), _lib.ptr(bt), _lib.ptr(bw), _lib.stream_ptr())
    _lib.check(rc, "iif_rpn_stage_dense")
    sizes = [B * n for n in t.num_level_anchors]
    out = []
    for buf in (labels, lw, bt, bw):
        out.append([p.view((B, n) + tuple(buf.shape[1:])) for p, n in zip(torch.split(buf, sizes, 0), t.num_level_anchors)])
    return tuple(out)


def _loss_params(loss_cls, loss_bbox):
    hint = "; use rpn_stage_dense with the dense losses (binary_cross_entropy / l1_loss / smooth_l1_loss) instead"
    if type(loss_cls).__name__ != "CrossEntropyLoss" or not getattr(loss_cls, "use_sigmoid", False) or getattr(loss_cls, "use_mask", False) \
            or loss_cls.reduction != "mean" or loss_cls.class_weight is not None:
        raise NotImplementedError("rpn_loss: loss_cls must be CrossEntropyLoss(use_sigmoid=True, reduction='mean', "
                                  "class_weight=None)" + hint)
    name = type(loss_bbox).__name__
    if name not in ("L1Loss", "SmoothL1Loss") or loss_bbox.reduction != "mean":
        raise NotImplementedError("rpn_loss: loss_bbox must be L1Loss or SmoothL1Loss with reduction='mean'" + hint)
    beta = 0.0
    if name == "SmoothL1Loss":
        beta = float(loss_bbox.beta)
        assert beta > 0
    return float(loss_cls.loss_weight), float(loss_bbox.loss_weight), beta


def _strides4(t):
    return (ctypes.c_int64 * 4)(*[int(s) for s in t.stride()])


def _levels(scores, deltas, g_scores=None, g_deltas=None):
    lv = (_lib.RpnLossLevel * len(scores))()
    for l, (s, d) in enumerate(zip(scores, deltas)):
        lv[l].scores, lv[l].deltas = _lib.ptr(s), _lib.ptr(d)
        lv[l].score_strides, lv[l].delta_strides = _strides4(s), _strides4(d)
        if g_scores is not None:
            lv[l].grad_scores, lv[l].grad_deltas = _lib.ptr(g_scores[l]), _lib.ptr(g_deltas[l])
            lv[l].grad_score_strides, lv[l].grad_delta_strides = _strides4(g_scores[l]), _strides4(g_deltas[l])
    return lv


class _RPNLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, targets, params, n_levels, *maps):
        scores, deltas = maps[:n_levels], maps[n_levels:]
        t = targets
        B, nep = t.pos_inds.shape
        num = t.neg_inds.size(1)
        dev = scores[0].device
        out = [torch.empty((n_levels,), dtype=torch.float32, device=dev) for _ in range(2)]
        pos_weight, w_cls, w_box, beta = params
        with torch.cuda.device(dev):
            rc = _lib.lib().iif_rpn_loss_fwd(ctypes.byref(t.grid), _levels(scores, deltas), B, _lib.ptr(t.pos_inds), _lib.ptr(t.neg_inds),
                                             _lib.ptr(t.counts), _lib.ptr(t.pos_bbox_targets), nep, num, _lib.ptr(t.num_total_samples),
                                             pos_weight, w_cls, w_box, beta, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.stream_ptr())
        _lib.check(rc, "iif_rpn_loss_fwd")
        ctx.targets, ctx.params, ctx.n_levels = t, params, n_levels
        ctx.save_for_backward(*maps)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cls, g_box):
        maps = ctx.saved_tensors
        L = ctx.n_levels
        scores, deltas = maps[:L], maps[L:]
        t = ctx.targets
        B, nep = t.pos_inds.shape
        num = t.neg_inds.size(1)
        dev = scores[0].device
        arena = torch.zeros((sum(m.numel() for m in maps),), dtype=torch.float32, device=dev)     # the one clear
        grads, at = [], 0
        for m in maps:
            n = m.numel()
            piece = arena[at:at + n]
            at += n
            Bm, C, H, W = m.shape
            if m.is_contiguous(memory_format=torch.channels_last) and not m.is_contiguous():
                grads.append(piece.view(Bm, H, W, C).permute(0, 3, 1, 2))
            else:
                grads.append(piece.view(Bm, C, H, W))
        g_cls = g_cls.to(torch.float32).contiguous()
        g_box = g_box.to(torch.float32).contiguous()
        pos_weight, w_cls, w_box, beta = ctx.params
        with torch.cuda.device(dev):
            rc = _lib.lib().iif_rpn_loss_bwd(ctypes.byref(t.grid), _levels(scores, deltas, grads[:L], grads[L:]), B, _lib.ptr(t.pos_inds),
                                             _lib.ptr(t.neg_inds), _lib.ptr(t.counts), _lib.ptr(t.pos_bbox_targets), nep, num,
                                             _lib.ptr(t.num_total_samples), pos_weight, w_cls, w_box, beta, _lib.ptr(g_cls),
                                             _lib.ptr(g_box), _lib.stream_ptr())
        _lib.check(rc, "iif_rpn_loss_bwd")
        return (None, None, None) + tuple(grads)


def rpn_loss(cls_scores, bbox_preds, targets, loss_cls, loss_bbox, pos_weight=-1):
    """``dict(loss_rpn_cls=[L tensors], loss_rpn_bbox=[L tensors])`` from the sampled anchors alone.  ``cls_scores[l]``
    ``[B, A_l / (H_l W_l), H_l, W_l]`` and ``bbox_preds[l]`` ``[B, 4 A_l / (H_l W_l), H_l, W_l]``, float32, NCHW or
    ``channels_last``, read in place.  Accepted losses: ``CrossEntropyLoss(use_sigmoid=True, reduction='mean',
    class_weight=None)`` and ``L1Loss`` / ``SmoothL1Loss`` with ``reduction='mean'``; anything else raises
    ``NotImplementedError``.  Nothing synchronises the host."""
    w_cls, w_box, beta = _loss_params(loss_cls, loss_bbox)
    t = targets
    L = len(t.featmap_sizes)
    if len(cls_scores) != L or len(bbox_preds) != L:
        raise ValueError("rpn_loss: %d levels in the targets, %d score maps, %d delta maps" % (L, len(cls_scores), len(bbox_preds)))
    B = t.pos_inds.size(0)
    for l, (s, d) in enumerate(zip(cls_scores, bbox_preds)):
        H, W = t.featmap_sizes[l]
        nb = int(t.grid.num_base[l])
        if tuple(s.shape) != (B, nb, H, W) or tuple(d.shape) != (B, 4 * nb, H, W):
            raise ValueError("rpn_loss: level %d: score map [%d, %d, %d, %d] and delta map [%d, %d, %d, %d] expected (got %s, %s)"
                             % (l, B, nb, H, W, B, 4 * nb, H, W, tuple(s.shape), tuple(d.shape)))
        if s.dtype != torch.float32 or d.dtype != torch.float32:
            raise NotImplementedError("rpn_loss: float32 maps only (got %s, %s)" % (s.dtype, d.dtype))
    _lib.require_gpu(*cls_scores, *bbox_preds)
    cls, box = _RPNLoss.apply(t, (float(pos_weight), w_cls, w_box, beta), L, *cls_scores, *bbox_preds)
    return dict(loss_rpn_cls=list(cls.unbind(0)), loss_rpn_bbox=list(box.unbind(0)))


def rpn_head_loss(anchor_generator, assigner, sampler, coder, loss_cls, loss_bbox, cls_scores, bbox_preds, gt_bboxes, img_metas,
                  gt_bboxes_ignore=None, allowed_border=-1, pos_weight=-1, keys=None):
    """``RPNHead.loss`` (rpn_head.py with anchor_head.py:423-491) on layers 1 to 3: the head's ``anchor_generator``, ``assigner``,
    ``sampler``, ``bbox_coder``, ``loss_cls`` and ``loss_bbox``, then ``loss``'s own arguments; ``allowed_border`` and
    ``pos_weight`` are ``train_cfg``'s.  Returns ``dict(loss_rpn_cls=..., loss_rpn_bbox=...)``."""
    featmap_sizes = [tuple(int(v) for v in m.shape[-2:]) for m in cls_scores]
    assert len(featmap_sizes) == anchor_generator.num_levels
    t = rpn_stage_targets(featmap_sizes, anchor_generator, [m["pad_shape"] for m in img_metas], [m["img_shape"] for m in img_metas],
                          gt_bboxes, assigner, sampler, coder, allowed_border=allowed_border, pos_weight=pos_weight, keys=keys,
                          gt_bboxes_ignore_list=gt_bboxes_ignore)
    return rpn_loss(cls_scores, bbox_preds, t, loss_cls, loss_bbox, pos_weight=pos_weight)
