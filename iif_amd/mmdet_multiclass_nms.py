"""mmdet's ``multiclass_nms`` and the box half of ``BBoxHead.get_bboxes`` on the gfx950 kernels (csrc/multiclass_nms.hip).

Mirror of instance_segmentation/mmdet/core/post_processing/bbox_nms.py:8-95 and models/roi_heads/bbox_heads/bbox_head.py:356-377
with mmcv 1.3.8's ``batched_nms`` (ops/nms.py) inside.  One image has ``n`` rows and ``C`` foreground classes:

 1. ``multi_scores`` is ``[n, C + 1]``, the last column is ignored; ``multi_bboxes`` is ``[n, 4 C]`` or ``[n, 4]``.  The
    candidates are the pairs ``(r, c)`` with flat index ``f = r * C + c``; one takes part iff ``score[r, c] > score_thr``
    (strict, the raw score).
 2. With ``score_factors [n]`` the score used for ranking and output is ``score[r, c] * factor[r]``: one float32 multiply,
    applied after the threshold test.
 3. ``M`` = the number of candidates that take part.  ``M == 0``: the empty result.  ``M < split_thr``
    (``nms_cfg['split_thr']``, default 10000): mmcv's NMS over all pairs of the shifted boxes.  Otherwise one plain NMS per
    class on the same shifted boxes, the results merged by score.
 4. Shifted boxes: ``box + float32(c) * (max + 1)`` in float32, ``max`` over all four coordinates of the boxes that take part
    (for ``[n, 4]`` boxes: of the rows with at least one valid class).
 5. In both regimes the output is ordered by score descending, equal scores to the lower flat index.  The overlap test is the
    one at the top of csrc/nms.hip: single float32 operations in mmcv's order, NaN never suppresses.
 6. ``nms_cfg['max_num']`` is applied first, then the function's own ``max_num``; both only truncate the ranked result.
 7. ``dets [k, 5]``: the unshifted boxes and the ranked score; ``labels [k]`` int64, 0-based; ``inds [k]``: the flat index
    (the reference's ``inds[keep]`` under ``return_inds=True``).

  * ``multiclass_nms_padded``: ``iif_multiclass_nms``, 12 enqueued operations for all images, no host read; the regime is
    decided on the device and reported as ``num_candidates``.
  * ``multiclass_nms``: the reference's signature and shapes for ONE host read (the count).
  * ``bbox_head_get_bboxes``: the native ``delta2bbox`` launch, the division by ``scale_factor``, then the padded entry.

Deliberately not offered: a result without a bound (``max_num <= 0`` and no ``nms_cfg['max_num']``: it has no padded form of
sensible size); ``nms_cfg['type']`` other than ``'nms'``; ``nms_cfg['score_threshold'] > 0``; ``class_agnostic=True``; a
``split_thr`` above ``MAX_BOXES`` while ``n * C`` exceeds it (the all-pairs regime holds ``MAX_BOXES`` candidates); other dtypes
than float32; the ONNX branches; more than 1 024 rows, 4 096 classes, 2^24 candidates, 16 images or 4 096 detections per
image.  Nothing registers itself into mmdet: its modules import ``multiclass_nms`` by name (INTEGRATION.md shows the switch).
"""
import torch

from . import _lib
from .mmdet_nms import MAX_BOXES, _get, _workspace

MAX_ROWS, MAX_CLASSES, MAX_CAP, MAX_IMAGES = 1024, 4096, 4096, 16


def workspace_bytes(B, R, C, cap):
    """``IIF_MULTICLASS_NMS_WORKSPACE_BYTES(B, R, C, cap)`` of include/iif_amd.h."""
    B, R, C, cap = int(B), int(R), int(C), int(cap)
    return 4096 + B * (212992 + 4 * ((C + 3) // 4 * 4) + 16 * R * C + 8 * cap)


def _settings(nms_cfg, max_num, n_candidates):
    """(iou_threshold, offset, split_thr, cap) from ``nms_cfg`` and ``max_num``, or the refusal."""
    if torch.onnx.is_in_onnx_export():
        raise NotImplementedError("multiclass_nms: the ONNX export branches are not offered on the native path")
    cfg = dict(nms_cfg)
    nms_type = cfg.pop("type", "nms")
    if nms_type != "nms":
        raise NotImplementedError("multiclass_nms: nms_cfg['type'] = %r is not offered on the native path (only 'nms')" % (nms_type,))
    if cfg.pop("class_agnostic", False):
        raise NotImplementedError("multiclass_nms: class_agnostic=True is not offered (the segmented kernels work per class)")
    if cfg.pop("score_threshold", 0) > 0:
        raise NotImplementedError("multiclass_nms: nms_cfg['score_threshold'] > 0 is not offered; use score_thr")
    split_thr = int(cfg.pop("split_thr", 10000))
    iou, offset, nms_max = float(cfg.pop("iou_threshold")), int(cfg.pop("offset", 0)), int(cfg.pop("max_num", -1))
    if cfg:
        raise TypeError("multiclass_nms: unexpected keys in nms_cfg: %s" % sorted(cfg))
    assert offset in (0, 1)
    bounds = [m for m in (nms_max, int(max_num)) if m > 0]
    if not bounds:
        raise NotImplementedError("multiclass_nms: max_num <= 0 and no nms_cfg['max_num']: the reference's unbounded result has no "
                                  "padded form of sensible size; give one of them")
    cap = min(bounds)
    if cap > MAX_CAP:
        raise ValueError("multiclass_nms: at most %d detections per image (got %d)" % (MAX_CAP, cap))
    if split_thr > MAX_BOXES and n_candidates > MAX_BOXES:
        raise ValueError("multiclass_nms: split_thr = %d above %d with %d candidates per image: the all-pairs regime holds at most "
                         "%d candidates" % (split_thr, MAX_BOXES, n_candidates, MAX_BOXES))
    return iou, offset, split_thr, cap


def multiclass_nms_padded(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num, score_factors=None, row_counts=None,
                          workspace=None):
    """``multiclass_nms`` without a host read, for one image (2-D inputs) or ``B`` images (``[B, R, ...]``):
    ``(dets [.., cap, 5], labels [.., cap], inds [.., cap], counts [B], num_candidates [B])`` on the device,
    ``cap = min`` of the positive ones of ``nms_cfg['max_num']`` and ``max_num``; the detections in rank order, then zero rows
    / -1.  ``row_counts`` (int64 ``[B]`` on the device): rows at or beyond it take no part.  ``num_candidates`` is ``M``: below
    ``split_thr`` the all-pairs regime ran.  ``workspace`` (optional): the caller's uint8 tensor of ``workspace_bytes(B, R, C, cap)``."""
    if not isinstance(multi_bboxes, torch.Tensor) or not isinstance(multi_scores, torch.Tensor):
        raise NotImplementedError("multiclass_nms: tensors only")
    if multi_bboxes.dtype != torch.float32 or multi_scores.dtype != torch.float32:
        raise NotImplementedError("multiclass_nms: float32 boxes and scores only (got %s, %s)" % (multi_bboxes.dtype, multi_scores.dtype))
    if score_factors is not None and score_factors.dtype != torch.float32:
        raise NotImplementedError("multiclass_nms: float32 score_factors only (got %s)" % score_factors.dtype)
    single = multi_scores.dim() == 2
    if multi_scores.dim() not in (2, 3) or multi_bboxes.dim() != multi_scores.dim():
        raise ValueError("multiclass_nms: [n, C + 1] scores with [n, 4 C] or [n, 4] boxes, or both with a leading image dimension")
    s = multi_scores[None] if single else multi_scores
    bx = multi_bboxes[None] if single else multi_bboxes
    B, R, C = s.size(0), s.size(1), s.size(2) - 1
    assert bx.size(0) == B and bx.size(1) == R
    if C < 1 or C > MAX_CLASSES or R > MAX_ROWS or R * C >= 1 << 24 or not 1 <= B <= MAX_IMAGES:
        raise ValueError("multiclass_nms: 1 .. %d images of at most %d rows and 1 .. %d classes, fewer than 2^24 candidates each "
                         "(got %d x %d x %d)" % (MAX_IMAGES, MAX_ROWS, MAX_CLASSES, B, R, C))
    if bx.size(2) not in (4, 4 * C):
        raise ValueError("multiclass_nms: boxes of %d columns for %d classes (4 or %d expected)" % (bx.size(2), C, 4 * C))
    per_class = bx.size(2) > 4
    iou, offset, split_thr, cap = _settings(nms_cfg, max_num, R * C)
    _lib.require_gpu(s, bx, score_factors, row_counts)
    dev = s.device
    s, bx = s.detach().contiguous(), bx.detach().contiguous()
    f = None
    if score_factors is not None:
        f = score_factors.detach().reshape(B, R).contiguous()
    rc = None
    if row_counts is not None:
        rc = row_counts.reshape(B).to(torch.int64).contiguous()
    dets = torch.empty((B, cap, 5), dtype=torch.float32, device=dev)
    labels = torch.empty((B, cap), dtype=torch.int64, device=dev)
    inds = torch.empty((B, cap), dtype=torch.int64, device=dev)
    counts = torch.empty((B,), dtype=torch.int64, device=dev)
    ncand = torch.empty((B,), dtype=torch.int64, device=dev)
    if R == 0:
        dets.zero_(), labels.fill_(-1), inds.fill_(-1), counts.zero_(), ncand.zero_()
        return (dets[0], labels[0], inds[0], counts, ncand) if single else (dets, labels, inds, counts, ncand)
    ws_bytes = workspace_bytes(B, R, C, cap)
    ws = _workspace(workspace, ws_bytes, dev)
    status = _lib.lib().iif_multiclass_nms(_lib.ptr(bx), bx.size(2), int(per_class), _lib.ptr(s), C + 1, _lib.ptr(f), _lib.ptr(rc),
                                           B, R, C, float(score_thr), iou, offset, split_thr, cap, _lib.ptr(dets), _lib.ptr(labels),
                                           _lib.ptr(inds), _lib.ptr(counts), _lib.ptr(ncand), _lib.ptr(ws), ws_bytes,
                                           _lib.stream_ptr())
    _lib.check(status, "iif_multiclass_nms")
    if single:
        dets, labels, inds = dets[0], labels[0], inds[0]
    return dets, labels, inds, counts, ncand


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None, return_inds=False):
    """bbox_nms.py:8-95: ``(dets [k, 5], labels [k])``, with ``return_inds`` also the flat indices ``[k]``; nothing above
    ``score_thr`` gives ``dets [0, 5]``, ``labels [0]``.  ONE host read: the count."""
    if multi_scores.dim() != 2:
        raise ValueError("multiclass_nms: one image ([n, C + 1] scores); multiclass_nms_padded takes a batch")
    dets, labels, inds, counts, _ = multiclass_nms_padded(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num, score_factors)
    k = int(counts.item())
    return (dets[:k], labels[:k], inds[:k]) if return_inds else (dets[:k], labels[:k])


def bbox_head_get_bboxes(rois, scores, bbox_pred, img_shape, scale_factor, rescale, cfg, bbox_coder, padded=False):
    """bbox_head.py:356-377 on already-activated ``scores [n, C + 1]`` (softmax and the IIF / Seesaw ``get_activation`` are native
    elsewhere): decode ``rois [n, 5]`` with ``bbox_pred`` (the coder's one launch), divide by ``scale_factor`` under ``rescale``
    (float32), then ``multiclass_nms(bboxes, scores, cfg.score_thr, cfg.nms, cfg.max_per_img)``.

    ``bbox_pred is None`` takes the rois' boxes as they are: the reference clamps copies that advanced indexing made
    (``bboxes[:, [0, 2]].clamp_``), so its boxes stay unclamped too.  ``cfg=None`` returns ``(bboxes, scores)`` as the reference
    does.  Returns ``(det_bboxes [k, 5], det_labels [k])`` for one host read, or with ``padded=True`` what
    ``multiclass_nms_padded`` returns, without one."""
    if bbox_pred is not None:
        bboxes = bbox_coder.decode(rois[..., 1:], bbox_pred, max_shape=img_shape)
    else:
        bboxes = rois[:, 1:].clone()
    if rescale and bboxes.size(0) > 0:
        factor = bboxes.new_tensor(scale_factor)
        bboxes = (bboxes.view(bboxes.size(0), -1, 4) / factor).view(bboxes.size(0), -1)
    if cfg is None:
        return bboxes, scores
    score_thr, nms_cfg, max_per_img = _get(cfg, "score_thr"), _get(cfg, "nms"), _get(cfg, "max_per_img")
    if padded:
        return multiclass_nms_padded(bboxes, scores, score_thr, nms_cfg, max_per_img)
    return multiclass_nms(bboxes, scores, score_thr, nms_cfg, max_per_img)
