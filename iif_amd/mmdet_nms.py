"""mmcv's ``nms`` / ``batched_nms`` and mmdet's ``RPNHead.get_bboxes`` on the gfx950 kernels (csrc/nms.hip).

Mirror of mmcv 1.3.8 ``ops/nms.py`` (``nms``, ``batched_nms``) and instance_segmentation/mmdet/models/dense_heads/
rpn_head.py:79-225 (``get_bboxes`` / ``_get_bboxes_single``): signatures, assertions, the empty results ``zeros(0, 5)``.

  * ``nms`` / ``batched_nms``: ``iif_nms``, 5 enqueued operations whatever N and the data, then ONE host read (the count) to
    return exact sizes.  ``nms_padded`` / ``batched_nms_padded`` return the padded tensors and the device count without a read.
  * ``rpn_proposals_padded``: ``iif_rpn_proposals``, 10 enqueued operations for all images and levels, no synchronisation.
  * ``rpn_get_bboxes``: the reference's list of ``[n, 5]`` tensors for ONE host read of the B counts.

Ranking is by score descending with equal scores to the lower index (the reference's sort is unstable, so any tie order is one
of its outputs); the overlap test and the id shift are mmcv's float32 operations in mmcv's order, so ``keep`` is exactly what
the reference keeps.

``multiclass_nms`` (1 000 x 1 203 candidates on LVIS) has a segmented per-class design of its own, not this N^2 matrix:
mmdet_multiclass_nms.py.  Deliberately not offered: ``soft_nms``, ``nms_match``, ``fast_nms``; more than 16 384 boxes; the two-class softmax RPN; ``rescale``; the ONNX
branches; a tensor ``max_shape``; ``with_nms=False``; on the RPN path ``split_thr`` candidates or more per image (the
reference's data-dependent switch to a per-level NMS).  The padded proposals feed the RoI stage without a read:
``mmdet_roi_stage.roi_stage_targets_padded`` takes ``(dets, counts)`` as they are.  The head's training side (anchors, batch
targets, the loss at the sampled anchors) is ``mmdet_anchor.AnchorGenerator`` and ``mmdet_rpn_stage.rpn_head_loss``; it is not
wired into the class registered here.  When mmdet is importable a subclass of its ``RPNHead`` registers itself as ``RPNHead``.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .mmdet_targets import _f4

MAX_BOXES = 16384


def workspace_bytes(B, N):
    """``IIF_NMS_WORKSPACE_BYTES(B, N)`` of include/iif_amd.h."""
    n64 = (int(N) + 63) // 64 * 64
    return 4096 + int(B) * (659456 + n64 * (64 + n64 // 8))


def _get(cfg, key, *default):
    if isinstance(cfg, dict):
        return cfg.get(key, *default) if default else cfg[key]
    return getattr(cfg, key, *default)


def _workspace(given, nbytes, dev):
    """The call's workspace: its own allocation, or the caller's uint8 tensor (16-byte aligned, large enough, contents free)."""
    if given is None:
        return torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if given.dtype != torch.uint8 or not given.is_contiguous() or given.numel() < nbytes or given.data_ptr() % 16:
        raise ValueError("workspace: a contiguous, 16-byte aligned uint8 tensor of at least %d bytes expected" % nbytes)
    _lib.require_gpu(given)
    return given


def _check_inputs(boxes, scores, what):
    if not isinstance(boxes, torch.Tensor) or not isinstance(scores, torch.Tensor):
        raise NotImplementedError("%s: tensors only (numpy inputs are not offered on the native path)" % what)
    if boxes.dim() != 2:
        raise NotImplementedError("%s: [n, 4] boxes only (got %s)" % (what, tuple(boxes.shape)))
    assert boxes.size(1) == 4
    assert boxes.size(0) == scores.size(0)
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32:
        raise NotImplementedError("%s: float32 boxes and scores only (got %s, %s)" % (what, boxes.dtype, scores.dtype))
    if boxes.size(0) > MAX_BOXES:
        raise ValueError("%s: at most %d boxes (got %d): the suppression matrix is N^2 / 8 bytes" % (what, MAX_BOXES, boxes.size(0)))
    _lib.require_gpu(boxes, scores)


def _nms_padded(boxes, scores, ids, id_mode, iou_threshold, offset, score_threshold, max_num, workspace=None):
    assert offset in (0, 1)
    N = boxes.size(0)
    dev = boxes.device
    b = boxes if boxes.stride(1) == 1 and (N <= 1 or boxes.stride(0) >= 4) else boxes.contiguous()
    ld = b.stride(0) if N > 1 else 4
    s = scores.reshape(-1).contiguous()
    max_num = int(max_num)
    cap = min(max_num, N) if max_num > 0 else N
    keep = torch.empty((cap,), dtype=torch.int64, device=dev)
    dets = torch.empty((cap, 5), dtype=torch.float32, device=dev)
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    ws_bytes = workspace_bytes(1, N)
    ws = _workspace(workspace, ws_bytes if N else 16, dev)
    rc = _lib.lib().iif_nms(_lib.ptr(b), ld, _lib.ptr(s), _lib.ptr(ids), N, id_mode, float(iou_threshold), int(offset),
                            float(score_threshold), max_num, _lib.ptr(keep), _lib.ptr(dets), _lib.ptr(count), _lib.ptr(ws), ws_bytes,
                            _lib.stream_ptr())
    _lib.check(rc, "iif_nms")
    return dets, keep, count


def nms_padded(boxes, scores, iou_threshold, offset=0, score_threshold=0, max_num=-1, workspace=None):
    """``nms`` without a host read: ``(dets [cap, 5], keep [cap], count [1])`` on the device, ``cap = min(max_num, N)`` or N;
    the kept boxes in rank order, then zero rows / -1."""
    _check_inputs(boxes, scores, "nms")
    return _nms_padded(boxes, scores, None, 0, iou_threshold, offset, score_threshold, max_num, workspace)


def nms(boxes, scores, iou_threshold, offset=0, score_threshold=0, max_num=-1):
    """mmcv ``nms``: ``(dets [n, 5], inds [n])``.  One host read (the count)."""
    dets, keep, count = nms_padded(boxes, scores, iou_threshold, offset, score_threshold, max_num)
    n = int(count.item())
    return dets[:n], keep[:n]


def _batched_args(boxes, scores, idxs, nms_cfg, class_agnostic):
    cfg = dict(nms_cfg)
    class_agnostic = cfg.pop("class_agnostic", class_agnostic)
    nms_type = cfg.pop("type", "nms")
    if nms_type != "nms":
        raise NotImplementedError("batched_nms: nms_cfg['type'] = %r is not offered on the native path (only 'nms')" % (nms_type,))
    split_thr = cfg.pop("split_thr", 10000)
    kw = dict(iou_threshold=cfg.pop("iou_threshold"), offset=cfg.pop("offset", 0), score_threshold=cfg.pop("score_threshold", 0),
              max_num=cfg.pop("max_num", -1))
    if cfg:
        raise TypeError("batched_nms: unexpected keys in nms_cfg: %s" % sorted(cfg))
    _check_inputs(boxes, scores, "batched_nms")
    if class_agnostic:
        return None, 0, kw
    assert idxs.size(0) == boxes.size(0)
    _lib.require_gpu(idxs)
    ids = idxs.reshape(-1).to(torch.int64).contiguous()
    return ids, (1 if boxes.size(0) < split_thr else 2), kw


def batched_nms_padded(boxes, scores, idxs, nms_cfg, class_agnostic=False, workspace=None):
    """``batched_nms`` without a host read: ``(dets [cap, 5], keep [cap], count [1])``."""
    ids, mode, kw = _batched_args(boxes, scores, idxs, nms_cfg, class_agnostic)
    return _nms_padded(boxes, scores, ids, mode, workspace=workspace, **kw)


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """mmcv ``batched_nms``: ``(dets [n, 5], keep [n])`` - boxes of different ``idxs`` do not suppress each other (through
    mmcv's coordinate shift, quirks included).  Honours ``class_agnostic``, ``split_thr``, ``max_num``, ``iou_threshold``,
    ``offset`` and ``score_threshold`` in ``nms_cfg``.  One host read (the count)."""
    dets, keep, count = batched_nms_padded(boxes, scores, idxs, nms_cfg, class_agnostic)
    n = int(count.item())
    return dets[:n], keep[:n]


# ------------------------------------------------------------------------------------------------------------ RPN
class RPNCandidates:
    """The ranked candidates of ``rpn_proposals_padded(..., return_candidates=True)``, each ``[B, Ncand, ...]``: ``index`` (into
    the concatenated anchors), ``boxes``, ``scores``, ``level``, ``valid`` (passed the min-size filter); per image in NMS order,
    the candidates that take no part behind the others."""

    def __init__(self, index, boxes, scores, level, valid):
        self.index, self.boxes, self.scores, self.level, self.valid = index, boxes, scores, level, valid


def _nms_settings(cfg):
    nms_cfg = _get(cfg, "nms")
    nms_cfg = dict(nms_cfg)
    if nms_cfg.pop("type", "nms") != "nms":
        raise NotImplementedError("rpn proposals: cfg.nms.type other than 'nms' is not offered on the native path")
    if nms_cfg.pop("class_agnostic", False):
        raise NotImplementedError("rpn proposals: class_agnostic NMS over the levels is not offered")
    if nms_cfg.pop("score_threshold", 0) > 0:
        raise NotImplementedError("rpn proposals: cfg.nms.score_threshold is not offered")
    split_thr = nms_cfg.pop("split_thr", 10000)
    iou, offset, max_num = nms_cfg.pop("iou_threshold"), nms_cfg.pop("offset", 0), nms_cfg.pop("max_num", -1)
    if nms_cfg:
        raise TypeError("rpn proposals: unexpected keys in cfg.nms: %s" % sorted(nms_cfg))
    return float(iou), int(offset), int(max_num), int(split_thr)


def rpn_proposals_padded(cls_scores, bbox_preds, mlvl_anchors, img_shapes, cfg, bbox_coder, return_candidates=False, workspace=None):
    """rpn_head.py:111-225 for all images in one call, without a synchronisation: ``(dets [B, max_per_img, 5], counts [B])``
    on the device (kept proposals in rank order, then zero rows), with ``return_candidates`` also an ``RPNCandidates``.

    ``cls_scores[l]`` ``[B, A, H, W]`` and ``bbox_preds[l]`` ``[B, 4 A, H, W]`` float32, read in place (any strides);
    ``mlvl_anchors[l]`` ``[A H W, 4]``; ``img_shapes`` one ``(H, W[, C])`` per image; ``cfg`` anything with ``nms_pre``,
    ``max_per_img``, ``min_bbox_size``, ``nms`` as attributes or keys; ``bbox_coder`` a ``DeltaXYWHBBoxCoder``; ``workspace`` (optional) the caller's uint8 tensor of ``workspace_bytes(B, Ncand)``."""
    assert len(cls_scores) == len(bbox_preds) == len(mlvl_anchors)
    L = len(cls_scores)
    if not 1 <= L <= 8:
        raise ValueError("rpn proposals: 1 .. 8 levels (got %d)" % L)
    B = cls_scores[0].size(0)
    assert len(img_shapes) == B
    if not 1 <= B <= 16:
        raise ValueError("rpn proposals: 1 .. 16 images per call (got %d)" % B)
    if isinstance(img_shapes, torch.Tensor) or any(isinstance(x, torch.Tensor) for x in img_shapes):
        raise NotImplementedError("rpn proposals: a tensor max_shape is not offered; pass (H, W) per image")
    nms_pre, max_per_img = int(_get(cfg, "nms_pre")), int(_get(cfg, "max_per_img"))
    min_size = float(_get(cfg, "min_bbox_size"))
    iou, offset, max_num, split_thr = _nms_settings(cfg)
    if max_num > 0:
        max_per_img = min(max_per_img, max_num)
    if max_per_img < 1:
        raise ValueError("rpn proposals: max_per_img must be positive")
    levels = (_lib.RpnLevel * L)()
    held = []
    ncand = 0
    for l in range(L):
        s, d, a = cls_scores[l], bbox_preds[l], mlvl_anchors[l]
        if s.dtype != torch.float32 or d.dtype != torch.float32 or a.dtype != torch.float32:
            raise NotImplementedError("rpn proposals: float32 only (got %s, %s, %s)" % (s.dtype, d.dtype, a.dtype))
        assert s.dim() == 4 and d.dim() == 4 and s.size(0) == B and d.size(0) == B
        assert s.size()[-2:] == d.size()[-2:]
        A, H, W = s.size(1), s.size(2), s.size(3)
        if d.size(1) != 4 * A:
            raise NotImplementedError("rpn proposals: the sigmoid classifier only (use_sigmoid_cls=True): %d score channels "
                                      "against %d delta channels" % (A, d.size(1)))
        assert a.dim() == 2 and a.size(0) == A * H * W and a.size(1) == 4
        s, d = s.detach(), d.detach()
        if a.stride(1) != 1:
            a = a.contiguous()
        held += [s, d, a]
        lv = levels[l]
        lv.scores, lv.deltas, lv.anchors = s.data_ptr(), d.data_ptr(), a.data_ptr()
        lv.score_strides = (ctypes.c_int64 * 4)(*s.stride())
        lv.delta_strides = (ctypes.c_int64 * 4)(*d.stride())
        lv.ld_anchors = a.stride(0) if a.size(0) > 1 else 4
        lv.A, lv.H, lv.W = A, H, W
        n = A * H * W
        ncand += nms_pre if 0 < nms_pre < n else n
    if ncand > MAX_BOXES:
        raise ValueError("rpn proposals: at most %d candidates per image (got %d): lower nms_pre" % (MAX_BOXES, ncand))
    if ncand >= split_thr:
        # the reference runs the NMS per level once the candidates that pass the min-size filter number split_thr or more; how many
        # pass is known on the device only, and this entry always tests all pairs on the shifted boxes
        raise NotImplementedError("rpn proposals: %d candidates per image reach cfg.nms.split_thr = %d, where the reference may "
                                  "switch to a per-level NMS; that switch is not offered here: lower nms_pre or raise split_thr"
                                  % (ncand, split_thr))
    _lib.require_gpu(*held)
    dev = cls_scores[0].device
    hw = (ctypes.c_float * (2 * B))(*[float(v) for shp in img_shapes for v in shp[:2]])
    dets = torch.empty((B, max_per_img, 5), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int64, device=dev)
    cand = None
    if return_candidates:
        cand = RPNCandidates(torch.empty((B, ncand), dtype=torch.int64, device=dev),
                             torch.empty((B, ncand, 4), dtype=torch.float32, device=dev),
                             torch.empty((B, ncand), dtype=torch.float32, device=dev),
                             torch.empty((B, ncand), dtype=torch.int32, device=dev),
                             torch.empty((B, ncand), dtype=torch.int8, device=dev))
    ws_bytes = workspace_bytes(B, ncand)
    ws = _workspace(workspace, ws_bytes, dev)
    means, stds = _f4(bbox_coder.means, "target_means"), _f4(bbox_coder.stds, "target_stds")
    max_ratio = float(np.abs(np.log(16 / 1000)))
    c = cand
    rc = _lib.lib().iif_rpn_proposals(levels, L, B, hw, nms_pre, max_per_img, min_size, iou, offset, means, stds, max_ratio,
                                      int(bool(bbox_coder.add_ctr_clamp)), float(bbox_coder.ctr_clamp),
                                      int(bool(bbox_coder.clip_border)), _lib.ptr(dets), _lib.ptr(counts),
                                      _lib.ptr(c.index if c else None), _lib.ptr(c.boxes if c else None),
                                      _lib.ptr(c.scores if c else None), _lib.ptr(c.level if c else None),
                                      _lib.ptr(c.valid if c else None), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
    _lib.check(rc, "iif_rpn_proposals")
    del held
    return (dets, counts, cand) if return_candidates else (dets, counts)


def rpn_get_bboxes(cls_scores, bbox_preds, mlvl_anchors, img_metas, cfg, bbox_coder, rescale=False, with_nms=True):
    """rpn_head.py:79-133: the reference's list of ``[n, 5]`` proposals, one per image (``zeros(0, 5)`` where nothing
    survives).  ONE host read: the B counts."""
    if not with_nms:
        raise ValueError("rpn_get_bboxes: ``with_nms`` in RPNHead should always be True")
    if rescale:
        raise NotImplementedError("rpn_get_bboxes: rescale=True is not offered on the native path")
    img_shapes = [m["img_shape"] for m in img_metas]
    dets, counts = rpn_proposals_padded(cls_scores, bbox_preds, mlvl_anchors, img_shapes, cfg, bbox_coder)
    return [dets[i, :n] for i, n in enumerate(counts.tolist())]


def register_into_mmdet():
    """Register a subclass of mmdet's ``RPNHead`` whose ``get_bboxes`` is the native one, as ``RPNHead``, if mmdet is importable."""
    try:
        from mmdet.models.builder import HEADS
        from mmdet.models.dense_heads.rpn_head import RPNHead as _RPNHead
    except Exception:
        return False

    class RPNHead(_RPNHead):
        def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=False, with_nms=True):
            if not self.use_sigmoid_cls:
                raise NotImplementedError("native RPNHead: use_sigmoid_cls=False (the two-class softmax RPN) is not offered")
            if torch.onnx.is_in_onnx_export():
                raise NotImplementedError("native RPNHead: the ONNX export branches are not offered")
            assert len(cls_scores) == len(bbox_preds)
            cfg = self.test_cfg if cfg is None else cfg
            sizes = [s.shape[-2:] for s in cls_scores]
            anchors = self.anchor_generator.grid_anchors(sizes, device=cls_scores[0].device)
            return rpn_get_bboxes([s.float() for s in cls_scores], [d.float() for d in bbox_preds], anchors, img_metas, cfg,
                                  self.bbox_coder, rescale=rescale, with_nms=with_nms)

    HEADS.register_module(name="RPNHead", force=True, module=RPNHead)
    return True


register_into_mmdet()
