"""Mask-side class-channel selection of the Mask R-CNN head on the gfx950 kernels.

Mirrors ``mask_cross_entropy`` (instance_segmentation/mmdet/models/losses/cross_entropy_loss.py:112-162)
and the per-RoI channel pick of ``FCNMaskHead.get_seg_masks`` (fcn_mask_head.py:289-290).  The labels are
the ones the IIF classifier produced; nothing else of the mask head changes.

The test end of the head, ``FCNMaskHead.get_seg_masks`` with ``_do_paste_mask`` (fcn_mask_head.py:179-310, 344-412), is
``paste_masks`` / ``get_seg_masks`` on ``iif_paste_masks`` (csrc/mask_ops.hip): class channel, sigmoid, the paste grid,
``grid_sample`` (bilinear, ``align_corners=False``, zero padding) and ``>= threshold`` in one launch that writes the boolean
image and nothing else - no float32 grid, no chunks under a memory limit, no ``isinf(...).any()`` synchronisation.  bf16 logits
are widened to float32 before the sigmoid (the reference rounds the probabilities to bf16).  Deliberately not offered:
``mask_thr_binary < 0`` (the uint8 visualisation branch), predicted masks above 64 x 64, images of 2^31 pixels or more, more than
65 535 detections per call, and a box edge pair that makes a coordinate NaN (a zero-size side whose edge lies exactly on a pixel
centre: 0 / 0) - such pixels come out as padding.
"""
import warnings

import numpy as np
import torch

from . import _lib


def _prep(pred, label):
    _lib.require_gpu(pred, label)
    if pred.dim() < 3:
        raise ValueError("pred must be [N, C, *]")
    if pred.dtype not in (torch.float32, torch.bfloat16):
        pred = pred.float()
    pred = pred.contiguous()
    n, c = pred.shape[0], pred.shape[1]
    hw = pred[0, 0].numel() if n else int(torch.tensor(pred.shape[2:]).prod())
    label = label.reshape(-1).to(torch.int64).contiguous()
    if label.numel() != n:
        raise ValueError("one label per RoI expected")
    return pred, label, n, c, hw


def gather_class_masks(mask_pred, labels):
    """``mask_pred[range(N), labels]`` -> [N, *] fp32 (fcn_mask_head.py:289-290)."""
    pred, label, n, c, hw = _prep(mask_pred, labels)
    out = torch.empty((n,) + tuple(pred.shape[2:]), dtype=torch.float32, device=pred.device)
    if n == 0:
        return out
    status = torch.zeros(1, dtype=torch.int32, device=pred.device)
    _lib.check(_lib.lib().iif_mask_gather(_lib.ptr(pred), _lib.dtype_code(pred), _lib.ptr(label), n, c, hw, _lib.ptr(out),
                                          _lib.ptr(status), _lib.stream_ptr()), "iif_mask_gather")
    return out


class _MaskBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, label):
        p, lb, n, c, hw = _prep(pred.detach(), label)
        t = target.detach().reshape(n, hw).float().contiguous()
        dev = p.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        rows = torch.empty(n, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        need = pred.requires_grad
        dpred = torch.zeros(p.shape, dtype=torch.float32, device=dev) if need else None
        _lib.check(_lib.lib().iif_mask_bce_fwd_bwd(_lib.ptr(p), _lib.dtype_code(p), _lib.ptr(t), _lib.ptr(lb), n, c, hw, 1.0,
                                                   _lib.ptr(rows), _lib.ptr(loss), _lib.ptr(dpred), _lib.ptr(status),
                                                   _lib.stream_ptr()), "iif_mask_bce_fwd_bwd")
        ctx.dpred = dpred
        ctx.in_dtype = pred.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        d = ctx.dpred
        if d is None:
            return None, None, None
        d = d * g.reshape(()).to(d.dtype)
        return d.to(ctx.in_dtype), None, None


def mask_cross_entropy(pred, target, label, reduction="mean", avg_factor=None, class_weight=None, ignore_index=None):
    """cross_entropy_loss.py:112-162: BCE-with-logits on the class channel of every RoI, mean over all
    pixels, returned with shape ``(1,)``.  Loss and gradient come out of one pass over the selected channels."""
    assert ignore_index is None, "BCE loss does not support ignore_index"
    assert reduction == "mean" and avg_factor is None
    if class_weight is not None:
        raise NotImplementedError("class_weight is broadcast against [N, H, W] by the reference; not supported natively")
    if pred.size(0) == 0:
        return pred.sum()[None] * 0 + float("nan")        # mean over an empty slice, as the reference
    return _MaskBCE.apply(pred, target, label)


def paste_masks(mask_pred, det_bboxes, det_labels, img_h, img_w, threshold, class_agnostic=False, activated=False):
    """fcn_mask_head.py:228-306 between the logits and the boolean image: bool ``[N, img_h, img_w]``, one launch, no host
    synchronisation.  ``mask_pred [N, C, h, w]`` float32 / bf16 logits (``activated``: probabilities); ``det_bboxes [N, >= 4]``
    float32, read in place; ``det_labels [N]`` (unused under ``class_agnostic``: channel 0).  A label outside ``[0, C)`` gives an
    all-false mask."""
    if not isinstance(mask_pred, torch.Tensor) or mask_pred.dim() != 4:
        raise ValueError("paste_masks: mask_pred [N, C, h, w] expected")
    if mask_pred.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError("paste_masks: float32 / bfloat16 mask_pred only (got %s)" % mask_pred.dtype)
    if det_bboxes.dtype != torch.float32:
        raise NotImplementedError("paste_masks: float32 boxes only (got %s)" % det_bboxes.dtype)
    if det_bboxes.dim() != 2 or det_bboxes.size(1) < 4 or det_bboxes.size(0) != mask_pred.size(0):
        raise ValueError("paste_masks: det_bboxes [N, 4 or 5] expected")
    threshold = float(threshold)
    if not threshold >= 0:
        raise NotImplementedError("paste_masks: threshold >= 0 only (mask_thr_binary < 0 is the reference's uint8 visualisation "
                                  "branch, which is not offered)")
    img_h, img_w = int(img_h), int(img_w)
    n, c, h, w = mask_pred.shape
    if h > 64 or w > 64 or img_h * img_w >= 1 << 31 or n > 65535:
        raise NotImplementedError("paste_masks: predicted masks of at most 64 x 64, images below 2^31 pixels, at most 65535 detections")
    labels = None
    if not class_agnostic:
        labels = det_labels.detach().reshape(-1).to(torch.int64).contiguous()
        if labels.numel() != n:
            raise ValueError("paste_masks: one label per detection expected")
    _lib.require_gpu(mask_pred, det_bboxes, labels)
    out = torch.empty((n, img_h, img_w), dtype=torch.uint8, device=mask_pred.device)
    if n == 0:
        return out.view(torch.bool)
    pred, boxes = mask_pred.detach().contiguous(), det_bboxes.detach()
    if boxes.stride(1) != 1:
        boxes = boxes.contiguous()
    _lib.check(_lib.lib().iif_paste_masks(_lib.ptr(pred), _lib.dtype_code(pred), int(bool(activated)), _lib.ptr(labels), _lib.ptr(boxes),
                                          boxes.stride(0) if n > 1 else boxes.size(1), n, c, h, w, img_h, img_w, threshold,
                                          _lib.ptr(out), _lib.stream_ptr()), "iif_paste_masks")
    return out.view(torch.bool)


def get_seg_masks(mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale, num_classes,
                  class_agnostic=False, pin_memory=True):
    """``FCNMaskHead.get_seg_masks`` (fcn_mask_head.py:179-310; ``num_classes`` / ``class_agnostic`` are the head's attributes):
    ``cls_segms``, one list per class of bool ndarrays ``[img_h, img_w]`` in detection order.  TWO device-to-host copies - the
    labels and the whole boolean block - against the reference's N + 1.  An ndarray ``mask_pred`` (the AugTest branch) is taken
    as already activated.  ``pin_memory``: the boolean block lands in ONE page-locked host buffer from torch's caching host
    allocator and the returned arrays are views into it (the same copy into a fresh pageable buffer measures six to seven times
    slower, profiles/mask_head.txt); it returns to the allocator when the last of the arrays is dropped.  ``False``: a pageable
    buffer, for a caller that keeps the raw masks of many images instead of encoding them."""
    from .mmdet_nms import _get
    activated = not isinstance(mask_pred, torch.Tensor)
    if activated:
        mask_pred = det_bboxes.new_tensor(mask_pred)
    cls_segms = [[] for _ in range(num_classes)]
    bboxes = det_bboxes[:, :4]
    if not isinstance(scale_factor, torch.Tensor):
        if isinstance(scale_factor, float):
            scale_factor = np.array([scale_factor] * 4)
            warnings.warn('Scale_factor should be a Tensor or ndarray with shape (4,), float would be deprecated. ')
        assert isinstance(scale_factor, np.ndarray)
        scale_factor = torch.Tensor(scale_factor)
    if rescale:
        img_h, img_w = ori_shape[:2]
        bboxes = bboxes / scale_factor.to(bboxes.device)
    else:
        sf = scale_factor.cpu()             # a copy of its own when the caller keeps the factor on the device
        w_scale, h_scale = sf[0], sf[1]
        img_h = np.round(ori_shape[0] * h_scale.item()).astype(np.int32)
        img_w = np.round(ori_shape[1] * w_scale.item()).astype(np.int32)
    im_mask = paste_masks(mask_pred, bboxes, det_labels, int(img_h), int(img_w), _get(rcnn_test_cfg, "mask_thr_binary"),
                          class_agnostic=class_agnostic, activated=activated)
    labels = det_labels.detach().cpu().numpy()
    if pin_memory and im_mask.numel():
        host = torch.empty(im_mask.shape, dtype=im_mask.dtype, pin_memory=True)
        host.copy_(im_mask, non_blocking=True)
        torch.cuda.current_stream(im_mask.device).synchronize()
        block = host.numpy()
    else:
        block = im_mask.cpu().numpy()
    for i in range(block.shape[0]):
        cls_segms[labels[i]].append(block[i])
    return cls_segms
