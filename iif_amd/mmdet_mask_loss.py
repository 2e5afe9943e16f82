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

What every caller does with those masks next - ``encode_mask_results`` (mmdet/core/mask/utils.py:37-64, apis/test.py:61,101), one
``pycocotools.mask.encode`` per mask on the host - is ``paste_masks_rle`` / ``get_seg_masks_rle`` on ``iif_paste_rle_*``
(csrc/mask_rle.hip): the COCO run lengths come straight from the logits tile and the box, the work is proportional to the box
area, and the boolean image exists neither on the device nor on the host.  ``encode_masks`` does the same for bitmaps that are
already on the device.  The result is the list of ``{'size': [H, W], 'counts': bytes}`` that ``mask_util.encode`` returns.  Not
offered on RLE: ``area`` / ``toBbox`` / ``merge`` / ``iou``, decoding on the device, the mask-scoring tuple form of
``mask_results``, polygons.
"""
import ctypes
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


def _label_status(device):
    """The sticky label-status word the fused loss heads share: ``custom.check_label_status()`` raises on it."""
    from . import custom
    return custom._workspace(device, 0, False)[2]


def gather_class_masks(mask_pred, labels):
    """``mask_pred[range(N), labels]`` -> [N, *] fp32 (fcn_mask_head.py:289-290).  A label outside ``[0, C)`` (the reference
    raises) gives a row of zeros and sets the flag that ``custom.check_label_status()`` raises on; no host synchronisation."""
    pred, label, n, c, hw = _prep(mask_pred, labels)
    out = torch.empty((n,) + tuple(pred.shape[2:]), dtype=torch.float32, device=pred.device)
    if n == 0:
        return out
    status = _label_status(pred.device)
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
        status = _label_status(dev)
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
    pixels, returned with shape ``(1,)``.  Loss and gradient come out of one pass over the selected channels.  A label outside
    ``[0, C)`` (the reference raises) contributes zero loss and no gradient and sets the flag that
    ``custom.check_label_status()`` raises on."""
    assert ignore_index is None, "BCE loss does not support ignore_index"
    assert reduction == "mean" and avg_factor is None
    if class_weight is not None:
        raise NotImplementedError("class_weight is broadcast against [N, H, W] by the reference; not supported natively")
    if pred.size(0) == 0:
        return pred.sum()[None] * 0 + float("nan")        # mean over an empty slice, as the reference
    return _MaskBCE.apply(pred, target, label)


def _paste_args(who, mask_pred, det_bboxes, det_labels, img_h, img_w, threshold, class_agnostic):
    """The argument checks of ``paste_masks`` (shared with ``paste_masks_rle``) -> (pred, boxes, ld_boxes, labels, threshold,
    img_h, img_w); pred / boxes are ``None`` for N == 0."""
    if not isinstance(mask_pred, torch.Tensor) or mask_pred.dim() != 4:
        raise ValueError("%s: mask_pred [N, C, h, w] expected" % who)
    if mask_pred.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError("%s: float32 / bfloat16 mask_pred only (got %s)" % (who, mask_pred.dtype))
    if det_bboxes.dtype != torch.float32:
        raise NotImplementedError("%s: float32 boxes only (got %s)" % (who, det_bboxes.dtype))
    if det_bboxes.dim() != 2 or det_bboxes.size(1) < 4 or det_bboxes.size(0) != mask_pred.size(0):
        raise ValueError("%s: det_bboxes [N, 4 or 5] expected" % who)
    threshold = float(threshold)
    if not threshold >= 0:
        raise NotImplementedError("%s: threshold >= 0 only (mask_thr_binary < 0 is the reference's uint8 visualisation "
                                  "branch, which is not offered)" % who)
    img_h, img_w = int(img_h), int(img_w)
    n, c, h, w = mask_pred.shape
    if h > 64 or w > 64 or img_h * img_w >= 1 << 31 or n > 65535:
        raise NotImplementedError("%s: predicted masks of at most 64 x 64, images below 2^31 pixels, at most 65535 detections" % who)
    labels = None
    if not class_agnostic:
        labels = det_labels.detach().reshape(-1).to(torch.int64).contiguous()
        if labels.numel() != n:
            raise ValueError("%s: one label per detection expected" % who)
    _lib.require_gpu(mask_pred, det_bboxes, labels)
    if n == 0:
        return None, None, 4, labels, threshold, img_h, img_w
    pred, boxes = mask_pred.detach().contiguous(), det_bboxes.detach()
    if boxes.stride(1) != 1:
        boxes = boxes.contiguous()
    return pred, boxes, (boxes.stride(0) if n > 1 else boxes.size(1)), labels, threshold, img_h, img_w


def paste_masks(mask_pred, det_bboxes, det_labels, img_h, img_w, threshold, class_agnostic=False, activated=False):
    """fcn_mask_head.py:228-306 between the logits and the boolean image: bool ``[N, img_h, img_w]``, one launch, no host
    synchronisation.  ``mask_pred [N, C, h, w]`` float32 / bf16 logits (``activated``: probabilities); ``det_bboxes [N, >= 4]``
    float32, read in place; ``det_labels [N]`` (unused under ``class_agnostic``: channel 0).  A label outside ``[0, C)`` gives an
    all-false mask."""
    pred, boxes, ldb, labels, threshold, img_h, img_w = _paste_args("paste_masks", mask_pred, det_bboxes, det_labels, img_h, img_w,
                                                                    threshold, class_agnostic)
    n, c, h, w = mask_pred.shape
    out = torch.empty((n, img_h, img_w), dtype=torch.uint8, device=mask_pred.device)
    if n == 0:
        return out.view(torch.bool)
    _lib.check(_lib.lib().iif_paste_masks(_lib.ptr(pred), _lib.dtype_code(pred), int(bool(activated)), _lib.ptr(labels), _lib.ptr(boxes),
                                          ldb, n, c, h, w, img_h, img_w, threshold, _lib.ptr(out), _lib.stream_ptr()), "iif_paste_masks")
    return out.view(torch.bool)


def _rle_encode(what, lead, n, H, W, device, extra=None):
    """The two steps of csrc/mask_rle.hip around the one read that sizes the run buffer.  ``lead``: the entry's arguments up to
    the workspace; ``extra``: an int64 device vector that comes to the host in the same copy as the totals (the labels).  Returns
    (list of n RLE dicts, extra on the host).  Two device-to-host copies: the totals, then the runs."""
    L = _lib.lib()
    if n == 0:
        return [], (None if extra is None else extra.cpu().numpy())
    ws_bytes = L.iif_rle_workspace_bytes(n, H, W)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=device)
    totals = torch.empty(n, dtype=torch.int32, device=device)
    _lib.check(getattr(L, what + "_count")(*lead, _lib.ptr(ws), ws_bytes, _lib.ptr(totals), _lib.stream_ptr()), what + "_count")
    if extra is None:
        tot = totals.cpu().numpy().astype(np.int64)
    else:
        both = torch.cat([totals.to(torch.int64), extra]).cpu().numpy()
        tot, extra = both[:n], both[n:]
    total = int(tot.sum())
    dev = torch.empty((2, total), dtype=torch.int32, device=device)           # transition positions (scratch), runs
    _lib.check(getattr(L, what + "_fill")(*lead, _lib.ptr(ws), ws_bytes, _lib.ptr(totals), total, _lib.ptr(dev[0]), _lib.ptr(dev[1]),
                                          _lib.stream_ptr()), what + "_fill")
    runs = np.ascontiguousarray(dev[1].cpu().numpy()).view(np.uint32)
    return _rle_strings(runs, tot, H, W), extra


def _rle_strings(runs, totals, H, W):
    """Host: the flat uint32 counts of consecutive masks -> ``{'size': [H, W], 'counts': bytes}`` each (``iif_rle_to_string``)."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(max(1, 7 * int(totals.max()) if len(totals) else 1))
    length = ctypes.c_int64(0)
    base, item, out, at = runs.ctypes.data, runs.itemsize, [], 0
    for m in totals.tolist():
        _lib.check(L.iif_rle_to_string(base + at * item, m, buf, len(buf), ctypes.byref(length)), "iif_rle_to_string")
        out.append({"size": [H, W], "counts": ctypes.string_at(buf, length.value)})
        at += m
    return out


def _paste_rle(mask_pred, det_bboxes, det_labels, img_h, img_w, threshold, class_agnostic, activated, extra):
    pred, boxes, ldb, labels, threshold, img_h, img_w = _paste_args("paste_masks_rle", mask_pred, det_bboxes, det_labels, img_h, img_w,
                                                                    threshold, class_agnostic)
    n, c, h, w = mask_pred.shape
    lead = () if n == 0 else (_lib.ptr(pred), _lib.dtype_code(pred), int(bool(activated)), _lib.ptr(labels), _lib.ptr(boxes), ldb,
                              n, c, h, w, img_h, img_w, threshold)
    return _rle_encode("iif_paste_rle", lead, n, img_h, img_w, mask_pred.device, extra)


def paste_masks_rle(mask_pred, det_bboxes, det_labels, img_h, img_w, threshold, class_agnostic=False, activated=False):
    """``paste_masks`` followed by pycocotools' ``mask.encode`` on every mask, without the masks: a list of N dicts
    ``{'size': [img_h, img_w], 'counts': bytes}`` in detection order, byte for byte what ``encode`` gives for
    ``paste_masks(...)[i]``.  The same arguments, checks and limits as ``paste_masks``.  Two device-to-host copies: N int32
    (the run count of every mask, which sizes the run buffer), then the runs themselves."""
    return _paste_rle(mask_pred, det_bboxes, det_labels, img_h, img_w, threshold, class_agnostic, activated, None)[0]


def encode_masks(masks):
    """pycocotools' ``mask.encode`` for masks that are on the device: ``[N, H, W]`` or ``[H, W]``, ``bool`` or ``uint8`` (any
    non-zero byte is inside), or a ``DeviceBitmapMasks``; a list of RLE dicts (one dict's worth for ``[H, W]``: a list of one).
    The masks are read in place whatever their row and mask pitch, as long as a row's elements are adjacent."""
    if hasattr(masks, "device_masks"):
        if not torch.cuda.is_available():
            raise _lib.IIFNativeError("encode_masks runs on MI355X only (no CPU fallback; host masks are pycocotools' own ground)")
        masks = masks.device_masks(torch.device("cuda", torch.cuda.current_device()))
    if not isinstance(masks, torch.Tensor):
        raise NotImplementedError("encode_masks: a device tensor or DeviceBitmapMasks expected (got %s)" % type(masks).__name__)
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    if masks.dtype != torch.uint8:
        raise NotImplementedError("encode_masks: bool / uint8 masks only (got %s)" % masks.dtype)
    if masks.dim() == 2:
        masks = masks[None]
    if masks.dim() != 3:
        raise ValueError("encode_masks: masks [N, H, W] or [H, W] expected (got %s)" % (tuple(masks.shape),))
    n, H, W = masks.shape
    if n > 65535 or H * W >= 1 << 31:
        raise NotImplementedError("encode_masks: images below 2^31 pixels, at most 65535 masks")
    _lib.require_gpu(masks)
    if n == 0:
        return []
    if H == 0 or W == 0:
        raise ValueError("encode_masks: empty masks")
    masks = masks.detach()
    ld_row = masks.stride(1) if H > 1 else W
    ld_mask = masks.stride(0) if n > 1 else (H - 1) * ld_row + W
    if (W > 1 and masks.stride(2) != 1) or ld_row < W or ld_mask < (H - 1) * ld_row + W:
        masks = masks.contiguous()
        ld_row, ld_mask = W, H * W
    return _rle_encode("iif_mask_rle", (_lib.ptr(masks), ld_row, ld_mask, n, H, W), n, H, W, masks.device)[0]


def _seg_geometry(mask_pred, det_bboxes, ori_shape, scale_factor, rescale):
    """fcn_mask_head.py:228-262: the boxes in the output image's coordinates and that image's size ->
    (mask_pred, activated, bboxes, img_h, img_w)."""
    activated = not isinstance(mask_pred, torch.Tensor)
    if activated:
        mask_pred = det_bboxes.new_tensor(mask_pred)
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
    return mask_pred, activated, bboxes, int(img_h), int(img_w)


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
    mask_pred, activated, bboxes, img_h, img_w = _seg_geometry(mask_pred, det_bboxes, ori_shape, scale_factor, rescale)
    cls_segms = [[] for _ in range(num_classes)]
    im_mask = paste_masks(mask_pred, bboxes, det_labels, img_h, img_w, _get(rcnn_test_cfg, "mask_thr_binary"),
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


def get_seg_masks_rle(mask_pred, det_bboxes, det_labels, rcnn_test_cfg, ori_shape, scale_factor, rescale, num_classes,
                      class_agnostic=False):
    """``encode_mask_results(get_seg_masks(...))`` (mmdet/core/mask/utils.py:37-64 on fcn_mask_head.py:179-310) without the
    masks: ``cls_segms``, one list per class of RLE dicts ``{'size': [img_h, img_w], 'counts': bytes}`` in detection order - what
    the test loop keeps (apis/test.py:61), so that line needs no ``encode_mask_results`` any more.  TWO device-to-host copies: the
    run count of every mask together with the labels, then the runs - a few kilobytes per detection instead of the boolean block."""
    from .mmdet_nms import _get
    mask_pred, activated, bboxes, img_h, img_w = _seg_geometry(mask_pred, det_bboxes, ori_shape, scale_factor, rescale)
    cls_segms = [[] for _ in range(num_classes)]
    labels = det_labels.detach().reshape(-1).to(torch.int64)
    rles, labels = _paste_rle(mask_pred, bboxes, det_labels, img_h, img_w, _get(rcnn_test_cfg, "mask_thr_binary"), class_agnostic,
                              activated, labels)
    for i, rle in enumerate(rles):
        cls_segms[labels[i]].append(rle)
    return cls_segms
