"""mmdet's ``mask_target`` and ``BitmapMasks.crop_and_resize`` on the gfx950 kernel ``iif_mask_targets`` (csrc/mask_ops.hip).

Mirror of instance_segmentation/mmdet/core/mask/mask_target.py:7-127 and core/mask/structures.py:333-367.  Per positive
proposal: clip the box to the image (``np.clip`` on the float32 proposal), mmcv's RoIAlign (``spatial_scale=1``,
``sampling_ratio=0``, ``'avg'``, ``aligned=True``) on the gt mask the assigned index names, then ``>= 0.5`` (or the raw average
under ``cfg.soft_mask_target``).  The reference reads proposals and indices back, uploads every mask, ``index_select``s them into a
float32 ``[P, H, W]`` tensor, and brings the result through numpy; here the mask bytes are read in place through the index, all
images go in one launch, and nothing is read back:

  * ``mask_target`` / ``mask_target_single``: the reference's signatures and return values (a float32 device tensor).  On
    device-resident masks they make no host read; with host masks, uploads only.
  * ``mask_targets_padded``: for the ``rois`` / ``pos_assigned_gt_inds`` that ``mmdet_targets.bbox_targets`` returns for padded
    samplings (image index -1 on padding rows): ``[K, mh, mw]`` with zero rows for padding.
  * ``DeviceBitmapMasks``: the gt masks of one image, uploaded once.  Its ``crop_and_resize`` returns a device tensor and clips
    the boxes to the image like ``mask_target_single`` does before it calls the reference's.

An item of ``gt_masks_list`` may be anything with ``.masks`` (ndarray ``[G, H, W]``), ``.height`` and ``.width`` (``BitmapMasks``
by duck type), a numpy array, a uint8 / bool device tensor (rows contiguous; a view into a wider buffer is read in place), or a
``DeviceBitmapMasks``.  Deliberately not offered: ``PolygonMasks`` (rasterise them first), an interpolation other than
``'bilinear'``, proposals in another dtype than float32, masks wider than 4 096 pixels and mask sizes above 64.  A row whose image
index is outside the list, whose gt index is outside ``[0, G)`` or whose coordinates are not finite is a zero row (the reference
would raise or read out of bounds).  Nothing registers itself into mmdet: ``fcn_mask_head.py`` imports ``mask_target`` by name
(INTEGRATION.md shows the switch).
"""
import numpy as np
import torch
from torch.nn.modules.utils import _pair

from . import _lib
from .mmdet_nms import _get

MAX_IMAGES, MAX_WIDTH, MAX_MASK_SIZE = 16, 4096, 64


def _host_to_uint8(masks, height=None, width=None):
    """ndarray (or list of 2-D ndarrays) -> contiguous uint8 ``[G, H, W]``, any non-zero value -> kept non-zero."""
    if isinstance(masks, list):
        if len(masks) and not isinstance(masks[0], np.ndarray):
            raise NotImplementedError("mask_target: polygon masks are not offered on the native path; rasterise them to bitmaps first")
        masks = np.stack(masks) if len(masks) else np.empty((0, height or 0, width or 0), dtype=np.uint8)
    if not isinstance(masks, np.ndarray):
        raise NotImplementedError("mask_target: masks of type %s are not offered (ndarray, uint8 / bool tensor, DeviceBitmapMasks "
                                  "or an object with .masks / .height / .width)" % type(masks).__name__)
    if height is not None:
        masks = masks.reshape(-1, height, width)
    if masks.ndim != 3:
        raise ValueError("mask_target: masks must be [G, H, W] (got %s)" % (masks.shape,))
    if masks.dtype == np.bool_:
        masks = masks.view(np.uint8)
    elif masks.dtype != np.uint8:
        masks = (masks != 0).astype(np.uint8)
    masks = np.ascontiguousarray(masks)
    return masks if masks.flags.writeable else masks.copy()        # torch.from_numpy wants a writable array


def _device_uint8(t):
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise NotImplementedError("mask_target: uint8 / bool mask tensors only (got %s)" % t.dtype)
    if t.dim() != 3:
        raise ValueError("mask_target: masks must be [G, H, W] (got %s)" % (tuple(t.shape),))
    _lib.require_gpu(t)
    if t.size(2) > 1 and t.stride(2) != 1:
        t = t.contiguous()
    return t


class DeviceBitmapMasks:
    """The gt masks of one image for the native mask targets: ``masks`` (ndarray, list of ndarrays or a uint8 / bool tensor
    ``[G, H, W]``), uploaded ONCE per device on first use and cached."""

    def __init__(self, masks, height, width):
        self.height, self.width = int(height), int(width)
        if isinstance(masks, torch.Tensor):
            self.masks = masks.reshape(-1, self.height, self.width) if masks.numel() == 0 else masks
            assert self.masks.dim() == 3 and tuple(self.masks.shape[1:]) == (self.height, self.width)
            self._cache = {self.masks.device: _device_uint8(self.masks)} if self.masks.is_cuda else {}
        else:
            self.masks = _host_to_uint8(masks, self.height, self.width)
            self._cache = {}

    def device_masks(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._cache.get(device)
        if t is None:
            src = self.masks if isinstance(self.masks, torch.Tensor) else torch.from_numpy(self.masks)
            t = _device_uint8(src.to(device))
            self._cache[device] = t
        return t

    def __len__(self):
        return int(self.masks.shape[0])

    def __getitem__(self, index):
        m = self.masks[index]
        return DeviceBitmapMasks(m.reshape(-1, self.height, self.width), self.height, self.width)

    def __repr__(self):
        return "DeviceBitmapMasks(num_masks=%d, height=%d, width=%d)" % (len(self), self.height, self.width)

    def crop_and_resize(self, bboxes, out_shape, inds, device=None, interpolation='bilinear', binarize=True):
        """structures.py:333-367 with the clip of mask_target.py:112-113: a float32 device tensor ``[n, oh, ow]``."""
        if interpolation != 'bilinear':
            raise NotImplementedError("crop_and_resize: interpolation %r is not offered (only 'bilinear')" % (interpolation,))
        if device is None:
            device = bboxes.device if isinstance(bboxes, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        out_shape = _pair(out_shape)
        if isinstance(bboxes, np.ndarray):
            bboxes = torch.from_numpy(np.ascontiguousarray(bboxes, dtype=np.float32))
        if isinstance(inds, np.ndarray):
            inds = torch.from_numpy(inds)
        bboxes, inds = bboxes.to(device), inds.to(device)
        if len(self) == 0:
            return bboxes.new_zeros((0,) + out_shape, dtype=torch.float32)
        return mask_target_single(bboxes, inds, self, dict(mask_size=out_shape, soft_mask_target=not binarize))


def _resolve(item, device):
    """One item of gt_masks_list -> its uint8 device tensor ``[G, H, W]`` (rows contiguous)."""
    if isinstance(item, DeviceBitmapMasks):
        return item.device_masks(device)
    if isinstance(item, torch.Tensor):
        return _device_uint8(item)
    if isinstance(item, np.ndarray):
        return _device_uint8(torch.from_numpy(_host_to_uint8(item)).to(device))
    if type(item).__name__ == "PolygonMasks":
        raise NotImplementedError("mask_target: PolygonMasks are not offered on the native path; rasterise them to bitmaps first")
    if hasattr(item, "masks") and hasattr(item, "height") and hasattr(item, "width"):
        return _device_uint8(torch.from_numpy(_host_to_uint8(item.masks, int(item.height), int(item.width))).to(device))
    raise NotImplementedError("mask_target: gt masks of type %s are not offered" % type(item).__name__)


def _launch(rois, gt_inds, masks, mask_size, binarize):
    """rois [K, 5] (image index into ``masks``), gt_inds [K], masks: the resolved tensors of at most MAX_IMAGES images."""
    mh, mw = mask_size
    K = rois.size(0)
    out = torch.empty((K, mh, mw), dtype=torch.float32, device=rois.device)
    if K == 0:
        return out
    arr = (_lib.MaskImage * len(masks))()
    for d, m in zip(arr, masks):
        G, H, W = m.shape
        if W > MAX_WIDTH:
            raise NotImplementedError("mask_target: masks of at most %d pixels width (got %d)" % (MAX_WIDTH, W))
        d.ptr, d.G, d.H, d.W = (m.data_ptr() if G else None), G, H, W
        d.ld_row = m.stride(1) if H > 1 else W
        d.ld_mask = m.stride(0) if G > 1 else (H - 1) * d.ld_row + W
    ld_rois = rois.stride(0) if K > 1 else rois.size(1)          # one row: its stride is arbitrary
    status = _lib.lib().iif_mask_targets(arr, len(masks), _lib.ptr(rois), ld_rois, _lib.ptr(gt_inds), K, mh, mw, int(binarize),
                                         _lib.ptr(out), _lib.stream_ptr())
    _lib.check(status, "iif_mask_targets")
    return out


def _check_size(mask_size):
    mh, mw = (int(v) for v in _pair(mask_size))
    if not (1 <= mh <= MAX_MASK_SIZE and 1 <= mw <= MAX_MASK_SIZE):
        raise NotImplementedError("mask_target: mask sizes of 1 .. %d (got %s)" % (MAX_MASK_SIZE, (mh, mw)))
    return mh, mw


def mask_targets_padded(rois, pos_assigned_gt_inds, gt_masks_list, mask_size, binarize=True):
    """``[K, mh, mw]`` float32 for ``rois [K, 5]`` (image index, x1, y1, x2, y2) and ``pos_assigned_gt_inds [K]`` as
    ``mmdet_targets.bbox_targets`` returns them for padded samplings; a row with image index -1 is a zero row.  One launch, and no
    host synchronisation when the masks are on the device already."""
    if not isinstance(rois, torch.Tensor) or rois.dim() != 2 or rois.size(1) < 5:
        raise ValueError("mask_targets_padded: rois [K, 5] expected")
    if rois.dtype != torch.float32:
        raise NotImplementedError("mask_target: float32 proposals only (got %s)" % rois.dtype)
    if len(gt_masks_list) < 1 or len(gt_masks_list) > MAX_IMAGES:
        raise ValueError("mask_targets_padded: 1 .. %d images (got %d)" % (MAX_IMAGES, len(gt_masks_list)))
    mask_size = _check_size(mask_size)
    _lib.require_gpu(rois, pos_assigned_gt_inds)
    rois = rois.detach()
    if rois.stride(1) != 1:
        rois = rois.contiguous()
    gt = pos_assigned_gt_inds.detach().reshape(-1).to(torch.int64).contiguous()
    if gt.numel() != rois.size(0):
        raise ValueError("mask_targets_padded: one gt index per roi expected")
    masks = [_resolve(m, rois.device) for m in gt_masks_list]
    return _launch(rois, gt, masks, mask_size, binarize)


def mask_target(pos_proposals_list, pos_assigned_gt_inds_list, gt_masks_list, cfg):
    """mask_target.py:7-64: the targets of all images, concatenated (an empty list comes back as the list)."""
    n = len(pos_proposals_list)
    if n == 0:
        return []
    assert len(pos_assigned_gt_inds_list) == n and len(gt_masks_list) == n
    mask_size = _check_size(_get(cfg, "mask_size"))
    binarize = not _get(cfg, "soft_mask_target", False)
    outs = []
    for i0 in range(0, n, MAX_IMAGES):
        props = pos_proposals_list[i0:i0 + MAX_IMAGES]
        for p in props:
            if p.dtype != torch.float32:
                raise NotImplementedError("mask_target: float32 proposals only (got %s)" % p.dtype)
        rois = torch.cat([torch.cat([p.new_full((p.size(0), 1), float(j)), p.detach()[:, :4]], dim=1) for j, p in enumerate(props)])
        gt = torch.cat([g.detach().reshape(-1).to(torch.int64) for g in pos_assigned_gt_inds_list[i0:i0 + MAX_IMAGES]])
        if rois.size(0) == 0:
            outs.append(rois.new_zeros((0,) + mask_size))
            continue
        _lib.require_gpu(rois, gt)
        masks = [_resolve(m, rois.device) for m in gt_masks_list[i0:i0 + MAX_IMAGES]]
        outs.append(_launch(rois, gt, masks, mask_size, binarize))
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def mask_target_single(pos_proposals, pos_assigned_gt_inds, gt_masks, cfg):
    """mask_target.py:67-127: ``[num_pos, mh, mw]``; no positives: ``new_zeros((0, mh, mw))``."""
    return mask_target([pos_proposals], [pos_assigned_gt_inds], [gt_masks], cfg)
