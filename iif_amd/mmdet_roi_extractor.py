"""mmdet's ``SingleRoIExtractor`` and mmcv's ``RoIAlign`` on the gfx950 kernels (csrc/roi_align.hip): the step after
``bbox_targets`` (mmdet_targets.py) hands back its ``rois``.

Mirror of instance_segmentation/mmdet/models/roi_heads/roi_extractors/base_roi_extractor.py:10-88 and
single_level_roi_extractor.py:9-115 (constructors, attributes, the empty result) and of ``mmcv.ops.RoIAlign`` /
``mmcv.ops.roi_align`` (arguments, defaults, attribute names).

  * ``SingleRoIExtractor.forward``: ``iif_roi_extract_forward``, ONE launch for all levels - level mapping, optional rescaling,
    RoIAlign and the scatter into ``[K, C, PH, PW]`` - where the reference runs, per level, a ``nonzero`` (a host
    synchronisation), a gather, a RoIAlign launch and an ``index_put``.  Under autograd the backward is
    ``iif_roi_extract_backward``: one clear of one arena that holds every level's gradient, one launch of float atomic adds.
    Neither direction synchronises the host.  A level no roi maps to gets an all-zero gradient (the reference's
    ``feats[i].sum() * 0.`` terms).
  * ``roi_align`` / ``RoIAlign``: the one-level case of the same entries.
  * ``extract_forward`` / ``extract_backward``: the two entries as functions, without autograd.

Layout: the kernels read features as NHWC (``torch.channels_last``).  A level that is already channels-last is read in place;
an NCHW-contiguous level costs one ``contiguous(memory_format=torch.channels_last)`` copy per call
(``neck.to(memory_format=torch.channels_last)`` removes it).  Gradients come back with channels-last strides.

Rows that give zeros and no gradient: a batch index outside ``[0, N)`` (a way to mark padding in fixed-length roi lists), a
NaN scale (negative area product; the reference leaves that row at its ``new_zeros`` value), non-finite coordinates.

Deliberately not offered, raising instead of falling back: ``pool_mode='max'``, features that are not float32, levels with
different ``N`` or ``C``, more than 8 levels, ``GenericRoIExtractor``, the ONNX export branches, a gradient with respect to
``rois``.  When mmdet is importable ``SingleRoIExtractor`` registers itself in ``ROI_EXTRACTORS``.
"""
import torch
import torch.nn as nn

from . import _lib

MAX_LEVELS = 8


def _pair(v):
    if isinstance(v, int):
        return (v, v)
    v = tuple(int(x) for x in v)
    if len(v) != 2:
        raise AssertionError("output_size: an int or a pair expected (got %r)" % (v,))
    return v


def _check_levels(feats):
    feats = list(feats)
    if not 1 <= len(feats) <= MAX_LEVELS:
        raise NotImplementedError("roi extraction: 1 .. %d feature levels are offered (got %d)" % (MAX_LEVELS, len(feats)))
    for f in feats:
        if f.dim() != 4:
            raise AssertionError("roi extraction: [N, C, H, W] features expected (got %s)" % (tuple(f.shape),))
        if f.dtype != torch.float32:
            raise NotImplementedError("roi extraction: float32 features only (got %s); there is no half-precision kernel" % f.dtype)
        if f.shape[:2] != feats[0].shape[:2]:
            raise NotImplementedError("roi extraction: every level needs the same N and C (got %s and %s)"
                                      % (tuple(feats[0].shape), tuple(f.shape)))
    return feats


def _levels_nhwc(feats):
    """The levels as channels-last tensors (no copy where they already are), after the checks."""
    feats = _check_levels(feats)
    _lib.require_gpu(*feats)
    return [f if f.is_contiguous(memory_format=torch.channels_last) else f.contiguous(memory_format=torch.channels_last) for f in feats]


def _rois5(rois):
    if rois.dim() != 2 or rois.size(1) != 5:
        raise AssertionError("rois: [K, 5] rows of (batch index, x1, y1, x2, y2) expected (got %s)" % (tuple(rois.shape),))
    if rois.dtype != torch.float32:
        raise NotImplementedError("rois: float32 only (got %s)" % rois.dtype)
    if rois.requires_grad:
        raise RuntimeError("roi extraction: a gradient with respect to rois is not offered; detach them")
    if rois.size(0) > 1 and (rois.stride(1) != 1 or rois.stride(0) < 5):
        rois = rois.contiguous()
    elif rois.size(0) <= 1 and rois.stride(1) != 1:
        rois = rois.contiguous()
    return rois, (rois.stride(0) if rois.size(0) > 1 else 5)


def _level_array(tensors, shapes, scales):
    arr = (_lib.RoiLevel * len(shapes))()
    for i, ((H, W), s) in enumerate(zip(shapes, scales)):
        arr[i].ptr = tensors[i].data_ptr()
        arr[i].H, arr[i].W, arr[i].spatial_scale = H, W, float(s)
    return arr


class _Geometry:
    """What both entries take besides the tensors."""

    def __init__(self, output_size, spatial_scales, sampling_ratio, aligned, finest_scale, roi_scale_factor):
        self.out = _pair(output_size)
        self.scales = tuple(float(s) for s in spatial_scales)
        self.sampling_ratio = int(sampling_ratio)
        self.aligned = bool(aligned)
        self.finest_scale = float(finest_scale)
        self.factor = 0.0 if roi_scale_factor is None else float(roi_scale_factor)
        if roi_scale_factor is not None and not self.factor > 0:
            raise AssertionError("roi_scale_factor must be positive (got %r)" % (roi_scale_factor,))

    def tail(self):
        return (self.out[0], self.out[1], self.sampling_ratio, int(self.aligned), self.finest_scale, self.factor)


def _forward(levels, rois, ld, geo, channels_last_out, want_levels):
    N, C = levels[0].shape[:2]
    K = rois.size(0)
    PH, PW = geo.out
    out = torch.empty((K, C, PH, PW), dtype=torch.float32, device=rois.device,
                      memory_format=torch.channels_last if channels_last_out else torch.contiguous_format)
    lvls = torch.empty((K,), dtype=torch.int32, device=rois.device) if want_levels else None
    if K > 0:
        if len(geo.scales) != len(levels):
            raise AssertionError("one spatial scale per level expected")
        arr = _level_array(levels, [f.shape[2:] for f in levels], geo.scales)
        rc = _lib.lib().iif_roi_extract_forward(arr, len(levels), N, C, _lib.ptr(rois), ld, K, *geo.tail(), _lib.ptr(out),
                                                int(channels_last_out), _lib.ptr(lvls), _lib.stream_ptr())
        _lib.check(rc, "iif_roi_extract_forward")
    return out, lvls


def _backward(shapes, N, C, rois, ld, geo, grad_out):
    """Channels-last gradients (views of ONE arena) for levels of spatial ``shapes``."""
    sizes = [N * H * W * C for H, W in shapes]
    K = rois.size(0)
    arena = (torch.empty if K > 0 else torch.zeros)((sum(sizes),), dtype=torch.float32, device=grad_out.device)
    grads, off = [], 0
    for (H, W), n in zip(shapes, sizes):
        grads.append(arena[off:off + n].view(N, H, W, C).permute(0, 3, 1, 2))
        off += n
    if K > 0:
        if grad_out.is_contiguous():
            cl = False
        elif grad_out.is_contiguous(memory_format=torch.channels_last):
            cl = True
        else:
            grad_out, cl = grad_out.contiguous(), False
        arr = _level_array(grads, shapes, geo.scales)
        rc = _lib.lib().iif_roi_extract_backward(arr, len(shapes), N, C, _lib.ptr(rois), ld, K, *geo.tail(), _lib.ptr(grad_out),
                                                 int(cl), _lib.ptr(arena), arena.numel() * 4, _lib.stream_ptr())
        _lib.check(rc, "iif_roi_extract_backward")
    return grads


def extract_forward(feats, rois, output_size, spatial_scales, sampling_ratio=0, aligned=True, finest_scale=56,
                    roi_scale_factor=None, channels_last_out=False, return_levels=False):
    """``iif_roi_extract_forward`` on ``feats`` (a sequence of ``[N, C, H, W]`` levels) and ``rois [K, 5]``, no autograd:
    ``[K, C, PH, PW]`` (with channels-last strides if asked), and with ``return_levels`` the int32 level of every roi (-1 for
    a NaN scale)."""
    _check_levels(feats)
    rois, ld = _rois5(rois)
    _lib.require_gpu(rois)
    levels = _levels_nhwc([f.detach() for f in feats])
    out, lvls = _forward(levels, rois, ld, _Geometry(output_size, spatial_scales, sampling_ratio, aligned, finest_scale,
                                                     roi_scale_factor), channels_last_out, return_levels)
    return (out, lvls) if return_levels else out


def extract_backward(feat_shapes, rois, grad_out, output_size, spatial_scales, sampling_ratio=0, aligned=True, finest_scale=56,
                     roi_scale_factor=None):
    """``iif_roi_extract_backward``: one gradient (channels-last strides) per level of shape ``feat_shapes[i] = (N, C, H, W)``
    for ``grad_out [K, C, PH, PW]`` (NCHW-contiguous or channels-last)."""
    N, C = feat_shapes[0][:2]
    rois, ld = _rois5(rois)
    _lib.require_gpu(rois, grad_out)
    return _backward([tuple(s[2:]) for s in feat_shapes], N, C, rois, ld,
                     _Geometry(output_size, spatial_scales, sampling_ratio, aligned, finest_scale, roi_scale_factor), grad_out)


class _Extract(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rois, ld, geo, *feats):
        levels = _levels_nhwc(feats)
        out, _ = _forward(levels, rois, ld, geo, False, False)
        ctx.rois, ctx.ld, ctx.geo = rois, ld, geo
        ctx.shapes = [tuple(f.shape[2:]) for f in levels]
        ctx.nc = tuple(levels[0].shape[:2])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        grads = _backward(ctx.shapes, ctx.nc[0], ctx.nc[1], ctx.rois, ctx.ld, ctx.geo, grad_out)
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))


def _extract(feats, rois, geo):
    _check_levels(feats)
    rois, ld = _rois5(rois)
    _lib.require_gpu(rois, *feats)
    return _Extract.apply(rois, ld, geo, *feats)


def roi_align(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True):
    """``mmcv.ops.roi_align`` for a float32 ``[N, C, H, W]`` input and ``rois [K, 5]``: ``[K, C, PH, PW]``, differentiable
    in ``input``."""
    if pool_mode != 'avg':
        raise NotImplementedError("roi_align: pool_mode=%r is not offered (only 'avg' has a kernel)" % (pool_mode,))
    assert rois.size(1) == 5, 'RoI must be (idx, x1, y1, x2, y2)!'
    return _extract([input], rois, _Geometry(output_size, (spatial_scale,), sampling_ratio, aligned, 56, None))


class RoIAlign(nn.Module):
    """``mmcv.ops.RoIAlign``: the same arguments, defaults and attribute names.  ``use_torchvision`` is accepted and ignored
    (torchvision's operator is the same definition as ``aligned``'s two settings); ``pool_mode='max'`` raises."""

    def __init__(self, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True, use_torchvision=False):
        super().__init__()
        if pool_mode != 'avg':
            raise NotImplementedError("RoIAlign: pool_mode=%r is not offered (only 'avg' has a kernel)" % (pool_mode,))
        self.output_size = _pair(output_size)
        self.spatial_scale = float(spatial_scale)
        self.sampling_ratio = int(sampling_ratio)
        self.pool_mode = pool_mode
        self.aligned = aligned
        self.use_torchvision = use_torchvision

    def forward(self, input, rois):
        return roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio, self.pool_mode, self.aligned)

    def __repr__(self):
        s = self.__class__.__name__
        s += '(output_size=%s, ' % (self.output_size,)
        s += 'spatial_scale=%s, ' % self.spatial_scale
        s += 'sampling_ratio=%s, ' % self.sampling_ratio
        s += 'pool_mode=%s, ' % self.pool_mode
        s += 'aligned=%s, ' % self.aligned
        s += 'use_torchvision=%s)' % self.use_torchvision
        return s


class SingleRoIExtractor(nn.Module):
    """single_level_roi_extractor.py:9-115 in one launch.  ``roi_layer``: ``dict(type='RoIAlign', output_size=..,
    sampling_ratio=.., ...)``; any other type raises."""

    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg
        self.roi_layers = self.build_roi_layers(roi_layer, featmap_strides)
        self.out_channels = out_channels
        self.featmap_strides = featmap_strides
        self.fp16_enabled = False
        self.finest_scale = finest_scale

    @property
    def num_inputs(self):
        """int: Number of input feature maps."""
        return len(self.featmap_strides)

    def build_roi_layers(self, layer_cfg, featmap_strides):
        cfg = layer_cfg.copy()
        layer_type = cfg.pop('type')
        if layer_type != 'RoIAlign':
            raise NotImplementedError("SingleRoIExtractor: roi_layer type %r is not offered (only RoIAlign has a kernel)" % (layer_type,))
        if len(featmap_strides) > MAX_LEVELS:
            raise NotImplementedError("SingleRoIExtractor: at most %d levels (got %d)" % (MAX_LEVELS, len(featmap_strides)))
        return nn.ModuleList([RoIAlign(spatial_scale=1 / s, **cfg) for s in featmap_strides])

    def map_roi_levels(self, rois, num_levels):
        """single_level_roi_extractor.py:37-58 in torch ops (the kernel does this itself; kept for callers of the method)."""
        scale = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
        target_lvls = torch.floor(torch.log2(scale / self.finest_scale + 1e-6))
        return target_lvls.clamp(min=0, max=num_levels - 1).long()

    def roi_rescale(self, rois, scale_factor):
        """base_roi_extractor.py:62-84 in torch ops (the kernel does this itself; kept for callers of the method)."""
        cx = (rois[:, 1] + rois[:, 3]) * 0.5
        cy = (rois[:, 2] + rois[:, 4]) * 0.5
        w = rois[:, 3] - rois[:, 1]
        h = rois[:, 4] - rois[:, 2]
        new_w = w * scale_factor
        new_h = h * scale_factor
        return torch.stack((rois[:, 0], cx - new_w * 0.5, cy - new_h * 0.5, cx + new_w * 0.5, cy + new_h * 0.5), dim=-1)

    def forward(self, feats, rois, roi_scale_factor=None):
        if torch.onnx.is_in_onnx_export():
            raise NotImplementedError("SingleRoIExtractor: the ONNX export branches are not offered")
        num_levels = len(feats)
        if num_levels > len(self.roi_layers):
            raise AssertionError("SingleRoIExtractor: %d feature levels for %d strides" % (num_levels, len(self.roi_layers)))
        layer = self.roi_layers[0]
        if feats[0].size(1) != self.out_channels:
            raise AssertionError("SingleRoIExtractor: features have %d channels, out_channels is %d" % (feats[0].size(1), self.out_channels))
        # one level: the reference calls its RoIAlign directly, without level mapping and without rescaling
        factor = roi_scale_factor if num_levels > 1 else None
        geo = _Geometry(layer.output_size, [l.spatial_scale for l in self.roi_layers[:num_levels]], layer.sampling_ratio,
                        layer.aligned, self.finest_scale, factor)
        return _extract(list(feats), rois, geo)


class GenericRoIExtractor(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("GenericRoIExtractor is not offered (no kernel sums levels); use SingleRoIExtractor")


def register_into_mmdet():
    """Register the native class as mmdet's ``SingleRoIExtractor`` if mmdet is importable."""
    try:
        from mmdet.models.builder import ROI_EXTRACTORS
    except Exception:
        return False
    ROI_EXTRACTORS.register_module(name="SingleRoIExtractor", force=True, module=SingleRoIExtractor)
    return True


register_into_mmdet()
