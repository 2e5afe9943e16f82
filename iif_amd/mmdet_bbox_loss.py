"""mmdet's box-regression losses ``L1Loss`` / ``SmoothL1Loss`` on the gfx950 kernels, and the regression half of
``BBoxHead.loss`` without its host round trips.

Mirror of instance_segmentation/mmdet/models/losses/smooth_l1_loss.py:10-146 + losses/utils.py:29-101 (constructors,
attributes, ``forward`` signatures, assertions and errors) and of roi_heads/bbox_heads/bbox_head.py:284-311.

  * ``l1_loss`` / ``smooth_l1_loss`` / the two modules: ``iif_bbox_reg_fwd`` (csrc/bbox_reg_head.hip) in plain mode, one
    launch for the loss, the gradient and, for ``reduction='none'``, the element losses; backward scales the saved
    gradient by the upstream scalar on the device.
  * ``bbox_head_reg_loss``: the same entry in gather mode - the kernel tests ``0 <= label < num_classes`` itself and reads
    the four deltas of a positive row's class out of ``bbox_pred [N, 4C]`` - and ``iif_bbox_reg_scatter_grad`` in
    backward, which writes the dense ``[N, 4C]`` gradient once, already scaled.  Two launches, no ``pos_inds.any()``, no
    ``nonzero``.

Forward plus backward never synchronise the host for 'mean' and 'sum' (``avg_factor`` a Python number).  When mmdet is
importable the classes register themselves as ``L1Loss`` / ``SmoothL1Loss``.
"""
import torch
import torch.nn as nn

from . import _lib
from . import custom
from .loss_reduction import check_reduction, reduction_scale, register_losses, scale_by_device_scalar


def _launch_fwd(pred, labels, num_classes, C, target, weight, beta, scale, want_grad, want_elems):
    """One launch of the forward kernel.  Plain mode (``labels`` None): ``pred`` / ``target`` / ``weight`` contiguous and
    of one shape.  Gather mode: ``pred [N, 4C]`` with unit column stride, ``target`` / ``weight`` contiguous ``[N, 4]``.
    Returns (loss, elems-or-None, dsel-or-None), the last two fp32 in ``target``'s shape."""
    dev = pred.device
    n = target.numel()
    N = labels.numel() if labels is not None else 0
    ld = pred.stride(0) if (labels is not None and N > 1) else 4 * C
    dsel = torch.empty(target.shape, dtype=torch.float32, device=dev) if want_grad else None
    elems = torch.empty(target.shape, dtype=torch.float32, device=dev) if want_elems else None
    loss = torch.empty((), dtype=torch.float32, device=dev)                  # written by the kernel (0 for n == 0)
    _, ticket, _ = custom._workspace(dev, 0, False)
    rc = _lib.lib().iif_bbox_reg_fwd(
        _lib.ptr(pred), _lib.dtype_code(pred), ld, _lib.ptr(labels), int(num_classes), int(C), _lib.ptr(target),
        _lib.ptr(weight), float(beta), float(scale), n, N, _lib.ptr(elems), _lib.ptr(loss), _lib.ptr(dsel), _lib.ptr(ticket),
        _lib.stream_ptr())
    _lib.check(rc, "iif_bbox_reg_fwd", ticket[:1])
    return loss, elems, dsel


class _FusedReg(torch.autograd.Function):
    """Scalar loss from ONE launch in plain mode; the gradient comes out of the same launch and backward only multiplies
    it by the upstream scalar on the device."""

    @staticmethod
    def forward(ctx, pred, target, weight, beta, scale):
        loss, _, dsel = _launch_fwd(pred, None, 1, 1, target, weight, beta, scale, ctx.needs_input_grad[0], False)
        ctx.save_for_backward(dsel)
        ctx.pred_dtype = pred.dtype
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        (dsel,) = ctx.saved_tensors
        if dsel is None:
            return (None,) * 5
        return (scale_by_device_scalar(dsel, g_loss, ctx.pred_dtype),) + (None,) * 4


class _FusedRegElems(torch.autograd.Function):
    """reduction='none' in plain mode: the element losses; backward scales the unit-scale gradient elementwise."""

    @staticmethod
    def forward(ctx, pred, target, weight, beta):
        _, elems, dsel = _launch_fwd(pred, None, 1, 1, target, weight, beta, 1.0, ctx.needs_input_grad[0], True)
        ctx.save_for_backward(dsel)
        ctx.pred_dtype = pred.dtype
        return elems

    @staticmethod
    def backward(ctx, g):
        (dsel,) = ctx.saved_tensors
        if dsel is None:
            return (None,) * 4
        return ((dsel * g.to(torch.float32)).to(ctx.pred_dtype),) + (None,) * 3


class _FusedRegGather(torch.autograd.Function):
    """``BBoxHead.loss``'s regression term: forward keeps the gradient compact (``[N, 4]``); backward writes the dense
    ``[N, 4C]`` gradient in one launch, scaled by the upstream scalar on the device."""

    @staticmethod
    def forward(ctx, pred, labels, target, weight, num_classes, C, beta, scale):
        loss, _, dsel = _launch_fwd(pred, labels, num_classes, C, target, weight, beta, scale, ctx.needs_input_grad[0], False)
        ctx.save_for_backward(dsel, labels)
        ctx.geom = (num_classes, C, pred.dtype, tuple(pred.shape))
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        dsel, labels = ctx.saved_tensors
        if dsel is None:
            return (None,) * 8
        num_classes, C, dtype, shape = ctx.geom
        g = g_loss.to(torch.float32).contiguous()
        N = labels.numel()
        dpred = torch.empty((N, 4 * C), dtype=dtype, device=dsel.device)
        rc = _lib.lib().iif_bbox_reg_scatter_grad(_lib.ptr(dsel), _lib.ptr(labels), int(num_classes), N, int(C), _lib.ptr(g),
                                                  _lib.ptr(dpred), _lib.dtype_code(dpred), 4 * C, _lib.stream_ptr())
        _lib.check(rc, "iif_bbox_reg_scatter_grad")
        return (dpred.view(shape),) + (None,) * 7


def _native_dtype(pred):
    return pred if pred.dtype in (torch.float32, torch.bfloat16) else pred.float()


def _reg_loss(pred, target, weight, beta, reduction, avg_factor, loss_weight=1.0):
    """``loss_weight *`` the weighted, reduced element loss of smooth_l1_loss.py:10-52 (``beta`` 0: L1) under
    weight_reduce_loss (losses/utils.py:29-55), ``loss_weight`` folded into the kernel's scale."""
    check_reduction(reduction, avg_factor)
    _lib.require_gpu(pred, target, weight)
    if target.numel() == 0:
        # the reference returns pred.sum() * 0 here, a 0-d zero, and THEN applies the weight and the reduction to it:
        # without a weight every reduction leaves the 0-d zero; an (empty) weight makes it an empty tensor, whose mean is
        # NaN and whose sum is 0
        zero = _FusedReg.apply(_native_dtype(pred).contiguous(), target, None, beta, 0.0)        # n == 0: no launch
        if weight is None:
            return zero
        if reduction == "none":
            return zero * weight.to(torch.float32)
        if reduction == "mean" and avg_factor is None and weight.numel() == 0:
            return zero * float("nan")              # torch: mean of an empty tensor
        return zero
    assert pred.size() == target.size()
    shape = pred.shape
    x = _native_dtype(pred).contiguous()
    t = target.to(torch.float32).contiguous()
    w = None if weight is None else weight.to(torch.float32).expand(shape).contiguous()
    if reduction == "none":                         # 'none' ignores avg_factor (utils.py:50-52)
        elems = _FusedRegElems.apply(x, t, w, beta)
        return elems if loss_weight == 1.0 else loss_weight * elems
    return _FusedReg.apply(x, t, w, beta, reduction_scale(reduction, avg_factor, x.numel(), loss_weight))     # (numel >= 1 here)


def smooth_l1_loss(pred, target, weight=None, reduction="mean", avg_factor=None, beta=1.0):
    """smooth_l1_loss.py:10-32 under ``weighted_loss``: one fused launch.  'none' returns the float32 element losses in
    ``pred``'s shape and ignores ``avg_factor``; 'sum' with an ``avg_factor`` raises ``ValueError``."""
    assert beta > 0
    return _reg_loss(pred, target, weight, beta, reduction, avg_factor)


def l1_loss(pred, target, weight=None, reduction="mean", avg_factor=None):
    """smooth_l1_loss.py:35-52 under ``weighted_loss``: one fused launch (the gradient at ``pred == target`` is 0)."""
    return _reg_loss(pred, target, weight, 0.0, reduction, avg_factor)


class SmoothL1Loss(nn.Module):
    """smooth_l1_loss.py:55-104."""

    def __init__(self, beta=1.0, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.beta = beta
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        assert self.beta > 0
        return _reg_loss(pred, target, weight, self.beta, reduction, avg_factor, self.loss_weight, **kwargs)


class L1Loss(nn.Module):
    """smooth_l1_loss.py:107-146."""

    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        return _reg_loss(pred, target, weight, 0.0, reduction, avg_factor, self.loss_weight)


def bbox_head_reg_loss(loss_bbox, bbox_pred, labels, bbox_targets, bbox_weights, num_classes, reg_class_agnostic=False,
                       reduction_override=None):
    """``losses['loss_bbox']`` of bbox_head.py:284-311 (``reg_decoded_bbox=False``; decode first otherwise), with
    ``avg_factor = bbox_targets.size(0)``.

    With a native ``L1Loss`` / ``SmoothL1Loss`` and the 'mean' reduction: one launch forward, one backward, no host
    synchronisation; a batch without positives gives 0.0 and an all-zero gradient.  'sum' raises ``ValueError`` (an
    ``avg_factor`` is always passed).  'none' has a data-dependent ``[P, 4]`` result, and any other ``loss_bbox`` object
    is not ours to fuse: both take the reference's formulation (boolean indexing, which synchronises) around
    ``loss_bbox``."""
    native = isinstance(loss_bbox, (L1Loss, SmoothL1Loss))
    if native:
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else loss_bbox.reduction
        check_reduction(reduction, bbox_targets.size(0))
    if not native or reduction == "none":
        pos_inds = (labels >= 0) & (labels < num_classes)
        if not pos_inds.any():
            return bbox_pred[pos_inds].sum()
        if reg_class_agnostic:
            pos_bbox_pred = bbox_pred.view(bbox_pred.size(0), 4)[pos_inds]
        else:
            pos_bbox_pred = bbox_pred.view(bbox_pred.size(0), -1, 4)[pos_inds, labels[pos_inds]]
        return loss_bbox(pos_bbox_pred, bbox_targets[pos_inds], bbox_weights[pos_inds], avg_factor=bbox_targets.size(0),
                         reduction_override=reduction_override)
    _lib.require_gpu(bbox_pred, labels, bbox_targets, bbox_weights)
    N = bbox_pred.size(0)
    x = _native_dtype(bbox_pred)
    if x.dim() != 2:
        raise ValueError("bbox_pred must be [N, 4C], got %s" % (tuple(bbox_pred.shape),))
    if reg_class_agnostic:
        if x.size(1) != 4:
            raise ValueError("a class-agnostic head predicts [N, 4], got %s" % (tuple(bbox_pred.shape),))
        C = 1
    else:
        C = x.size(1) // 4
        if x.size(1) != 4 * C or num_classes > C:
            raise ValueError("bbox_pred %s does not hold 4 deltas for each of %d classes" % (tuple(bbox_pred.shape), num_classes))
    if x.stride(1) != 1 or (N > 1 and x.stride(0) < 4 * C):
        x = x.contiguous()
    lab = labels.reshape(-1).to(torch.int64).contiguous()
    if lab.numel() != N or bbox_targets.numel() != 4 * N or bbox_weights.numel() != 4 * N:
        raise ValueError("one label, four targets and four weights per row expected: %d rows, %d labels, %s targets, %s weights"
                         % (N, lab.numel(), tuple(bbox_targets.shape), tuple(bbox_weights.shape)))
    t = bbox_targets.to(torch.float32).reshape(N, 4).contiguous()
    w = bbox_weights.to(torch.float32).reshape(N, 4).contiguous()
    beta = float(loss_bbox.beta) if isinstance(loss_bbox, SmoothL1Loss) else 0.0
    assert isinstance(loss_bbox, L1Loss) or beta > 0
    scale = loss_bbox.loss_weight / float(N) if N else 0.0
    return _FusedRegGather.apply(x, lab, t, w, int(num_classes), C, beta, scale)


def register_into_mmdet():
    """Register the native classes as mmdet's ``L1Loss`` / ``SmoothL1Loss`` if mmdet is importable."""
    return register_losses({"L1Loss": L1Loss, "SmoothL1Loss": SmoothL1Loss})


register_into_mmdet()
