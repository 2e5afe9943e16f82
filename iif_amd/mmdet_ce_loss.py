"""mmdet's ``CrossEntropyLoss`` family on the gfx950 kernels: the loss most detection configs name.

Mirror of instance_segmentation/mmdet/models/losses/cross_entropy_loss.py:10-249 and fasa_loss.py:9-101: the three
criteria ``cross_entropy`` / ``binary_cross_entropy`` / ``mask_cross_entropy`` and the classes ``CrossEntropyLoss`` and
``CrossEntropyCounterLoss`` with the reference's constructors, attributes and ``forward`` signatures.

  * ``cross_entropy`` (softmax): the fused ``iif_ce_fwd_bwd`` with an all-ones table (x * 1.0 is exact).
  * ``binary_cross_entropy`` (sigmoid): ``iif_bce_det_fwd_bwd`` (csrc/bce_head.hip), one launch for the loss, the
    gradient and, for ``reduction='none'``, the ``[N, C]`` element losses.  A label ``>= C`` is a background row, a
    label ``< 0`` or equal to ``ignore_index`` a row of weight zero, ``class_weight`` is a ``pos_weight``.
  * ``mask_cross_entropy``: ``mmdet_mask_loss.mask_cross_entropy``, as is.

Forward plus backward never synchronise the host for 'mean' and 'sum' (``avg_factor`` a Python number).  When mmdet is
importable the classes register themselves as ``CrossEntropyLoss`` / ``CrossEntropyCounterLoss``.
"""
import torch
import torch.nn as nn

from . import _lib
from . import custom
from .loss_reduction import check_reduction, reduction_scale, register_losses, scale_by_device_scalar
from .mmdet_mask_loss import mask_cross_entropy          # noqa: F401  (re-exported)

_ONES = {}


def _ones_table(device, C):
    t = _ONES.get((device, C))
    if t is None:
        t = _ONES[(device, C)] = torch.ones(C, dtype=torch.float32, device=device)
    return t


def cross_entropy(pred, label, weight=None, reduction="mean", avg_factor=None, class_weight=None, ignore_index=-100):
    """cross_entropy_loss.py:10-50 + losses/utils.py:29-55 in one fused launch: softmax cross entropy with per-class
    weights, ignore index, per-row weights; 'mean' divides by N (ignored rows included) or by ``avg_factor``."""
    ignore_index = -100 if ignore_index is None else ignore_index
    check_reduction(reduction, avg_factor)
    if reduction == "none":
        avg_factor = None            # 'none' ignores avg_factor (utils.py:50-52)
    _lib.require_gpu(pred)
    if pred.dim() != 2:
        raise ValueError("pred must be [N, C], got %s" % (tuple(pred.shape),))
    return custom.fused_iif_cross_entropy(pred, _ones_table(pred.device, pred.shape[1]), label, row_weight=weight,
                                          class_weight=class_weight, ignore_index=ignore_index, reduction=reduction,
                                          avg_factor=avg_factor)


def _empty_in_phase(pred, N, C, dtype):
    """An uninitialised contiguous ``[N, C]`` tensor whose 16-byte phase follows ``pred``'s: the element of ``pred`` that
    sits on a 16-byte boundary does so here too, which is what the kernel's 16-byte form asks of its outputs."""
    es = pred.element_size()
    h = ((16 - pred.data_ptr() % 16) % 16) // es if N * C else 0
    per16 = 128 // torch.finfo(dtype).bits
    off = (-h) % per16
    if off == 0:
        return torch.empty((N, C), dtype=dtype, device=pred.device)
    return torch.empty(N * C + off, dtype=dtype, device=pred.device)[off:].view(N, C)


def _launch_bce(pred, labels, row_weight, ignore_index, targets, elem_weight, class_weight, scale, want_grad, want_elems):
    """One launch of the detection BCE kernel.  Returns (loss, elems-or-None, dpred-or-None)."""
    _lib.require_gpu(pred, labels, row_weight, targets, elem_weight, class_weight)
    N, C = pred.shape
    x = pred
    if (C > 1 and x.stride(1) != 1) or (N > 1 and x.stride(0) < C):
        x = x.contiguous()
    ld = x.stride(0) if N > 1 else C
    dev = x.device
    if class_weight is not None:
        class_weight = class_weight.to(torch.float32).reshape(-1)
        if class_weight.numel() == 1:
            class_weight = class_weight.expand(C)
        if class_weight.numel() != C:
            raise ValueError("class_weight has %d entries, pred has %d channels" % (class_weight.numel(), C))
        class_weight = class_weight.contiguous()
    if labels is not None:
        labels = labels.reshape(-1).to(torch.int64).contiguous()
        if labels.numel() != N:
            raise ValueError("one label per row expected: %d labels, %d rows" % (labels.numel(), N))
        if row_weight is not None:
            row_weight = row_weight.reshape(-1).to(torch.float32).contiguous()
            if row_weight.numel() != N:
                raise ValueError("one weight per row expected: %d weights, %d rows" % (row_weight.numel(), N))
    else:
        targets = targets.to(torch.float32).contiguous()
        if elem_weight is not None:
            elem_weight = elem_weight.to(torch.float32).expand(N, C).contiguous()
    dense_rows = ld == C or N <= 1
    dpred = elems = None
    if want_grad:
        dpred = _empty_in_phase(x, N, C, x.dtype) if dense_rows else torch.empty((N, C), dtype=x.dtype, device=dev)
    if want_elems:
        elems = _empty_in_phase(x, N, C, torch.float32) if dense_rows else torch.empty((N, C), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)                  # written by the kernel (0 for N == 0)
    if N * C == 0:
        N, C, ld = 0, max(C, 1), max(C, 1)                                   # nothing to read: a zero loss, no launch
    _, ticket, _ = custom._workspace(dev, 0, False)
    rc = _lib.lib().iif_bce_det_fwd_bwd(
        _lib.ptr(x), _lib.dtype_code(x), ld, _lib.ptr(labels), _lib.ptr(row_weight), int(ignore_index), _lib.ptr(targets),
        _lib.ptr(elem_weight), _lib.ptr(class_weight), float(scale), N, C, _lib.ptr(elems), _lib.ptr(loss), _lib.ptr(dpred), C,
        _lib.ptr(ticket), _lib.stream_ptr())
    _lib.check(rc, "iif_bce_det_fwd_bwd", ticket[:1])
    return loss, elems, dpred


class _FusedBCE(torch.autograd.Function):
    """Scalar loss from ONE launch; d(loss)/d(pred) comes out of the same launch and backward only multiplies it by the
    upstream scalar on the device."""

    @staticmethod
    def forward(ctx, pred, labels, row_weight, ignore_index, targets, elem_weight, class_weight, scale):
        loss, _, dpred = _launch_bce(pred, labels, row_weight, ignore_index, targets, elem_weight, class_weight, scale,
                                     ctx.needs_input_grad[0], False)
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        (dpred,) = ctx.saved_tensors
        if dpred is None:
            return (None,) * 8
        return (scale_by_device_scalar(dpred, g_loss),) + (None,) * 7


class _FusedBCEElems(torch.autograd.Function):
    """reduction='none': the [N, C] element losses; backward scales the unit-scale gradient elementwise."""

    @staticmethod
    def forward(ctx, pred, labels, row_weight, ignore_index, targets, elem_weight, class_weight):
        _, elems, dpred = _launch_bce(pred, labels, row_weight, ignore_index, targets, elem_weight, class_weight, 1.0,
                                      ctx.needs_input_grad[0], True)
        ctx.save_for_backward(dpred)
        return elems

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        if dpred is None:
            return (None,) * 7
        return (dpred * g.to(dpred.dtype),) + (None,) * 6


def binary_cross_entropy(pred, label, weight=None, reduction="mean", avg_factor=None, class_weight=None,
                         ignore_index=-100):
    """cross_entropy_loss.py:53-111 + losses/utils.py:29-55 in one launch.

    ``label`` with fewer dimensions than ``pred`` holds one class index per row of ``pred [N, C]`` (``weight``: one
    value per row); with as many it is a float target per element (``weight``: per element, no ignore index).  'none'
    returns the float32 element losses in ``pred``'s shape and ignores ``avg_factor``; 'mean' over nothing is NaN."""
    ignore_index = -100 if ignore_index is None else ignore_index
    check_reduction(reduction, avg_factor)
    _lib.require_gpu(pred, label, weight)
    if pred.dtype not in (torch.float32, torch.bfloat16):
        pred = pred.float()
    shape = pred.shape
    if pred.dim() != label.dim():
        if pred.dim() != 2:
            raise ValueError("pred must be [N, C] with one label per row, got %s" % (tuple(shape),))
        x, modes = pred, (label, weight, ignore_index, None, None)
    else:
        if tuple(label.shape) != tuple(shape):
            raise ValueError("target shape %s differs from pred %s" % (tuple(label.shape), tuple(shape)))
        x = pred.reshape(-1, shape[-1]) if pred.dim() >= 1 else pred.reshape(1, 1)
        w = None if weight is None else weight.to(torch.float32).expand(shape).reshape(x.shape)
        modes = (None, None, ignore_index, label.reshape(x.shape), w)
    if reduction == "none":
        return _FusedBCEElems.apply(x, *modes, class_weight).view(shape)
    n = x.numel()
    loss = _FusedBCE.apply(x, *modes, class_weight, reduction_scale(reduction, avg_factor, n))
    if n == 0 and reduction == "mean" and avg_factor is None:
        return loss * float("nan")              # torch: mean of an empty tensor
    return loss


class _CEBase(nn.Module):
    def _pick_criterion(self):
        if self.use_sigmoid:
            self.cls_criterion = binary_cross_entropy
        elif self.use_mask:
            self.cls_criterion = mask_cross_entropy
        else:
            self.cls_criterion = cross_entropy

    def _class_weight(self, like):
        """The device copy of ``class_weight``, made once per device (the reference builds it on every call)."""
        if self.class_weight is None:
            return None
        cache = self.__dict__.setdefault("_cw_cache", {})
        hit = cache.get(like.device)
        if hit is None or hit[0] is not self.class_weight:
            hit = cache[like.device] = (self.class_weight,
                                        torch.as_tensor(self.class_weight, dtype=torch.float32).to(like.device))
        return hit[1]


class CrossEntropyLoss(_CEBase):
    """cross_entropy_loss.py:165-249, native in all three modes (softmax, ``use_sigmoid``, ``use_mask``)."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None, ignore_index=None,
                 loss_weight=1.0):
        super().__init__()
        assert (use_sigmoid is False) or (use_mask is False)
        self.use_sigmoid = use_sigmoid
        self.use_mask = use_mask
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.class_weight = class_weight
        self.ignore_index = ignore_index
        self._pick_criterion()

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, ignore_index=None,
                **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        if ignore_index is None:
            ignore_index = self.ignore_index
        return self.loss_weight * self.cls_criterion(cls_score, label, weight, class_weight=self._class_weight(cls_score),
                                                     reduction=reduction, avg_factor=avg_factor,
                                                     ignore_index=ignore_index, **kwargs)


def accumulate_per_class(loss_cls, label, num_classes, cum_losses, cum_labels):
    """fasa_loss.py:93-98 for every class at once on the device: ``cum_labels[c] += #{label == c}`` and ``cum_losses[c]
    += `` the sum of the 'none' losses of those rows (all columns of a row for the sigmoid loss).  No ``unique()``, no
    host loop."""
    rows = loss_cls.detach().float()
    if rows.dim() == 0:
        raise IndexError("the class counters need the reduction 'none' result, got a scalar loss")
    if rows.dim() > 1:
        rows = rows.reshape(rows.shape[0], -1).sum(dim=1)
    rows = rows.contiguous()
    lb = label.reshape(-1).to(torch.int64).contiguous()
    if lb.numel() != rows.numel():
        raise ValueError("one label per row expected: %d labels, %d rows" % (lb.numel(), rows.numel()))
    _lib.check(_lib.lib().iif_class_accumulate(_lib.ptr(rows), _lib.ptr(lb), rows.numel(), num_classes + 1,
                                               _lib.ptr(cum_losses), _lib.ptr(cum_labels), _lib.stream_ptr()),
               "iif_class_accumulate")


class CrossEntropyCounterLoss(_CEBase):
    """fasa_loss.py:9-101: ``CrossEntropyLoss`` plus, while the counters are open (``open_cums`` ... ``close_cums``),
    per-class sums of the 'none' losses and label counts; the returned value is then the mean of the 'none' result.
    ``device``: where the counters live (the reference's ``.cuda()``)."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None, loss_weight=1.0,
                 use_cums=False, num_classes=1203, device="cuda"):
        super().__init__()
        assert (use_sigmoid is False) or (use_mask is False)
        self.use_sigmoid = use_sigmoid
        self.use_mask = use_mask
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.class_weight = class_weight
        self._pick_criterion()
        self.num_classes = num_classes
        self._device = device
        self.use_cums = use_cums
        if self.use_cums:
            self.open_cums()

    def open_cums(self):
        self.use_cums = True
        self.reduction_old = self.reduction
        self.reduction = "none"
        self.cum_losses = torch.zeros(self.num_classes + 1, device=self._device)
        self.cum_labels = torch.zeros(self.num_classes + 1, device=self._device)

    def close_cums(self):
        self.use_cums = False
        self.reduction = self.reduction_old
        self.cum_losses = torch.zeros(self.num_classes + 1, device=self._device)
        self.cum_labels = torch.zeros(self.num_classes + 1, device=self._device)

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        loss_cls = self.loss_weight * self.cls_criterion(cls_score, label, weight,
                                                         class_weight=self._class_weight(cls_score),
                                                         reduction=reduction, avg_factor=avg_factor, **kwargs)
        if self.use_cums:
            if self.cum_losses.device != cls_score.device:
                self.cum_losses = self.cum_losses.to(cls_score.device)
                self.cum_labels = self.cum_labels.to(cls_score.device)
            accumulate_per_class(loss_cls, label, self.num_classes, self.cum_losses, self.cum_labels)
            loss_cls = loss_cls.mean()
        return loss_cls


def register_into_mmdet():
    """Register the native classes as mmdet's ``CrossEntropyLoss`` / ``CrossEntropyCounterLoss`` if mmdet is importable."""
    return register_losses({"CrossEntropyLoss": CrossEntropyLoss, "CrossEntropyCounterLoss": CrossEntropyCounterLoss})


register_into_mmdet()
