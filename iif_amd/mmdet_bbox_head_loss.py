"""``BBoxHead.loss`` without a host read: the classification half with ``avg_factor`` counted on the device, joined with the
regression half of ``mmdet_bbox_loss.bbox_head_reg_loss``.

Mirror of instance_segmentation/mmdet/models/roi_heads/bbox_heads/bbox_head.py:256-312.  The reference opens that function
with ``avg_factor = max(torch.sum(label_weights > 0).float().item(), 1.)``: two launches and a host read, once per image
batch and once per cascade stage, and with the padded rows of ``roi_stage_targets_padded`` the count cannot be a host number.

  * ``head_cls_loss``: ``iif_head_loss_fwd`` (csrc/head_loss.hip), ONE launch for the loss, the device-counted
    ``avg_factor``, the top-1 accuracy over the rows with ``label_weights > 0`` and the gradient without its
    ``loss_weight / avg_factor`` factor; backward is ONE launch (``iif_head_loss_bwd``) that applies
    ``upstream * loss_weight / avg_factor`` from device scalars.  Native for our ``IIFLoss`` and our softmax
    ``CrossEntropyLoss`` under the 'mean' reduction.  The sigmoid mode (``iif_head_bce_loss_fwd``, the same file) and our
    ``SeesawLoss`` (``iif_seesaw_head_fwd`` / ``_bwd``, csrc/seesaw_head.hip, with both accuracies and the ``cum_samples``
    update) are native in the same way.
  * ``bbox_head_loss``: all of ``BBoxHead.loss``, the reference's keys and ``None`` handling.

Differences from the reference on the native path, both deliberate ("BBoxHead.loss"):
  * a row with ``label_weights == 0`` is not read.  The reference computes ``0 * nll``, which is NaN for a non-finite
    padding row, and its ``accuracy`` divides the hits by ALL rows, padding included; here the accuracy is over the rows
    with ``label_weights > 0``, the rows ``avg_factor`` counts.  Without zero-weight rows the two agree bit for bit.
  * a label outside ``[0, C)`` that is not the ignore index contributes zero and sets the device flag that
    ``custom.check_label_status()`` reports (the reference asserts inside ``nll_loss``).
"""
import torch

from . import _lib
from . import custom
from .mmdet_bbox_loss import bbox_head_reg_loss
from .mmdet_ce_loss import CrossEntropyLoss
from . import mmdet_seesaw_loss as seesaw
from .mmdet_iif_loss import IIFLoss
from .mmdet_seesaw_loss import SeesawLoss
from .utils import topk_hit_counts

__all__ = ["head_cls_loss", "bbox_head_loss", "MAX_CLASSES", "MAX_ROWS"]

MAX_CLASSES = 2048          # IIF_HEAD_LOSS_MAX_CLASSES (the Seesaw head: C + 2 columns)
MAX_ROWS = 65535            # IIF_HEAD_LOSS_MAX_ROWS
SEESAW_HEAD_WORKSPACE_WORDS = 4 + 2048 + 4 + 4 * 1024          # IIF_SEESAW_HEAD_WORKSPACE_BYTES / 4


class _HeadClsLoss(torch.autograd.Function):
    """(loss, acc, avg_factor) from one launch; the saved gradient lacks ``loss_weight / avg_factor``, which backward applies
    together with the upstream scalar, all three read on the device.  The saved tensors stay intact: backward may run twice."""

    @staticmethod
    def forward(ctx, x, table, labels, weights, class_weight, ignore_index, loss_weight):
        N, C = x.shape
        dev = x.device
        f32 = torch.float32
        loss = torch.empty((), dtype=f32, device=dev)
        acc = torch.empty((1,), dtype=f32, device=dev)               # accuracy.py:49-51: a one-element tensor
        avg = torch.empty((), dtype=f32, device=dev)
        du = torch.empty((N, C), dtype=x.dtype, device=dev) if ctx.needs_input_grad[0] else None
        _, ticket, status = custom._workspace(dev, 0, False)
        rc = _lib.lib().iif_head_loss_fwd(
            _lib.ptr(x), _lib.dtype_code(x), x.stride(0) if N > 1 else C, _lib.ptr(table), _lib.ptr(labels), _lib.ptr(weights),
            _lib.ptr(class_weight), int(ignore_index), float(loss_weight), N, C, _lib.ptr(du), C, _lib.ptr(loss), _lib.ptr(acc),
            _lib.ptr(avg), _lib.ptr(status), _lib.ptr(ticket), _lib.stream_ptr())
        _lib.check(rc, "iif_head_loss_fwd", ticket[:1])
        ctx.save_for_backward(du, avg)
        ctx.loss_weight = float(loss_weight)
        ctx.mark_non_differentiable(acc, avg)
        return loss, acc, avg

    @staticmethod
    def backward(ctx, g_loss, g_acc, g_avg):
        return (_scaled_gradient(ctx, g_loss),) + (None,) * 6


def _scaled_gradient(ctx, g_loss):
    """``saved gradient * (upstream * loss_weight / avg_factor)`` in one launch (``iif_head_loss_bwd``), or None."""
    du, avg = ctx.saved_tensors
    if du is None:
        return None
    g = g_loss.to(torch.float32).contiguous()
    out = torch.empty_like(du)
    rc = _lib.lib().iif_head_loss_bwd(_lib.ptr(du), _lib.dtype_code(du), du.numel(), _lib.ptr(g), _lib.ptr(avg), ctx.loss_weight,
                                      _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "iif_head_loss_bwd")
    return out


class _HeadBceLoss(torch.autograd.Function):
    """``_HeadClsLoss`` for the sigmoid head (``iif_head_bce_loss_fwd``); the backward launch is the same."""

    @staticmethod
    def forward(ctx, x, labels, weights, class_weight, ignore_index, loss_weight):
        N, C = x.shape
        dev = x.device
        f32 = torch.float32
        loss = torch.empty((), dtype=f32, device=dev)
        acc = torch.empty((1,), dtype=f32, device=dev)
        avg = torch.empty((), dtype=f32, device=dev)
        du = torch.empty((N, C), dtype=x.dtype, device=dev) if ctx.needs_input_grad[0] else None
        _, ticket, _ = custom._workspace(dev, 0, False)
        rc = _lib.lib().iif_head_bce_loss_fwd(
            _lib.ptr(x), _lib.dtype_code(x), x.stride(0) if N > 1 else C, _lib.ptr(labels), _lib.ptr(weights), _lib.ptr(class_weight),
            int(ignore_index), float(loss_weight), N, C, _lib.ptr(du), C, _lib.ptr(loss), _lib.ptr(acc), _lib.ptr(avg),
            _lib.ptr(ticket), _lib.stream_ptr())
        _lib.check(rc, "iif_head_bce_loss_fwd", ticket[:1])
        ctx.save_for_backward(du, avg)
        ctx.loss_weight = float(loss_weight)
        ctx.mark_non_differentiable(acc, avg)
        return loss, acc, avg

    @staticmethod
    def backward(ctx, g_loss, g_acc, g_avg):
        return (_scaled_gradient(ctx, g_loss),) + (None,) * 5


class _HeadSeesawLoss(torch.autograd.Function):
    """``iif_seesaw_head_fwd``: two launches for both losses (or their sum, ``summed``), both accuracies, the device-counted
    ``avg_factor``, the ``cum_samples`` update and the unit-scale gradient; backward is ONE launch (``iif_seesaw_head_bwd``)
    that applies ``upstream * loss_weight / avg_factor`` per column group from device scalars.  Backward may run twice."""

    @staticmethod
    def forward(ctx, x, labels, weights, cum, p, q, eps, loss_weight, summed):
        N, C = x.shape[0], x.shape[1] - 2
        dev = x.device
        f32 = torch.float32
        losses = torch.empty(3, dtype=f32, device=dev)
        acc = torch.empty(2, dtype=f32, device=dev)
        avg = torch.empty((), dtype=f32, device=dev)
        d = torch.empty((N, C + 2), dtype=f32, device=dev) if ctx.needs_input_grad[0] else None
        stream = _lib.stream_ptr()
        ws = seesaw._workspace(dev, stream)
        if "head" not in ws:
            ws["head"] = torch.zeros(SEESAW_HEAD_WORKSPACE_WORDS, dtype=torch.int32, device=dev)
        rc = _lib.lib().iif_seesaw_head_fwd(
            _lib.ptr(x), _lib.dtype_code(x), x.stride(0) if N > 1 else C + 2, _lib.ptr(labels), _lib.ptr(weights), _lib.ptr(cum),
            float(p), float(q), float(eps), float(loss_weight), N, C, _lib.ptr(d), C + 2, _lib.ptr(losses), _lib.ptr(acc),
            _lib.ptr(avg), _lib.ptr(ws["status"]), _lib.ptr(ws["head"]), stream)
        _lib.check(rc, "iif_seesaw_head_fwd", ws["head"][:2])
        ctx.save_for_backward(d, avg)
        ctx.loss_weight, ctx.C, ctx.summed = float(loss_weight), C, summed
        ctx.set_materialize_grads(False)
        acc_obj, acc_cls = acc[0:1], acc[1:2]
        ctx.mark_non_differentiable(acc_obj, acc_cls, avg)
        if summed:
            return losses[2], acc_obj, acc_cls, avg
        return losses[0], losses[1], acc_obj, acc_cls, avg

    @staticmethod
    def backward(ctx, *grads):
        d, avg = ctx.saved_tensors
        if d is None:
            return (None,) * 9
        g_cls, g_obj = (grads[0], grads[0]) if ctx.summed else grads[:2]
        gc, go = (torch.zeros_like(avg) if g is None else g.to(torch.float32).contiguous() for g in (g_cls, g_obj))
        out = torch.empty_like(d)
        rc = _lib.lib().iif_seesaw_head_bwd(_lib.ptr(d), ctx.C + 2, d.shape[0], ctx.C, _lib.ptr(gc), _lib.ptr(go), _lib.ptr(avg),
                                            ctx.loss_weight, _lib.ptr(out), ctx.C + 2, _lib.stream_ptr())
        _lib.check(rc, "iif_seesaw_head_bwd")
        return (out,) + (None,) * 8


def _is_native(loss_cls, reduction_override):
    """Our IIFLoss, or our CrossEntropyLoss in its softmax mode, reducing with 'mean'."""
    if isinstance(loss_cls, IIFLoss):
        pass
    elif isinstance(loss_cls, CrossEntropyLoss) and not loss_cls.use_sigmoid and not loss_cls.use_mask:
        pass
    else:
        return False
    assert reduction_override in (None, "none", "mean", "sum")
    return (reduction_override if reduction_override else loss_cls.reduction) == "mean"


def _native_kind(loss_cls, reduction_override):
    """Which kernel serves ``loss_cls`` under the 'mean' reduction: 'softmax' (exactly where ``_is_native`` holds: every
    ``IIFLoss`` instance, ``FasaIIFLoss`` with its flags included, and our softmax ``CrossEntropyLoss``), 'sigmoid' (our
    ``CrossEntropyLoss(use_sigmoid=True)``), 'seesaw' (our ``SeesawLoss``), or None: ``use_mask``, ``CrossEntropyCounterLoss``,
    a module that is not ours, the reductions 'none' / 'sum'."""
    if _is_native(loss_cls, reduction_override):
        return "softmax"
    if isinstance(loss_cls, CrossEntropyLoss):
        kind = "sigmoid" if loss_cls.use_sigmoid and not loss_cls.use_mask else None
    elif isinstance(loss_cls, SeesawLoss):
        kind = "seesaw"
    else:
        kind = None
    if kind is None or (reduction_override if reduction_override else loss_cls.reduction) != "mean":
        return None
    return kind


def _within_limits(kind, loss_cls, cls_score, labels, label_weights):
    """Whether the sigmoid / Seesaw kernels take this call; otherwise it keeps the reference's lines and their host read."""
    if cls_score.dim() != 2 or cls_score.shape[1] > MAX_CLASSES or cls_score.shape[0] > MAX_ROWS:
        return False
    if cls_score.dtype not in ((torch.float32, torch.bfloat16) if kind == "sigmoid" else (torch.float32,)):
        return False
    if kind == "seesaw" and cls_score.shape[1] != loss_cls.num_classes + 2:
        return False
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        return False
    return label_weights is None or label_weights.dtype in (torch.float32, torch.bfloat16, torch.float16)


def _class_weight(loss_cls, like):
    """The device copy of ``loss_cls.class_weight``, made once per device (not on every call, as the reference does)."""
    if loss_cls.class_weight is None:
        return None
    if hasattr(loss_cls, "_class_weight"):                  # CrossEntropyLoss keeps its own
        return loss_cls._class_weight(like)
    cache = loss_cls.__dict__.setdefault("_head_loss_cw", {})
    hit = cache.get(like.device)
    if hit is None or hit[0] is not loss_cls.class_weight:
        hit = cache[like.device] = (loss_cls.class_weight, torch.as_tensor(loss_cls.class_weight, dtype=torch.float32).to(like.device))
    return hit[1]


def _prep(loss_cls, cls_score, labels, label_weights):
    """Checked, kernel-ready arguments of the native path: (x, table, labels, weights, class_weight, ignore_index)."""
    _lib.require_gpu(cls_score, labels, label_weights)
    if cls_score.dim() != 2:
        raise ValueError("cls_score must be [N, C], got %s" % (tuple(cls_score.shape),))
    N, C = cls_score.shape
    if C < 2:
        raise ValueError("a softmax head has at least 2 channels, got %s" % (tuple(cls_score.shape),))
    if labels.numel() != N or label_weights.numel() != N:
        raise ValueError("one label and one weight per row expected: %d rows, %d labels, %d weights"
                         % (N, labels.numel(), label_weights.numel()))
    what = type(loss_cls).__name__
    if cls_score.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError("head_cls_loss: float32 / bfloat16 scores only (got %s); call %s.forward and get_accuracy "
                                  "(loss_cls.forward) with a host avg_factor instead" % (cls_score.dtype, what))
    if labels.dtype.is_floating_point or labels.dtype == torch.bool or label_weights.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise NotImplementedError("head_cls_loss: integer labels and float32 / half weights only (got %s, %s); call %s.forward "
                                  "(loss_cls.forward) with a host avg_factor instead" % (labels.dtype, label_weights.dtype, what))
    if C > MAX_CLASSES or N > MAX_ROWS:
        raise NotImplementedError("head_cls_loss: at most %d channels and %d rows (got %s); call %s.forward and get_accuracy "
                                  "(loss_cls.forward) with a host avg_factor instead" % (MAX_CLASSES, MAX_ROWS, tuple(cls_score.shape), what))
    table = None
    if isinstance(loss_cls, IIFLoss):
        table = loss_cls._table(cls_score).reshape(-1).to(torch.float32).contiguous()
        if table.numel() != C:
            raise ValueError("the IIF table has %d classes, cls_score has %d channels" % (table.numel(), C))
    cw = _class_weight(loss_cls, cls_score)
    if cw is not None:
        cw = cw.reshape(-1).to(torch.float32).contiguous()
        if cw.numel() != C:
            raise ValueError("class_weight has %d entries, cls_score has %d channels" % (cw.numel(), C))
    x = cls_score
    if x.stride(1) != 1 or (N > 1 and x.stride(0) < C):
        x = x.contiguous()
    lab = labels.reshape(-1).to(torch.int64).contiguous()
    w = label_weights.reshape(-1).to(torch.float32).contiguous()
    ignore_index = -100 if loss_cls.ignore_index is None else int(loss_cls.ignore_index)
    return x, table, lab, w, cw, ignore_index


def _sigmoid_or_seesaw(kind, loss_cls, cls_score, labels, label_weights):
    """The two further native kinds, inside the kernels' limits (``_within_limits``)."""
    _lib.require_gpu(cls_score, labels, label_weights)
    N = cls_score.shape[0]
    if labels.numel() != N or (label_weights is not None and label_weights.numel() != N):
        raise ValueError("one label and one weight per row expected: %d rows, %d labels, %d weights"
                         % (N, labels.numel(), N if label_weights is None else label_weights.numel()))
    x = cls_score
    if x.stride(1) != 1 or (N > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    lab = labels.reshape(-1).to(torch.int64).contiguous()
    w = None if label_weights is None else label_weights.reshape(-1).to(torch.float32).contiguous()
    if kind == "sigmoid":
        cw = _class_weight(loss_cls, cls_score)
        if cw is not None:
            cw = cw.reshape(-1).to(torch.float32)
            if cw.numel() == 1:
                cw = cw.expand(x.shape[1])
            if cw.numel() != x.shape[1]:
                raise ValueError("class_weight has %d entries, cls_score has %d channels" % (cw.numel(), x.shape[1]))
            cw = cw.contiguous()
        ignore_index = -100 if loss_cls.ignore_index is None else int(loss_cls.ignore_index)
        loss, acc, avg = _HeadBceLoss.apply(x, lab, w, cw, ignore_index, float(loss_cls.loss_weight))
        return {"loss_cls": loss, "acc": acc, "avg_factor": avg}
    if loss_cls.cum_samples.device != x.device:
        loss_cls.cum_samples = loss_cls.cum_samples.to(x.device)
    args = (x, lab, w, loss_cls.cum_samples, loss_cls.p, loss_cls.q, loss_cls.eps, float(loss_cls.loss_weight))
    if loss_cls.return_dict:
        l_cls, l_obj, acc_obj, acc_cls, avg = _HeadSeesawLoss.apply(*args, False)
        return {"loss_cls_objectness": l_obj, "loss_cls_classes": l_cls, "acc_objectness": acc_obj, "acc_classes": acc_cls,
                "avg_factor": avg}
    loss, acc_obj, acc_cls, avg = _HeadSeesawLoss.apply(*args, True)
    return {"loss_cls": loss, "acc_objectness": acc_obj, "acc_classes": acc_cls, "avg_factor": avg}


def head_cls_loss(loss_cls, cls_score, labels, label_weights, reduction_override=None):
    """The classification lines of ``BBoxHead.loss`` (bbox_head.py:267-283):
    ``dict(loss_cls=..., acc_classes=... (IIFLoss) | acc=..., avg_factor=...)``.

    Native (our ``IIFLoss``; our ``CrossEntropyLoss(use_sigmoid=False, use_mask=False)``; reduction 'mean'): one launch
    forward, one backward, no host read.  ``avg_factor = max(#{label_weights > 0}, 1)`` is a 0-d device tensor, the
    accuracy a one-element device tensor over the rows with ``label_weights > 0``; rows of weight 0 are not read (the
    module docstring has the two differences from the reference).  ``loss_weight``, ``class_weight`` and ``ignore_index``
    are the module's.  An empty ``[0, C]`` batch gives loss 0, accuracy 0, ``avg_factor`` 1.

    Native as well, under 'mean', with the same ``avg_factor``, zero-weight rows and device outputs (``label_weights=None``
    means all ones):
      * our ``CrossEntropyLoss(use_sigmoid=True)``: ``iif_head_bce_loss_fwd``, one launch forward, one backward;
        ``{loss_cls, acc, avg_factor}``.  A valid label ``>= C`` is a background row, never a hit.
      * our ``SeesawLoss``: ``iif_seesaw_head_fwd`` / ``_bwd``, two launches forward, one backward, ``cum_samples`` updated in
        place by the rows of weight ``!= 0``; ``{loss_cls_objectness, loss_cls_classes, acc_objectness, acc_classes,
        avg_factor}``, or ``{loss_cls, acc_objectness, acc_classes, avg_factor}`` with ``return_dict=False``.
        ``acc_classes`` is over the positive rows with ``label_weights > 0``.
    A sigmoid or Seesaw call outside the kernels' limits (more than 2048 columns or 65535 rows, a score dtype the kernel
    does not take, floating-point labels) takes the lines below instead of raising.

    Every other ``loss_cls`` - ``use_mask``, ``CrossEntropyCounterLoss``, a module that is not ours - and the reductions
    'none' / 'sum' take the reference's own lines through ``loss_cls.forward`` / ``get_accuracy``:
    ``torch.sum(label_weights > 0).item()`` SYNCHRONISES the host there, once per call, and ``avg_factor`` is a Python
    float.  As in the reference nothing but ``avg_factor`` is returned for an empty batch on that path."""
    kind = _native_kind(loss_cls, reduction_override)
    if kind in ("sigmoid", "seesaw") and _within_limits(kind, loss_cls, cls_score, labels, label_weights):
        return _sigmoid_or_seesaw(kind, loss_cls, cls_score, labels, label_weights)
    if kind != "softmax":
        avg_factor = max(torch.sum(label_weights > 0).float().item(), 1.)
        out = dict()
        if cls_score.numel() > 0:
            loss_cls_ = loss_cls(cls_score, labels, label_weights, avg_factor=avg_factor, reduction_override=reduction_override)
            if isinstance(loss_cls_, dict):
                out.update(loss_cls_)
            else:
                out["loss_cls"] = loss_cls_
            if getattr(loss_cls, "custom_activation", False):
                out.update(loss_cls.get_accuracy(cls_score, labels))
            else:
                out["acc"] = topk_hit_counts(cls_score, labels, (1,)).to(torch.float32) * (100.0 / cls_score.size(0))
        out["avg_factor"] = avg_factor
        return out
    args = _prep(loss_cls, cls_score, labels, label_weights)
    loss, acc, avg = _HeadClsLoss.apply(*args, float(loss_cls.loss_weight))
    key = "acc_classes" if isinstance(loss_cls, IIFLoss) else "acc"
    return {"loss_cls": loss, key: acc, "avg_factor": avg}


def bbox_head_loss(loss_cls, loss_bbox, cls_score, bbox_pred, rois, labels, label_weights, bbox_targets, bbox_weights, num_classes,
                   reg_class_agnostic=False, reduction_override=None, bbox_coder=None, reg_decoded_bbox=False):
    """``BBoxHead.loss`` (bbox_head.py:256-312) from the head's attributes: ``head_cls_loss`` for the classification keys,
    ``bbox_head_reg_loss`` for ``loss_bbox``.  ``cls_score is None`` or ``bbox_pred is None`` drops that half, and an empty
    ``cls_score`` adds no classification key, as in the reference.  With native loss modules: three launches forward, three
    backward, nothing read back - the padded rows of ``roi_stage_targets_padded`` go in as they are.

    ``reg_decoded_bbox``: ``bbox_coder.decode(rois[:, 1:], bbox_pred)`` runs first, unconditionally (the reference decodes
    only behind ``pos_inds.any()``, a host read; without positives the loss and the gradient are zero either way)."""
    losses = dict()
    if cls_score is not None:
        if cls_score.numel() > 0:
            out = head_cls_loss(loss_cls, cls_score, labels, label_weights, reduction_override)
            out.pop("avg_factor")
            losses.update(out)
    if bbox_pred is not None:
        if reg_decoded_bbox:
            if bbox_coder is None:
                raise ValueError("reg_decoded_bbox needs the head's bbox_coder")
            bbox_pred = bbox_coder.decode(rois[:, 1:], bbox_pred)
        losses["loss_bbox"] = bbox_head_reg_loss(loss_bbox, bbox_pred, labels, bbox_targets, bbox_weights, num_classes,
                                                 reg_class_agnostic, reduction_override)
    return losses
