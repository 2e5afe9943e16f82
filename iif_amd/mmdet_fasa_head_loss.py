"""``ConvFCFASABBoxHead.loss`` without a host read: the feature bank fed from padded rows, the classification loss with open
accumulators on the device-counted path, and the loss of the virtual embeddings over a fixed number of rows.

Mirror of instance_segmentation/mmdet/models/roi_heads/bbox_heads/fasa_bbox_head.py:217-300 with
losses/fasa_iif_loss.py:117-162.  The reference reads the host four times per step from epoch 1 on: two boolean indexings
for the bank update (:259-260), ``torch.sum(label_weights > 0).item()`` (:265), ``len(aug_embedding)`` behind
``fa_generate`` and ``aug_avg_factor = ....item()`` (:284-292) - and once per class inside ``fa_update`` and inside
``FasaIIFLoss.forward`` while its accumulators are open.

  * ``head_cls_loss_cums``: ``iif_head_loss_cums_fwd`` (csrc/head_loss.hip) - ``FasaIIFLoss`` in its softmax mode with
    ``use_cums`` open: the row losses, their per-class sums and counts into ``cum_losses`` / ``cum_labels``, the returned
    ``rows.mean()`` and the top-1 accuracy.  Two launches forward, one backward.
  * ``fasa_cls_loss``: the classification lines of the head for any ``loss_cls``: ``head_cls_loss_cums`` with open
    accumulators, ``mmdet_bbox_head_loss.head_cls_loss`` with closed ones, and the reference's own lines (one host read)
    for everything that is not a softmax criterion of ours - the sigmoid and mask modes of ``FasaIIFLoss`` among them.
  * ``fasa_bbox_head_loss``: all of ``ConvFCFASABBoxHead.loss``.

The policy of ``mmdet_bbox_head_loss`` carries over: a row with ``label_weights == 0`` is NOT READ.  With open
accumulators such a row enters neither ``cum_losses`` / ``cum_labels``, nor the accuracy, nor the divisor of the mean, which
is ``max(#{label_weights != 0}, 1)`` (the reference divides by all N rows and counts a padding row's label).  Without
zero-weight rows every value equals the reference's.
"""
import torch

from . import _lib
from . import custom
from .mmdet_bbox_head_loss import MAX_CLASSES, MAX_ROWS, _is_native, _prep, head_cls_loss
from .mmdet_bbox_loss import bbox_head_reg_loss
from .mmdet_fasa import FasaIIFLoss
from .utils import topk_hit_counts

__all__ = ["head_cls_loss_cums", "fasa_cls_loss", "fasa_bbox_head_loss", "ENQUEUED_TRAIN", "ENQUEUED_VAL"]

# Operations fasa_bbox_head_loss enqueues forward, whatever the data holds, with native loss modules, float32 contiguous
# inputs, the default draws and fc_cls counted as one:
#   training, epoch >= 1: regression 1, bank update 2, classification 1, torch.rand + torch.randn 2, generate 1, fc_cls 1,
#                         aug classification 1, the sum of the two losses 1
#   validation, open accumulators: regression 1, classification 2
ENQUEUED_TRAIN = 11
ENQUEUED_VAL = 3


def _softmax_mode(loss_cls):
    """``FasaIIFLoss`` keeps ``use_sigmoid`` / ``use_mask`` and swaps the criterion (fasa_iif_loss.py:35-40): an
    ``IIFLoss`` instance that must not reach a softmax kernel."""
    return not getattr(loss_cls, "use_sigmoid", False) and not getattr(loss_cls, "use_mask", False)


class _HeadClsLossCums(torch.autograd.Function):
    """(loss, acc, avg) and the two accumulators, updated in place; backward is ``_HeadClsLoss``'s: the saved gradient lacks
    ``loss_weight / avg``, applied with the upstream scalar from device scalars in one launch."""

    @staticmethod
    def forward(ctx, x, table, labels, weights, class_weight, ignore_index, loss_weight, cum_losses, cum_labels):
        N, C = x.shape
        dev = x.device
        f32 = torch.float32
        loss = torch.empty((), dtype=f32, device=dev)
        acc = torch.empty((1,), dtype=f32, device=dev)
        avg = torch.empty((), dtype=f32, device=dev)
        rows = torch.empty((N,), dtype=f32, device=dev)
        du = torch.empty((N, C), dtype=x.dtype, device=dev) if ctx.needs_input_grad[0] else None
        _, ticket, status = custom._workspace(dev, 0, False)
        rc = _lib.lib().iif_head_loss_cums_fwd(
            _lib.ptr(x), _lib.dtype_code(x), x.stride(0) if N > 1 else C, _lib.ptr(table), _lib.ptr(labels), _lib.ptr(weights),
            _lib.ptr(class_weight), int(ignore_index), float(loss_weight), N, C, _lib.ptr(du), C, _lib.ptr(rows),
            _lib.ptr(cum_losses), _lib.ptr(cum_labels), _lib.ptr(loss), _lib.ptr(acc), _lib.ptr(avg), _lib.ptr(status),
            _lib.ptr(ticket), _lib.stream_ptr())
        _lib.check(rc, "iif_head_loss_cums_fwd", ticket[:1])
        ctx.save_for_backward(du, avg)
        ctx.loss_weight = float(loss_weight)
        ctx.mark_non_differentiable(acc, avg, rows)
        return loss, acc, avg, rows

    @staticmethod
    def backward(ctx, g_loss, g_acc, g_avg, g_rows):
        du, avg = ctx.saved_tensors
        if du is None:
            return (None,) * 9
        g = g_loss.to(torch.float32).contiguous()
        out = torch.empty_like(du)
        rc = _lib.lib().iif_head_loss_bwd(_lib.ptr(du), _lib.dtype_code(du), du.numel(), _lib.ptr(g), _lib.ptr(avg), ctx.loss_weight,
                                          _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "iif_head_loss_bwd")
        return (out,) + (None,) * 8


def head_cls_loss_cums(loss_cls, cls_score, labels, label_weights, reduction_override=None):
    """The classification lines of the head (fasa_bbox_head.py:264-281) for a ``FasaIIFLoss`` in its softmax mode whose
    accumulators are OPEN (``open_cums()``: reduction 'none', the rows summed per class, ``rows.mean()`` returned;
    fasa_iif_loss.py:145-160): ``dict(loss_cls=..., acc_classes=..., avg_factor=..., rows=...)``.

    Two launches forward - the loss kernel, which also stores the row losses ``loss_weight * w_i * nll_i``, and the
    per-class sums in ascending row order - and one backward; nothing is read back.  ``loss_cls.cum_losses[c]`` grows by
    the sum and ``loss_cls.cum_labels[c]`` by the number of the rows of label ``c``.  A row of weight 0 is not read and
    enters neither the accumulators, nor the accuracy, nor the divisor of the mean: ``avg_factor`` here is
    ``max(#{label_weights != 0}, 1)``, a 0-d device tensor.  Without zero-weight rows all of it equals the reference
    (its mean over all N rows, its accuracy over all N rows).  All weights zero: loss 0, accumulators untouched,
    ``avg_factor`` 1.  An empty ``[0, C]`` batch gives the same and launches nothing but the loss kernel.

    Raises ``ValueError`` for a ``loss_cls`` that is not a ``FasaIIFLoss``, for its sigmoid or mask mode (another
    criterion: ``fasa_cls_loss`` sends those down the reference's lines), for closed accumulators and for a
    ``reduction_override`` other than None / 'none' (the reference cannot index a reduced loss); the shape, dtype and
    size limits are ``head_cls_loss``'s."""
    if not isinstance(loss_cls, FasaIIFLoss):
        raise ValueError("head_cls_loss_cums: a FasaIIFLoss expected, got %s" % type(loss_cls).__name__)
    if not _softmax_mode(loss_cls):
        raise ValueError("head_cls_loss_cums: FasaIIFLoss(use_sigmoid=True | use_mask=True) is not a softmax criterion; "
                         "fasa_cls_loss takes the reference's lines for it")
    if not loss_cls.use_cums:
        raise ValueError("head_cls_loss_cums: the accumulators are closed (open_cums()); head_cls_loss is the closed path")
    if reduction_override not in (None, "none"):
        raise ValueError("head_cls_loss_cums: open accumulators need the row losses, reduction_override=%r reduces them"
                         % (reduction_override,))
    x, table, lab, w, cw, ignore_index = _prep(loss_cls, cls_score, labels, label_weights)
    cl, cn = loss_cls.cum_losses, loss_cls.cum_labels
    C = x.shape[1]
    for t in (cl, cn):
        _lib.require_gpu(t)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C:
            raise ValueError("head_cls_loss_cums: float32 accumulators of %d entries expected, got %s %s" % (C, t.dtype, tuple(t.shape)))
    loss, acc, avg, rows = _HeadClsLossCums.apply(x, table, lab, w, cw, ignore_index, float(loss_cls.loss_weight), cl, cn)
    return {"loss_cls": loss, "acc_classes": acc, "avg_factor": avg, "rows": rows}


def _reference_lines(loss_cls, cls_score, labels, label_weights, reduction_override):
    """fasa_bbox_head.py:264-281 as they stand: ``.item()`` synchronises the host once."""
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


def fasa_cls_loss(loss_cls, cls_score, labels, label_weights, reduction_override=None):
    """The classification keys and ``avg_factor`` for any ``loss_cls``:

      * a ``FasaIIFLoss`` in its sigmoid or mask mode is an ``IIFLoss`` instance with another criterion
        (``binary_cross_entropy`` / ``mask_cross_entropy``): the reference's lines through ``loss_cls.forward``, one host
        read, never a softmax kernel - ``head_cls_loss`` is not asked, it would take the instance for a plain ``IIFLoss``;
      * a softmax ``FasaIIFLoss`` with open accumulators and no reducing override: ``head_cls_loss_cums`` (without its
        ``rows``);
      * everything else: ``head_cls_loss`` - native for our softmax modules under 'mean', else the reference's lines."""
    if isinstance(loss_cls, FasaIIFLoss) and not _softmax_mode(loss_cls):
        return _reference_lines(loss_cls, cls_score, labels, label_weights, reduction_override)
    if isinstance(loss_cls, FasaIIFLoss) and loss_cls.use_cums and reduction_override in (None, "none") and cls_score.numel() > 0 \
            and cls_score.dim() == 2 and cls_score.shape[1] <= MAX_CLASSES and cls_score.shape[0] <= MAX_ROWS:
        out = head_cls_loss_cums(loss_cls, cls_score, labels, label_weights, reduction_override)
        out.pop("rows")
        return out
    return head_cls_loss(loss_cls, cls_score, labels, label_weights, reduction_override)


def fasa_bbox_head_loss(bank, loss_cls, loss_bbox, fc_cls, cls_score, bbox_pred, rois, labels, label_weights, bbox_targets,
                        bbox_weights, embedding, num_classes, training=True, epoch=None, reg_class_agnostic=False,
                        reduction_override=None, aug_capacity=None, rand=None, normal=None, bbox_coder=None,
                        reg_decoded_bbox=False):
    """``ConvFCFASABBoxHead.loss`` (fasa_bbox_head.py:217-300) from the head's attributes, the reference's keys and ``None``
    handling, in the reference's order:

      1. ``bbox_pred is not None``: ``losses['loss_bbox']`` through ``bbox_head_reg_loss`` (``reg_decoded_bbox`` as in
         ``bbox_head_loss``).
      2. ``training``: ``bank.fa_update_rows(embedding.detach(), labels)`` - the positives ``0 <= label < num_classes`` are
         selected on the device (:258-262).
      3. ``cls_score is not None`` and not empty: ``fasa_cls_loss`` - ``head_cls_loss`` with closed accumulators,
         ``head_cls_loss_cums`` with open ones (``loss_cls`` / ``acc_classes`` or ``acc``).
      4. ``training`` and ``epoch >= 1`` (``epoch`` defaults to ``bank.epoch``) and there is a ``loss_cls`` key:
         ``bank.fa_generate_padded(rand, normal, aug_capacity)``, ``fc_cls`` (any callable: ``nn.Linear``, the native
         ``NormedLinear``) on ALL K padded rows, the same classification function on the result with the padded weights
         - zero-weight rows are not read, ``avg_factor = max(count, 1)`` is counted on the device, the reference's
         ``aug_avg_factor`` - and ``losses['loss_cls'] += loss_cls_aug`` (:283-299).  Where the reference adds nothing
         because no class was drawn, an exact 0 with an all-zero gradient is added.

    ``bank``: the ``FasaFeatureBank``; ``num_classes`` must be its own.  With native loss modules (our ``FasaIIFLoss`` /
    ``IIFLoss`` / softmax ``CrossEntropyLoss``, ``L1Loss`` / ``SmoothL1Loss``, reduction 'mean'), float32 contiguous inputs
    and ``fc_cls`` counted as one operation, a training call at ``epoch >= 1`` enqueues ``ENQUEUED_TRAIN`` = 11 operations
    forward (9 when ``rand`` and ``normal`` are given) and a validation call with open accumulators ``ENQUEUED_VAL`` = 3,
    whatever the data holds, and nothing is read back.  A ``loss_cls`` that is not a softmax criterion of ours takes the
    reference's lines for both classification calls (one host read each); the virtual rows are still the K padded ones,
    so a criterion that does not skip zero-weight rows sees K - count rows of zeros, label ``num_classes``, weight 0."""
    if num_classes != bank.num_classes:
        raise ValueError("fasa_bbox_head_loss: num_classes %d is not the bank's %d" % (num_classes, bank.num_classes))
    losses = dict()
    if bbox_pred is not None:
        if reg_decoded_bbox:
            if bbox_coder is None:
                raise ValueError("reg_decoded_bbox needs the head's bbox_coder")
            bbox_pred = bbox_coder.decode(rois[:, 1:], bbox_pred)
        losses["loss_bbox"] = bbox_head_reg_loss(loss_bbox, bbox_pred, labels, bbox_targets, bbox_weights, num_classes,
                                                 reg_class_agnostic, reduction_override)
    if training:
        bank.fa_update_rows(embedding.detach(), labels)
    if cls_score is not None:
        if cls_score.numel() > 0:
            out = fasa_cls_loss(loss_cls, cls_score, labels, label_weights, reduction_override)
            out.pop("avg_factor")
            losses.update(out)
    epoch = bank.epoch if epoch is None else epoch
    if training and epoch >= 1 and "loss_cls" in losses:
        aug_embedding, aug_labels, aug_weights, _ = bank.fa_generate_padded(rand, normal, aug_capacity)
        aug_cls_score = fc_cls(aug_embedding)
        aug = fasa_cls_loss(loss_cls, aug_cls_score, aug_labels, aug_weights, reduction_override)
        losses["loss_cls"] = losses["loss_cls"] + aug["loss_cls"]
    return losses
