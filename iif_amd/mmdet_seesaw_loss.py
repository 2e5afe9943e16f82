"""mmdet ``SeesawLoss`` plugin over the fused gfx950 kernels of ``csrc/seesaw_head.hip``.

Mirror of instance_segmentation/mmdet/models/losses/seesaw_loss.py:79-262: same constructor keywords, the
``cum_samples`` buffer (``[C + 1]`` float32, so a reference checkpoint's ``state_dict`` loads), the
``custom_cls_channels / custom_activation / custom_accuracy`` attributes and the ``forward / get_activation /
get_cls_channels / get_accuracy`` methods that ``BBoxHead`` reads (bbox_head.py:96-106,269-281,349-350).

A forward call is two launches (label histogram, then loss + gradient + both scalar losses) and never synchronises the
host, except for ``reduction='none'``, whose output shape is the number of positive rows (the reference syncs there
too).  Backward is one launch that scales the saved gradient by the upstream value of each of the two losses.
When mmdet is importable the class registers itself as ``SeesawLoss`` (``force=True`` replaces the stock one).
"""
import torch
import torch.nn as nn

from . import _lib
from . import custom
from .loss_reduction import check_avg_factor, reduction_scale, register_losses

MAX_CHANNELS = 2048          # C + 2: the row is register resident (csrc/seesaw_head.hip)
_WS = {}


def _workspace(device, stream):
    """Per (device, stream) scratch: the kernels' workspace (IIF_SEESAW_WORKSPACE_BYTES, zero between launches), the
    accuracy counters, and the status word shared with ``custom.check_label_status``."""
    key = (device, stream)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = {"loss": torch.zeros(4 + 2048 + 2 * 1024, dtype=torch.int32, device=device),
                         "acc": torch.zeros(4, dtype=torch.int32, device=device),
                         "status": custom._workspace(device, 0, False)[2]}
    return ws


def _check_scores(cls_score, num_classes):
    _lib.require_gpu(cls_score)
    if cls_score.dim() != 2:
        raise ValueError("cls_score must be [N, C + 2], got %s" % (tuple(cls_score.shape),))
    if cls_score.dtype != torch.float32:
        raise _lib.IIFNativeError("the Seesaw kernels take float32 scores (mmdet hands the loss fp32 under force_fp32), "
                                  "got %s" % cls_score.dtype)
    if num_classes + 2 > MAX_CHANNELS:
        raise _lib.IIFNativeError("the Seesaw kernels hold a row in registers: C + 2 = %d exceeds %d"
                                  % (num_classes + 2, MAX_CHANNELS))
    x = cls_score
    if x.stride(1) != 1:
        x = x.contiguous()
    return x


def _launch(cls_score, labels, weights, cum, update, p, q, eps, scale_cls, div_pos, scale_obj, C, want_grad):
    x = _check_scores(cls_score, C)
    _lib.require_gpu(labels, weights, cum)
    N = x.shape[0]
    dev = x.device
    stream = _lib.stream_ptr()
    ws = _workspace(dev, stream)
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    rows = torch.empty((2, N), dtype=torch.float32, device=dev)
    d = torch.empty((N, C + 2), dtype=torch.float32, device=dev) if want_grad else None
    lab = labels.to(torch.int64).contiguous()
    w = None if weights is None else weights.to(torch.float32).contiguous()
    rc = _lib.lib().iif_seesaw_fwd_bwd(
        _lib.ptr(x), _lib.dtype_code(x), x.stride(0) if N else C + 2, _lib.ptr(lab), _lib.ptr(w), _lib.ptr(cum),
        1 if update else 0, float(p), float(q), float(eps), float(scale_cls), 1 if div_pos else 0, float(scale_obj), N, C,
        _lib.ptr(rows[0]), _lib.ptr(rows[1]), _lib.ptr(losses), _lib.ptr(d), C + 2, _lib.ptr(ws["status"]), _lib.ptr(ws["loss"]),
        stream)
    _lib.check(rc, "iif_seesaw_fwd_bwd", ws["loss"][:2])
    return losses, rows, d


def _scale_grad(d, C, g_cls, g_obj, per_row):
    out = torch.empty_like(d)                      # the saved gradient stays intact: backward may run twice
    gc = g_cls.to(torch.float32).contiguous()
    go = g_obj.to(torch.float32).contiguous()
    rc = _lib.lib().iif_seesaw_scale_grad(_lib.ptr(d), C + 2, d.shape[0], C, _lib.ptr(gc), _lib.ptr(go),
                                          1 if per_row else 0, _lib.ptr(out), C + 2, _lib.stream_ptr())
    _lib.check(rc, "iif_seesaw_scale_grad")
    return out


class _FusedSeesaw(torch.autograd.Function):
    """(class loss, objectness loss) as two scalars; the gradient of both w.r.t. cls_score comes out of the forward
    launch and backward only scales its class / objectness columns by the two upstream scalars on the device."""

    @staticmethod
    def forward(ctx, cls_score, labels, weights, cum, p, q, eps, scale_cls, div_pos, scale_obj, C):
        losses, _, d = _launch(cls_score, labels, weights, cum, True, p, q, eps, scale_cls, div_pos, scale_obj, C,
                               ctx.needs_input_grad[0])
        ctx.save_for_backward(d)
        ctx.C = C
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_cls, g_obj):
        (d,) = ctx.saved_tensors
        if d is None:
            return (None,) * 11
        return (_scale_grad(d, ctx.C, g_cls, g_obj, False),) + (None,) * 10


class _FusedSeesawRows(torch.autograd.Function):
    """reduction='none': the two per-row loss vectors ([N] each, zero class loss on background rows); backward scales
    the rows of the unit-scale gradient by the upstream vectors."""

    @staticmethod
    def forward(ctx, cls_score, labels, weights, cum, p, q, eps, C):
        _, rows, d = _launch(cls_score, labels, weights, cum, True, p, q, eps, 1.0, False, 1.0, C,
                             ctx.needs_input_grad[0])
        ctx.save_for_backward(d)
        ctx.C = C
        return rows[0], rows[1]

    @staticmethod
    def backward(ctx, g_cls, g_obj):
        (d,) = ctx.saved_tensors
        if d is None:
            return (None,) * 8
        return (_scale_grad(d, ctx.C, g_cls, g_obj, True),) + (None,) * 7


class SeesawLoss(nn.Module):
    """Seesaw Loss for Long-Tailed Instance Segmentation (CVPR 2021, arXiv:2008.10032), native.

    ``cls_score`` is ``[N, C + 2]`` float32 on the MI355X (C class channels, two objectness channels), ``labels`` in
    ``[0, C]`` with ``C`` the background.  ``forward`` returns ``{'loss_cls_objectness', 'loss_cls_classes'}`` (or their
    sum with ``return_dict=False``), scaled by ``loss_weight``; 'mean' without ``avg_factor`` divides the class loss by
    the number of positive rows (taken on the device: no positives give 0) and the objectness loss by N.  A label outside
    ``[0, C]`` is not counted, contributes nothing and sets the flag that ``custom.check_label_status()`` raises on.
    """

    def __init__(self, use_sigmoid=False, p=0.8, q=2.0, num_classes=1203, eps=1e-2, reduction="mean", loss_weight=1.0,
                 return_dict=True, device="cuda"):
        super().__init__()
        assert not use_sigmoid
        self.use_sigmoid = False
        self.p = p
        self.q = q
        self.num_classes = num_classes
        self.eps = eps
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.return_dict = return_dict
        # cumulative samples of each category (and of the background)
        self.register_buffer("cum_samples", torch.zeros(self.num_classes + 1, dtype=torch.float, device=device))
        self.custom_cls_channels = True
        self.custom_activation = True
        self.custom_accuracy = True

    # --- plugin protocol -------------------------------------------------
    def get_cls_channels(self, num_classes):
        assert num_classes == self.num_classes
        return num_classes + 2

    def get_activation(self, cls_score):
        """``[N, C + 2] -> [N, C + 1]``: softmax(classes) * P(object), then P(background) (seesaw_loss.py:157-175)."""
        assert cls_score.size(-1) == self.num_classes + 2
        C = self.num_classes
        x = _check_scores(cls_score.detach(), C)
        N = x.shape[0]
        out = torch.empty((N, C + 1), dtype=torch.float32, device=x.device)
        rc = _lib.lib().iif_seesaw_activation(_lib.ptr(x), _lib.dtype_code(x), x.stride(0) if N else C + 2, N, C,
                                              _lib.ptr(out), C + 1, _lib.stream_ptr())
        _lib.check(rc, "iif_seesaw_activation")
        return out

    def get_accuracy(self, cls_score, labels):
        """``{'acc_objectness', 'acc_classes'}`` in percent, one-element tensors (seesaw_loss.py:177-197); counts and
        division on the device, ``acc_classes`` 0 without a positive row."""
        assert cls_score.size(-1) == self.num_classes + 2
        C = self.num_classes
        x = _check_scores(cls_score.detach(), C)
        _lib.require_gpu(labels)
        N = x.shape[0]
        stream = _lib.stream_ptr()
        ws = _workspace(x.device, stream)
        out = torch.empty(2, dtype=torch.float32, device=x.device)
        lab = labels.to(torch.int64).contiguous()
        rc = _lib.lib().iif_seesaw_accuracy(_lib.ptr(x), _lib.dtype_code(x), x.stride(0) if N else C + 2, _lib.ptr(lab),
                                            N, C, _lib.ptr(out), _lib.ptr(ws["acc"]), stream)
        _lib.check(rc, "iif_seesaw_accuracy", ws["acc"])
        return dict(acc_objectness=out[0:1], acc_classes=out[1:2])

    # --- loss ------------------------------------------------------------
    def forward(self, cls_score, labels, label_weights=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        C = self.num_classes
        assert cls_score.size(-1) == C + 2
        check_avg_factor(reduction, avg_factor)
        _lib.require_gpu(cls_score, labels, label_weights)
        if self.cum_samples.device != cls_score.device:
            self.cum_samples = self.cum_samples.to(cls_score.device)
        N = cls_score.shape[0]
        lw = float(self.loss_weight)
        if reduction == "none":
            rows_cls, rows_obj = _FusedSeesawRows.apply(cls_score, labels, label_weights, self.cum_samples, self.p,
                                                        self.q, self.eps, C)
            loss_cls_classes = lw * rows_cls[labels < C]          # the output's shape is the positive count: one sync
            loss_cls_objectness = lw * rows_obj
        else:
            scale_obj = reduction_scale(reduction, avg_factor, N, lw)
            div_pos = reduction != "sum" and avg_factor is None      # the class loss is divided by the positive count on the device
            scale_cls = lw if div_pos else scale_obj
            loss_cls_classes, loss_cls_objectness = _FusedSeesaw.apply(
                cls_score, labels, label_weights, self.cum_samples, self.p, self.q, self.eps, scale_cls, div_pos,
                scale_obj, C)
            if N == 0 and reduction == "mean" and avg_factor is None:
                loss_cls_objectness = loss_cls_objectness * float("nan")       # torch: mean of an empty tensor
        if self.return_dict:
            return dict(loss_cls_objectness=loss_cls_objectness, loss_cls_classes=loss_cls_classes)
        return loss_cls_classes + loss_cls_objectness


def register_into_mmdet():
    """Register the native class as mmdet's ``SeesawLoss`` if mmdet is importable."""
    return register_losses({"SeesawLoss": SeesawLoss})


register_into_mmdet()
