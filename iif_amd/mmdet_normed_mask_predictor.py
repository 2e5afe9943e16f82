"""The class-selected mask predictor of the cosine-norm heads: ``NormedConv2d`` as ``FCNMaskHead.conv_logits``, evaluated at each
RoI's label only (csrc/normed_mask_predictor.hip).

The cos-norm LVIS recipes (configs/activations/iif/iif_r50_rfs_cos_norm_4x4_1x.py, configs/fasa/*cos_norm*.py) build the mask
head with ``predictor_cfg=dict(type='NormedConv2d', tempearture=20)``: ``conv_logits`` normalises every weight row and every
pixel of its input over the channels (instance_segmentation/mmdet/models/utils/normed_predictor.py:104-124; for the 1x1 kernel
``norm_over_kernel`` is the same normalisation).  Neither normalisation involves another class, ``mask_cross_entropy``
(losses/cross_entropy_loss.py:158-162) keeps ``pred[inds, label]`` and ``get_seg_masks`` (fcn_mask_head.py:289-290)
``mask_pred[range(N), labels]``: the gradient of every other class row is exactly zero, as for the plain convolution of
``mmdet_mask_predictor.py``, and the ``[N, C, H, W]`` logits and their gradient are never formed.

  ``normed_class_mask_logits(x, weight, bias, labels, ...)``           the selected logits ``[N, 1, H, W]``, differentiable
  ``normed_class_mask_loss(x, weight, bias, labels, targets, ...)``    fused with ``mask_cross_entropy``, shape ``(1,)``
  ``ClassSelectedNormedMaskPredictor``                                 the module that stands where ``conv_logits`` stood

``valid_rows=True`` divides the loss by ``max(1, #valid RoIs) * H * W`` instead of ``N * H * W``, the count taken on the device:
a padded row of the padded RoI pipeline (label ``num_classes``) then neither adds a BCE term nor inflates the divisor.  In both
modes a label outside ``[0, C)`` contributes zero loss, a zero ``dx`` slice and nothing to ``dweight`` / ``dbias``, and that RoI's
``x`` is not read.

Dtypes, layout, limits and determinism are those of ``mmdet_mask_predictor.py``: ``x`` float32 or bfloat16 NCHW-contiguous
(otherwise one layout copy), float32 parameters, fp32 sums in a fixed order without float atomics, ``Cin <= 2048``,
``H * W <= 4096``, ``N <= 65535``; no host synchronisation.  Kept between forward and backward: three ``[N, H * W]`` float32
arrays (two when ``x`` needs no gradient) - nothing of the size of ``x``.

Deliberately not offered: k x k normed predictors, float16, ``class_weight``, a native ``channels_last`` kernel, and this
predictor inside ``FusedMaskHeadTail`` (mmdet_mask_tail.py fuses the plain convolution only).  ``tempearture`` is the reference's
spelling.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .mmdet_mask_predictor import _TILE, _SelectedPredictor, _empty_result, _is_empty, _is_plain_1x1, _ld, _needs, _prep, _up


def _cfg(tempearture, power, eps):
    t, q, e = float(tempearture), float(power), float(eps)
    if not q > 0:
        raise ValueError("power must be positive (got %r)" % (power,))
    return t, q, e


def _backward(x, weight, labels, g, ca, cb, up, inv, dims, cfg, need_x, need_w, need_b):
    """The two backward entries on the compact arrays g, A, B [N, HW] (g times the device scalars `up` and `inv`, or 1)."""
    n, c, cin, hw = dims
    _, q, eps = cfg
    L, st = _lib.lib(), _lib.stream_ptr()
    dx = dw = db = None
    if need_x:
        dx = torch.empty_like(x)
        _lib.check(L.iif_normed_mask_predict_bwd_input(_lib.ptr(x), _lib.dtype_code(x), _lib.ptr(g), _lib.ptr(ca), _lib.ptr(cb),
                                                       _lib.ptr(up), _lib.ptr(inv), _lib.ptr(weight), _ld(weight), _lib.ptr(labels),
                                                       n, c, cin, hw, q, eps, _lib.ptr(dx), st), "iif_normed_mask_predict_bwd_input")
    if need_w or need_b:
        scratch = torch.empty((n, cin + 1), dtype=torch.float32, device=g.device)
        if need_w:
            dw = torch.empty((c, cin), dtype=torch.float32, device=g.device)
        if need_b:
            db = torch.empty(c, dtype=torch.float32, device=g.device)
        _lib.check(L.iif_normed_mask_predict_bwd_weight(_lib.ptr(x), _lib.dtype_code(x), _lib.ptr(g), _lib.ptr(ca), _lib.ptr(up),
                                                        _lib.ptr(inv), _lib.ptr(weight), _ld(weight), _lib.ptr(labels), n, c, cin,
                                                        hw, q, eps, _lib.ptr(scratch), _lib.ptr(dw), _lib.ptr(db), st),
                   "iif_normed_mask_predict_bwd_weight")
    return dx, dw, db


class _Logits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, labels, wshape, cfg):
        xc, w2, b, lb, n, c, cin, hw = _prep(x.detach(), weight.detach(), None if bias is None else bias.detach(), labels)
        need_x, need_w, need_b = _needs(x, weight, bias)
        need_wb = need_w or need_b
        dev = xc.device
        z = torch.empty((n, 1) + tuple(x.shape[2:]), dtype=torch.float32, device=dev)
        coef = torch.empty((2 if need_x else 1 if need_wb else 0, n, hw), dtype=torch.float32, device=dev)
        ca = coef[0] if need_x or need_wb else None
        cb = coef[1] if need_x else None
        _lib.check(_lib.lib().iif_normed_mask_predict_fwd(_lib.ptr(xc), _lib.dtype_code(xc), _lib.ptr(w2), _ld(w2), _lib.ptr(b),
                                                          _lib.ptr(lb), 0, n, c, cin, hw, cfg[0], cfg[1], cfg[2], 0, _lib.ptr(z), 0,
                                                          _lib.ptr(ca), _lib.ptr(cb), 0, 0, 0, _lib.stream_ptr()),
                   "iif_normed_mask_predict_fwd")
        keep = need_x or need_wb
        ctx.save_for_backward(xc if keep else None, w2 if keep else None, lb, ca, cb)
        ctx.dims, ctx.cfg, ctx.wshape = (n, c, cin, hw), cfg, wshape
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        xc, w2, lb, ca, cb = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        n, _, _, hw = ctx.dims
        g = gz.detach().reshape(n, hw).to(torch.float32).contiguous()
        dx, dw, db = _backward(xc, w2, lb, g, ca, cb, None, None, ctx.dims, ctx.cfg, need_x, need_w, need_b)
        return dx, None if dw is None else dw.reshape(ctx.wshape), db, None, None, None


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, labels, targets, wshape, cfg, valid_rows):
        xc, w2, b, lb, n, c, cin, hw = _prep(x.detach(), weight.detach(), None if bias is None else bias.detach(), labels)
        if targets.numel() != n * hw:
            raise ValueError("targets must be [N, H, W] (got %s for x %s)" % (tuple(targets.shape), tuple(x.shape)))
        _lib.require_gpu(targets)
        t = targets.detach().reshape(n, hw).to(torch.float32).contiguous()
        dev = xc.device
        need_x, need_w, need_b = _needs(x, weight, bias)
        need_wb = need_w or need_b
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        inv = torch.empty(1, dtype=torch.float32, device=dev)                      # 1 / divisor, written by the forward
        rows = torch.empty(n * ((hw + _TILE - 1) // _TILE), dtype=torch.float32, device=dev)
        coef = torch.empty((3 if need_x else 2 if need_wb else 0, n, hw), dtype=torch.float32, device=dev)
        keep = need_x or need_wb
        g, ca = (coef[0], coef[1]) if keep else (None, None)
        cb = coef[2] if need_x else None
        _lib.check(_lib.lib().iif_normed_mask_predict_fwd(_lib.ptr(xc), _lib.dtype_code(xc), _lib.ptr(w2), _ld(w2), _lib.ptr(b),
                                                          _lib.ptr(lb), _lib.ptr(t), n, c, cin, hw, cfg[0], cfg[1], cfg[2],
                                                          1 if valid_rows else 0, 0, _lib.ptr(g), _lib.ptr(ca), _lib.ptr(cb),
                                                          _lib.ptr(rows), _lib.ptr(loss), _lib.ptr(inv), _lib.stream_ptr()),
                   "iif_normed_mask_predict_fwd")
        ctx.save_for_backward(xc if keep else None, w2 if keep else None, lb, g, ca, cb, inv if keep else None)
        ctx.dims, ctx.cfg, ctx.wshape = (n, c, cin, hw), cfg, wshape
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gl):
        xc, w2, lb, g, ca, cb, inv = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if g is None or not (need_x or need_w or need_b):
            return (None,) * 8
        dx, dw, db = _backward(xc, w2, lb, g, ca, cb, _up(gl), inv, ctx.dims, ctx.cfg, need_x, need_w, need_b)
        return (dx, None if dw is None else dw.reshape(ctx.wshape), db) + (None,) * 5


def normed_class_mask_logits(x, weight, bias, labels, tempearture=20, power=1.0, eps=1e-6):
    """``NormedConv2d(Cin, C, 1)(x)[range(N), labels][:, None]`` -> ``[N, 1, H, W]`` float32 without the other channels.
    ``x [N, Cin, H, W]`` float32 / bfloat16; ``weight [C, Cin]`` or ``[C, Cin, 1, 1]`` float32; ``bias [C]`` float32 or ``None``;
    ``labels [N]`` integer.  Differentiable in ``x``, ``weight`` and ``bias`` (not twice).  A RoI with a label outside ``[0, C)``
    gets zeros.  A non-contiguous or ``channels_last`` ``x`` costs one layout copy."""
    cfg = _cfg(tempearture, power, eps)
    if _is_empty(x):
        _prep(x, weight, bias, labels)
        return _empty_result(x, (weight, bias), (0, 1) + tuple(x.shape[2:]))
    return _Logits.apply(x, weight, bias, labels, tuple(weight.shape), cfg)


def normed_class_mask_loss(x, weight, bias, labels, targets, tempearture=20, power=1.0, eps=1e-6, valid_rows=False):
    """``mask_cross_entropy(NormedConv2d(Cin, C, 1)(x), targets, labels)`` -> shape ``(1,)``, as ONE autograd node: the forward is
    one pass over ``x`` that leaves the loss and three compact ``[N, H * W]`` arrays, the backward reads ``x`` once more per
    requested gradient.  Only what ``requires_grad`` asks for is computed and stored; the upstream gradient and the divisor are
    applied on the device.  ``valid_rows``: divide by ``max(1, #{n: 0 <= labels[n] < C}) * H * W`` instead of ``N * H * W``.
    ``targets [N, H, W]``.  ``N == 0``: a zero connected to ``x``, ``weight`` and ``bias``."""
    cfg = _cfg(tempearture, power, eps)
    if _is_empty(x):
        _prep(x, weight, bias, labels)
        return _empty_result(x, (weight, bias), (1,))
    return _Loss.apply(x, weight, bias, labels, targets, tuple(weight.shape), cfg, bool(valid_rows))


class ClassSelectedNormedMaskPredictor(_SelectedPredictor):
    """Stands where ``FCNMaskHead.conv_logits`` stood in a head built with ``predictor_cfg=dict(type='NormedConv2d', ...)``
    (fcn_mask_head.py:106-111): the same parameters - ``weight [C, Cin, 1, 1]``, ``bias [C]``, ``C = 1`` for a ``class_agnostic``
    head - under the ``state_dict`` keys of the reference's ``NormedConv2d(Cin, C, 1)``, so a checkpoint's
    ``mask_head.conv_logits.*`` loads unchanged, and the initialisation ``FCNMaskHead.init_weights`` gives that layer
    (``kaiming_normal_(mode='fan_out', nonlinearity='relu')``, zero bias, fcn_mask_head.py:117-125).  ``norm_over_kernel`` is
    accepted and kept: for a 1x1 kernel both settings are the same normalisation."""

    def __init__(self, in_channels, num_classes, class_agnostic=False, tempearture=20, power=1.0, eps=1e-6, norm_over_kernel=False):
        _cfg(tempearture, power, eps)
        super().__init__(in_channels, num_classes, class_agnostic)
        self.tempearture, self.power, self.eps, self.norm_over_kernel = tempearture, power, eps, bool(norm_over_kernel)

    def forward(self, x, labels):
        """The selected logits ``[N, 1, H, W]``: ``pos_labels`` in training, ``det_labels`` at test time."""
        return normed_class_mask_logits(x, self.weight, self.bias, self._labels(labels), self.tempearture, self.power, self.eps)

    def loss(self, x, labels, mask_targets, valid_rows=False):
        """``FCNMaskHead.loss`` (fcn_mask_head.py:147-177) on the head's features instead of its logits."""
        return dict(loss_mask=normed_class_mask_loss(x, self.weight, self.bias, self._labels(labels, valid_rows), mask_targets,
                                                     self.tempearture, self.power, self.eps, valid_rows))

    @classmethod
    def from_conv(cls, conv, class_agnostic=None):
        """From the head's ``conv_logits`` - ``iif_amd.mmdet_normed_predictor.NormedConv2d`` or the reference's class; the
        parameters are copied bit for bit."""
        if not isinstance(conv, nn.Conv2d) or not all(hasattr(conv, k) for k in ("tempearture", "power", "eps")):
            raise NotImplementedError("a NormedConv2d expected")
        if not _is_plain_1x1(conv):
            raise NotImplementedError("a plain 1x1 NormedConv2d expected")
        return cls._from_conv(conv, class_agnostic, tempearture=conv.tempearture, power=conv.power, eps=conv.eps,
                              norm_over_kernel=getattr(conv, "norm_over_kernel", False))

    def to_conv(self):
        """The dense ``iif_amd.mmdet_normed_predictor.NormedConv2d`` with these parameters: the full ``[N, C, H, W]`` logits for
        whoever needs them."""
        from .mmdet_normed_predictor import NormedConv2d
        return self._into_conv(NormedConv2d(self.in_channels, self.weight.size(0), 1, tempearture=self.tempearture, power=self.power,
                                            eps=self.eps, norm_over_kernel=self.norm_over_kernel))

    def extra_repr(self):
        return "in_channels=%d, num_classes=%d, class_agnostic=%s, tempearture=%s, power=%s, eps=%s" % (
            self.in_channels, self.num_classes, self.class_agnostic, self.tempearture, self.power, self.eps)
