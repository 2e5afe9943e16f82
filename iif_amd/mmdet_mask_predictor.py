"""The class-selected mask predictor: ``FCNMaskHead.conv_logits`` evaluated at each RoI's label only (csrc/mask_predictor.hip).

``FCNMaskHead.forward`` (instance_segmentation/mmdet/models/roi_heads/mask_heads/fcn_mask_head.py:127-136) ends with
``mask_pred = self.conv_logits(x)``, a 1x1 convolution to ``num_classes`` channels for every RoI; ``mask_cross_entropy``
(losses/cross_entropy_loss.py:158-162) keeps ``pred[inds, label]`` and ``get_seg_masks`` (fcn_mask_head.py:289-290)
``mask_pred[range(N), labels]``: one channel per RoI.  The gradient of every other channel is exactly zero, so the predictor is
evaluated at the label channel alone, with the same loss and the same gradients for ``x``, ``weight`` and ``bias``; the
``[N, C, H, W]`` logits (966 MB at the LVIS training shape: 256 RoIs, 1203 classes, 28 x 28) and their gradient are never formed.
The label is known before the mask head runs: ``pos_labels`` in ``_mask_forward_train``, ``det_labels`` in ``simple_test_mask``.

  ``class_mask_logits(x, weight, bias, labels)``            the selected logits ``[N, 1, H, W]``, differentiable
  ``class_mask_loss(x, weight, bias, labels, targets)``     the predictor fused with ``mask_cross_entropy``, shape ``(1,)``
                                                            (``valid_rows=True``: the padded RoI pipeline's divisor)
  ``ClassSelectedMaskPredictor``                            the module that stands where ``conv_logits`` stood

Test end: the ``[N, 1, h, w]`` logits go into ``mmdet_mask_loss.paste_masks`` / ``get_seg_masks`` with ``class_agnostic=True``
(which reads channel 0); ``get_seg_masks`` still files each mask under ``det_labels``.

``x`` is float32 or bfloat16 (``dx`` comes back in that dtype), ``weight`` / ``bias`` float32.  The kernels read ``x`` as
NCHW-contiguous: a non-contiguous or ``channels_last`` ``x`` costs one layout copy.  ``weight`` rows are read through their
stride (a row-strided view is read in place).  Every sum is fp32 in a fixed order without float atomics: the same bits from call
to call.  A label outside ``[0, C)`` contributes zero loss, a zero ``dx`` slice and nothing to ``dweight`` / ``dbias``, and that
RoI's ``x`` and targets are not read.  The divisor is ``N * H * W``; with ``valid_rows=True`` it is ``max(1, K) * H * W``, ``K``
the number of RoIs with a label in ``[0, C)``, counted on the device: a padded row of the padded RoI pipeline (image index -1,
label ``num_classes``) then neither adds a term nor dilutes the loss, and nothing is read back.  ``K = 0``: the loss is exactly 0
and every gradient exact zeros.  Limits: ``Cin <= 2048``, ``H * W <= 4096``, ``N <= 65535``.

Deliberately not offered: the full ``[N, C, H, W]`` logits (``to_conv()`` gives the convolution back), a ``predictor_cfg`` other
than a plain convolution (``NormedConv2d``: mmdet_normed_mask_predictor.py), ``class_weight``, float16 and a native ``channels_last`` kernel.  The deconv + ReLU in front are fused
with this predictor in ``mmdet_mask_tail.py`` (``FusedMaskHeadTail``).
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib

_MAX_CIN, _MAX_HW, _MAX_N = 2048, 4096, 65535
# Pixels per row partial of the loss: the SMALLEST tile any forward kernel of the family may use (kMinTile in
# csrc/mask_predict_core.h, which checks kTile = 128 and the tail's kPix = 64 against it), so n * ceil(hw / _TILE) floats are an
# upper bound of what a forward writes.
_TILE = 64


def _prep(x, weight, bias, labels):
    """Checks in the order devices, shapes, dtypes; returns (x NCHW-contiguous, weight with unit column stride, bias, labels
    int64, N, C, Cin, HW)."""
    for t in (x, weight, labels):
        if not isinstance(t, torch.Tensor):
            raise ValueError("class-selected mask predictor: tensors expected")
    _lib.require_gpu(x, weight, bias, labels)
    if x.dim() != 4:
        raise ValueError("x must be [N, Cin, H, W] (got %s)" % (tuple(x.shape),))
    if weight.dim() == 4:
        if weight.size(2) != 1 or weight.size(3) != 1:
            raise ValueError("weight must be [C, Cin] or [C, Cin, 1, 1] (got %s)" % (tuple(weight.shape),))
        weight = weight[:, :, 0, 0]
    elif weight.dim() != 2:
        raise ValueError("weight must be [C, Cin] or [C, Cin, 1, 1] (got %s)" % (tuple(weight.shape),))
    n, cin, h, w = x.shape
    c = weight.size(0)
    if weight.size(1) != cin:
        raise ValueError("weight has %d input channels, x has %d" % (weight.size(1), cin))
    if bias is not None and tuple(bias.shape) != (c,):
        raise ValueError("bias must be [C] (got %s)" % (tuple(bias.shape),))
    if labels.numel() != n:
        raise ValueError("one label per RoI expected (%d labels, %d RoIs)" % (labels.numel(), n))
    if c < 1 or not 1 <= cin <= _MAX_CIN or not 1 <= h * w <= _MAX_HW or n > _MAX_N:
        raise ValueError("class-selected mask predictor: C >= 1, 1 <= Cin <= %d, 1 <= H * W <= %d, N <= %d"
                         % (_MAX_CIN, _MAX_HW, _MAX_N))
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError("float32 / bfloat16 x only (got %s)" % x.dtype)
    if weight.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise NotImplementedError("float32 weight and bias only")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise NotImplementedError("integer labels only (got %s)" % labels.dtype)
    x = x.contiguous()
    if weight.stride(1) != 1 or (c > 1 and weight.stride(0) < cin):
        weight = weight.contiguous()
    if bias is not None:
        bias = bias.contiguous()
    labels = labels.reshape(-1).to(torch.int64).contiguous()
    return x, weight, bias, labels, n, c, cin, h * w


def _ld(weight):
    return weight.stride(0) if weight.size(0) > 1 else weight.size(1)


def _backward(x, xmeta, weight, labels, g, up, n, c, cin, hw, need_x, need_w, need_b, inv=None):
    """The two backward entries on the compact gradient g [N, HW] (times the device scalar `up`, or 1).  xmeta: shape and dtype
    of x, which itself is only there when dweight / dbias are asked for.  inv: the device scalar 1 / divisor of a forward that
    stored g undivided (valid_rows); the kernels multiply it in."""
    L, st = _lib.lib(), _lib.stream_ptr()
    dx = dw = db = None
    if need_x:
        dx = torch.empty(xmeta[0], dtype=xmeta[1], device=g.device)
        if inv is None:
            _lib.check(L.iif_mask_predict_bwd_input(_lib.ptr(g), _lib.ptr(up), _lib.ptr(weight), _ld(weight), _lib.ptr(labels), n, c,
                                                    cin, hw, _lib.ptr(dx), _lib.dtype_code(dx), st), "iif_mask_predict_bwd_input")
        else:
            _lib.check(L.iif_mask_predict_loss_bwd_input(_lib.ptr(g), _lib.ptr(up), _lib.ptr(inv), _lib.ptr(weight), _ld(weight),
                                                         _lib.ptr(labels), n, c, cin, hw, _lib.ptr(dx), _lib.dtype_code(dx), st),
                       "iif_mask_predict_loss_bwd_input")
    if need_w or need_b:
        scratch = torch.empty((n, cin + 1), dtype=torch.float32, device=g.device)
        if need_w:
            dw = torch.empty((c, cin), dtype=torch.float32, device=g.device)
        if need_b:
            db = torch.empty(c, dtype=torch.float32, device=g.device)
        if inv is None:
            _lib.check(L.iif_mask_predict_bwd_weight(_lib.ptr(x), _lib.dtype_code(x), _lib.ptr(g), _lib.ptr(up), _lib.ptr(labels), n,
                                                     c, cin, hw, _lib.ptr(scratch), _lib.ptr(dw), _lib.ptr(db), st),
                       "iif_mask_predict_bwd_weight")
        else:
            _lib.check(L.iif_mask_predict_loss_bwd_weight(_lib.ptr(x), _lib.dtype_code(x), _lib.ptr(g), _lib.ptr(up), _lib.ptr(inv),
                                                          _lib.ptr(labels), n, c, cin, hw, _lib.ptr(scratch), _lib.ptr(dw),
                                                          _lib.ptr(db), st), "iif_mask_predict_loss_bwd_weight")
    return dx, dw, db


def _up(g):
    return g.detach().reshape(1).to(torch.float32).contiguous()


def _needs(*tensors):
    """Which of the tensors (None allowed) ask for a gradient."""
    return tuple(t is not None and t.requires_grad for t in tensors)


def _is_empty(x):
    """N == 0: no kernel runs; the callers check the other arguments and return _empty_result."""
    return isinstance(x, torch.Tensor) and x.dim() == 4 and x.size(0) == 0


def _empty_result(x, params, shape):
    """N == 0: a zero of `shape` that is still connected to x and every parameter (the reference returns mask_pred.sum())."""
    z = x.sum().float()
    for p in params:
        if p is not None:
            z = z + p.sum() * 0
    return z * x.new_zeros(shape, dtype=torch.float32) if 0 in shape else z.reshape(shape)


def _copy_params(dst, src):
    """weight and bias of src into dst, bit for bit; a bias src does not have leaves dst's as it is."""
    with torch.no_grad():
        dst.weight.copy_(src.weight)
        if src.bias is not None:
            dst.bias.copy_(src.bias)


def _is_plain_1x1(conv):
    return conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1 \
        and conv.dilation == (1, 1)


class _Logits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, labels, wshape):
        xc, w2, b, lb, n, c, cin, hw = _prep(x.detach(), weight.detach(), None if bias is None else bias.detach(), labels)
        z = torch.empty((n, 1) + tuple(x.shape[2:]), dtype=torch.float32, device=xc.device)
        status = torch.zeros(1, dtype=torch.int32, device=xc.device)
        _lib.check(_lib.lib().iif_mask_predict_fwd(_lib.ptr(xc), _lib.dtype_code(xc), _lib.ptr(w2), _ld(w2), _lib.ptr(b), _lib.ptr(lb), 0,
                                                   n, c, cin, hw, _lib.ptr(z), 0, 0, 0, _lib.ptr(status), _lib.stream_ptr()),
                   "iif_mask_predict_fwd")
        need_x, need_w, need_b = _needs(x, weight, bias)
        ctx.save_for_backward(xc if need_w or need_b else None, w2 if need_x else None, lb)
        ctx.dims = (n, c, cin, hw, (tuple(x.shape), x.dtype), wshape)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        xc, w2, lb = ctx.saved_tensors
        n, c, cin, hw, xmeta, wshape = ctx.dims
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        g = gz.detach().reshape(n, hw).to(torch.float32).contiguous()
        dx, dw, db = _backward(xc, xmeta, w2, lb, g, None, n, c, cin, hw, need_x, need_w, need_b)
        return dx, None if dw is None else dw.reshape(wshape), db, None, None


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, labels, targets, wshape, valid_rows):
        xc, w2, b, lb, n, c, cin, hw = _prep(x.detach(), weight.detach(), None if bias is None else bias.detach(), labels)
        if targets.numel() != n * hw:
            raise ValueError("targets must be [N, H, W] (got %s for x %s)" % (tuple(targets.shape), tuple(x.shape)))
        _lib.require_gpu(targets)
        t = targets.detach().reshape(n, hw).to(torch.float32).contiguous()
        dev = xc.device
        need_x, need_w, need_b = _needs(x, weight, bias)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        rows = torch.empty(n * ((hw + _TILE - 1) // _TILE), dtype=torch.float32, device=dev)
        g0 = torch.empty((n, hw), dtype=torch.float32, device=dev) if need_x or need_w or need_b else None
        inv = None
        if valid_rows:                                   # g0 undivided; the divisor is the device scalar `inv`
            inv = torch.empty(1, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().iif_mask_predict_loss_fwd(_lib.ptr(xc), _lib.dtype_code(xc), _lib.ptr(w2), _ld(w2), _lib.ptr(b),
                                                            _lib.ptr(lb), _lib.ptr(t), n, c, cin, hw, 1, _lib.ptr(g0), _lib.ptr(rows),
                                                            _lib.ptr(loss), _lib.ptr(inv), _lib.stream_ptr()),
                       "iif_mask_predict_loss_fwd")
        else:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().iif_mask_predict_fwd(_lib.ptr(xc), _lib.dtype_code(xc), _lib.ptr(w2), _ld(w2), _lib.ptr(b),
                                                       _lib.ptr(lb), _lib.ptr(t), n, c, cin, hw, 0, _lib.ptr(g0), _lib.ptr(rows),
                                                       _lib.ptr(loss), _lib.ptr(status), _lib.stream_ptr()), "iif_mask_predict_fwd")
        ctx.save_for_backward(xc if need_w or need_b else None, w2 if need_x else None, lb, g0, inv if g0 is not None else None)
        ctx.dims = (n, c, cin, hw, (tuple(x.shape), x.dtype), wshape)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gl):
        xc, w2, lb, g0, inv = ctx.saved_tensors
        n, c, cin, hw, xmeta, wshape = ctx.dims
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if g0 is None or not (need_x or need_w or need_b):
            return (None,) * 7
        dx, dw, db = _backward(xc, xmeta, w2, lb, g0, _up(gl), n, c, cin, hw, need_x, need_w, need_b, inv)
        return (dx, None if dw is None else dw.reshape(wshape), db) + (None,) * 4


def class_mask_logits(x, weight, bias, labels):
    """``conv_logits(x)[range(N), labels][:, None]`` -> ``[N, 1, H, W]`` float32 without the other channels.  ``x [N, Cin, H, W]``
    float32 / bfloat16; ``weight [C, Cin]`` or ``[C, Cin, 1, 1]`` float32; ``bias [C]`` float32 or ``None``; ``labels [N]``
    integer.  Differentiable in ``x``, ``weight`` and ``bias`` (not twice).  A non-contiguous or ``channels_last`` ``x`` costs one
    layout copy."""
    if _is_empty(x):
        _prep(x, weight, bias, labels)
        return _empty_result(x, (weight, bias), (0, 1) + tuple(x.shape[2:]))
    return _Logits.apply(x, weight, bias, labels, tuple(weight.shape))


def class_mask_loss(x, weight, bias, labels, targets, valid_rows=False):
    """``mask_cross_entropy(conv_logits(x), targets, labels)`` (cross_entropy_loss.py:114-162) -> shape ``(1,)``, as ONE autograd
    node: the forward is one pass over ``x`` that leaves the loss and the compact gradient ``[N, H * W]``, the backward writes
    ``dx`` from it without reading ``x`` and sums ``dweight`` / ``dbias`` in a fixed order.  Only what ``requires_grad`` asks for
    is computed and stored; the upstream gradient is applied on the device.  ``targets [N, H, W]``.  ``valid_rows``: divide by
    ``max(1, #{n: 0 <= labels[n] < C}) * H * W`` instead of ``N * H * W``, the count taken on the device; the compact gradient is
    then kept undivided and the backward kernels apply the divisor, in as many launches as without it.  ``N == 0``: a zero
    connected to ``x``, ``weight`` and ``bias`` (the reference's ``mask_pred.sum()``).  A non-contiguous or ``channels_last`` ``x``
    costs one layout copy."""
    if _is_empty(x):
        _prep(x, weight, bias, labels)
        return _empty_result(x, (weight, bias), (1,))
    return _Loss.apply(x, weight, bias, labels, targets, tuple(weight.shape), bool(valid_rows))


def _agnostic_labels(labels, num_classes, valid_rows):
    """The label mapping of a ``class_agnostic`` head, shared with ``FusedMaskHeadTail``."""
    if valid_rows:
        return torch.where((labels >= 0) & (labels < num_classes), torch.zeros_like(labels), torch.full_like(labels, -1))
    return torch.zeros_like(labels)


class _SelectedPredictor(nn.Module):
    """What the class-selected predictor modules share: ``weight [C, Cin, 1, 1]`` and ``bias [C]`` (``C = 1`` for a
    ``class_agnostic`` head) with the initialisation ``FCNMaskHead.init_weights`` gives ``conv_logits``, the label mapping of the
    ``class_agnostic`` head, and the two ends of ``from_conv`` / ``to_conv``."""

    def __init__(self, in_channels, num_classes, class_agnostic=False):
        super().__init__()
        self.in_channels, self.num_classes, self.class_agnostic = int(in_channels), int(num_classes), bool(class_agnostic)
        out_channels = 1 if self.class_agnostic else self.num_classes
        self.weight = nn.Parameter(torch.empty(out_channels, self.in_channels, 1, 1))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.init_weights()

    def init_weights(self):
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.bias, 0)

    def _labels(self, labels, valid_rows=False):
        """The weight row of each RoI: its label, or row 0 of a ``class_agnostic`` head.  With ``valid_rows`` a ``class_agnostic``
        head keeps a padded row apart: row 0 for a label in ``[0, num_classes)``, the invalid -1 for any other."""
        return _agnostic_labels(labels, self.num_classes, valid_rows) if self.class_agnostic else labels

    @classmethod
    def _from_conv(cls, conv, class_agnostic, **kwargs):
        """A module of conv's shape, device and dtype with conv's parameters."""
        agnostic = conv.out_channels == 1 if class_agnostic is None else class_agnostic
        m = cls(conv.in_channels, conv.out_channels, class_agnostic=agnostic, **kwargs)
        m.to(device=conv.weight.device, dtype=conv.weight.dtype)
        _copy_params(m, conv)
        return m

    def _into_conv(self, conv):
        conv.to(device=self.weight.device, dtype=self.weight.dtype)
        _copy_params(conv, self)
        return conv


class ClassSelectedMaskPredictor(_SelectedPredictor):
    """Stands where ``FCNMaskHead.conv_logits`` stood (fcn_mask_head.py:106-111, ``predictor_cfg=dict(type='Conv')``): the same
    parameters - ``weight [C, Cin, 1, 1]``, ``bias [C]``, ``C = 1`` for a ``class_agnostic`` head - under the same ``state_dict``
    keys as ``nn.Conv2d(Cin, C, 1)``, so a reference checkpoint's ``mask_head.conv_logits.*`` loads unchanged, and the
    reference's initialisation (``kaiming_normal_(mode='fan_out', nonlinearity='relu')``, zero bias, fcn_mask_head.py:123-125)."""

    def forward(self, x, labels):
        """The selected logits ``[N, 1, H, W]``: ``pos_labels`` in training, ``det_labels`` at test time."""
        return class_mask_logits(x, self.weight, self.bias, self._labels(labels))

    def loss(self, x, labels, mask_targets, valid_rows=False):
        """``FCNMaskHead.loss`` (fcn_mask_head.py:147-177) on the head's features instead of its logits.  ``valid_rows``: the
        rows of the padded RoI pipeline (label ``num_classes`` = padding), divided by the device-counted number of real rows."""
        return dict(loss_mask=class_mask_loss(x, self.weight, self.bias, self._labels(labels, valid_rows), mask_targets, valid_rows))

    @classmethod
    def from_conv(cls, conv, class_agnostic=None):
        """From the reference head's ``conv_logits``; the parameters are copied bit for bit."""
        if not isinstance(conv, nn.Conv2d) or not _is_plain_1x1(conv):
            raise NotImplementedError("a plain 1x1 nn.Conv2d expected")
        return cls._from_conv(conv, class_agnostic)

    def to_conv(self):
        """The ``nn.Conv2d`` with these parameters: the full ``[N, C, H, W]`` logits for whoever needs them."""
        return self._into_conv(nn.Conv2d(self.in_channels, self.weight.size(0), 1))

    def extra_repr(self):
        return "in_channels=%d, num_classes=%d, class_agnostic=%s" % (self.in_channels, self.num_classes, self.class_agnostic)
