"""The mask head's tail fused: ``upsample`` (2x2 / stride-2 deconvolution) + ReLU + the class-selected ``conv_logits``
(csrc/mask_tail.hip).

``FCNMaskHead.forward`` (instance_segmentation/mmdet/models/roi_heads/mask_heads/fcn_mask_head.py:127-136) ends with
``x = self.relu(self.upsample(x)); mask_pred = self.conv_logits(x)``.  The tensor between the two layers is
``[N, Co, 2h, 2w]`` float32 - 205.5 MB at the LVIS training shape (256 RoIs, 256 channels, 28 x 28), and as much again for its
gradient.  A ``ConvTranspose2d`` with ``kernel = stride = 2`` is a plain GEMM (each input pixel's ``Ci`` vector times a
``[Ci, 4 Co]`` matrix gives the four output pixels below it), and the class-selected predictor (mmdet_mask_predictor.py) keeps one
dot product over ``Co`` per output pixel, so the activation lives in registers between the GEMM and the dot product and is never
stored, forward or backward.  With ``l = labels[n]``, ``P = (2i + a, 2j + b)``::

    pre[n, co, P] = up_bias[co] + sum_ci f[n, ci, i, j] * up_weight[ci, co, a, b]
    z[n, P]       = bias[l] + sum_co weight[l, co] * max(pre[n, co, P], 0)

  ``upsampled_class_mask_logits(f, up_weight, up_bias, weight, bias, labels)``            ``[N, 1, 2h, 2w]``, differentiable
  ``upsampled_class_mask_loss(f, up_weight, up_bias, weight, bias, labels, targets)``     fused with ``mask_cross_entropy``, ``(1,)``
  ``FusedMaskHeadTail``                            the module that stands where ``upsample``, ``relu`` and ``conv_logits`` stood

The forward is one MFMA kernel (fp32-input MFMA: exact float32, bit for bit an ordered ``fmaf`` chain) that leaves ``z`` or, with
targets, the loss and the compact gradient ``[N, 2h, 2w]``.  The backward recomputes the GEMM once - which yields the sign of
``pre`` as a bitmask (``N * Co * 4hw / 8`` bytes) and the per-RoI rows of ``dweight`` / ``dbias`` - and runs two more GEMMs whose
second operand ``g * weight[l, co] * [pre > 0]`` is generated on the fly: ``df`` (every element written once) and ``dup_weight``
(split over RoI ranges, the partials summed in range order).  The gradient at ``pre == 0`` is zero, as in torch.  No float
atomics: the same bits from call to call.

``f`` is float32 or bfloat16 (widened exactly; ``df`` comes back in that dtype), the parameters float32.  A non-contiguous or
``channels_last`` ``f`` costs one layout copy.  ``weight`` rows are read through their stride.  A label outside ``[0, C)``
contributes zero loss, a zero ``df`` slice and nothing to any parameter gradient, and that RoI's ``f`` and targets are not read.
The divisor is ``N * 4hw``; with ``valid_rows=True`` it is ``max(1, K) * 4hw``, ``K`` the number of RoIs with a label in
``[0, C)``, counted on the device (the padded RoI pipeline: a padded row neither adds a term nor dilutes the loss, nothing is read
back; ``K = 0`` gives exactly 0 and exact zero gradients).  Limits: scale factor 2, ``1 <= Ci, Co <= 1024``, ``h * w <= 1024``,
``N <= 65535``.

Not offered: the four 3x3 ``convs`` in front, ``nearest`` / ``bilinear`` / ``carafe`` upsampling, other scale factors, float16,
bf16 MFMA arithmetic, ``class_weight``, a native ``channels_last`` kernel.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .mmdet_mask_predictor import _TILE, _agnostic_labels, _copy_params, _empty_result, _is_empty, _is_plain_1x1, _ld, _needs, _up

_MAX_C, _MAX_HW, _MAX_N = 1024, 1024, 65535


def _prep(f, up_weight, up_bias, weight, bias, labels):
    """Checks in the order devices, shapes, dtypes; returns (f NCHW-contiguous, up_weight contiguous and 16-byte aligned, up_bias,
    weight [C, Co] with unit column stride, bias, labels int64, N, C, Ci, Co, h, w)."""
    for t in (f, up_weight, weight, labels):
        if not isinstance(t, torch.Tensor):
            raise ValueError("fused mask head tail: tensors expected")
    _lib.require_gpu(f, up_weight, up_bias, weight, bias, labels)
    if f.dim() != 4:
        raise ValueError("f must be [N, Ci, h, w] (got %s)" % (tuple(f.shape),))
    n, ci, h, w = f.shape
    if up_weight.dim() != 4 or up_weight.size(0) != ci or tuple(up_weight.shape[2:]) != (2, 2):
        raise ValueError("up_weight must be [Ci, Co, 2, 2] with Ci = %d (got %s)" % (ci, tuple(up_weight.shape)))
    co = up_weight.size(1)
    if up_bias is not None and tuple(up_bias.shape) != (co,):
        raise ValueError("up_bias must be [Co] (got %s)" % (tuple(up_bias.shape),))
    if weight.dim() == 4:
        if weight.size(2) != 1 or weight.size(3) != 1:
            raise ValueError("weight must be [C, Co] or [C, Co, 1, 1] (got %s)" % (tuple(weight.shape),))
        weight = weight[:, :, 0, 0]
    elif weight.dim() != 2:
        raise ValueError("weight must be [C, Co] or [C, Co, 1, 1] (got %s)" % (tuple(weight.shape),))
    c = weight.size(0)
    if weight.size(1) != co:
        raise ValueError("weight has %d input channels, up_weight gives %d" % (weight.size(1), co))
    if bias is not None and tuple(bias.shape) != (c,):
        raise ValueError("bias must be [C] (got %s)" % (tuple(bias.shape),))
    if labels.numel() != n:
        raise ValueError("one label per RoI expected (%d labels, %d RoIs)" % (labels.numel(), n))
    if c < 1 or not 1 <= ci <= _MAX_C or not 1 <= co <= _MAX_C or not 1 <= h * w <= _MAX_HW or n > _MAX_N:
        raise ValueError("fused mask head tail: C >= 1, 1 <= Ci, Co <= %d, 1 <= h * w <= %d, N <= %d" % (_MAX_C, _MAX_HW, _MAX_N))
    if f.dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError("float32 / bfloat16 f only (got %s)" % f.dtype)
    for p in (up_weight, up_bias, weight, bias):
        if p is not None and p.dtype != torch.float32:
            raise NotImplementedError("float32 parameters only (got %s)" % p.dtype)
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise NotImplementedError("integer labels only (got %s)" % labels.dtype)
    f = f.contiguous()
    up_weight = up_weight.contiguous()
    if up_weight.data_ptr() % 16:
        up_weight = up_weight.clone()
    if up_bias is not None:
        up_bias = up_bias.contiguous()
    if weight.stride(1) != 1 or (c > 1 and weight.stride(0) < co):
        weight = weight.contiguous()
    if bias is not None:
        bias = bias.contiguous()
    labels = labels.reshape(-1).to(torch.int64).contiguous()
    return f, up_weight, up_bias, weight, bias, labels, n, c, ci, co, h, w


def _forward(f, up_weight, up_bias, weight, bias, labels, targets, need_g0, valid_rows=False):
    """One forward launch.  targets None: returns z [N, 1, 2h, 2w]; else (loss (1,), g0 [N, 4hw] or None).  valid_rows: g0 is
    left undivided and the last result is the device scalar 1 / divisor (None otherwise)."""
    fc, uw, ub, w2, b, lb, n, c, ci, co, h, w = _prep(f, up_weight, up_bias, weight, bias, labels)
    dev, hw = fc.device, h * w
    z = g0 = rows = loss = t = inv = None
    if targets is None:
        z = torch.empty((n, 1, 2 * h, 2 * w), dtype=torch.float32, device=dev)
    else:
        if not isinstance(targets, torch.Tensor) or targets.numel() != n * 4 * hw:
            raise ValueError("targets must be [N, 2h, 2w] (got %s for f %s)" % (tuple(getattr(targets, "shape", ())), tuple(f.shape)))
        _lib.require_gpu(targets)
        t = targets.detach().reshape(n, 4 * hw).to(torch.float32).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        rows = torch.empty(n * ((hw + _TILE - 1) // _TILE), dtype=torch.float32, device=dev)
        g0 = torch.empty((n, 4 * hw), dtype=torch.float32, device=dev) if need_g0 else None
    if valid_rows and targets is not None:
        inv = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().iif_mask_tail_loss_fwd(_lib.ptr(fc), _lib.dtype_code(fc), _lib.ptr(uw), _lib.ptr(ub), _lib.ptr(w2),
                                                     _ld(w2), _lib.ptr(b), _lib.ptr(lb), _lib.ptr(t), n, c, ci, co, h, w, 1,
                                                     _lib.ptr(g0), _lib.ptr(rows), _lib.ptr(loss), _lib.ptr(inv), _lib.stream_ptr()),
                   "iif_mask_tail_loss_fwd")
    else:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().iif_mask_tail_fwd(_lib.ptr(fc), _lib.dtype_code(fc), _lib.ptr(uw), _lib.ptr(ub), _lib.ptr(w2), _ld(w2),
                                                _lib.ptr(b), _lib.ptr(lb), _lib.ptr(t), n, c, ci, co, h, w, _lib.ptr(z), _lib.ptr(g0),
                                                _lib.ptr(rows), _lib.ptr(loss), _lib.ptr(status), _lib.stream_ptr()),
                   "iif_mask_tail_fwd")
    return (fc, uw, ub, w2, lb), (n, c, ci, co, h, w), (z if targets is None else loss), g0, inv


def _backward(saved, dims, g, up, needs, inv=None):
    """The backward entries on the compact gradient g [N, 4hw] (times the device scalar `up`, or 1).  needs: f, up_weight, up_bias,
    weight, bias.  inv: the device scalar 1 / divisor of a forward that stored g undivided (valid_rows); the kernels multiply
    it in.  Returns the five gradients (None where not asked for)."""
    fc, uw, ub, w2, lb = saved
    n, c, ci, co, h, w = dims
    need_f, need_uw, need_ub, need_w, need_b = needs
    L, st, dev, hw = _lib.lib(), _lib.stream_ptr(), g.device, h * w
    df = duw = dub = dw = db = None
    signs = torch.empty((n, (hw + 31) // 32, 4 * co), dtype=torch.int32, device=dev)
    rows = torch.empty((n, co + 1), dtype=torch.float32, device=dev) if (need_w or need_b) else None
    if inv is None:
        _lib.check(L.iif_mask_tail_bwd_rows(_lib.ptr(fc), _lib.dtype_code(fc), _lib.ptr(uw), _lib.ptr(ub), _lib.ptr(g), _lib.ptr(up),
                                            _lib.ptr(lb), n, c, ci, co, h, w, _lib.ptr(signs), _lib.ptr(rows), st),
                   "iif_mask_tail_bwd_rows")
    else:
        _lib.check(L.iif_mask_tail_loss_bwd_rows(_lib.ptr(fc), _lib.dtype_code(fc), _lib.ptr(uw), _lib.ptr(ub), _lib.ptr(g),
                                                 _lib.ptr(up), _lib.ptr(inv), _lib.ptr(lb), n, c, ci, co, h, w, _lib.ptr(signs),
                                                 _lib.ptr(rows), st), "iif_mask_tail_loss_bwd_rows")
    if rows is not None:
        if need_w:
            dw = torch.empty((c, co), dtype=torch.float32, device=dev)
        if need_b:
            db = torch.empty(c, dtype=torch.float32, device=dev)
        _lib.check(L.iif_mask_tail_bwd_classes(_lib.ptr(rows), _lib.ptr(lb), n, c, co, _lib.ptr(dw), _lib.ptr(db), st),
                   "iif_mask_tail_bwd_classes")
    if need_f:
        df = torch.empty((n, ci, h, w), dtype=fc.dtype, device=dev)
        if inv is None:
            _lib.check(L.iif_mask_tail_bwd_input(_lib.ptr(g), _lib.ptr(up), _lib.ptr(uw), _lib.ptr(w2), _ld(w2), _lib.ptr(lb),
                                                 _lib.ptr(signs), n, c, ci, co, h, w, _lib.ptr(df), _lib.dtype_code(df), st),
                       "iif_mask_tail_bwd_input")
        else:
            _lib.check(L.iif_mask_tail_loss_bwd_input(_lib.ptr(g), _lib.ptr(up), _lib.ptr(inv), _lib.ptr(uw), _lib.ptr(w2), _ld(w2),
                                                      _lib.ptr(lb), _lib.ptr(signs), n, c, ci, co, h, w, _lib.ptr(df),
                                                      _lib.dtype_code(df), st), "iif_mask_tail_loss_bwd_input")
    if need_uw or need_ub:
        splits = L.iif_mask_tail_splits(n, ci, co)
        partial = torch.empty(splits * (ci + 1) * 4 * co, dtype=torch.float32, device=dev)
        if need_uw:
            duw = torch.empty((ci, co, 2, 2), dtype=torch.float32, device=dev)
        if need_ub:
            dub = torch.empty(co, dtype=torch.float32, device=dev)
        if inv is None:
            _lib.check(L.iif_mask_tail_bwd_params(_lib.ptr(fc), _lib.dtype_code(fc), _lib.ptr(g), _lib.ptr(up), _lib.ptr(w2), _ld(w2),
                                                  _lib.ptr(lb), _lib.ptr(signs), n, c, ci, co, h, w, _lib.ptr(partial),
                                                  _lib.ptr(duw), _lib.ptr(dub), st), "iif_mask_tail_bwd_params")
        else:
            _lib.check(L.iif_mask_tail_loss_bwd_params(_lib.ptr(fc), _lib.dtype_code(fc), _lib.ptr(g), _lib.ptr(up), _lib.ptr(inv),
                                                       _lib.ptr(w2), _ld(w2), _lib.ptr(lb), _lib.ptr(signs), n, c, ci, co, h, w,
                                                       _lib.ptr(partial), _lib.ptr(duw), _lib.ptr(dub), st),
                       "iif_mask_tail_loss_bwd_params")
    return df, duw, dub, dw, db


def _det(t):
    return None if t is None else t.detach()


class _Logits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, up_weight, up_bias, weight, bias, labels, wshape):
        saved, dims, z, _, _ = _forward(f.detach(), up_weight.detach(), _det(up_bias), weight.detach(), _det(bias), labels, None, False)
        ctx.save_for_backward(*saved)
        ctx.meta = (dims, wshape)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        dims, wshape = ctx.meta
        needs = ctx.needs_input_grad[:5]                 # (False for a bias that is None)
        if not any(needs):
            return (None,) * 7
        n, hw4 = dims[0], 4 * dims[4] * dims[5]
        g = gz.detach().reshape(n, hw4).to(torch.float32).contiguous()
        df, duw, dub, dw, db = _backward(ctx.saved_tensors, dims, g, None, needs)
        return df, duw, dub, None if dw is None else dw.reshape(wshape), db, None, None


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, up_weight, up_bias, weight, bias, labels, targets, wshape, valid_rows):
        need = any(_needs(f, up_weight, up_bias, weight, bias))
        saved, dims, loss, g0, inv = _forward(f.detach(), up_weight.detach(), _det(up_bias), weight.detach(), _det(bias), labels,
                                              targets, need, valid_rows)
        if need:
            ctx.save_for_backward(*saved, g0, inv)
        ctx.meta = (dims, wshape, need)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gl):
        dims, wshape, need = ctx.meta
        needs = ctx.needs_input_grad[:5]                 # (False for a bias that is None)
        if not need or not any(needs):
            return (None,) * 9
        *saved, g0, inv = ctx.saved_tensors
        df, duw, dub, dw, db = _backward(saved, dims, g0, _up(gl), needs, inv)
        return (df, duw, dub, None if dw is None else dw.reshape(wshape), db) + (None,) * 4


def upsampled_class_mask_logits(f, up_weight, up_bias, weight, bias, labels):
    """``conv_logits(relu(upsample(f)))[range(N), labels][:, None]`` -> ``[N, 1, 2h, 2w]`` float32 without the activation between
    the layers.  ``f [N, Ci, h, w]`` float32 / bfloat16; ``up_weight [Ci, Co, 2, 2]`` and ``up_bias [Co]`` (or ``None``) as in
    ``nn.ConvTranspose2d(Ci, Co, 2, stride=2)``; ``weight [C, Co]`` or ``[C, Co, 1, 1]``; ``bias [C]`` or ``None``; ``labels [N]``
    integer.  Differentiable in all five tensors (not twice).  Feeds ``paste_masks`` / ``get_seg_masks(class_agnostic=True)``."""
    if _is_empty(f):
        _prep(f, up_weight, up_bias, weight, bias, labels)
        return _empty_result(f, (up_weight, up_bias, weight, bias), (0, 1, 2 * f.size(2), 2 * f.size(3)))
    return _Logits.apply(f, up_weight, up_bias, weight, bias, labels, tuple(weight.shape))


def upsampled_class_mask_loss(f, up_weight, up_bias, weight, bias, labels, targets, valid_rows=False):
    """``mask_cross_entropy(conv_logits(relu(upsample(f))), targets, labels)`` (cross_entropy_loss.py:114-162) -> shape ``(1,)``
    as ONE autograd node.  Only what ``requires_grad`` asks for is computed; the upstream gradient is applied on the device.
    ``targets [N, 2h, 2w]``.  ``valid_rows``: divide by ``max(1, #{n: 0 <= labels[n] < C}) * 4hw`` instead of ``N * 4hw``, the
    count taken on the device; the backward kernels apply the divisor, in as many launches as without it.  ``N == 0``: a zero
    connected to every input."""
    if _is_empty(f):
        _prep(f, up_weight, up_bias, weight, bias, labels)
        return _empty_result(f, (up_weight, up_bias, weight, bias), (1,))
    return _Loss.apply(f, up_weight, up_bias, weight, bias, labels, targets, tuple(weight.shape), bool(valid_rows))


class _Params(nn.Module):
    """A bare weight / bias pair: gives the parameters the state-dict prefix of the layer they come from."""

    def __init__(self, weight_shape, bias_len):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(weight_shape))
        self.bias = nn.Parameter(torch.empty(bias_len))


class FusedMaskHeadTail(nn.Module):
    """Stands where ``FCNMaskHead``'s ``upsample`` (``deconv``, scale factor 2), ``relu`` and ``conv_logits`` stood
    (fcn_mask_head.py:84-111).  The parameters sit under the reference's state-dict keys - ``upsample.weight [Ci, Co, 2, 2]``,
    ``upsample.bias [Co]``, ``conv_logits.weight [C, Co, 1, 1]``, ``conv_logits.bias [C]`` (``C = 1`` for a ``class_agnostic``
    head) - so a reference checkpoint's ``mask_head.*`` loads unchanged, with the reference's initialisation
    (``kaiming_normal_(mode='fan_out', nonlinearity='relu')``, zero biases, fcn_mask_head.py:115-125)."""

    def __init__(self, in_channels, conv_out_channels, num_classes, class_agnostic=False):
        super().__init__()
        self.in_channels, self.conv_out_channels = int(in_channels), int(conv_out_channels)
        self.num_classes, self.class_agnostic = int(num_classes), bool(class_agnostic)
        out_channels = 1 if self.class_agnostic else self.num_classes
        self.upsample = _Params((self.in_channels, self.conv_out_channels, 2, 2), self.conv_out_channels)
        self.conv_logits = _Params((out_channels, self.conv_out_channels, 1, 1), out_channels)
        self.init_weights()

    def init_weights(self):
        for m in (self.upsample, self.conv_logits):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(m.bias, 0)

    def _labels(self, labels, valid_rows=False):
        return _agnostic_labels(labels, self.num_classes, valid_rows) if self.class_agnostic else labels

    def _args(self):
        return self.upsample.weight, self.upsample.bias, self.conv_logits.weight, self.conv_logits.bias

    def forward(self, f, labels):
        """The selected logits ``[N, 1, 2h, 2w]``: ``pos_labels`` in training, ``det_labels`` at test time."""
        return upsampled_class_mask_logits(f, *self._args(), self._labels(labels))

    def loss(self, f, labels, mask_targets, valid_rows=False):
        """``FCNMaskHead.loss`` (fcn_mask_head.py:147-177) on the input of ``upsample`` instead of the logits.  ``valid_rows``: the
        rows of the padded RoI pipeline (label ``num_classes`` = padding), divided by the device-counted number of real rows."""
        return dict(loss_mask=upsampled_class_mask_loss(f, *self._args(), self._labels(labels, valid_rows), mask_targets, valid_rows))

    @classmethod
    def from_modules(cls, upsample, conv_logits, class_agnostic=None):
        """From the reference head's ``upsample`` and ``conv_logits``; the parameters are copied bit for bit."""
        u, c = upsample, conv_logits
        if not isinstance(u, nn.ConvTranspose2d) or u.kernel_size != (2, 2) or u.stride != (2, 2) or u.padding != (0, 0) \
                or u.output_padding != (0, 0) or u.groups != 1 or u.dilation != (1, 1):
            raise NotImplementedError("a 2x2 / stride-2 / no-padding nn.ConvTranspose2d expected")
        if not isinstance(c, nn.Conv2d) or not _is_plain_1x1(c):
            raise NotImplementedError("a plain 1x1 nn.Conv2d expected")
        if c.in_channels != u.out_channels:
            raise ValueError("conv_logits takes %d channels, upsample gives %d" % (c.in_channels, u.out_channels))
        agnostic = c.out_channels == 1 if class_agnostic is None else class_agnostic
        m = cls(u.in_channels, u.out_channels, c.out_channels, class_agnostic=agnostic)
        m.to(device=c.weight.device, dtype=c.weight.dtype)
        _copy_params(m.upsample, u)
        _copy_params(m.conv_logits, c)
        return m

    def to_modules(self):
        """``(nn.ConvTranspose2d, nn.Conv2d)`` with these parameters: the composed path for whoever needs it."""
        u = nn.ConvTranspose2d(self.in_channels, self.conv_out_channels, 2, stride=2)
        c = nn.Conv2d(self.conv_out_channels, self.conv_logits.weight.size(0), 1)
        for dst, src in ((u, self.upsample), (c, self.conv_logits)):
            dst.to(device=src.weight.device, dtype=src.weight.dtype)
            _copy_params(dst, src)
        return u, c

    def extra_repr(self):
        return "in_channels=%d, conv_out_channels=%d, num_classes=%d, class_agnostic=%s" % (
            self.in_channels, self.conv_out_channels, self.num_classes, self.class_agnostic)
