"""The RPN head trained at the sampled pixels only (csrc/rpn_head_sampled.hip): the backward of ``rpn_conv`` / ``rpn_cls`` /
``rpn_reg`` without a dense gradient and without the stored hidden activation.

Mirror of instance_segmentation/mmdet/models/dense_heads/rpn_head.py:30-44 (``_init_layers`` / ``forward_single``).  The loss
weights every unsampled anchor by 0 (anchor_head.py:373-421; ``rpn_loss``'s gradient is exactly zero off the sample) and proposals
take no gradient, so the gradient that reaches the score and delta maps sits at the pixels of at most ``B * (nep + num)`` sampled
anchors.  Everything the three convolutions' backward needs is formed from those pixels alone.

  * ``rpn_sampled_pixels``: ``iif_rpn_sampled_pixels``.  Slot ``e`` of the ``B * (nep + num)`` entries of an ``RPNStageTargets`` ->
    ``(image, level, y, x)`` (flat index -> pixel: ``(idx - level_start) // A_l``; anchor order ``(level, y, x, a)``).  Two sampled
    anchors of one pixel make ONE active slot: the lowest slot index owns the pixel (an integer ``atomicMin`` into a cleared
    owner map).  Three enqueued operations, no host read.
  * ``rpn_head_forward_sampled``: one autograd function over all levels.  Forward: the three modules' own convolutions under
    ``no_grad``, level by level - the maps are those of ``RPNHead.forward`` bit for bit - with the hidden activation freed per
    level; only the features and the parameters are saved.  Backward: nine launches; the hidden rows of the active slots are
    recomputed from gathered 3x3 patches, the six parameter gradients are sums over slots in fixed ranges, and ``d feats`` is one
    cleared arena (each level in its input's memory format) in which every pixel of an active pixel's 3x3 neighbourhood is
    written once.  Exact float32 on the fp32-input MFMA, no float atomics: the same bits from call to call.
    CONTRACT: the incoming gradient maps are zero outside ``sample`` - they are read at the active slots' pixels only.  This
    holds for ``rpn_loss`` on the same targets by construction; a caller that adds another loss on the maps must use the plain
    modules.
  * ``rpn_head_forward_train``: ``rpn_stage_targets`` (they do not depend on the head's outputs), ``rpn_sampled_pixels``,
    ``rpn_head_forward_sampled``, ``rpn_loss``; returns the loss dict and the detached maps for ``rpn_proposals_padded``.

Limits (beyond them a ``NotImplementedError`` that names the plain modules): those of ``rpn_stage_targets`` - 1 .. 16 images, at
most 8 levels, at most 16 base anchors, the same number on every level, ``sampler.num <= 1024``; float32 features and parameters;
``rpn_conv`` 3x3 / stride 1 / padding 1 and ``rpn_cls`` / ``rpn_reg`` plain 1x1 (no dilation, no groups, zero padding mode);
``Ci`` and ``Co`` multiples of 8, at most 2048 (the kernels read both 16 bytes at a time); no autocast.  The workspace of a
backward is about ``4 * S * (2 * 9 Ci + 2 Co) + 4 * 16 * Co * 9 Ci`` bytes for ``S = B * (nep + num)`` slots: 44 MB at ``S = 768``,
``Ci = Co = 256``.
"""
import collections
import ctypes

import torch

from . import _lib
from .mmdet_rpn_stage import MAX_IMAGES, _strides4, rpn_loss, rpn_stage_targets

__all__ = ["RPNSample", "rpn_sampled_pixels", "rpn_head_forward_sampled", "rpn_head_forward_train", "MAX_CHANNELS"]

MAX_CHANNELS = 2048

# ``owner [B, P]`` int32, ``P = sum_l H_l W_l``: per pixel the lowest slot index sampled there, -1 elsewhere; ``slots [S, 4]`` int32:
# ``(image, level, y, x)`` of a slot that owns its pixel, level -1 for an inactive slot; ``grid`` / ``featmap_sizes`` /
# ``num_base``: the targets' description of the anchor grid (host); ``num_images``: B.
RPNSample = collections.namedtuple("RPNSample", ["owner", "slots", "grid", "featmap_sizes", "num_base", "num_images"])


def _plain_hint(what):
    return NotImplementedError("%s; rpn_head_forward_sampled takes 1 .. %d images, <= 8 levels with the same <= 16 base anchors, "
                               "float32 features and parameters, a 3x3 / stride 1 / padding 1 rpn_conv, plain 1x1 rpn_cls and "
                               "rpn_reg, Ci and Co multiples of 8 up to %d - anything else goes through the plain modules "
                               "(rpn_reg(relu(rpn_conv(x))) under torch autograd) with rpn_loss" % (what, MAX_IMAGES, MAX_CHANNELS))


def rpn_sampled_pixels(targets):
    """The ``RPNSample`` of an ``RPNStageTargets``: device tensors only, three enqueued operations, no host read."""
    t = targets
    B, nep = t.pos_inds.shape
    num = t.neg_inds.size(1)
    L = len(t.featmap_sizes)
    nb = [int(t.grid.num_base[l]) for l in range(L)]
    if len(set(nb)) != 1:
        raise _plain_hint("levels with %s base anchors" % nb)
    _lib.require_gpu(t.pos_inds, t.neg_inds, t.counts)
    dev = t.pos_inds.device
    P = sum(h * w for h, w in t.featmap_sizes)
    if P < 1 or B * (nep + num) < 1:
        raise ValueError("rpn_sampled_pixels: no pixels or no slots")
    owner = torch.empty((B, P), dtype=torch.int32, device=dev)
    slots = torch.empty((B * (nep + num), 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().iif_rpn_sampled_pixels(ctypes.byref(t.grid), B, _lib.ptr(t.pos_inds), _lib.ptr(t.neg_inds), _lib.ptr(t.counts),
                                               _lib.ptr(t.pos_bbox_targets), nep, num, _lib.ptr(owner), _lib.ptr(slots),
                                               _lib.stream_ptr())
    _lib.check(rc, "iif_rpn_sampled_pixels")
    return RPNSample(owner, slots, t.grid, list(t.featmap_sizes), nb[0], B)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _check_conv(m, name, k, pad):
    if not isinstance(m, torch.nn.Conv2d) or isinstance(m, torch.nn.ConvTranspose2d):
        raise _plain_hint("%s is %s" % (name, type(m).__name__))
    if _pair(m.kernel_size) != (k, k) or _pair(m.stride) != (1, 1) or _pair(m.padding) != (pad, pad) or _pair(m.dilation) != (1, 1) \
            or m.groups != 1 or (pad and m.padding_mode != "zeros"):
        raise _plain_hint("%s is a %s" % (name, m))
    if m.weight.dtype != torch.float32:
        raise _plain_hint("%s has %s parameters" % (name, m.weight.dtype))


def _like_format(piece, x):
    B, C, H, W = x.shape
    if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
        return piece.view(B, H, W, C).permute(0, 3, 1, 2)
    return piece.view(B, C, H, W)


class _HeadSampled(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sample, modules, n_levels, *args):
        feats, params = args[:n_levels], args[n_levels:]
        conv, cls, reg = modules
        scores, deltas = [], []
        for x in feats:                                  # (grad mode is off in here: nothing of this is recorded)
            h = torch.nn.functional.relu(conv(x), inplace=True)
            scores.append(cls(h))
            deltas.append(reg(h))
            del h                                        # the hidden activation lives for its own level only
        ctx.sample, ctx.n_levels = sample, n_levels
        ctx.save_for_backward(*feats, *[p for p in params if p is not None])
        ctx.has = [p is not None for p in params]
        return tuple(scores) + tuple(deltas)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        L, sm = ctx.n_levels, ctx.sample
        saved = list(ctx.saved_tensors)
        feats = saved[:L]
        it = iter(saved[L:])
        w_conv, b_conv, w_cls, b_cls, w_reg, b_reg = [next(it) if h else None for h in ctx.has]
        dev = feats[0].device
        B, ci = feats[0].shape[:2]
        co, A = w_conv.size(0), sm.num_base
        g_scores, g_deltas = [], []
        for l in range(L):
            H, W = sm.featmap_sizes[l]
            for g, c, out in ((grads[l], A, g_scores), (grads[L + l], 4 * A, g_deltas)):
                if g is None:
                    g = torch.zeros((B, c, H, W), dtype=torch.float32, device=dev)
                out.append(g if g.dtype == torch.float32 else g.to(torch.float32))
        want_input = any(ctx.needs_input_grad[3:3 + L])
        d_feats = [None] * L
        if want_input:
            arena = torch.zeros((sum(x.numel() for x in feats),), dtype=torch.float32, device=dev)     # the one clear
            at = 0
            for l, x in enumerate(feats):
                d_feats[l] = _like_format(arena[at:at + x.numel()], x)
                at += x.numel()
        lv = (_lib.RpnHeadLevel * L)()
        for l, x in enumerate(feats):
            lv[l].feat, lv[l].feat_strides = _lib.ptr(x), _strides4(x)
            lv[l].grad_scores, lv[l].grad_score_strides = _lib.ptr(g_scores[l]), _strides4(g_scores[l])
            lv[l].grad_deltas, lv[l].grad_delta_strides = _lib.ptr(g_deltas[l]), _strides4(g_deltas[l])
            if want_input:
                lv[l].grad_feat, lv[l].grad_feat_strides = _lib.ptr(d_feats[l]), _strides4(d_feats[l])
        w_conv_c, w_cls_c, w_reg_c = w_conv.contiguous(), w_cls.contiguous(), w_reg.contiguous()
        if w_conv_c.data_ptr() % 16:                     # a view into a flat arena at an odd offset: the kernels read 16 bytes at a time
            w_conv_c = w_conv_c.clone()
        S = sm.slots.size(0)
        L_ = _lib.lib()
        ws_bytes = int(L_.iif_rpn_head_sampled_workspace_bytes(S, ci, co, A))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)                                  # this call's own
        f32 = dict(dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad[3 + L:]              # a frozen parameter's gradient is not formed
        shapes = (w_conv.shape, (co,), w_cls.shape, (A,), w_reg.shape, (4 * A,))
        d_w_conv, d_b_conv, d_w_cls, d_b_cls, d_w_reg, d_b_reg = [
            torch.empty(shape, **f32) if has and want else None for has, want, shape in zip(ctx.has, need, shapes)]
        with torch.cuda.device(dev):
            rc = L_.iif_rpn_head_sampled_bwd(
                ctypes.byref(sm.grid), lv, B, S, _lib.ptr(sm.owner), _lib.ptr(sm.slots), _lib.ptr(w_conv_c),
                _lib.ptr(b_conv.contiguous() if b_conv is not None else None), _lib.ptr(w_cls_c), _lib.ptr(w_reg_c), ci, co,
                _lib.ptr(d_w_conv), _lib.ptr(d_b_conv), _lib.ptr(d_w_cls), _lib.ptr(d_b_cls), _lib.ptr(d_w_reg), _lib.ptr(d_b_reg),
                _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
        _lib.check(rc, "iif_rpn_head_sampled_bwd")
        return (None, None, None) + tuple(d_feats) + (d_w_conv, d_b_conv, d_w_cls, d_b_cls, d_w_reg, d_b_reg)


def rpn_head_forward_sampled(feats, rpn_conv, rpn_cls, rpn_reg, sample):
    """``(cls_scores, bbox_preds)``: per level what ``rpn_cls(relu(rpn_conv(x)))`` and ``rpn_reg(relu(rpn_conv(x)))`` give, bit
    for bit, attached to ONE autograd node whose backward runs at ``sample``'s active slots only.  ``feats[l]`` float32
    ``[B, Ci, H_l, W_l]``, NCHW or ``channels_last``; the three modules ``torch.nn.Conv2d``.  The gradient maps that come back must be
    zero outside ``sample`` (``rpn_loss`` on the same targets: by construction).  Nothing synchronises the host."""
    L = len(sample.featmap_sizes)
    feats = list(feats)
    if len(feats) != L:
        raise ValueError("rpn_head_forward_sampled: %d levels in the sample, %d feature maps" % (L, len(feats)))
    _check_conv(rpn_conv, "rpn_conv", 3, 1)
    _check_conv(rpn_cls, "rpn_cls", 1, 0)
    _check_conv(rpn_reg, "rpn_reg", 1, 0)
    ci, co, A, B = rpn_conv.in_channels, rpn_conv.out_channels, sample.num_base, sample.num_images
    if not 1 <= B <= MAX_IMAGES:
        raise _plain_hint("%d images" % B)
    if ci % 8 or co % 8 or not 8 <= ci <= MAX_CHANNELS or not 8 <= co <= MAX_CHANNELS:
        raise _plain_hint("rpn_conv has %d -> %d channels" % (ci, co))
    if rpn_cls.in_channels != co or rpn_reg.in_channels != co or rpn_cls.out_channels != A or rpn_reg.out_channels != 4 * A:
        raise _plain_hint("rpn_cls %d -> %d and rpn_reg %d -> %d channels for %d hidden channels and %d base anchors"
                          % (rpn_cls.in_channels, rpn_cls.out_channels, rpn_reg.in_channels, rpn_reg.out_channels, co, A))
    for l, x in enumerate(feats):
        H, W = sample.featmap_sizes[l]
        if x.dim() != 4 or tuple(x.shape) != (B, ci, H, W):
            raise ValueError("rpn_head_forward_sampled: level %d: features [%d, %d, %d, %d] expected (got %s)"
                             % (l, B, ci, H, W, tuple(x.shape)))
        if x.dtype != torch.float32:
            raise _plain_hint("level %d has %s features" % (l, x.dtype))
    if torch.is_autocast_enabled(feats[0].device.type):  # the backward recomputes the hidden rows in float32
        raise _plain_hint("autocast is enabled")
    _lib.require_gpu(*feats, rpn_conv.weight, rpn_cls.weight, rpn_reg.weight)
    out = _HeadSampled.apply(sample, (rpn_conv, rpn_cls, rpn_reg), L, *feats, rpn_conv.weight, rpn_conv.bias, rpn_cls.weight,
                             rpn_cls.bias, rpn_reg.weight, rpn_reg.bias)
    return list(out[:L]), list(out[L:])


def rpn_head_forward_train(head_modules, anchor_generator, assigner, sampler, coder, loss_cls, loss_bbox, feats, gt_bboxes, img_metas,
                           gt_bboxes_ignore=None, allowed_border=-1, pos_weight=-1, keys=None):
    """``RPNHead.forward_train``'s loss half on the sampled path: ``(losses, cls_scores, bbox_preds)``.  ``head_modules``: the
    head's ``(rpn_conv, rpn_cls, rpn_reg)`` (or an object with these attributes); the other arguments and the keys of ``losses``
    are ``rpn_head_loss``'s.  The maps come back detached, ready for ``rpn_proposals_padded``."""
    if not isinstance(head_modules, (tuple, list)):
        head_modules = (head_modules.rpn_conv, head_modules.rpn_cls, head_modules.rpn_reg)
    rpn_conv, rpn_cls, rpn_reg = head_modules
    featmap_sizes = [tuple(int(v) for v in x.shape[-2:]) for x in feats]
    assert len(featmap_sizes) == anchor_generator.num_levels
    try:
        t = rpn_stage_targets(featmap_sizes, anchor_generator, [m["pad_shape"] for m in img_metas], [m["img_shape"] for m in img_metas],
                              gt_bboxes, assigner, sampler, coder, allowed_border=allowed_border, pos_weight=pos_weight, keys=keys,
                              gt_bboxes_ignore_list=gt_bboxes_ignore)
    except ValueError as e:
        if "per-image chain" in str(e):                  # a limit of the batch call: this path shares it
            raise _plain_hint(str(e))
        raise
    sample = rpn_sampled_pixels(t)
    cls_scores, bbox_preds = rpn_head_forward_sampled(feats, rpn_conv, rpn_cls, rpn_reg, sample)
    losses = rpn_loss(cls_scores, bbox_preds, t, loss_cls, loss_bbox, pos_weight=pos_weight)
    return losses, [s.detach() for s in cls_scores], [d.detach() for d in bbox_preds]
