#!/usr/bin/env python3
"""Generate tests/golden/g31_mask_predictor.npz by RUNNING THE REFERENCE's own ``FCNMaskHead.forward`` and ``.loss`` on the CPU,
once in float64 and once in float32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mask_predictor.py <reference checkout>

``roi_heads/mask_heads/fcn_mask_head.py`` and ``losses/cross_entropy_loss.py`` are imported as they are, under placeholder
modules (as make_golden_mask_head.py imports the head): ``mmcv.cnn`` supplies ``build_conv_layer -> nn.Conv2d``,
``build_upsample_layer -> nn.ConvTranspose2d`` and a minimal ``ConvModule`` (convolution + ReLU), ``mmdet.models.builder`` a
``build_loss`` that instantiates the reference's ``CrossEntropyLoss(use_mask=True)``.

Per case a small head (``num_convs=1``, 8 channels, 5 x 5 RoI features -> 10 x 10 masks, 4 RoIs with repeated labels; one case
``class_agnostic``) runs forward and loss; a forward hook on ``conv_logits`` keeps its INPUT (the deconv + ReLU output), and
autograd gives the gradients of the loss with respect to that input and the layer's parameters.  Stored per case and precision
(``_f64`` / ``_f32``): x (the input of conv_logits), weight, bias, labels, targets, loss, dx, dweight, dbias.  The float32 head
holds the float64 head's parameters rounded once.

Asserted before anything is stored: in the reference's own float64 gradients every dweight / dbias row of a class that no RoI
has is EXACTLY zero - the equivalence the class-selected predictor rests on.
"""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden_targets import _Registry, _identity_decorator, _pkg        # noqa: E402

torch.set_num_threads(4)

# name -> (num_classes, class_agnostic, labels, soft targets)
CASES = {
    "multi": (5, False, [4, 0, 2, 2], False),
    "soft": (5, False, [1, 1, 1, 3], True),
    "agnostic": (5, True, [4, 0, 2, 2], False),
}
CIN, FEAT, N = 8, 5, 4


class ConvModule(nn.Module):
    """The part of mmcv's ConvModule the head uses without norm_cfg: convolution, then ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, conv_cfg=None, norm_cfg=None):
        super().__init__()
        assert conv_cfg is None and norm_cfg is None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding)
        self.activate = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.activate(self.conv(x))


def build_conv_layer(cfg, *args, **kwargs):
    assert cfg is None or cfg.get("type") in (None, "Conv", "Conv2d")
    return nn.Conv2d(*args, **kwargs)


def build_upsample_layer(cfg):
    cfg = dict(cfg)
    assert cfg.pop("type") == "deconv"
    return nn.ConvTranspose2d(**cfg)


def reference(ref_root):
    mm = os.path.join(ref_root, "instance_segmentation", "mmdet")
    losses = {}

    def build_loss(cfg):
        cfg = dict(cfg)
        return getattr(losses["ce"], cfg.pop("type"))(**cfg)

    _pkg("mmcv", jit=_identity_decorator)
    _pkg("mmcv.ops")
    _pkg("mmcv.ops.carafe", CARAFEPack=type("CARAFEPack", (), {}))
    _pkg("mmcv.cnn", ConvModule=ConvModule, build_conv_layer=build_conv_layer, build_upsample_layer=build_upsample_layer)

    class BaseModule(nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()

        def init_weights(self):
            pass

    _pkg("mmcv.runner", BaseModule=BaseModule, ModuleList=nn.ModuleList, auto_fp16=_identity_decorator, force_fp32=_identity_decorator)
    _pkg("mmdet")
    _pkg("mmdet.core", mask_target=None)
    _pkg("mmdet.models")
    _pkg("mmdet.models.builder", HEADS=_Registry(), LOSSES=_Registry(), build_loss=build_loss)
    _pkg("mmdet.models.losses", os.path.join(mm, "models", "losses"))
    losses["ce"] = importlib.import_module("mmdet.models.losses.cross_entropy_loss")
    spec = importlib.util.spec_from_file_location("ref_fcn_mask_head", os.path.join(mm, "models", "roi_heads", "mask_heads", "fcn_mask_head.py"))
    head = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(head)
    return head


def run(head_mod, name, dt, state=None):
    c, agnostic, labels, soft = CASES[name]
    g = torch.Generator().manual_seed(31 + sorted(CASES).index(name))
    torch.manual_seed(310 + sorted(CASES).index(name))
    head = head_mod.FCNMaskHead(num_convs=1, in_channels=CIN, conv_out_channels=CIN, num_classes=c, class_agnostic=agnostic)
    head.init_weights()
    with torch.no_grad():
        head.conv_logits.bias.copy_(torch.randn(head.conv_logits.bias.shape, generator=g) * 0.1)     # a zero bias would hide it
    head = head.to(dt)
    if state is not None:
        head.load_state_dict({k: v.to(dt) for k, v in state.items()})
    feats = torch.randn(N, CIN, FEAT, FEAT, generator=g, dtype=torch.float64).to(dt)
    u = torch.rand(N, 2 * FEAT, 2 * FEAT, generator=g, dtype=torch.float64)
    targets = (u if soft else (u < 0.5).double()).to(dt)
    labels = torch.tensor(labels, dtype=torch.int64)
    kept = {}

    def hook(mod, inp):
        inp[0].retain_grad()
        kept["x"] = inp[0]
    head.conv_logits.register_forward_pre_hook(hook)
    mask_pred = head(feats)
    assert mask_pred.shape == (N, 1 if agnostic else c, 2 * FEAT, 2 * FEAT) and mask_pred.dtype == dt
    loss = head.loss(mask_pred, targets, labels)["loss_mask"]
    assert loss.shape == (1,)
    loss.sum().backward()
    out = dict(x=kept["x"].detach(), weight=head.conv_logits.weight.detach(), bias=head.conv_logits.bias.detach(), labels=labels,
               targets=targets, loss=loss.detach(), dx=kept["x"].grad, dweight=head.conv_logits.weight.grad,
               dbias=head.conv_logits.bias.grad)
    return {k: v.numpy().copy() for k, v in out.items()}, {k: v.detach().clone() for k, v in head.state_dict().items()}


def main():
    head_mod = reference(sys.argv[1])
    store = {}
    for name in CASES:
        c, agnostic, labels, _ = CASES[name]
        r64, state = run(head_mod, name, torch.float64)
        r32, _ = run(head_mod, name, torch.float32, state)
        assert r64["x"].dtype == np.float64 and r32["x"].dtype == np.float32 and (r64["x"] >= 0).all()
        unsel = np.ones(r64["dweight"].shape[0], dtype=bool)
        unsel[[0] if agnostic else labels] = False
        for r in (r64, r32):
            assert not r["dweight"][unsel].any() and not r["dbias"][unsel].any(), name
            assert r["dweight"][~unsel].any(1).all()
        for k, v in r64.items():
            store["%s_%s_f64" % (name, k)] = v
        for k, v in r32.items():
            store["%s_%s_f32" % (name, k)] = v
        print("%-9s loss %.9f  f32 loss error %.2e  unselected rows %d" % (name, float(r64["loss"][0]),
                                                                          abs(float(r32["loss"][0]) - float(r64["loss"][0])), int(unsel.sum())))
    path = os.path.join(HERE, "g31_mask_predictor.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
