#!/usr/bin/env python3
"""Generate tests/golden/g35_normed_mask_predictor.npz by RUNNING THE REFERENCE's own ``FCNMaskHead`` with
``predictor_cfg=dict(type='NormedConv2d', tempearture=20)`` - forward and ``.loss`` - on the CPU, once in float64 and once in
float32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_normed_mask_predictor.py <reference checkout>

On the pattern of make_golden_mask_predictor.py: ``roi_heads/mask_heads/fcn_mask_head.py`` and ``losses/cross_entropy_loss.py`` are
imported as they are under placeholder modules.  Here ``build_conv_layer`` hands ``type='NormedConv2d'`` to the reference's OWN
class, loaded from ``models/utils/normed_predictor.py`` (as make_golden_mmdet.py loads it: ``mmcv.cnn.CONV_LAYERS`` and
``mmdet.models.utils.builder.LINEAR_LAYERS`` are placeholder registries).

Per case a small head (``num_convs=1``, 8 channels, 5 x 5 RoI features -> 10 x 10 masks, 4 RoIs) runs forward and loss; a forward
pre-hook on ``conv_logits`` keeps its INPUT, and autograd gives the gradients of the loss with respect to that input and the
layer's parameters.  In the case ``zeropix`` the same hook first zeroes three whole pixels of that input in every channel, so the
``r == 0`` branch (the sub-gradient of the norm at 0) is the reference's.  Stored per case and precision (``_f64`` / ``_f32``):
x, weight, bias, labels, targets, loss, dx, dweight, dbias, and ``cfg = (tempearture, power, eps)``.

Asserted before anything is stored: in the reference's own gradients every dweight / dbias row of a class that no RoI has is
EXACTLY zero - the equivalence the class-selected predictor rests on.
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
from make_golden_mask_predictor import ConvModule, build_upsample_layer        # noqa: E402
from make_golden_targets import _Registry, _identity_decorator, _pkg           # noqa: E402

torch.set_num_threads(4)

# name -> (num_classes, class_agnostic, labels, soft targets, power, pixels of conv_logits' input zeroed in every channel)
CASES = {
    "multi": (5, False, [4, 0, 2, 2], False, 1.0, ()),
    "soft": (5, False, [1, 1, 1, 3], True, 1.0, ()),
    "agnostic": (5, True, [4, 0, 2, 2], False, 1.0, ()),
    "power2": (5, False, [3, 0, 3, 1], False, 2, ()),
    "zeropix": (5, False, [4, 0, 2, 2], False, 1.0, ((0, 0, 0), (1, 4, 7), (3, 9, 9))),       # (roi, y, x)
}
CIN, FEAT, N, TEMP = 8, 5, 4, 20
REF = {}


def build_conv_layer(cfg, *args, **kwargs):
    cfg = dict(cfg)
    assert cfg.pop("type") == "NormedConv2d"
    return REF["normed"].NormedConv2d(*args, **kwargs, **cfg)


def reference(ref_root):
    mm = os.path.join(ref_root, "instance_segmentation", "mmdet")
    losses = {}

    def build_loss(cfg):
        cfg = dict(cfg)
        return getattr(losses["ce"], cfg.pop("type"))(**cfg)

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    _pkg("mmcv", jit=_identity_decorator)
    _pkg("mmcv.ops")
    _pkg("mmcv.ops.carafe", CARAFEPack=type("CARAFEPack", (), {}))
    _pkg("mmcv.cnn", ConvModule=ConvModule, build_conv_layer=build_conv_layer, build_upsample_layer=build_upsample_layer,
         CONV_LAYERS=_Registry())

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
    _pkg("mmdet.models.utils")
    _pkg("mmdet.models.utils.builder", LINEAR_LAYERS=_Registry())
    try:
        import pandas  # noqa: F401
    except ImportError:                                  # only IIFNormedLinear reads a CSV
        _pkg("pandas")
    REF["normed"] = load("mmdet.models.utils.normed_predictor", os.path.join(mm, "models", "utils", "normed_predictor.py"))
    return load("ref_fcn_mask_head", os.path.join(mm, "models", "roi_heads", "mask_heads", "fcn_mask_head.py"))


def run(head_mod, name, dt, state=None):
    c, agnostic, labels, soft, power, zeroed = CASES[name]
    g = torch.Generator().manual_seed(35 + sorted(CASES).index(name))
    torch.manual_seed(350 + sorted(CASES).index(name))
    head = head_mod.FCNMaskHead(num_convs=1, in_channels=CIN, conv_out_channels=CIN, num_classes=c, class_agnostic=agnostic,
                                predictor_cfg=dict(type="NormedConv2d", tempearture=TEMP, power=power))
    assert type(head.conv_logits) is REF["normed"].NormedConv2d and head.conv_logits.tempearture == TEMP
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
    keep = torch.ones(N, 1, 2 * FEAT, 2 * FEAT, dtype=dt)
    for n, y, x in zeroed:
        keep[n, 0, y, x] = 0
    kept = {}

    def hook(mod, inp):
        x = inp[0] * keep if zeroed else inp[0]
        x.retain_grad()
        kept["x"] = x
        return (x,)
    head.conv_logits.register_forward_pre_hook(hook)
    mask_pred = head(feats)
    assert mask_pred.shape == (N, 1 if agnostic else c, 2 * FEAT, 2 * FEAT) and mask_pred.dtype == dt
    loss = head.loss(mask_pred, targets, labels)["loss_mask"]
    assert loss.shape == (1,)
    loss.sum().backward()
    for n, y, x in zeroed:
        assert not kept["x"][n, :, y, x].any()
    out = dict(x=kept["x"].detach(), weight=head.conv_logits.weight.detach(), bias=head.conv_logits.bias.detach(), labels=labels,
               targets=targets, loss=loss.detach(), dx=kept["x"].grad, dweight=head.conv_logits.weight.grad,
               dbias=head.conv_logits.bias.grad,
               cfg=torch.tensor([head.conv_logits.tempearture, head.conv_logits.power, head.conv_logits.eps], dtype=torch.float64))
    return {k: v.numpy().copy() for k, v in out.items()}, {k: v.detach().clone() for k, v in head.state_dict().items()}


def main():
    head_mod = reference(sys.argv[1])
    store = {}
    for name in CASES:
        c, agnostic, labels = CASES[name][:3]
        r64, state = run(head_mod, name, torch.float64)
        r32, _ = run(head_mod, name, torch.float32, state)
        assert r64["x"].dtype == np.float64 and r32["x"].dtype == np.float32 and (r64["x"] >= 0).all()
        unsel = np.ones(r64["dweight"].shape[0], dtype=bool)
        unsel[[0] if agnostic else labels] = False
        for r in (r64, r32):
            assert np.isfinite(r["dx"]).all() and np.isfinite(r["dweight"]).all()
            assert not r["dweight"][unsel].any() and not r["dbias"][unsel].any(), name
            assert r["dweight"][~unsel].reshape(int((~unsel).sum()), -1).any(1).all()
        for k, v in r64.items():
            store["%s_%s_f64" % (name, k)] = v
        for k, v in r32.items():
            store["%s_%s_f32" % (name, k)] = v
        print("%-9s loss %.9f  f32 loss error %.2e  unselected rows %d" % (name, float(r64["loss"][0]),
                                                                          abs(float(r32["loss"][0]) - float(r64["loss"][0])), int(unsel.sum())))
    path = os.path.join(HERE, "g35_normed_mask_predictor.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
