#!/usr/bin/env python3
"""Generate tests/golden/g32_mask_tail.npz by RUNNING THE REFERENCE's own ``FCNMaskHead.forward`` and ``.loss`` on the CPU, once in
float64 and once in float32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mask_tail.py <reference checkout>

The head is ``FCNMaskHead(num_convs=0, in_channels=8, conv_out_channels=8)`` under the placeholder modules of
make_golden_mask_predictor.py (imported, not copied): without the 3x3 convolutions the head's input IS the input of ``upsample``,
so the whole run is upsample (ConvTranspose2d 2x2 / stride 2) -> ReLU -> conv_logits -> mask_cross_entropy.

Three heads as in g31 (multi-class, soft targets, class-agnostic), 4 RoIs of 5 x 5 features -> 10 x 10 masks.  The features and
the ``upsample`` parameters are overwritten with values on the dyadic grid of tests/mask_tail_cases.py, on which the ReLU's input
is exact in float32: no sign of it differs between the two precisions.  Stored per case and precision (``_f64`` / ``_f32``):
f, up_weight, up_bias, weight, bias, labels, targets, loss, df, dup_weight, dup_bias, dweight, dbias.  The float32 head holds the
float64 head's parameters rounded once.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_golden_mask_predictor import CASES, CIN, FEAT, N, reference        # noqa: E402

torch.set_num_threads(4)


def run(head_mod, name, dt, state=None):
    c, agnostic, labels, soft = CASES[name]
    g = torch.Generator().manual_seed(32 + sorted(CASES).index(name))
    torch.manual_seed(320 + sorted(CASES).index(name))
    head = head_mod.FCNMaskHead(num_convs=0, in_channels=CIN, conv_out_channels=CIN, num_classes=c, class_agnostic=agnostic)
    head.init_weights()
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)        # noqa: E731
    with torch.no_grad():
        head.conv_logits.bias.copy_(rn(*head.conv_logits.bias.shape) * 0.1)                       # a zero bias would hide it
        head.upsample.weight.copy_(torch.clamp(torch.round(rn(CIN, CIN, 2, 2) * (2.0 / CIN) ** 0.5 * 64), -64, 64) / 64)
        head.upsample.bias.copy_(torch.round(rn(CIN) * 6.4) / 64)
    head = head.to(dt)
    if state is not None:
        head.load_state_dict({k: v.to(dt) for k, v in state.items()})
    feats = (torch.clamp(torch.round(torch.relu(rn(N, CIN, FEAT, FEAT)) * 8), 0, 32) / 8).to(dt).requires_grad_(True)
    u = torch.rand(N, 2 * FEAT, 2 * FEAT, generator=g, dtype=torch.float64)
    targets = (u if soft else (u < 0.5).double()).to(dt)
    labels = torch.tensor(labels, dtype=torch.int64)
    mask_pred = head(feats)
    assert mask_pred.shape == (N, 1 if agnostic else c, 2 * FEAT, 2 * FEAT) and mask_pred.dtype == dt
    loss = head.loss(mask_pred, targets, labels)["loss_mask"]
    assert loss.shape == (1,)
    loss.sum().backward()
    out = dict(f=feats.detach(), up_weight=head.upsample.weight.detach(), up_bias=head.upsample.bias.detach(),
               weight=head.conv_logits.weight.detach(), bias=head.conv_logits.bias.detach(), labels=labels, targets=targets,
               loss=loss.detach(), df=feats.grad, dup_weight=head.upsample.weight.grad, dup_bias=head.upsample.bias.grad,
               dweight=head.conv_logits.weight.grad, dbias=head.conv_logits.bias.grad)
    return {k: v.numpy().copy() for k, v in out.items()}, {k: v.detach().clone() for k, v in head.state_dict().items()}


def main():
    head_mod = reference(sys.argv[1])
    store = {}
    for name in CASES:
        r64, state = run(head_mod, name, torch.float64)
        r32, _ = run(head_mod, name, torch.float32, state)
        assert r64["f"].dtype == np.float64 and r32["f"].dtype == np.float32
        for k in ("f", "up_weight", "up_bias"):                                  # the grid survives the rounding to float32
            assert np.array_equal(r64[k], r32[k].astype(np.float64)), k
        for k, v in r64.items():
            store["%s_%s_f64" % (name, k)] = v
        for k, v in r32.items():
            store["%s_%s_f32" % (name, k)] = v
        print("%-9s loss %.9f  f32 loss error %.2e" % (name, float(r64["loss"][0]), abs(float(r32["loss"][0]) - float(r64["loss"][0]))))
    path = os.path.join(HERE, "g32_mask_tail.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
