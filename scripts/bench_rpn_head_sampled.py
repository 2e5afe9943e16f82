#!/usr/bin/env python3
"""Time the RPN head trained at the sampled pixels (csrc/rpn_head_sampled.hip, iif_amd/mmdet_rpn_head.py) against the same three
modules under plain torch autograd, on the same GPU, same process, the variants alternating round by round.

    python scripts/bench_rpn_head_sampled.py [--out profiles/rpn_head_sampled.txt]

Shape     the LVIS training shape: B = 2 images, batch padded to 800 x 1344, five levels (strides 4 .. 64), 89 523 pixels per
          image, 3 anchors per pixel (268 569 anchors), Ci = Co = 256, num = 256, pos_fraction 0.5, G = 20 boxes per image.
Both      the SAME targets (one ``rpn_stage_targets`` call before anything is timed) and ``rpn_loss`` on them; forward of the
          head on features that require a gradient, the loss, backward to the features and the six parameters.
sampled   ``rpn_sampled_pixels``, ``rpn_head_forward_sampled``, ``rpn_loss``, backward.
plain     ``rpn_cls(relu(rpn_conv(x)))`` / ``rpn_reg(...)`` under autograd, ``rpn_loss``, backward.
Before anything is timed the script asserts that both sides agree (under torch's deterministic convolutions): the maps bit for
bit, every gradient to 1e-4 of its largest element.  End-to-end times are wall-clock microseconds per call between two device synchronisations, host work included; the
plain path is measured TWICE in the same run and the difference of its two medians is its run-to-run spread.  Peak memory is
``torch.cuda.max_memory_allocated`` over one call minus what was allocated before it.  Device times per kernel come from torch's
profiler in a pass of its own."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_nms as bn  # noqa: E402
from bench_roi_stage import device_ops  # noqa: E402
from bench_rpn_stage import FEATMAPS, IMGS, PADS, STRIDES  # noqa: E402
from iif_amd.mmdet_anchor import AnchorGenerator  # noqa: E402
from iif_amd.mmdet_assigner import MaxIoUAssigner  # noqa: E402
from iif_amd.mmdet_bbox_loss import L1Loss  # noqa: E402
from iif_amd.mmdet_ce_loss import CrossEntropyLoss  # noqa: E402
from iif_amd.mmdet_rpn_head import rpn_head_forward_sampled, rpn_sampled_pixels  # noqa: E402
from iif_amd.mmdet_rpn_stage import rpn_loss, rpn_stage_targets  # noqa: E402
from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler  # noqa: E402

NUM, FRAC, BORDER, G, CI, CO, A = 256, 0.5, 0, 20, 256, 256, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rpn_head_sampled.py measures on the MI355X; there is nothing to report without one"
    dev = "cuda"
    rng = torch.Generator(device="cpu").manual_seed(2039)
    gen = AnchorGenerator(strides=list(STRIDES), ratios=[0.5, 1.0, 2.0], scales=[8])
    asg = MaxIoUAssigner(0.7, 0.3, min_pos_iou=0.3, match_low_quality=True)
    smp = RandomSampler(NUM, FRAC, add_gt_as_proposals=False)
    coder = DeltaXYWHBBoxCoder((0., 0., 0., 0.), (1., 1., 1., 1.))
    ce, reg_loss = CrossEntropyLoss(use_sigmoid=True), L1Loss()
    conv = torch.nn.Conv2d(CI, CO, 3, padding=1).to(dev)
    cls = torch.nn.Conv2d(CO, A, 1).to(dev)
    reg = torch.nn.Conv2d(CO, 4 * A, 1).to(dev)
    with torch.no_grad():
        for m in (conv, cls, reg):                       # mmdet's init: normal, std 0.01
            m.weight.copy_((torch.randn(m.weight.shape, generator=rng) * 0.01).to(dev))
            m.bias.zero_()
    params = [p for m in (conv, cls, reg) for p in (m.weight, m.bias)]
    feats = [torch.randn((2, CI, h, w), generator=rng).to(dev).requires_grad_(True) for h, w in FEATMAPS]
    gts = []
    for b in range(2):
        xy = torch.rand((G, 2), generator=rng) * torch.tensor([IMGS[b][1] - 330.0, IMGS[b][0] - 330.0])
        gts.append(torch.cat([xy, xy + 16 + torch.rand((G, 2), generator=rng) * 304], 1).to(dev))
    t = rpn_stage_targets(FEATMAPS, gen, PADS, IMGS, gts, asg, smp, coder, allowed_border=BORDER)

    def clear():
        for x in feats + params:
            x.grad = None

    def finish(scores, deltas):
        out = rpn_loss(scores, deltas, t, ce, reg_loss)
        (sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"])).backward()
        return scores, deltas

    def sampled():
        clear()
        return finish(*rpn_head_forward_sampled(feats, conv, cls, reg, rpn_sampled_pixels(t)))

    def plain():
        clear()
        hs = [torch.relu(conv(x)) for x in feats]
        return finish([cls(h) for h in hs], [reg(h) for h in hs])

    # ---- agreement
    # (torch's deterministic convolutions for the comparison: its default 1x1 channels_last convolution does not give the same
    # bits twice, so two plain forwards would not agree either)
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        maps_s = [m.detach().clone() for pair in sampled() for m in pair]
        grads_s = [x.grad.clone() for x in feats + params]
        maps_p = [m.detach() for pair in plain() for m in pair]
    for a, b in zip(maps_s, maps_p):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the maps differ"
    worst = 0.0
    for a, x in zip(grads_s, feats + params):
        scale = float(x.grad.abs().max())
        err = float((a - x.grad).abs().max())
        assert err <= 1e-4 * max(scale, 1e-12), "gradients differ: %g against a largest element of %g" % (err, scale)
        worst = max(worst, err / max(scale, 1e-30))
    del maps_s, maps_p, grads_s
    active = int((rpn_sampled_pixels(t).slots[:, 1] >= 0).sum())
    lines = ["RPN head at the sampled pixels, fp32, %s: B = 2, %d pixels per image on five levels, Ci = Co = %d, %d anchors per "
             "pixel, num = %d: %d slots, %d active" % (torch.cuda.get_device_name(0), sum(h * w for h, w in FEATMAPS), CI, A, NUM,
                                                       2 * (NUM + int(NUM * FRAC)), active),
             "the maps are the same bits on both paths (both under torch's deterministic convolutions); every gradient within "
             "%.2g of its largest element" % worst,
             "%d rounds, the variants alternating; per round the median of %d calls, each timed on the host between two device "
             "synchronisations (host work included); microseconds: median over the rounds [min .. max]" % (bn.ROUNDS, bn.ITERS)]

    # ---- timing
    tt, med = bn.measure([("plain", plain), ("sampled", sampled), ("plain again", plain)])
    for name in ("sampled", "plain", "plain again"):
        lines.append("    %-11s forward + loss + backward %9.1f us  [%9.1f .. %9.1f]" % (name, med[name], min(tt[name]), max(tt[name])))
    spread = abs(med["plain"] - med["plain again"])
    base = min(med["plain"], med["plain again"])
    lines.append("    the plain path's run-to-run spread (its two medians): %.1f us; sampled vs plain: %.2fx its speed"
                 % (spread, base / med["sampled"]))

    # ---- peak memory
    for name, fn in (("sampled", sampled), ("plain", plain)):
        clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del out
        lines.append("    %-11s peak memory above the resident tensors %8.1f MB" % (name, peak / 1e6))
    lines.append("    (arithmetic: the hidden activation autograd keeps is %.1f MB, d feats %.1f MB on both paths)"
                 % (sum(2 * CO * h * w * 4 for h, w in FEATMAPS) / 1e6, sum(2 * CI * h * w * 4 for h, w in FEATMAPS) / 1e6))

    # ---- device time
    def forward_only():
        with torch.no_grad():
            for x in feats:
                h = torch.relu(conv(x))
                cls(h), reg(h)
    for name, fn in (("sampled", sampled), ("plain", plain), ("forward only", forward_only)):
        ops = device_ops(fn)
        if ops is None:
            lines.append("    %s: device time not measured" % name)
            continue
        total, count, names = ops
        lines.append("    %-12s device time %9.1f us per call in %.0f enqueued operations" % (name, total, count))
        for k, v in sorted(names.items(), key=lambda kv: -kv[1])[:8]:
            lines.append("        %-70s %9.1f us" % (k[:70], v))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
