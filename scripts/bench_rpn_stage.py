#!/usr/bin/env python3
"""Time the RPN head's training side (csrc/rpn_stage.hip, iif_amd/mmdet_rpn_stage.py) against the chain that exists without it,
on the same GPU, same process, the variants alternating round by round.

    python scripts/bench_rpn_stage.py [--out profiles/rpn_stage.txt]

Shape   the LVIS training shape: B = 2 images, batch padded to 800 x 1344, five levels (strides 4 .. 64, 3 anchors per cell),
        268 569 anchors, num = 256, pos_fraction 0.5, RPN thresholds (0.7 / 0.3 / 0.3, low-quality matching), allowed_border 0,
        G = 20 and G = 300 ground-truth boxes per image; pad shapes (800, 1344) and (768, 1216).
new     rpn_stage_targets (the key draw and five enqueued operations), rpn_loss forward and backward.
chain   the reference-structure anchors and valid flags as torch operations per level and image, anchor_inside_flags,
        anchor_targets_single per image (a boolean-index compaction: one synchronisation each), images_to_levels, ten dense
        native loss calls on permute(0, 2, 3, 1).reshape copies, the num_total_samples read, and autograd's backward.
Before anything is timed the script asserts that both sides agree: the chain is run once with its key draw replaced by the new
path's keys (compacted), the dense targets must then be the same bits as rpn_stage_dense's and the losses agree to 1e-5.
End-to-end times are wall-clock microseconds per call between two device synchronisations, host work included; the chain is
measured TWICE in the same run and the difference of its two medians is its run-to-run spread.  Device times and the number of
enqueued operations come from torch's profiler in a pass of its own.  Bytes written for targets are arithmetic from the shapes."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_nms as bn  # noqa: E402
from bench_roi_stage import device_ops  # noqa: E402
from iif_amd.mmdet_anchor import AnchorGenerator  # noqa: E402
from iif_amd.mmdet_assigner import MaxIoUAssigner  # noqa: E402
from iif_amd.mmdet_bbox_loss import L1Loss  # noqa: E402
from iif_amd.mmdet_ce_loss import CrossEntropyLoss  # noqa: E402
from iif_amd.mmdet_rpn_stage import rpn_loss, rpn_stage_dense, rpn_stage_targets  # noqa: E402
from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler, anchor_inside_flags, anchor_targets_single  # noqa: E402

STRIDES = (4, 8, 16, 32, 64)
FEATMAPS = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
PADS = [(800, 1344, 3), (768, 1216, 3)]
IMGS = [(800, 1333, 3), (750, 1200, 3)]
NUM, FRAC, BORDER = 256, 0.5, 0


def torch_anchors(gen, dev):
    """anchor_generator.py:239-272 per level as torch operations."""
    out = []
    for base, (sw, sh), (H, W) in zip(gen.base_anchors, gen.strides, FEATMAPS):
        base = base.to(dev)
        sx = torch.arange(0, W, device=dev) * sw
        sy = torch.arange(0, H, device=dev) * sh
        xx = sx.repeat(H)
        yy = sy.view(-1, 1).repeat(1, W).view(-1)
        shifts = torch.stack([xx, yy, xx, yy], dim=-1).type_as(base)
        out.append((base[None, :, :] + shifts[:, None, :]).view(-1, 4))
    return out


def torch_flags(gen, pad, dev):
    """anchor_generator.py:383-440 per level as torch operations."""
    import numpy as np
    out = []
    h, w = pad[:2]
    for (sw, sh), (H, W), nb in zip(gen.strides, FEATMAPS, gen.num_base_anchors):
        vh, vw = min(int(np.ceil(h / sh)), H), min(int(np.ceil(w / sw)), W)
        vx = torch.zeros(W, dtype=torch.bool, device=dev)
        vy = torch.zeros(H, dtype=torch.bool, device=dev)
        vx[:vw] = 1
        vy[:vh] = 1
        v = vx.repeat(H) & vy.view(-1, 1).repeat(1, W).view(-1)
        out.append(v[:, None].expand(v.size(0), nb).contiguous().view(-1))
    return out


def chain(gen, gts, asg, smp, coder, ce, reg, scores, deltas, dev, backward=True):
    level_counts = [h * w * n for (h, w), n in zip(FEATMAPS, gen.num_base_anchors)]
    flat = torch.cat(torch_anchors(gen, dev))
    cols = []
    for b, g in enumerate(gts):
        inside = anchor_inside_flags(flat, torch.cat(torch_flags(gen, PADS[b], dev)), IMGS[b][:2], BORDER)
        cols.append(anchor_targets_single(flat, g, None, None, asg, smp, coder, 1, inside_flags=inside))
    counts = torch.stack([c[4] for c in cols]).tolist()                                    # the num_total_samples read
    avg = float(sum(max(p, 1) + max(n, 1) for p, n in counts))
    per_level = [[t.split(level_counts, 0) for t in (c[0], c[1], c[2], c[3])] for c in cols]
    losses = []
    for l in range(len(FEATMAPS)):
        labels, lw, bt, bw = (torch.stack([per_level[b][f][l] for b in range(len(gts))]) for f in range(4))
        s = scores[l].permute(0, 2, 3, 1).reshape(-1, 1)
        d = deltas[l].permute(0, 2, 3, 1).reshape(-1, 4)
        losses.append(ce(s, labels.reshape(-1), lw.reshape(-1), avg_factor=avg))
        losses.append(reg(d, bt.reshape(-1, 4), bw.reshape(-1, 4), avg_factor=avg))
    if backward:
        for x in scores + deltas:
            x.grad = None
        sum(losses).backward()
    return losses, per_level, avg


def new_path(gen, gts, asg, smp, coder, ce, reg, scores, deltas, keys=None, backward=True):
    t = rpn_stage_targets(FEATMAPS, gen, PADS, IMGS, gts, asg, smp, coder, allowed_border=BORDER, keys=keys)
    out = rpn_loss(scores, deltas, t, ce, reg)
    if backward:
        for x in scores + deltas:
            x.grad = None
        (sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"])).backward()
    return t, out


class CompactKeys:
    """torch.randint returns prepared keys while active: the chain's sampler then draws what the new path was given."""

    def __init__(self, queue):
        self.queue = list(queue)

    def __enter__(self):
        self._orig = torch.randint

        def randint(low, high, size, **kw):
            k = self.queue.pop(0)
            assert tuple(size) == tuple(k.shape)
            return k
        torch.randint = randint

    def __exit__(self, *exc):
        torch.randint = self._orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rpn_stage.py measures on the MI355X; there is nothing to report without one"
    dev = "cuda"
    gen = AnchorGenerator(strides=list(STRIDES), ratios=[0.5, 1.0, 2.0], scales=[8])
    A = sum(h * w * 3 for h, w in FEATMAPS)
    lines = ["RPN training side, fp32, %s: B = 2, %d anchors on five levels, num = %d" % (torch.cuda.get_device_name(0), A, NUM),
             "%d rounds, the variants alternating; per round the median of %d calls, each timed on the host between two device "
             "synchronisations (host work included); microseconds: median over the rounds [min .. max]" % (bn.ROUNDS, bn.ITERS)]
    rng = torch.Generator(device="cpu").manual_seed(2034)
    asg = MaxIoUAssigner(0.7, 0.3, min_pos_iou=0.3, match_low_quality=True)
    smp = RandomSampler(NUM, FRAC, add_gt_as_proposals=False)
    coder = DeltaXYWHBBoxCoder((0., 0., 0., 0.), (1., 1., 1., 1.))
    ce, reg = CrossEntropyLoss(use_sigmoid=True), L1Loss()
    scores = [torch.randn((2, 3, h, w), generator=rng).to(dev).requires_grad_(True) for h, w in FEATMAPS]
    deltas = [(torch.randn((2, 12, h, w), generator=rng) * 0.3).to(dev).requires_grad_(True) for h, w in FEATMAPS]
    for G in (20, 300):
        gts = []
        for b in range(2):
            xy = torch.rand((G, 2), generator=rng) * torch.tensor([IMGS[b][1] - 330.0, IMGS[b][0] - 330.0])
            gts.append(torch.cat([xy, xy + 16 + torch.rand((G, 2), generator=rng) * 304], 1).to(dev))
        keys = torch.randint(0, 2 ** 31, (2, A), dtype=torch.int32, generator=rng).to(dev)

        # ---- agreement
        t, out = new_path(gen, gts, asg, smp, coder, ce, reg, scores, deltas, keys=keys)
        g_new = [x.grad.clone() for x in scores + deltas]
        flat = torch.cat(gen.grid_anchors(FEATMAPS, device=dev))
        compact = [keys[b][anchor_inside_flags(flat, torch.cat(gen.valid_flags(FEATMAPS, PADS[b], device=dev)), IMGS[b][:2], BORDER)]
                   for b in range(2)]
        with CompactKeys(compact):
            losses, per_level, avg = chain(gen, gts, asg, smp, coder, ce, reg, scores, deltas, dev)
        assert avg == float(t.num_total_samples)
        dense = rpn_stage_dense(t)
        for f in range(4):
            for l in range(len(FEATMAPS)):
                want = torch.stack([per_level[b][f][l] for b in range(2)])
                got = dense[f][l]
                as_bits = (lambda x: x.view(torch.int32)) if want.dtype == torch.float32 else (lambda x: x)
                assert torch.equal(as_bits(got.contiguous()), as_bits(want.contiguous())), "dense targets differ: field %d level %d" % (f, l)
        mine = [v for pair in zip(out["loss_rpn_cls"], out["loss_rpn_bbox"]) for v in pair]
        for a, c in zip(mine, losses):
            assert abs(float(a) - float(c)) <= 1e-5 * max(abs(float(c)), 1e-3), (float(a), float(c))
        for a, x in zip(g_new, scores + deltas):
            assert torch.allclose(a, x.grad, rtol=1e-4, atol=1e-9), "gradients differ"

        # ---- timing
        new = lambda: new_path(gen, gts, asg, smp, coder, ce, reg, scores, deltas)                       # noqa: E731
        old = lambda: chain(gen, gts, asg, smp, coder, ce, reg, scores, deltas, dev)                     # noqa: E731
        tt, med = bn.measure([("chain", old), ("new", new), ("chain again", old)])
        lines.append("G = %d per image: %s positives and %s negatives kept; dense targets the same bits as the chain's, losses "
                     "agree to 1e-5" % (G, t.counts[:, 0].tolist(), t.counts[:, 1].tolist()))
        for name in ("new", "chain", "chain again"):
            lines.append("    %-11s end to end %9.1f us  [%9.1f .. %9.1f]" % (name, med[name], min(tt[name]), max(tt[name])))
        spread = abs(med["chain"] - med["chain again"])
        base = min(med["chain"], med["chain again"])
        lines.append("    the chain's run-to-run spread (its two medians): %.1f us; new vs chain: %.2fx its speed" % (spread, base / med["new"]))
        parts = (("new targets", lambda: rpn_stage_targets(FEATMAPS, gen, PADS, IMGS, gts, asg, smp, coder, allowed_border=BORDER)),
                 ("new total", new), ("chain total", old))
        for name, fn in parts:
            ops = device_ops(fn)
            if ops is None:
                lines.append("    %s: device time not measured" % name)
                continue
            total, count, names = ops
            lines.append("    %-12s device time %8.1f us per call in %.0f enqueued operations" % (name, total, count))
            if name != "chain total":
                for k, v in sorted(names.items(), key=lambda kv: -kv[1])[:5]:
                    lines.append("        %-60s %8.1f us" % (k[:60], v))
    nep = int(NUM * FRAC)
    lines.append("bytes written for targets per call (arithmetic): chain 44 A per image = %.1f MB for B = 2; new %d bytes of results "
                 "plus 12 A per image of workspace (maximum, argmax / gt_inds, selection word) = %.1f MB"
                 % (2 * 44 * A / 1e6, 2 * (8 * nep + 8 * NUM + 16 + 8 * nep + 16 * nep) + 4, 2 * 12 * A / 1e6))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
