#!/usr/bin/env python3
"""Time the box assignment (mmdet MaxIoUAssigner / bbox_overlaps, csrc/assign.hip) against the same mathematics as torch ops,
same GPU, same process, the variants alternating round by round.

    python scripts/bench_assign.py [--out profiles/assign.txt]

Shapes: N candidates x G ground-truth boxes for G in {8, 40, 300}
  [268569] x G     the RPN of a 1344 x 800 input (five FPN levels, three anchors per cell), thresholds (0.7, 0.3, 0.3)
  [1000 + G] x G   the RoI head with add_gt_as_proposals, thresholds (0.5, 0.5, 0.5), no low-quality matching
  fused    MaxIoUAssigner.assign of iif_amd.mmdet_assigner: at most three enqueued operations, no [G, N] array
  torch    max_iou_assigner.py:106-213 and iou2d_calculator.py:192-255 restated with torch ops on the same GPU: the [G, N] matrix
           and its temporaries, the two max reductions, the Python loop over the gts (one host round trip and two launches per
           gt with low-quality matching) and the final nonzero - what a user has without the native path
  overlaps / torch-ov   bbox_overlaps(gts, candidates), 'iou', pairwise: one launch against the torch ops
Beside the times: the operations each side enqueues (fused: by construction; torch: aten operations dispatched, each at least
one launch) and the rise of torch's peak allocation over one call.  Every round times each variant (median of its iterations);
the table gives the median over the rounds and their range.  No ratio is fixed in advance: the script reports."""
import argparse
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iif_amd.mmdet_assigner import MaxIoUAssigner, bbox_overlaps  # noqa: E402

ROUNDS, ITERS = 5, 8


def torch_overlaps(b1, b2, eps=1e-6):
    area1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    area2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    lt = torch.max(b1[:, None, :2], b2[None, :, :2])
    rb = torch.min(b1[:, None, 2:], b2[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = area1[:, None] + area2[None, :] - overlap
    union = torch.max(union, union.new_tensor([eps]))
    return overlap / union


def torch_assign(bboxes, gts, gt_labels, pos, neg, min_pos, mlq):
    overlaps = torch_overlaps(gts, bboxes)
    G, N = overlaps.shape
    gt_inds = overlaps.new_full((N,), -1, dtype=torch.long)
    max_overlaps, argmax = overlaps.max(dim=0)
    gt_max, _ = overlaps.max(dim=1)
    gt_inds[(max_overlaps >= 0) & (max_overlaps < neg)] = 0
    p = max_overlaps >= pos
    gt_inds[p] = argmax[p] + 1
    if mlq:
        for i in range(G):
            if gt_max[i] >= min_pos:
                gt_inds[overlaps[i, :] == gt_max[i]] = i + 1
    labels = gt_inds.new_full((N,), -1)
    pos_inds = torch.nonzero(gt_inds > 0, as_tuple=False).squeeze()
    if pos_inds.numel() > 0:
        labels[pos_inds] = gt_labels[gt_inds[pos_inds] - 1]
    return gt_inds, max_overlaps, labels


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def one_round(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return ts[len(ts) // 2]


def measure(variants):
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, fn in variants:
            t[name].append(one_round(fn))
    return t, {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def count_ops(fn):
    with CountOps() as c:
        fn()
    torch.cuda.synchronize()
    return c.n


def boxes(n, gen, W, H, smin, smax):
    """float32 [n, 4] on the half-pixel grid."""
    cx = torch.randint(0, 2 * W, (n,), generator=gen).float() * 0.5
    cy = torch.randint(0, 2 * H, (n,), generator=gen).float() * 0.5
    w = torch.randint(2 * smin, 2 * smax, (n,), generator=gen).float() * 0.25
    h = torch.randint(2 * smin, 2 * smax, (n,), generator=gen).float() * 0.25
    return torch.stack([cx - w, cy - h, cx + w, cy + h], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    lines = ["box assignment, fp32, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; per round the median of %d event pairs around one call; microseconds: median "
             "over the rounds [min .. max]" % (ROUNDS, ITERS)]
    slower = []
    for kind in ("rpn", "roi"):
        for G in (8, 40, 300):
            gen = torch.Generator(device="cpu").manual_seed(1000 + G)
            gts = boxes(G, gen, 1344, 800, 16, 400)
            if kind == "rpn":
                N = 268569
                cand = boxes(N, gen, 1344, 800, 16, 512)
                pos, neg, min_pos, mlq = 0.7, 0.3, 0.3, True
            else:
                N = 1000 + G
                jit = boxes(1000, gen, 1344, 800, 16, 400)
                jit[:500] = gts[torch.randint(0, G, (500,), generator=gen)] + torch.randint(-16, 17, (500, 4), generator=gen).float() * 0.5
                cand = torch.cat([gts, jit], dim=0)
                pos, neg, min_pos, mlq = 0.5, 0.5, 0.5, False
            cand, gts = cand.to(dev), gts.to(dev)
            labels = torch.randint(0, 1203, (G,), generator=gen).to(dev)
            asg = MaxIoUAssigner(pos, neg, min_pos_iou=min_pos, match_low_quality=mlq)

            def fused():
                return asg.assign(cand, gts, gt_labels=labels)

            def composed():
                return torch_assign(cand, gts, labels, pos, neg, min_pos, mlq)

            def fused_ov():
                return bbox_overlaps(gts, cand)

            def composed_ov():
                return torch_overlaps(gts, cand)
            variants = [("fused", fused), ("torch", composed), ("overlaps", fused_ov), ("torch-ov", composed_ov)]
            f, c = fused(), composed()
            same = (torch.equal(f.gt_inds, c[0]), torch.equal(f.max_overlaps.view(torch.int32), c[1].view(torch.int32)),
                    torch.equal(f.labels, c[2]), torch.equal(fused_ov().view(torch.int32), composed_ov().view(torch.int32)))
            npos = int((f.gt_inds > 0).sum())
            del f, c
            ops = {"fused": "%d enqueued" % (3 if mlq else 1), "torch": "%d aten ops" % count_ops(composed),
                   "overlaps": "1 enqueued", "torch-ov": "%d aten ops" % count_ops(composed_ov)}
            peak = {name: peak_rise(fn) for name, fn in variants}
            t, med = measure(variants)
            lines.append("%s [%d] x %d (%d positives): fused vs torch gt_inds / max_overlaps bits / labels / overlaps bits equal: %s"
                         % (kind, N, G, npos, " ".join(str(s) for s in same)))
            for name, _ in variants:
                lines.append("    %-9s %10.1f  [%10.1f .. %10.1f]   %-14s peak +%.2f MB"
                             % (name, med[name], min(t[name]), max(t[name]), ops[name], peak[name] * 1e-6))
            for a, b in (("fused", "torch"), ("overlaps", "torch-ov")):
                lines.append("    %s vs %s: %.2fx its speed (%.1f us %s)" % (a, b, med[b] / med[a], abs(med[b] - med[a]),
                                                                           "less" if med[a] <= med[b] else "MORE"))
                if med[a] > med[b]:
                    slower.append("%s at %s [%d] x %d" % (a, kind, N, G))
    lines.append("slower than the torch ops: %s" % (", ".join(slower) if slower else "nowhere"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
