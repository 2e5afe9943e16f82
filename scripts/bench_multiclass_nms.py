#!/usr/bin/env python3
"""Time the native multiclass_nms (csrc/multiclass_nms.hip, iif_amd/mmdet_multiclass_nms.py) against the same mathematics as torch
operations in the structure of the reference with mmcv 1.3.8, on the same GPU, same process, the variants alternating round by round.

    python scripts/bench_multiclass_nms.py [--out profiles/multiclass_nms.txt]

Shapes (one image each)
  lvis-5k   n = 1000 proposals, C = 1203, score_thr 1e-4, max_num 300; scores = a softmax of random logits scaled so that about
            5 000 candidates take part: below split_thr = 10000, mmcv's all-pairs regime
  lvis-50k  the same with about 50 000 candidates: the per-class regime
  coco      n = 1000, C = 80, score_thr 0.05, max_num 100
native  multiclass_nms: 12 enqueued operations and the one host read of the count
torch   bbox_nms.py line by line (the nonzero over all scores, the three gathers), then batched_nms as mmcv 1.3.8 runs it: below
        split_thr one nms over the shifted boxes, at or above it a Python loop over torch.unique(labels) with a nonzero and an
        nms per class; nms is bench_nms.py's t_nms (a sort, the suppression bit matrix built on the device with torch
        operations, the blocking copy to the host and the greedy scan in numpy).
Before anything is timed the script asserts that both sides return the same flat indices in the same order and the same bits.
End-to-end times are wall-clock microseconds per call between two device synchronisations; kernel times come from torch's
profiler in a pass of its own.  No ratio is fixed in advance: the script reports, says which native kernel takes the largest
share, and lists every shape at which the native path is slower."""
import argparse
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_nms as bn  # noqa: E402
from iif_amd import mmdet_multiclass_nms as mm  # noqa: E402


def t_batched_nms(boxes, scores, ids, thr, split_thr, max_num):
    off = ids.to(boxes) * (boxes.max() + 1)
    shifted = boxes + off[:, None]
    if boxes.shape[0] < split_thr:
        keep = bn.t_nms(shifted, scores, thr)
        if max_num > 0:
            keep = keep[:max_num]
        return torch.cat([boxes[keep], scores[keep, None]], -1), keep
    total = scores.new_zeros(scores.size(), dtype=torch.bool)
    for i in torch.unique(ids):
        mask = (ids == i).nonzero(as_tuple=False).view(-1)
        total[mask[bn.t_nms(shifted[mask], scores[mask], thr)]] = True
    keep = total.nonzero(as_tuple=False).view(-1)
    keep = keep[scores[keep].sort(descending=True, stable=True)[1]]
    if max_num > 0:
        keep = keep[:max_num]
    return torch.cat([boxes[keep], scores[keep, None]], -1), keep


def t_multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num):
    C = multi_scores.size(1) - 1
    bboxes = multi_bboxes.view(multi_scores.size(0), -1, 4)
    scores = multi_scores[:, :-1]
    labels = torch.arange(C, dtype=torch.long, device=scores.device).view(1, -1).expand_as(scores)
    bboxes, scores, labels = bboxes.reshape(-1, 4), scores.reshape(-1), labels.reshape(-1)
    inds = (scores > score_thr).nonzero(as_tuple=False).squeeze(1)
    bboxes, scores, labels = bboxes[inds], scores[inds], labels[inds]
    if bboxes.numel() == 0:
        return torch.cat([bboxes, scores[:, None]], -1), labels, inds
    dets, keep = t_batched_nms(bboxes, scores, labels, nms_cfg["iou_threshold"], nms_cfg.get("split_thr", 10000), nms_cfg.get("max_num", -1))
    if max_num > 0:
        dets, keep = dets[:max_num], keep[:max_num]
    return dets, labels[keep], inds[keep]


def make_inputs(dev, gen, n, C, target, score_thr):
    """Clustered proposals, per-class boxes a few pixels around them, and softmax scores whose logit scale is bisected until about
    ``target`` candidates exceed ``score_thr``."""
    base, _ = bn.clustered(n, gen)
    boxes = (base[:, None, :] + (torch.rand((n, C, 4), generator=gen) - 0.5) * 8).reshape(n, 4 * C)
    logits = torch.randn((n, C + 1), generator=gen)
    lo, hi = 0.0, 64.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        m = int((torch.softmax(logits * mid, dim=1)[:, :C] > score_thr).sum())
        lo, hi = (lo, mid) if m < target else (mid, hi)            # a sharper softmax leaves fewer classes above the threshold
    scores = torch.softmax(logits * (0.5 * (lo + hi)), dim=1)
    return boxes.to(dev), scores.to(dev), int((scores[:, :C] > score_thr).sum())


def _short(name):
    m = re.search(r"(mc_\w+?)(?:ENS|\b)", name)
    return (m.group(1) + (" (6 launches)" if m.group(1).startswith("mc_select") else "")) if m else name[:48]


def report(lines, slower, title, native, composed):
    t, med = bn.measure([("native", native), ("torch", composed)])
    lines.append(title)
    for name in ("native", "torch"):
        lines.append("    %-7s end to end %10.1f us  [%10.1f .. %10.1f]" % (name, med[name], min(t[name]), max(t[name])))
    lines.append("    native vs torch: %.2fx its speed" % (med["torch"] / med["native"]))
    if med["native"] > med["torch"]:
        slower.append(title.split(":")[0])
    ks = bn.kernel_split(native)
    if ks is None:
        lines.append("    per-kernel split: not measured (the profiler recorded no device activity)")
        return
    mine = {k: v for k, v in ks.items() if "mc_" in k or "emset" in k}
    total = sum(mine.values())
    lines.append("    native device time %.1f us per call in 12 enqueued operations:" % total)
    for k, v in sorted(mine.items(), key=lambda kv: -kv[1]):
        lines.append("        %-48s %9.1f us  %4.1f%%" % (_short(k), v, 100.0 * v / total))
    if mine:
        lines.append("    largest share: %s" % _short(max(mine, key=mine.get)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_multiclass_nms.py measures on the MI355X; there is nothing to report without one"
    dev = "cuda"
    lines = ["multiclass_nms, fp32, one image, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; per round the median of %d calls, each timed on the host between two device "
             "synchronisations; microseconds: median over the rounds [min .. max]" % (bn.ROUNDS, bn.ITERS)]
    slower = []
    gen = torch.Generator(device="cpu").manual_seed(2029)
    cfg = dict(type="nms", iou_threshold=0.5)
    for label, n, C, target, thr, max_num in (("lvis-5k", 1000, 1203, 5000, 1e-4, 300), ("lvis-50k", 1000, 1203, 50000, 1e-4, 300),
                                              ("coco", 1000, 80, 3000, 0.05, 100)):
        boxes, scores, M = make_inputs(dev, gen, n, C, target, thr)
        native = lambda: mm.multiclass_nms(boxes, scores, thr, cfg, max_num, return_inds=True)        # noqa: E731
        composed = lambda: t_multiclass_nms(boxes, scores, thr, cfg, max_num)                        # noqa: E731
        a, b = native(), composed()
        same = torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        assert same, "the torch formulation and the native path disagree at the %s shape" % label
        report(lines, slower, "%s: n = %d, C = %d, score_thr %g, max_num %d: M = %d candidates (%s regime), %d kept; the torch side "
               "returns the same detections: %s" % (label, n, C, thr, max_num, M, "all-pairs" if M < 10000 else "per-class",
                                                    a[2].numel(), same), native, composed)
    lines.append("slower than the torch formulation: %s" % (", ".join(slower) if slower else "nowhere"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
