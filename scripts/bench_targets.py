#!/usr/bin/env python3
"""Time box sampling, target building and the delta coder (csrc/targets.hip, iif_amd/mmdet_targets.py) against the same
mathematics as torch ops - the reference's lines restated, with its CPU ``torch.randperm`` - on the same GPU, same process, the
variants alternating round by round.

    python scripts/bench_targets.py [--out profiles/targets.txt]

Shapes (the assignment is given: it is timed by scripts/bench_assign.py)
  rpn  [268569] anchors x G gts, G in {300, 7}, num 256, fraction 0.5: sample, then the anchor targets (all anchors valid)
       native   RandomSampler.sample_padded + iif_anchor_targets: the key draw and four enqueued operations
       torch    random_sampler.py:64-82, base_sampler.py:83-98, sampling_result.py:26-50, anchor_head.py:224-254
  rcnn [1000 + G] proposals, num 512, fraction 0.25, add_gt_as_proposals: sample, then the RoI targets and rois
       native   sample_padded + iif_roi_targets (padded to 512 rows)
       torch    the sampler as above, bbox_head.py:155-186 and bbox2roi
  coder  encode [1000, 4]; decode [1000, 4] and [1000, 4 x 1203] with max_shape: one launch against delta_xywh_bbox_coder.py
Times are wall-clock microseconds per call between two device synchronisations (the torch side waits for the host inside the
call, so device events alone would not see what it costs).  Beside them: aten operations dispatched (each at least one launch) and
host synchronisations counted by torch's sync debug mode.  No ratio is fixed in advance: the script reports."""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iif_amd.mmdet_assigner import AssignResult  # noqa: E402
from iif_amd.mmdet_targets import (DeltaXYWHBBoxCoder, RandomSampler, anchor_targets_single, bbox_targets)  # noqa: E402

ROUNDS, ITERS = 5, 8


# ---- the reference's lines as torch ops
def t_bbox2delta(proposals, gt, means, stds):
    px = (proposals[..., 0] + proposals[..., 2]) * 0.5
    py = (proposals[..., 1] + proposals[..., 3]) * 0.5
    pw = proposals[..., 2] - proposals[..., 0]
    ph = proposals[..., 3] - proposals[..., 1]
    gx = (gt[..., 0] + gt[..., 2]) * 0.5
    gy = (gt[..., 1] + gt[..., 3]) * 0.5
    gw = gt[..., 2] - gt[..., 0]
    gh = gt[..., 3] - gt[..., 1]
    deltas = torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph)], dim=-1)
    return deltas.sub_(deltas.new_tensor(means).unsqueeze(0)).div_(deltas.new_tensor(stds).unsqueeze(0))


def t_delta2bbox(rois, deltas, means, stds, max_shape, wh_ratio_clip=16 / 1000):
    k = deltas.size(-1) // 4
    means = deltas.new_tensor(means).view(1, -1).repeat(1, k)
    stds = deltas.new_tensor(stds).view(1, -1).repeat(1, k)
    dn = deltas * stds + means
    dx, dy, dw, dh = dn[..., 0::4], dn[..., 1::4], dn[..., 2::4], dn[..., 3::4]
    px = ((rois[..., 0] + rois[..., 2]) * 0.5).unsqueeze(-1).expand_as(dx)
    py = ((rois[..., 1] + rois[..., 3]) * 0.5).unsqueeze(-1).expand_as(dy)
    pw = (rois[..., 2] - rois[..., 0]).unsqueeze(-1).expand_as(dw)
    ph = (rois[..., 3] - rois[..., 1]).unsqueeze(-1).expand_as(dh)
    dxw, dyh = pw * dx, ph * dy
    mr = np.abs(np.log(wh_ratio_clip))
    dw, dh = dw.clamp(min=-mr, max=mr), dh.clamp(min=-mr, max=mr)
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = px + dxw, py + dyh
    b = torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], dim=-1).view(deltas.size())
    ms = b.new_tensor(max_shape)[..., :2]
    max_xy = torch.cat([ms] * (deltas.size(-1) // 2), dim=-1).flip(-1).unsqueeze(-2)
    b = torch.where(b < b.new_tensor(0), b.new_tensor(0), b)
    return torch.where(b > max_xy, max_xy, b)


def t_choice(gallery, num):
    perm = torch.randperm(gallery.numel())[:num].to(device=gallery.device)
    return gallery[perm]


def t_sample(gt_inds, labels, bboxes, gts, gt_labels, num, frac, add_gt):
    bboxes = bboxes[:, :4]
    gt_flags = bboxes.new_zeros((bboxes.shape[0],), dtype=torch.uint8)
    if add_gt:
        bboxes = torch.cat([gts, bboxes], dim=0)
        k = len(gt_labels)
        gt_inds = torch.cat([torch.arange(1, k + 1, dtype=torch.long, device=gt_labels.device), gt_inds])
        labels = torch.cat([gt_labels, labels])
        gt_flags = torch.cat([bboxes.new_ones(k, dtype=torch.uint8), gt_flags])
    nep = int(num * frac)
    pos = torch.nonzero(gt_inds > 0, as_tuple=False)
    if pos.numel() != 0:
        pos = pos.squeeze(1)
    if pos.numel() > nep:
        pos = t_choice(pos, nep)
    pos = pos.unique()
    nen = num - pos.numel()
    neg = torch.nonzero(gt_inds == 0, as_tuple=False)
    if neg.numel() != 0:
        neg = neg.squeeze(1)
    if len(neg) > nen:
        neg = t_choice(neg, nen)
    neg = neg.unique()
    pos_gt = gt_inds[pos] - 1
    return dict(pos=pos, neg=neg, pos_bboxes=bboxes[pos], neg_bboxes=bboxes[neg], pos_is_gt=gt_flags[pos], pos_gt=pos_gt,
                pos_gt_bboxes=gts[pos_gt, :], pos_gt_labels=None if labels is None else labels[pos])


def t_rpn(anchors, gt_inds, gts, means, stds):
    s = t_sample(gt_inds, None, anchors, gts, None, 256, 0.5, False)
    n = anchors.shape[0]
    bt, bw = torch.zeros_like(anchors), torch.zeros_like(anchors)
    labels = anchors.new_full((n,), 1, dtype=torch.long)
    lw = anchors.new_zeros(n, dtype=torch.float)
    if len(s["pos"]) > 0:
        bt[s["pos"], :] = t_bbox2delta(s["pos_bboxes"], s["pos_gt_bboxes"], means, stds)
        bw[s["pos"], :] = 1.0
        labels[s["pos"]] = 0
        lw[s["pos"]] = 1.0
    if len(s["neg"]) > 0:
        lw[s["neg"]] = 1.0
    return labels, lw, bt, bw


def t_rcnn(props, gt_inds, cand_labels, gts, gt_labels, means, stds, classes):
    s = t_sample(gt_inds, cand_labels, props, gts, gt_labels, 512, 0.25, True)
    pb, nb = s["pos_bboxes"], s["neg_bboxes"]
    num_pos, num_neg = pb.size(0), nb.size(0)
    k = num_pos + num_neg
    labels = pb.new_full((k,), classes, dtype=torch.long)
    lw, bt, bw = pb.new_zeros(k), pb.new_zeros(k, 4), pb.new_zeros(k, 4)
    if num_pos > 0:
        labels[:num_pos] = s["pos_gt_labels"]
        lw[:num_pos] = 1.0
        bt[:num_pos, :] = t_bbox2delta(pb, s["pos_gt_bboxes"], means, stds)
        bw[:num_pos, :] = 1
    if num_neg > 0:
        lw[-num_neg:] = 1.0
    boxes = torch.cat([pb, nb])
    rois = torch.cat([boxes.new_full((boxes.size(0), 1), 0), boxes[:, :4]], dim=-1)
    return labels, lw, bt, bw, rois


# ---- measuring
class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def count_ops(fn):
    with CountOps() as c:
        fn()
    torch.cuda.synchronize()
    return c.n


def count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchroniz" in str(x.message) for x in w)


def one_round(fn):
    ts = []
    for _ in range(ITERS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return sorted(ts)[len(ts) // 2]


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


def boxes(n, gen, W, H, smin, smax):
    cx = torch.randint(0, 2 * W, (n,), generator=gen).float() * 0.5
    cy = torch.randint(0, 2 * H, (n,), generator=gen).float() * 0.5
    w = torch.randint(2 * smin, 2 * smax, (n,), generator=gen).float() * 0.25
    h = torch.randint(2 * smin, 2 * smax, (n,), generator=gen).float() * 0.25
    return torch.stack([cx - w, cy - h, cx + w, cy + h], dim=1)


class Given:
    """An assigner that returns a prepared result: the assignment is not what this script times."""

    def __init__(self, num_gts, gt_inds):
        self.num_gts, self.gt_inds = num_gts, gt_inds

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        return AssignResult(self.num_gts, self.gt_inds, None, None)


def report(lines, slower, title, variants, extra=""):
    ops = {name: count_ops(fn) for name, fn in variants}
    syncs = {name: count_syncs(fn) for name, fn in variants}
    t, med = measure(variants)
    lines.append(title + extra)
    for name, _ in variants:
        lines.append("    %-7s %10.1f  [%10.1f .. %10.1f]   %3d aten ops%s, %d host synchronisations"
                     % (name, med[name], min(t[name]), max(t[name]), ops[name],
                        " + native launches" if name == "native" else "", syncs[name]))
    a, b = variants[0][0], variants[1][0]
    lines.append("    %s vs %s: %.2fx its speed (%.1f us %s)" % (a, b, med[b] / med[a], abs(med[b] - med[a]),
                                                                "less" if med[a] <= med[b] else "MORE"))
    if med[a] > med[b]:
        slower.append(title.split(":")[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    means, stds = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
    coder = DeltaXYWHBBoxCoder(means, stds)
    lines = ["box sampling, target building and the delta coder, fp32, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; per round the median of %d calls, each timed on the host between two device "
             "synchronisations; microseconds: median over the rounds [min .. max]" % (ROUNDS, ITERS)]
    slower = []
    for G in (300, 7):
        gen = torch.Generator(device="cpu").manual_seed(2000 + G)
        N = 268569
        anchors = boxes(N, gen, 1344, 800, 16, 512).to(dev)
        gts = boxes(G, gen, 1344, 800, 16, 400).to(dev)
        gi = torch.zeros(N, dtype=torch.long)
        sel = torch.randperm(N, generator=gen)
        npos = 30 * G
        gi[sel[:npos]] = torch.randint(1, G + 1, (npos,), generator=gen)
        gi[sel[npos:npos + 2000]] = -1
        gi = gi.to(dev)
        smp = RandomSampler(256, 0.5, add_gt_as_proposals=False)
        given = Given(G, gi)

        def native():
            return anchor_targets_single(anchors, gts, None, None, given, smp, coder, 1)

        def composed():
            return t_rpn(anchors, gi, gts, means, stds)
        n, c = native(), composed()
        ok = (int(n[4][0]) == int((c[3][:, 0] > 0).sum()), int(n[4][1]) == int((c[1] > 0).sum() - (c[3][:, 0] > 0).sum()))
        report(lines, slower, "rpn [%d] x %d (%d positives): sample + anchor targets" % (N, G, npos), [("native", native), ("torch", composed)],
               "; sampled counts equal the torch side's: %s %s" % ok)
    for G in (300, 7):
        gen = torch.Generator(device="cpu").manual_seed(3000 + G)
        props = boxes(1000, gen, 1344, 800, 16, 400).to(dev)
        gts = boxes(G, gen, 1344, 800, 16, 400).to(dev)
        gl = torch.randint(0, 1203, (G,), generator=gen).to(dev)
        gi = torch.zeros(1000, dtype=torch.long)
        gi[:300] = torch.randint(1, G + 1, (300,), generator=gen)
        gi = gi[torch.randperm(1000, generator=gen)].to(dev)
        cl = torch.where(gi > 0, gl[(gi - 1).clamp(min=0)], torch.full_like(gi, -1))
        smp = RandomSampler(512, 0.25, add_gt_as_proposals=True)

        def native():
            p = smp.sample_padded(AssignResult(G, gi, torch.zeros(1000, device=dev), cl), props, gts, gl)
            return bbox_targets([p], [gts], [gl], coder, 1203)

        def composed():
            return t_rcnn(props, gi, cl, gts, gl, means, stds, 1203)
        report(lines, slower, "rcnn [1000 + %d]: sample + RoI targets + rois" % G, [("native", native), ("torch", composed)])
    gen = torch.Generator(device="cpu").manual_seed(4000)
    rois = boxes(1000, gen, 1344, 800, 16, 400).to(dev)
    gt = boxes(1000, gen, 1344, 800, 16, 400).to(dev)
    for K in (1, 1203):
        d = ((torch.rand((1000, 4 * K), generator=gen) - 0.5) * 4).to(dev)
        if K == 1:
            report(lines, slower, "coder encode [1000, 4]", [("native", lambda: coder.encode(rois, gt)),
                                                             ("torch", lambda: t_bbox2delta(rois, gt, means, stds))])
        report(lines, slower, "coder decode [1000, 4 x %d]" % K, [("native", lambda: coder.decode(rois, d, (800, 1344, 3))),
                                                                  ("torch", lambda: t_delta2bbox(rois, d, means, stds, (800, 1344, 3)))])
    lines.append("slower than the torch ops: %s" % (", ".join(slower) if slower else "nowhere"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
