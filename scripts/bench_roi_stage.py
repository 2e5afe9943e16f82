#!/usr/bin/env python3
"""Time the RoI stage in one launch (csrc/roi_stage.hip, iif_amd/mmdet_roi_stage.py) against the existing per-image chain of
native entries, on the same GPU, same process, fed the same keys, the variants alternating round by round.

    python scripts/bench_roi_stage.py [--out profiles/roi_stage.txt]

Shapes
  lvis-g20 / lvis-g300   the LVIS training shape: B = 2 images, P = 1000 proposals each with device counts, num = 512,
                         pos_fraction 0.25, thresholds 0.5 without low-quality matching, add_gt_as_proposals, 1203 classes,
                         G = 20 and G = 300 ground-truth boxes per image
  cascade                three stages (thresholds 0.5, 0.6, 0.7) at B = 2, G = 20: targets, then twice (refine, targets)
new     roi_stage_targets_padded (the key draw and one launch); in the cascade refine_bboxes_padded between the stages
chain   per image MaxIoUAssigner.assign, RandomSampler.sample_padded, then bbox_targets (what the parent commit offers), on the
        sliced proposals - the counts are known to the benchmark from the start, so the chain is NOT charged the host read it
        would need in training; in the cascade the reference-structure refine_bboxes as torch operations (unique, a nonzero
        per image, gather, the native delta2bbox, boolean indexing), which does read
Before anything is timed the script asserts that both sides return the same bits.  End-to-end times are wall-clock
microseconds per call between two device synchronisations, host work included; the chain is measured TWICE in the same run
("chain", "chain again") and the difference of the two medians is its run-to-run spread.  Device times and the number of enqueued
operations come from torch's profiler in a pass of its own."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_nms as bn  # noqa: E402
from iif_amd.mmdet_assigner import MaxIoUAssigner  # noqa: E402
from iif_amd.mmdet_roi_stage import refine_bboxes_padded, roi_stage_targets_padded  # noqa: E402
from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler, bbox_targets, delta2bbox  # noqa: E402

IMG = (800, 1333, 3)
CLASSES = 1203
NUM, FRAC = 512, 0.25
FIELDS = ("labels", "label_weights", "bbox_targets", "bbox_weights", "rois", "pos_assigned_gt_inds")


def make_inputs(gen, B, P, G, dev):
    """Ground-truth boxes of 16 .. 320 pixels and proposals of which a third are ground-truth boxes moved by up to 12 pixels."""
    gts, labs, props = [], [], torch.zeros((B, P, 5))
    for b in range(B):
        xy = torch.rand((G, 2), generator=gen) * torch.tensor([IMG[1] - 330.0, IMG[0] - 330.0])
        wh = 16 + torch.rand((G, 2), generator=gen) * 304
        g = torch.cat([xy, xy + wh], 1)
        pxy = torch.rand((P, 2), generator=gen) * torch.tensor([IMG[1] - 130.0, IMG[0] - 130.0])
        p = torch.cat([pxy, pxy + 8 + torch.rand((P, 2), generator=gen) * 120], 1)
        k = torch.arange(0, P, 3)
        p[k] = g[k % G] + (torch.rand((k.numel(), 2), generator=gen) * 24 - 12).repeat(1, 2)
        props[b, :, :4], props[b, :, 4] = p, torch.rand((P,), generator=gen)
        gts.append(g.to(dev))
        labs.append(torch.randint(0, CLASSES, (G,), generator=gen).to(dev))
    return props.to(dev), gts, labs


def chain_targets(props_list, gts, labs, asg, smp, coder, keys):
    ps = []
    for b, p in enumerate(props_list):
        front = gts[b].shape[0] if smp.add_gt_as_proposals else 0
        ar = asg.assign(p, gts[b], None, labs[b])
        ps.append(smp.sample_padded(ar, p, gts[b], labs[b], keys=keys[b, :front + p.shape[0]]))
    return bbox_targets(ps, gts, labs, coder, CLASSES), ps


def t_refine(rois, labels, preds, pos_is_gts, coder, B):
    """bbox_head.py:431-456 + regress_by_class in its structure; the decode is the native one."""
    rois[:, 0].long().unique(sorted=True)
    out = []
    for i in range(B):
        inds = torch.nonzero(rois[:, 0] == i, as_tuple=False).squeeze(dim=1)
        lab = labels[inds] * 4
        d = torch.gather(preds[inds], 1, torch.stack((lab, lab + 1, lab + 2, lab + 3), 1))
        boxes = delta2bbox(rois[inds, 1:], d, coder.means, coder.stds, IMG)
        keep = pos_is_gts[i].new_ones(inds.numel())
        keep[:len(pos_is_gts[i])] = 1 - pos_is_gts[i]
        out.append(boxes[keep.type(torch.bool)])
    return out


def device_ops(fn, calls=5):
    """(device microseconds per call, enqueued device operations per call, {name: microseconds per call}) from torch's profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        names, total, count = {}, 0.0, 0
        for e in prof.events():
            if "CUDA" in str(getattr(e, "device_type", "")):                    # a kernel, memset or copy on the device
                dt = e.time_range.elapsed_us()
                names[e.name] = names.get(e.name, 0.0) + dt / calls
                total += dt / calls
                count += 1
        return (total, count / calls, names) if count else None
    except Exception as exc:                                            # the end-to-end numbers stand without it
        print("profiler unavailable: %r" % (exc,))
        return None


def report(lines, title, new, chain):
    t, med = bn.measure([("chain", chain), ("new", new), ("chain again", chain)])
    lines.append(title)
    for name in ("new", "chain", "chain again"):
        lines.append("    %-11s end to end %9.1f us  [%9.1f .. %9.1f]" % (name, med[name], min(t[name]), max(t[name])))
    spread = abs(med["chain"] - med["chain again"])
    base = min(med["chain"], med["chain again"])
    lines.append("    the chain's run-to-run spread (its two medians): %.1f us; new vs chain: %.2fx its speed" % (spread, base / med["new"]))
    verdict = "not slower than the chain" if med["new"] <= base + spread else "SLOWER than the chain by more than its spread"
    lines.append("    condition (new <= chain + spread): %s" % verdict)
    for name, fn in (("new", new), ("chain", chain)):
        ops = device_ops(fn)
        if ops is None:
            lines.append("    %s: device time not measured (the profiler recorded no device activity)" % name)
            continue
        total, count, names = ops
        lines.append("    %-5s device time %8.1f us per call in %.0f enqueued operations" % (name, total, count))
        if name == "new":
            for k, v in sorted(names.items(), key=lambda kv: -kv[1])[:4]:
                lines.append("        %-60s %8.1f us" % (k[:60], v))
    return med["new"] <= base + spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_roi_stage.py measures on the MI355X; there is nothing to report without one"
    dev = "cuda"
    lines = ["RoI-stage targets, fp32, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; per round the median of %d calls, each timed on the host between two device "
             "synchronisations (host work included); microseconds: median over the rounds [min .. max]" % (bn.ROUNDS, bn.ITERS)]
    gen = torch.Generator(device="cpu").manual_seed(2033)
    coder = DeltaXYWHBBoxCoder((0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2))
    smp = RandomSampler(NUM, FRAC, add_gt_as_proposals=True)
    B, P = 2, 1000
    ok = True
    for G in (20, 300):
        props, gts, labs = make_inputs(gen, B, P, G, dev)
        counts = torch.tensor([P, P - 137], dtype=torch.int64).to(dev)
        ns = [P, P - 137]
        sliced = [props[b, :n] for b, n in enumerate(ns)]
        keys = torch.randint(0, 2 ** 31, (B, G + P), dtype=torch.int32, generator=gen).to(dev)
        asg = MaxIoUAssigner(0.5, 0.5, 0.5, match_low_quality=False)
        new = lambda: roi_stage_targets_padded(props, counts, gts, labs, asg, smp, coder, CLASSES, keys=keys)     # noqa: E731
        chain = lambda: chain_targets(sliced, gts, labs, asg, smp, coder, keys)[0]                                # noqa: E731
        a, c = new(), chain()
        same = all(torch.equal(getattr(a, f).view(-1).view(torch.int32 if w.dtype == torch.float32 else w.dtype),
                               w.view(-1).view(torch.int32 if w.dtype == torch.float32 else w.dtype)) for f, w in zip(FIELDS, c))
        assert same, "the single launch and the chain disagree at G = %d" % G
        ok &= report(lines, "lvis-g%d: B = %d, P = %d (counts %s), G = %d, num = %d, %d positives and %d negatives kept; the chain "
                     "returns the same bits: %s" % (G, B, P, ns, G, NUM, int(a.counts[:, 0].sum()), int(a.counts[:, 1].sum()), same),
                     new, chain)

    # ---- the three-stage cascade
    G = 20
    props, gts, labs = make_inputs(gen, B, P, G, dev)
    counts = torch.tensor([P, P - 137], dtype=torch.int64).to(dev)
    ns = [P, P - 137]
    sliced = [props[b, :n] for b, n in enumerate(ns)]
    stage_keys = [torch.randint(0, 2 ** 31, (B, G + P), dtype=torch.int32, generator=gen).to(dev) for _ in range(3)]
    asgs = [MaxIoUAssigner(t, t, t, match_low_quality=False) for t in (0.5, 0.6, 0.7)]
    preds = [(torch.randn((B * NUM, 4 * 8), generator=gen) * 0.5).to(dev) for _ in range(2)]
    shapes = [IMG] * B

    def cls_of(labels):
        return torch.where(labels < 8, labels, labels % 8)                                   # stands for the argmax over 8 classes

    def new_cascade():
        t = roi_stage_targets_padded(props, counts, gts, labs, asgs[0], smp, coder, CLASSES, keys=stage_keys[0])
        outs = [t]
        for i in range(2):
            boxes, kept = refine_bboxes_padded(t.rois, cls_of(t.labels), preds[i], t.pos_is_gt, t.counts, shapes, coder)
            t = roi_stage_targets_padded(boxes, kept, gts, labs, asgs[i + 1], smp, coder, CLASSES,
                                         keys=stage_keys[i + 1][:, :G + NUM].contiguous())
            outs.append(t)
        return outs

    def chain_cascade():
        cur, outs = sliced, []
        for i in range(3):
            t, ps = chain_targets(cur, gts, labs, asgs[i], smp, coder, stage_keys[i] if i == 0 else stage_keys[i][:, :G + NUM])
            outs.append(t)
            if i == 2:
                break
            cnt = torch.stack([p.counts for p in ps]).tolist()                                # the read the padded rows need here
            rows = torch.cat([torch.arange(b * NUM, b * NUM + sum(c), device=dev) for b, c in enumerate(cnt)])
            is_gts = [p.gt_flags[p.pos_inds[:c[0]]] for p, c in zip(ps, cnt)]
            cur = t_refine(t[4][rows], cls_of(t[0][rows]), preds[i][rows], is_gts, coder, B)
        return outs

    a, c = new_cascade(), chain_cascade()
    same = all(torch.equal(getattr(x, f).view(-1).view(torch.int32 if w.dtype == torch.float32 else w.dtype),
                           w.view(-1).view(torch.int32 if w.dtype == torch.float32 else w.dtype))
               for x, y in zip(a, c) for f, w in zip(FIELDS, y))
    assert same, "the cascade loops disagree"
    report(lines, "cascade: three stages (0.5, 0.6, 0.7) at B = %d, P = %d, G = %d, num = %d; the chain with the reference-structure "
           "refine_bboxes returns the same bits: %s" % (B, P, G, NUM, same), new_cascade, chain_cascade)
    lines.append("training shape, end to end: the single launch is %s" % (
        "not slower than the per-image chain at either G" if ok else
        "SLOWER than the per-image chain at one of the shapes above: one workgroup per image is the weak spot"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
