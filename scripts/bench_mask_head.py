#!/usr/bin/env python3
"""Time the two native ends of the mask branch (csrc/mask_ops.hip; iif_amd/mmdet_mask_target.py, iif_amd/mmdet_mask_loss.py)
against the reference's lines as torch operations, on the same GPU, same process, the variants alternating round by round.

    python scripts/bench_mask_head.py [--out profiles/mask_head.txt]

Shapes
  targets   the LVIS training shape: 2 images of 800 x 1333, G = 20 gt masks and 128 positives each, 28 x 28 targets
  paste     the LVIS test shape: N = 100 and N = 300 detections, C = 1203 classes, 28 x 28 logits into 800 x 1333
native  mask_target on device-resident masks (one launch, no host read) and on host masks (the uploads, one launch);
        get_seg_masks (one launch, two device-to-host copies; the block into page-locked or into pageable memory) and
        paste_masks alone (one launch, the result stays on the device)
torch   mask_target.py / structures.py line by line: the two blocking reads of proposals and indices, the upload of all gt
        masks, index_select into float32 [P, H, W], RoIAlign at C = 1 (this project's roi_align standing in for mmcv's), the
        threshold, the copy to the host, numpy, the upload; fcn_mask_head.py line by line: sigmoid, the class channel, chunks
        under the 1 GB limit, _do_paste_mask's grid with its isinf(...).any() checks, F.grid_sample, the threshold, the scatter
        into im_mask, N separate .cpu().numpy() copies
Before anything is timed the script asserts that both sides return the same bits (a pixel may differ only where its float32
value lies within 1e-5 of the threshold: the two sides sum in different orders; the count is reported).  End-to-end times are
wall-clock microseconds per call between two device synchronisations; kernel times come from torch's profiler in a pass of its
own and are set against the bytes each kernel must move.  No ratio is fixed in advance: the script reports, and lists every
shape at which the native path is slower."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_nms as bn  # noqa: E402
from iif_amd import mmdet_mask_loss as ml  # noqa: E402
from iif_amd import mmdet_mask_target as mt  # noqa: E402
from iif_amd.mmdet_roi_extractor import roi_align  # noqa: E402

ROUNDS, ITERS = 5, 3
IMG_H, IMG_W = 800, 1333
GPU_MEM_LIMIT = 1024 ** 3
NEAR = 1e-5            # two float32 evaluations in different summation orders may decide a value this close to 0.5 differently


# ---- the torch formulation
def t_mask_target_single(pos_proposals, pos_assigned_gt_inds, masks_np, mask_size):
    device = pos_proposals.device
    proposals_np = pos_proposals.cpu().numpy()
    maxh, maxw = masks_np.shape[1:]
    proposals_np[:, [0, 2]] = np.clip(proposals_np[:, [0, 2]], 0, maxw)
    proposals_np[:, [1, 3]] = np.clip(proposals_np[:, [1, 3]], 0, maxh)
    inds = torch.from_numpy(pos_assigned_gt_inds.cpu().numpy()).to(device=device)
    bboxes = torch.from_numpy(proposals_np).to(device=device)
    fake_inds = torch.arange(bboxes.shape[0], device=device).to(dtype=bboxes.dtype)[:, None]
    rois = torch.cat([fake_inds, bboxes], dim=1)
    gt_masks_th = torch.from_numpy(masks_np).to(device).index_select(0, inds).to(dtype=rois.dtype)
    targets = roi_align(gt_masks_th[:, None, :, :], rois, mask_size, 1.0, 0, 'avg', True).squeeze(1)
    resized = (targets >= 0.5).cpu().numpy()
    return torch.from_numpy(resized).float().to(device)


def t_mask_target(props, inds, masks_np, mask_size):
    return torch.cat([t_mask_target_single(p, i, m, mask_size) for p, i, m in zip(props, inds, masks_np)])


def t_do_paste_mask(masks, boxes, img_h, img_w):
    device = masks.device
    x0, y0, x1, y1 = torch.split(boxes, 1, dim=1)
    N = masks.shape[0]
    img_y = torch.arange(0, img_h, device=device).to(torch.float32) + 0.5
    img_x = torch.arange(0, img_w, device=device).to(torch.float32) + 0.5
    img_y = (img_y - y0) / (y1 - y0) * 2 - 1
    img_x = (img_x - x0) / (x1 - x0) * 2 - 1
    if torch.isinf(img_x).any():
        img_x[torch.where(torch.isinf(img_x))] = 0
    if torch.isinf(img_y).any():
        img_y[torch.where(torch.isinf(img_y))] = 0
    gx = img_x[:, None, :].expand(N, img_y.size(1), img_x.size(1))
    gy = img_y[:, :, None].expand(N, img_y.size(1), img_x.size(1))
    grid = torch.stack([gx, gy], dim=3)
    return F.grid_sample(masks.to(dtype=torch.float32), grid, align_corners=False)[:, 0]


def t_get_seg_masks(mask_pred, det_bboxes, det_labels, threshold, img_h, img_w, num_classes):
    mask_pred = mask_pred.sigmoid()
    device = mask_pred.device
    cls_segms = [[] for _ in range(num_classes)]
    bboxes, labels = det_bboxes[:, :4], det_labels
    N = len(mask_pred)
    num_chunks = int(np.ceil(N * int(img_h) * int(img_w) * 4 / GPU_MEM_LIMIT))
    chunks = torch.chunk(torch.arange(N, device=device), num_chunks)
    im_mask = torch.zeros(N, img_h, img_w, device=device, dtype=torch.bool)
    mask_pred = mask_pred[range(N), labels][:, None]
    for inds in chunks:
        masks_chunk = t_do_paste_mask(mask_pred[inds], bboxes[inds], img_h, img_w)
        im_mask[(inds,)] = (masks_chunk >= threshold).to(dtype=torch.bool)
    for i in range(N):
        cls_segms[labels[i]].append(im_mask[i].detach().cpu().numpy())
    return cls_segms


# ---- inputs
def blob_masks(G, gen):
    """uint8 [G, 800, 1333]: one ellipse per mask."""
    yy = torch.arange(IMG_H, dtype=torch.float32)[:, None]
    xx = torch.arange(IMG_W, dtype=torch.float32)[None, :]
    c = torch.rand((G, 2), generator=gen) * torch.tensor([IMG_W * 0.8, IMG_H * 0.8]) + torch.tensor([IMG_W * 0.1, IMG_H * 0.1])
    r = 20 + torch.rand((G, 2), generator=gen) * 160
    m = ((xx[None] - c[:, 0, None, None]) / r[:, 0, None, None]) ** 2 + ((yy[None] - c[:, 1, None, None]) / r[:, 1, None, None]) ** 2 <= 1
    return m.to(torch.uint8).numpy(), c, r


def positives(P, c, r, gen):
    """P proposals jittered around the ellipses' boxes (a few cross the image border) and their gt indices."""
    g = torch.randint(0, c.size(0), (P,), generator=gen)
    j = (torch.rand((P, 4), generator=gen) - 0.5) * 0.4 * torch.cat([r[g], r[g]], dim=1)
    box = torch.cat([c[g] - r[g], c[g] + r[g]], dim=1) + j
    return box.float(), g


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
        fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, fn in variants:
            t[name].append(one_round(fn))
    return t, {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def report(lines, slower, title, variants, native_name, torch_name, kernel_fn, kernel_word, must_move):
    t, med = measure(variants)
    lines.append(title)
    for name, _ in variants:
        lines.append("    %-28s end to end %12.1f us  [%12.1f .. %12.1f]" % (name, med[name], min(t[name]), max(t[name])))
    lines.append("    %s vs %s: %.2fx its speed" % (native_name, torch_name, med[torch_name] / med[native_name]))
    if med[native_name] > med[torch_name]:
        slower.append(title.split(":")[0])
    ks = bn.kernel_split(kernel_fn)
    mine = {k: v for k, v in (ks or {}).items() if kernel_word in k}
    if not mine:
        lines.append("    kernel time: not measured (the profiler recorded no device activity for %s)" % kernel_word)
        return
    us = sum(mine.values())
    lines.append("    %s: %.1f us per launch for %.2f MB that must move: %.1f GB/s" % (kernel_word, us, must_move / 1e6, must_move / us / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mask_head.py measures on the MI355X; there is nothing to report without one"
    dev = "cuda"
    lines = ["mask head ends, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; per round the median of %d calls, each timed on the host between two device "
             "synchronisations; microseconds: median over the rounds [min .. max]" % (ROUNDS, ITERS)]
    slower = []
    gen = torch.Generator(device="cpu").manual_seed(2030)

    # ---- training end
    G, P, size = 20, 128, (28, 28)
    masks_np, props, inds, area = [], [], [], 0.0
    for _ in range(2):
        m, c, r = blob_masks(G, gen)
        b, g = positives(P, c, r, gen)
        masks_np.append(m), props.append(b.to(dev)), inds.append(g.to(dev))
        cl = b.clone()
        cl[:, [0, 2]] = cl[:, [0, 2]].clamp(0, IMG_W)
        cl[:, [1, 3]] = cl[:, [1, 3]].clamp(0, IMG_H)
        area += float(((cl[:, 2] - cl[:, 0]) * (cl[:, 3] - cl[:, 1])).sum())
    masks_dev = [mt.DeviceBitmapMasks(m, IMG_H, IMG_W) for m in masks_np]
    for d in masks_dev:
        d.device_masks(dev)
    cfg = dict(mask_size=28)
    native_dev = lambda: mt.mask_target(props, inds, masks_dev, cfg)               # noqa: E731
    native_host = lambda: mt.mask_target(props, inds, masks_np, cfg)               # noqa: E731
    composed = lambda: t_mask_target(props, inds, masks_np, size)                  # noqa: E731
    a, b, c_ = native_dev(), native_host(), composed()
    assert torch.equal(a, b)
    soft = mt.mask_target(props, inds, masks_dev, dict(mask_size=28, soft_mask_target=True))
    bad = a != c_
    diff = int(bad.sum())
    assert diff == 0 or float((soft[bad] - 0.5).abs().max()) < NEAR, "the torch formulation and the native path disagree"
    same_t = "True" if diff == 0 else "but for %d pixels whose value lies within %g of 0.5" % (diff, NEAR)
    must = area + 2 * P * size[0] * size[1] * 4
    report(lines, slower, "targets: 2 images of %d x %d, G = %d, %d positives each, %d x %d; %.0f%% of the target pixels are 1; the torch "
           "side returns the same bits: %s" % (IMG_H, IMG_W, G, P, size[0], size[1], 100.0 * float(a.mean()), same_t),
           [("native, masks on the device", native_dev), ("native, host masks", native_host), ("torch", composed)],
           "native, host masks", "torch", native_dev, "mask_targets_kernel", must)
    lines.append("    the reference's float32 copy of the selected masks alone: %.0f MB written and read once per iteration"
                 % (2 * P * IMG_H * IMG_W * 4 / 1e6))

    # ---- test end
    C = 1203
    for N in (100, 300):
        boxes, _ = bn.clustered(N, gen)
        dets = torch.cat([boxes, torch.rand((N, 1), generator=gen)], dim=1).float().to(dev)
        labels = torch.randint(0, C, (N,), generator=gen).to(dev)
        pred = (torch.randn((N, C, 28, 28), generator=gen) * 3).to(dev)
        rcnn = dict(mask_thr_binary=0.5)
        native = lambda: ml.get_seg_masks(pred, dets, labels, rcnn, (IMG_H, IMG_W, 3), np.ones(4, dtype=np.float32), True, C)   # noqa: E731
        pageable = lambda: ml.get_seg_masks(pred, dets, labels, rcnn, (IMG_H, IMG_W, 3), np.ones(4, dtype=np.float32), True, C,   # noqa: E731
                                            pin_memory=False)
        launch = lambda: ml.paste_masks(pred, dets, labels, IMG_H, IMG_W, 0.5)                                                # noqa: E731
        composed = lambda: t_get_seg_masks(pred, dets, labels, 0.5, IMG_H, IMG_W, C)                                          # noqa: E731
        a, b = native(), composed()
        assert all(len(ca) == len(cb) for ca, cb in zip(a, b))
        diff = 0
        order = {int(c): [i for i in range(N) if int(labels[i]) == int(c)] for c in labels.unique()}
        for c, members in order.items():
            for i, x, y in zip(members, a[c], b[c]):
                bad = x != y
                if bad.any():                                   # a pixel may differ only where the value sits on the threshold
                    v = t_do_paste_mask(pred[i:i + 1, c].sigmoid()[:, None], dets[i:i + 1, :4], IMG_H, IMG_W)[0].cpu().numpy()
                    assert np.abs(v[bad] - 0.5).max() < NEAR, "the torch formulation and the native path disagree at N = %d" % N
                    diff += int(bad.sum())
        same_p = "True" if diff == 0 else "but for %d pixels whose value lies within %g of 0.5" % (diff, NEAR)
        must = N * IMG_H * IMG_W + N * 28 * 28 * 4
        report(lines, slower, "paste N = %d: C = %d, 28 x 28 into %d x %d, threshold 0.5; the torch side returns the same masks: %s"
               % (N, C, IMG_H, IMG_W, same_p), [("native get_seg_masks", native), ("native, pageable block", pageable), ("native paste_masks (device)", launch),
                                       ("torch", composed)],
               "native get_seg_masks", "torch", launch, "paste_masks_kernel", must)
    lines.append("slower than the torch formulation: %s" % (", ".join(slower) if slower else "nowhere"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
