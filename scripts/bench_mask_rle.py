#!/usr/bin/env python3
"""Time the test end of the mask branch with the COCO run-length encoding done on the device (csrc/mask_rle.hip;
iif_amd.mmdet_mask_loss.get_seg_masks_rle) against get_seg_masks, which stops at the boolean masks, on the same GPU, same
process, the variants alternating round by round.

    python scripts/bench_mask_rle.py [--out profiles/mask_rle.txt]

Shape   the LVIS test shape: N = 100 and N = 300 detections, C = 1203 classes, 28 x 28 logits into 800 x 1333, threshold 0.5
Logits  "blobs": one smooth ellipse per detection, two runs per column of the box (about a hundred per mask at these box sizes),
        what a trained head produces;  "noise": 3 * randn, the input of scripts/bench_mask_head.py - about a thousand runs per
        mask, far from real ones
rle        get_seg_masks_rle: count, scan, fill, differences; two device-to-host copies (run counts + labels, runs); the strings
baseline   get_seg_masks: one launch and the copy of the boolean block into page-locked memory.  It does LESS: no encoding.
encoded    encode_mask_results' loop over the baseline's masks - timed only where pycocotools imports, else "not measured"
Before anything is timed the script asserts that get_seg_masks_rle returns, byte for byte, tests/rle_ref.py's encoding of the
baseline's masks.  End-to-end times are wall-clock microseconds per call between two device synchronisations; device times come
from torch's profiler in a pass of its own.  No ratio is fixed in advance: the script reports what it measures."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_mask_head as bm  # noqa: E402
import bench_nms as bn  # noqa: E402
from iif_amd import mmdet_mask_loss as ml  # noqa: E402
from tests import rle_ref  # noqa: E402

IMG_H, IMG_W, C = bm.IMG_H, bm.IMG_W, 1203

try:
    import pycocotools.mask as mask_util
except Exception:                                                       # not a dependency: the row says "not measured"
    mask_util = None


def blob_logits(n, gen):
    """[n, 28, 28]: +4 inside an ellipse, -4 outside, a smooth edge."""
    yy = torch.arange(28, dtype=torch.float32)[:, None]
    xx = torch.arange(28, dtype=torch.float32)[None, :]
    c = 10 + torch.rand((n, 2), generator=gen) * 8
    r = 6 + torch.rand((n, 2), generator=gen) * 7
    d = ((xx[None] - c[:, 0, None, None]) / r[:, 0, None, None]) ** 2 + ((yy[None] - c[:, 1, None, None]) / r[:, 1, None, None]) ** 2
    return (1 - d).clamp(-1, 1) * 4


def encode_mask_results(cls_segms):
    """mmdet/core/mask/utils.py:37-64 for one image."""
    return [[mask_util.encode(np.array(m[:, :, np.newaxis], order='F', dtype='uint8'))[0] for m in ms] for ms in cls_segms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mask_rle.py measures on the MI355X; there is nothing to report without one"
    dev = "cuda"
    lines = ["mask RLE on the device, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; per round the median of %d calls, each timed on the host between two device "
             "synchronisations; microseconds: median over the rounds [min .. max]" % (bm.ROUNDS, bm.ITERS),
             "the baseline does less work: it returns boolean masks and encodes nothing"]
    gen = torch.Generator(device="cpu").manual_seed(2031)
    rcnn, ori, sf = dict(mask_thr_binary=0.5), (IMG_H, IMG_W, 3), np.ones(4, dtype=np.float32)
    for kind in ("blobs", "noise"):
        for N in (100, 300):
            boxes, _ = bn.clustered(N, gen)
            dets = torch.cat([boxes, torch.rand((N, 1), generator=gen)], dim=1).float().to(dev)
            labels = torch.randint(0, C, (N,), generator=gen).to(dev)
            if kind == "blobs":
                pred = torch.zeros((N, C, 28, 28))
                pred[torch.arange(N), labels.cpu()] = blob_logits(N, gen)
                pred = pred.to(dev)
            else:
                pred = (torch.randn((N, C, 28, 28), generator=gen) * 3).to(dev)
            rle = lambda: ml.get_seg_masks_rle(pred, dets, labels, rcnn, ori, sf, True, C)        # noqa: E731
            base = lambda: ml.get_seg_masks(pred, dets, labels, rcnn, ori, sf, True, C)           # noqa: E731
            a, b = rle(), base()
            runs = 0
            for ca, cb in zip(a, b):
                assert len(ca) == len(cb)
                for x, y in zip(ca, cb):
                    assert x == rle_ref.encode_rle(y), "get_seg_masks_rle and the encoded masks of get_seg_masks disagree"
                    runs += len(rle_ref.from_string(x["counts"]))
            copied = N * 4 + N * 8 + runs * 4
            variants = [("get_seg_masks_rle", rle), ("get_seg_masks (no encoding)", base)]
            if mask_util is not None:
                variants.append(("get_seg_masks + encode loop", lambda: encode_mask_results(base())))
            t, med = bm.measure(variants)
            lines.append("%s, N = %d: C = %d, 28 x 28 into %d x %d; %d runs in all (%.0f per mask); the same bytes as the encoded "
                         "baseline masks: True" % (kind, N, C, IMG_H, IMG_W, runs, runs / N))
            for name, _ in variants:
                lines.append("    %-30s end to end %12.1f us  [%12.1f .. %12.1f]" % (name, med[name], min(t[name]), max(t[name])))
            if mask_util is None:
                lines.append("    %-30s not measured (pycocotools does not import here)" % "get_seg_masks + encode loop")
            lines.append("    get_seg_masks_rle vs get_seg_masks: %.2fx its speed; copied to the host: %.1f KB against %.1f MB"
                         % (med["get_seg_masks (no encoding)"] / med["get_seg_masks_rle"], copied / 1e3, (N * IMG_H * IMG_W + N * 8) / 1e6))
            ks = bn.kernel_split(rle)
            mine = {k: v for k, v in (ks or {}).items() if "rle_" in k or "Memcpy" in k}
            if not mine:
                lines.append("    device time: not measured (the profiler recorded no device activity)")
                continue
            lines.append("    device time per call: %.1f us in all" % sum(mine.values()))
            for k, v in sorted(mine.items(), key=lambda kv: -kv[1]):
                short = k.replace("(anonymous namespace)::", "")
                short = short[short.index("rle_"):].split("(")[0][:60] if "rle_" in short else short[:60]
                lines.append("        %-60s %10.1f us" % (short, v))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
