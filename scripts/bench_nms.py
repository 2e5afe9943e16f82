#!/usr/bin/env python3
"""Time the native NMS / RPN proposals (csrc/nms.hip, iif_amd/mmdet_nms.py) against the same mathematics as torch operations in
mmcv 1.3.8's structure, on the same GPU, same process, the variants alternating round by round.

    python scripts/bench_nms.py [--out profiles/nms.txt]

Configurations
  train   B = 2, the five FPN levels of an 800 x 1333 image (200 x 336 ... 13 x 21, 3 anchors), nms_pre 2000, max_per_img 1000
  test    the same with nms_pre 1000
  nms     plain nms at N = 1000 and N = 8768, threshold 0.7
native  rpn_get_bboxes / nms (ten / five enqueued operations and the one host read of the counts)
torch   rpn_head.py:135-225 line by line (per-level sort, gathers, cat, torch decode, the min-size filter with its host
        read), then batched_nms as mmcv 1.3.8 runs it: boxes.max(), a sort, the suppression bit matrix built ON THE DEVICE with
        torch operations (the N x N IoU, packed to N x N / 64 words - mmcv's kernel makes the same matrix), a blocking copy to the
        host and the greedy scan in numpy over the words.  Before anything is timed the script asserts that both sides agree: the
        same kept indices for plain nms; for the RPN shapes the same number of proposals per image with every coordinate and score
        within 1e-2 (torch's exp on the device and expf differ in the last bits, so the rows are not compared as bit patterns).
End-to-end times are wall-clock microseconds per call between two device synchronisations (both sides wait for the host inside
the call).  Kernel times come from torch's profiler in a pass of its own (device durations per kernel name, averaged over the
profiled calls).  The scan's bytes per second are reported for plain nms only, where it walks the whole upper triangle, N (N / 64
+ 1) / 2 words of 8 bytes; at the RPN shapes it stops at max_per_img and how much it read is not known.
No ratio is fixed in advance: the script reports, and says which native kernel takes the largest share."""
import argparse
import os
import re
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iif_amd import mmdet_nms as mn  # noqa: E402
from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder  # noqa: E402

ROUNDS, ITERS = 5, 6
LEVELS = ((200, 336), (100, 168), (50, 84), (25, 42), (13, 21))
STRIDES = (4, 8, 16, 32, 64)
IMG = (800, 1333, 3)


# ---- the torch formulation
def t_delta2bbox(rois, deltas, max_shape, wh_ratio_clip=16 / 1000):
    dx, dy, dw, dh = deltas[:, 0::4], deltas[:, 1::4], deltas[:, 2::4], deltas[:, 3::4]
    px = ((rois[:, 0] + rois[:, 2]) * 0.5).unsqueeze(-1)
    py = ((rois[:, 1] + rois[:, 3]) * 0.5).unsqueeze(-1)
    pw = (rois[:, 2] - rois[:, 0]).unsqueeze(-1)
    ph = (rois[:, 3] - rois[:, 1]).unsqueeze(-1)
    mr = float(np.abs(np.log(wh_ratio_clip)))
    dw, dh = dw.clamp(min=-mr, max=mr), dh.clamp(min=-mr, max=mr)
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = px + pw * dx, py + ph * dy
    b = torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], dim=-1).view(deltas.size())
    hi = b.new_tensor([max_shape[1], max_shape[0]] * 2)
    b = torch.where(b < 0, b.new_zeros(()), b)
    return torch.where(b > hi, hi, b)


_bit = None


def t_nms(boxes, scores, thr):
    """mmcv 1.3.8's compiled nms in torch operations: sort, the bit matrix on the device, copy, the greedy scan on the host."""
    global _bit
    n = boxes.shape[0]
    order = scores.sort(descending=True, stable=True)[1]
    r = boxes[order]
    area = (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
    w = (torch.min(r[:, None, 2], r[None, :, 2]) - torch.max(r[:, None, 0], r[None, :, 0])).clamp_(min=0)
    h = (torch.min(r[:, None, 3], r[None, :, 3]) - torch.max(r[:, None, 1], r[None, :, 1])).clamp_(min=0)
    inter = w.mul_(h)
    hit = (inter / (area[:, None] + area[None, :] - inter) > thr).triu_(1)
    nw = (n + 63) // 64
    if _bit is None or _bit.device != boxes.device:
        _bit = (torch.ones(64, dtype=torch.int64, device=boxes.device) << torch.arange(64, device=boxes.device))
    padded = torch.zeros((n, nw * 64), dtype=torch.int64, device=boxes.device)
    padded[:, :n] = hit
    words = (padded.view(n, nw, 64) * _bit).sum(-1)                   # int64 wrap-around is the 64-bit word
    m = words.cpu().numpy().view(np.uint64)                             # the blocking copy
    removed = np.zeros(nw, dtype=np.uint64)
    keep = []
    one = np.uint64(1)
    for i in range(n):
        if not (removed[i >> 6] >> np.uint64(i & 63)) & one:
            keep.append(i)
            removed |= m[i]
    return order[torch.as_tensor(keep, dtype=torch.long, device=boxes.device)]


def t_batched_nms(boxes, scores, ids, thr):
    off = ids.to(boxes) * (boxes.max() + 1)
    keep = t_nms(boxes + off[:, None], scores, thr)
    return torch.cat([boxes[keep], scores[keep, None]], -1), keep


def t_rpn_single(cls, reg, anchors, img_shape, cfg):
    lvl_ids, sc, bp, an = [], [], [], []
    for i, (s, d) in enumerate(zip(cls, reg)):
        s = s.permute(1, 2, 0).reshape(-1).sigmoid()
        d = d.permute(1, 2, 0).reshape(-1, 4)
        a = anchors[i]
        if cfg.nms_pre > 0 and s.shape[0] > cfg.nms_pre:
            ranked, inds = s.sort(descending=True)
            inds = inds[:cfg.nms_pre]
            s, d, a = ranked[:cfg.nms_pre], d[inds, :], a[inds, :]
        sc.append(s)
        bp.append(d)
        an.append(a)
        lvl_ids.append(s.new_full((s.size(0),), i, dtype=torch.long))
    scores, anc, d, ids = torch.cat(sc), torch.cat(an), torch.cat(bp), torch.cat(lvl_ids)
    props = t_delta2bbox(anc, d, img_shape)
    if cfg.min_bbox_size >= 0:
        w, h = props[:, 2] - props[:, 0], props[:, 3] - props[:, 1]
        valid = (w > cfg.min_bbox_size) & (h > cfg.min_bbox_size)
        if not valid.all():
            props, scores, ids = props[valid], scores[valid], ids[valid]
    if props.numel() == 0:
        return props.new_zeros(0, 5)
    dets, _ = t_batched_nms(props, scores, ids, cfg.nms["iou_threshold"])
    return dets[:cfg.max_per_img]


def t_rpn(cls, reg, anchors, metas, cfg):
    return [t_rpn_single([c[b] for c in cls], [r[b] for r in reg], anchors, m["img_shape"], cfg) for b, m in enumerate(metas)]


# ---- measuring
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
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, fn in variants:
            t[name].append(one_round(fn))
    return t, {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def kernel_split(fn, calls=5):
    """{kernel name: mean device microseconds per call} from torch's profiler, or None where it records no device activity."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            dt = getattr(e, "device_time_total", None)
            if dt is None:
                dt = getattr(e, "cuda_time_total", 0.0)
            if dt and ("kernel" in e.key or "Memset" in e.key or "Memcpy" in e.key or "memset" in e.key):
                out[e.key] = dt / calls
        return out or None
    except Exception as exc:                                            # the end-to-end numbers stand without it
        print("profiler unavailable: %r" % (exc,))
        return None


def _short(name):
    m = re.search(r"(nms_\w+|rpn_\w+)", name)
    return (m.group(1) + (" (6 launches)" if m.group(1).startswith("rpn_select") else "")) if m else name[:48]


def report(lines, slower, title, native, composed, scan_bytes):
    t, med = measure([("native", native), ("torch", composed)])
    lines.append(title)
    for name in ("native", "torch"):
        lines.append("    %-7s end to end %10.1f us  [%10.1f .. %10.1f]" % (name, med[name], min(t[name]), max(t[name])))
    lines.append("    native vs torch: %.2fx its speed" % (med["torch"] / med["native"]))
    if med["native"] > med["torch"]:
        slower.append(title.split(":")[0])
    ks = kernel_split(native)
    if ks is None:
        lines.append("    per-kernel split: not measured (the profiler recorded no device activity)")
        return
    mine = {k: v for k, v in ks.items() if "nms_" in k or "rpn_" in k or "emset" in k}
    total = sum(mine.values())
    lines.append("    native device time %.1f us per call:" % total)
    for k, v in sorted(mine.items(), key=lambda kv: -kv[1]):
        short = _short(k)
        extra = ""
        if "nms_scan" in k and v > 0 and scan_bytes is None:
            extra = "   stops at max_per_img: bytes read not known"
        elif "nms_scan" in k and v > 0:
            extra = "   reads %.2f MB: %.1f GB/s" % (scan_bytes / 1e6, scan_bytes / v / 1e3)
        lines.append("        %-48s %9.1f us  %4.1f%%%s" % (short, v, 100.0 * v / total, extra))
    if mine:
        lines.append("    largest share: %s" % _short(max(mine, key=mine.get)))


def rpn_inputs(dev, B, gen):
    cls, reg, anchors = [], [], []
    for (h, w), s in zip(LEVELS, STRIDES):
        cls.append((torch.randn((B, 3, h, w), generator=gen) * 2.0 - 3.0).to(dev))
        reg.append((torch.randn((B, 12, h, w), generator=gen) * 0.3).to(dev))
        ratios = torch.tensor([0.5, 1.0, 2.0])
        ws, hs = 8.0 * s / ratios.sqrt(), 8.0 * s * ratios.sqrt()
        base = torch.stack([-0.5 * ws, -0.5 * hs, 0.5 * ws, 0.5 * hs], dim=-1)
        xx = (torch.arange(w) * s).float().repeat(h)
        yy = (torch.arange(h) * s).float().view(-1, 1).repeat(1, w).view(-1)
        shifts = torch.stack([xx, yy, xx, yy], dim=-1)
        anchors.append((base[None] + shifts[:, None]).view(-1, 4).to(dev))
    return cls, reg, anchors


def clustered(n, gen):
    nc_ = max(1, n // 6)
    c = torch.rand((nc_, 2), generator=gen) * torch.tensor([1333.0, 800.0])
    size = 16 + torch.rand((nc_, 2), generator=gen) * 120
    which = torch.randint(0, nc_, (n,), generator=gen)
    ctr = c[which] + (torch.rand((n, 2), generator=gen) - 0.5) * 24
    wh = size[which] + (torch.rand((n, 2), generator=gen) - 0.5) * 16
    return torch.cat([ctr - wh / 2, ctr + wh / 2], dim=1), torch.rand((n,), generator=gen)


def device_errors(dev, coder):
    """Lines on the device's decode and sigmoid against the float64 continuation, over the RPN cases of tests/nms_cases.py (the
    measure of tests/test_nms_gpu.py), next to the reference's own figures from the fixture."""
    from tests import nms_cases as nc
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(nc.__file__)), "golden", "g28_nms.npz"))
    worst_d, worst_s = 0.0, 0.0
    for name, c in nc.RPN_CASES.items():
        cls, reg, anchors = nc.rpn_inputs(name)
        t = lambda xs: [torch.from_numpy(x).to(dev) for x in xs]          # noqa: E731
        cfg = types.SimpleNamespace(nms_pre=c["nms_pre"], max_per_img=c["max_per_img"], min_bbox_size=c["min_size"],
                                    nms=dict(type="nms", iou_threshold=c["thr"]))
        _, _, cand = mn.rpn_proposals_padded(t(cls), t(reg), t(anchors), c["shapes"], cfg, coder, return_candidates=True)
        flat_anchors = np.concatenate(anchors)
        for b in range(len(c["shapes"])):
            idx = cand.index[b].cpu().numpy()
            flat = nc.rpn_flat(cls, reg, b)
            deltas = np.concatenate([d for _, d in flat])[idx]
            logits = np.concatenate([x for x, _ in flat])[idx]
            ok, kinds, err = nc.tc.decode_check(cand.boxes[b].cpu().numpy(), flat_anchors[idx], deltas, *nc.decode_args(c["shapes"][b]))
            assert ok and kinds
            worst_d, worst_s = max(worst_d, err), max(worst_s, nc.sigmoid_ulps(cand.scores[b].cpu().numpy(), logits))
    return ["error against the float64 continuation over the %d RPN cases of tests/nms_cases.py, float32 ulps: decode %.4f on the device "
            "(the reference's own float32 run: %.4f), sigmoid %.4f (the reference: %.4f)"
            % (len(nc.RPN_CASES), worst_d, float(g["ref_decode_ulps"]), worst_s, float(g["ref_sigmoid_ulps"]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nms.py measures on the MI355X; there is nothing to report without one"
    dev = "cuda"
    coder = DeltaXYWHBBoxCoder((0., 0., 0., 0.), (1., 1., 1., 1.))
    lines = ["NMS and the RPN proposal step, fp32, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; per round the median of %d calls, each timed on the host between two device "
             "synchronisations; microseconds: median over the rounds [min .. max]" % (ROUNDS, ITERS)]
    slower = []
    gen = torch.Generator(device="cpu").manual_seed(2028)
    B = 2
    cls, reg, anchors = rpn_inputs(dev, B, gen)
    metas = [dict(img_shape=IMG)] * B
    for label, pre, mpi in (("train", 2000, 1000), ("test", 1000, 1000)):
        cfg = types.SimpleNamespace(nms_pre=pre, max_per_img=mpi, min_bbox_size=0, nms=dict(type="nms", iou_threshold=0.7))
        native = lambda: mn.rpn_get_bboxes(cls, reg, anchors, metas, cfg, coder)          # noqa: E731
        composed = lambda: t_rpn(cls, reg, anchors, metas, cfg)                           # noqa: E731
        a, b = native(), composed()
        same = all(x.shape == y.shape and float((x - y).abs().max() if x.numel() else 0) < 1e-2 for x, y in zip(a, b))
        assert same, "the torch formulation and the native path disagree at the %s shape" % label
        ncand = sum(min(pre, 3 * h * w) for h, w in LEVELS)
        report(lines, slower, "%s: B = %d, %d candidates per image, nms_pre %d, max_per_img %d; kept %s; the torch side keeps the same "
               "proposals: %s" % (label, B, ncand, pre, mpi, [int(x.shape[0]) for x in a], same), native, composed, None)
    for n in (1000, 8768):
        boxes, scores = clustered(n, gen)
        boxes, scores = boxes.to(dev), scores.to(dev)
        native = lambda: mn.nms(boxes, scores, 0.7)                                         # noqa: E731
        composed = lambda: t_nms(boxes, scores, 0.7)                                        # noqa: E731
        same = torch.equal(native()[1], composed())
        assert same, "the torch formulation and the native nms keep different indices at N = %d" % n
        nw = (n + 63) // 64
        report(lines, slower, "nms N = %d, threshold 0.7: kept %d; the torch side keeps the same indices: %s"
               % (n, native()[1].numel(), same), native, composed, n * (nw + 1) // 2 * 8)
    lines.append("slower than the torch formulation: %s" % (", ".join(slower) if slower else "nowhere"))
    lines += device_errors(dev, coder)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
