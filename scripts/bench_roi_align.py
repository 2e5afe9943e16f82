#!/usr/bin/env python3
"""Time SingleRoIExtractor (csrc/roi_align.hip, iif_amd/mmdet_roi_extractor.py), forward and backward, at the shapes of the LVIS
recipes, against the same mathematics as per-level torch ops on the same GPU, same process, the variants alternating round by
round.

    python scripts/bench_roi_align.py [--out profiles/roi_align.txt]

Shapes  4 images, FPN levels 200 x 336, 100 x 168, 50 x 84, 25 x 42 (strides 4 .. 32), C = 256, finest_scale 56;
        box head   K = 2048 rois at 7 x 7;   mask head   K = 512 rois at 14 x 14.
        Rois: sqrt(area) log-uniform in [16, 700), aspect ratio in [1/3, 3), centres anywhere in the 800 x 1344 image.
Variants
  native       the module on channels-last features: one launch forward; one clear + one launch backward.
  native nchw  the same on NCHW-contiguous features (one layout copy per level and call).
  torch        single_level_roi_extractor.py:86-115 as torch ops: per level a nonzero (a host synchronisation), a gather of rois,
               RoIAlign as gathers of the four corners of every sample (the same definition; autograd gives the backward:
               index_put with accumulate), and an index_put into the output.  The parent commit has no RoIAlign: this is the only
               baseline there is.  It needs one grid for all rois, so the comparison runs at sampling_ratio = 2; the native
               module is also timed at the recipes' sampling_ratio = 0 (adaptive grid).
Times are HIP-event microseconds per call (median and minimum over the rounds).  For the backward the script also reports the bytes
the atomics add - (distinct pixels with a non-zero weight) x C x 4 per bin, counted by the numpy restatement of
tests/roi_align_cases.py - divided by the time, beside the chip-wide float-atomic rate of about 1.3 TB/s.  No ratio is fixed in
advance: the script reports."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iif_amd.mmdet_roi_extractor import SingleRoIExtractor  # noqa: E402
from tests import roi_align_cases as rc                      # noqa: E402

ROUNDS, ITERS = 7, 5
DEV = "cuda"
N, C = 4, 256
SIZES = ((200, 336), (100, 168), (50, 84), (25, 42))
STRIDES = (4, 8, 16, 32)
FINEST = 56
ATOMIC_RATE = 1.3e12


def make_rois(K, seed):
    g = np.random.default_rng(seed)
    s = 16.0 * (700.0 / 16.0) ** g.random(K)
    r = 3.0 ** (2 * g.random(K) - 1)
    w, h = s * np.sqrt(r), s / np.sqrt(r)
    cx, cy = g.random(K) * 1344, g.random(K) * 800
    rois = np.stack([g.integers(0, N, K).astype(np.float64), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    return rois.astype(np.float32)


# ---- the reference's lines as torch ops
def t_axis(start, bin_, grid, P, size):
    p = torch.arange(P, device=start.device, dtype=torch.float32)[None, :, None]
    i = torch.arange(grid, device=start.device, dtype=torch.float32)[None, None, :]
    y = start[:, None, None] + p * bin_[:, None, None] + (i + 0.5) * bin_[:, None, None] / grid
    kept = ~((y < -1.0) | (y > size))
    y = torch.where(kept, y.clamp(min=0), torch.zeros_like(y))
    low = y.long()
    edge = low >= size - 1
    low = torch.where(edge, torch.full_like(low, size - 1), low)
    high = torch.where(edge, low, low + 1)
    y = torch.where(edge, low.float(), y)
    l = y - low.float()
    K = start.numel()
    return kept.view(K, -1), low.view(K, -1), high.view(K, -1), l.view(K, -1), (1.0 - l).view(K, -1)


def t_roi_align(x, rois, out, scale, sr):
    """x [N, C, H, W] (channels-last strides), rois [k, 5], fixed grid sr: [k, C, PH, PW]."""
    _, Cc, H, W = x.shape
    PH, PW = out
    k = rois.size(0)
    b = rois[:, 0].long()
    sw, sh = rois[:, 1] * scale - 0.5, rois[:, 2] * scale - 0.5
    bw, bh = (rois[:, 3] * scale - 0.5 - sw) / PW, (rois[:, 4] * scale - 0.5 - sh) / PH
    ky, yl, yh, ly, hy = t_axis(sh, bh, sr, PH, H)
    kx, xl, xh, lx, hx = t_axis(sw, bw, sr, PW, W)
    f = x.permute(0, 2, 3, 1)                                  # [N, H, W, C]: a gather returns [k, Y, X, C]
    bb = b[:, None, None]

    def corner(wy, ys, wx, xs):
        return (wy[:, :, None] * wx[:, None, :])[..., None] * f[bb, ys[:, :, None], xs[:, None, :]]
    val = corner(hy, yl, hx, xl) + corner(hy, yl, lx, xh) + corner(ly, yh, hx, xl) + corner(ly, yh, lx, xh)
    val = val * (ky[:, :, None] & kx[:, None, :])[..., None]
    return (val.view(k, PH, sr, PW, sr, Cc).sum((2, 4)) / (sr * sr)).permute(0, 3, 1, 2)


def t_extract(feats, rois, out, sr):
    num_levels = len(feats)
    roi_feats = feats[0].new_zeros(rois.size(0), feats[0].size(1), *out)
    scale = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
    lvls = torch.floor(torch.log2(scale / FINEST + 1e-6)).clamp(min=0, max=num_levels - 1).long()
    for i in range(num_levels):
        inds = (lvls == i).nonzero(as_tuple=False).squeeze(1)
        if inds.numel() > 0:
            roi_feats[inds] = t_roi_align(feats[i], rois[inds], out, 1.0 / STRIDES[i], sr)
        else:
            roi_feats = roi_feats + feats[i].sum() * 0.
    return roi_feats


def atomic_bytes(rois, out, sr):
    geo = dict(sizes=SIZES, scales=tuple(1.0 / s for s in STRIDES), out=out, sampling_ratio=sr, aligned=True, finest_scale=FINEST,
               factor=None, N=N)
    pixels = bins = 0
    for k in range(rois.shape[0]):
        _, skip, lvl, _, sh, sw, bh, bw, gh, gw, _ = rc.roi_geometry(rois[k], rc.F32, **geo)
        if skip or gh <= 0 or gw <= 0:
            continue
        H, W = SIZES[lvl]
        ny = (rc.axis_weights(sh, bh, gh, out[0], H, rc.F32) != 0).sum(1)
        nx = (rc.axis_weights(sw, bw, gw, out[1], W, rc.F32) != 0).sum(1)
        pixels += int(ny.sum()) * int(nx.sum())
        bins += int((ny > 0).sum()) * int((nx > 0).sum())
    return pixels * C * 4, pixels / max(bins, 1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / ITERS


def bench(variants):
    """{name: callable} -> {name: (median, min)} microseconds, the variants alternating round by round."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            t[k].append(timed(fn))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in t.items()}


def shape(lines, title, K, out):
    rois_np = make_rois(K, 7 + K)
    rois = torch.from_numpy(rois_np).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    cl = [torch.randn((N, C, h, w), device=DEV, generator=g).contiguous(memory_format=torch.channels_last).requires_grad_(True) for h, w in SIZES]
    nchw = [f.detach().contiguous().requires_grad_(True) for f in cl]
    gout = torch.randn((K, C) + out, device=DEV, generator=g)
    ext = {sr: SingleRoIExtractor(dict(type='RoIAlign', output_size=out, sampling_ratio=sr), C, list(STRIDES), finest_scale=FINEST) for sr in (0, 2)}
    ref = t_extract([f.detach() for f in cl], rois, out, 2)
    got = ext[2]([f.detach() for f in cl], rois)
    lines.append("%s: K = %d, %d x %d; native against torch at sampling_ratio 2: max |difference| %.2e" % (
        title, K, out[0], out[1], float((ref - got).abs().max())))

    def fwd_bwd(fn, feats):
        def run():
            for f in feats:
                f.grad = None
            fn(feats).backward(gout)
        return run
    fw = bench({"native sr0": lambda: ext[0]([f.detach() for f in cl], rois), "native sr2": lambda: ext[2]([f.detach() for f in cl], rois),
                "native nchw sr2": lambda: ext[2]([f.detach() for f in nchw], rois), "torch sr2": lambda: t_extract([f.detach() for f in cl], rois, out, 2)})
    fb = bench({"native sr0": fwd_bwd(lambda f: ext[0](f, rois), cl), "native sr2": fwd_bwd(lambda f: ext[2](f, rois), cl),
                "native nchw sr2": fwd_bwd(lambda f: ext[2](f, rois), nchw), "torch sr2": fwd_bwd(lambda f: t_extract(f, rois, out, 2), cl)})
    lines.append("  %-18s %12s %12s %14s %14s" % ("", "fwd median", "fwd min", "fwd+bwd median", "fwd+bwd min"))
    for k in fw:
        lines.append("  %-18s %10.1f us %10.1f us %11.1f us %11.1f us" % (k, fw[k][0], fw[k][1], fb[k][0], fb[k][1]))
    lines.append("  torch / native at sampling_ratio 2: forward %.1fx, forward + backward %.1fx" % (
        fw["torch sr2"][0] / fw["native sr2"][0], fb["torch sr2"][0] / fb["native sr2"][0]))
    for sr in (0, 2):
        nbytes, per_bin = atomic_bytes(rois_np, out, sr)
        bwd = fb["native sr%d" % sr][0] - fw["native sr%d" % sr][0]
        lines.append("  backward at sampling_ratio %d (fwd+bwd minus fwd, the arena's clear included): %.1f us; atomics add %.3f GB "
                     "(%.1f distinct pixels per bin) -> %.2f TB/s against the %.1f TB/s float-atomic rate (floor %.1f us)" % (
                         sr, bwd, nbytes / 1e9, per_bin, nbytes / (bwd * 1e-6) / 1e12, ATOMIC_RATE / 1e12, nbytes / ATOMIC_RATE * 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = ["SingleRoIExtractor (iif_roi_extract_forward / iif_roi_extract_backward, csrc/roi_align.hip) on %s" % torch.cuda.get_device_name(0),
             "4 images, levels 200 x 336 .. 25 x 42, C = 256, float32; HIP events, %d rounds x %d calls, variants alternating" % (ROUNDS, ITERS), ""]
    shape(lines, "box head", 2048, (7, 7))
    lines.append("")
    shape(lines, "mask head", 512, (14, 14))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
