#!/usr/bin/env python3
"""Time the fused Seesaw loss (forward + backward) against the same math written as torch ops, same GPU, same process.

    python scripts/bench_seesaw_head.py [--out profiles/seesaw_head.txt]

Shapes: [1024, 1205] (the LVIS bbox head of one image batch) and [8192, 1205].  The torch composition is the
log-domain form the kernel evaluates (no [C, C] matrix and no host loop, so it is a FASTER baseline than the
reference module, which also syncs once per distinct label); the count is ``index_add_`` of ones, the positive count
stays on the device.  Median of 100 timed iterations after 20 warm-up ones, CUDA events around each iteration, no
``.item()`` in the loop.  Also prints the largest difference between the two paths."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iif_amd.mmdet_seesaw_loss import SeesawLoss      # noqa: E402


def torch_seesaw(x, labels, w, cum, C, p, q, eps):
    """(classes, objectness) 'mean' losses from torch ops; updates cum in place."""
    cum.index_add_(0, labels, torch.ones_like(labels, dtype=torch.float32))
    pos = (labels < C).to(torch.float32)
    t = labels.clamp(max=C - 1)
    z, o = x[:, :C], x[:, C:]
    lc = cum[:C].clamp(min=1).log()
    zd = z.detach()
    lse = torch.logsumexp(zd, dim=1, keepdim=True)
    zt = zd.gather(1, t[:, None])
    add = (p * (lc[None, :] - lc[t][:, None])).clamp(max=0)
    add = add + (q * (zd - lse - (zt - lse).clamp(min=math.log(eps)))).clamp(min=0)
    add = add.scatter(1, t[:, None], 0.0)
    rows = torch.nn.functional.cross_entropy(z + add, t, reduction="none") * w * pos
    loss_cls = rows.sum() / pos.sum().clamp(min=1)
    loss_obj = (torch.nn.functional.cross_entropy(o, (labels == C).long(), reduction="none") * w).mean()
    return loss_cls, loss_obj


def timed(fn, warmup=20, iters=100):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    C, p, q, eps = 1203, 0.8, 2.0, 1e-2
    lines = ["fused Seesaw loss vs the same math as torch ops, forward + backward, fp32, %s" % torch.cuda.get_device_name(0),
             "median (min) of 100 iterations after 20 warm-up, events around each iteration, microseconds"]
    ok = True
    for N in (1024, 8192):
        gen = torch.Generator(device="cpu").manual_seed(N)
        x = (torch.randn(N, C + 2, generator=gen) * 3).to(dev)
        labels = torch.randint(0, C, (N,), generator=gen)
        labels[torch.rand(N, generator=gen) < 0.75] = C              # mmdet samples about 1:3 positives
        labels = labels.to(dev)
        w = torch.ones(N, device=dev)
        cum0 = torch.randint(0, 1000, (C + 1,), generator=gen).float().to(dev)
        m = SeesawLoss(p=p, q=q, num_classes=C, eps=eps, device=dev)
        m.cum_samples.copy_(cum0)
        cum_t = cum0.clone()
        xf = x.clone().requires_grad_(True)
        xt = x.clone().requires_grad_(True)

        def fused():
            xf.grad = None
            out = m(xf, labels, w)
            (out["loss_cls_classes"] + out["loss_cls_objectness"]).backward()

        def composed():
            xt.grad = None
            lc, lo = torch_seesaw(xt, labels, w, cum_t, C, p, q, eps)
            (lc + lo).backward()

        fused(); composed()
        diff = float((xf.grad - xt.grad).abs().max() / xt.grad.abs().max())
        same_cum = bool(torch.equal(m.cum_samples, cum_t))
        tf, tf_min = timed(fused)
        tt, tt_min = timed(composed)
        lines.append("[%5d, %d]  fused %8.1f (%8.1f)   torch ops %8.1f (%8.1f)   ratio %5.1fx   max grad diff %.1e  cum equal %s"
                     % (N, C + 2, tf, tf_min, tt, tt_min, tt / tf, diff, same_cum))
        ok = ok and tf <= tt
    lines.append("fused path not slower than the torch-op composition at either shape: %s" % ok)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
