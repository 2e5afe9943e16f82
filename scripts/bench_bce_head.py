#!/usr/bin/env python3
"""Time the detection sigmoid BCE (mmdet CrossEntropyLoss(use_sigmoid=True), csrc/bce_head.hip) against two yardsticks, same
GPU, same process, the variants alternating round by round.

    python scripts/bench_bce_head.py [--out profiles/bce_head.txt]

Shapes: [1024, 1204] and [8192, 1204] (the LVIS sigmoid baseline) and [524288, 1] (RPN objectness), fp32.
  module   CrossEntropyLoss(use_sigmoid=True): forward + backward through autograd (loss and gradient leave one launch,
           backward scales the gradient by the upstream scalar)
  torch    (a) the same math as torch ops: one-hot targets, the [N, C] weight matrix, binary_cross_entropy_with_logits,
           multiply, mean, backward - what a user has without the native path
  kernel   iif_bce_det_fwd_bwd alone (loss + gradient), K launches between two events
  focal    (b) iif_sigmoid_focal_fwd_bwd at gamma 0 on the same [N, C] alone, measured the same way: it moves the same logits
           and gradient bytes and is the project's streaming level for this kind of pass
Every round times each variant (median of its iterations); the table gives the median over the rounds and their range, so
the spread of (b) in this very call is next to the difference it is compared with.  Bytes: logits read + gradient written +
what the kernel reads per row (label 8 B + weight 4 B; focal: target 8 B + row loss 4 B written)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iif_amd import _lib, custom                              # noqa: E402
from iif_amd.mmdet_ce_loss import CrossEntropyLoss            # noqa: E402

ROUNDS, ITERS, K = 7, 30, 20


def torch_bce(x, labels, w, C):
    valid = (labels >= 0) & (labels != -100)
    y = torch.nn.functional.one_hot(labels.clamp(0, C), C + 1)[:, :C].to(torch.float32)      # a label >= C: an all-zero row
    bw = (w * valid).view(-1, 1).expand(-1, C)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, y, reduction="none")
    return (loss * bw).mean()


def one_round(fn, inner):
    """Median microseconds per call of ITERS event pairs, each around `inner` calls."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for a, b in ev:
        a.record()
        for _ in range(inner):
            fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 / inner for a, b in ev)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    lib = _lib.lib()
    lines = ["detection sigmoid BCE, fp32, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; per round the median of %d event pairs (kernel / focal: %d launches per pair); "
             "microseconds: median over the rounds [min .. max]" % (ROUNDS, ITERS, K)]
    verdict = []
    for N, C in ((1024, 1204), (8192, 1204), (524288, 1)):
        gen = torch.Generator(device="cpu").manual_seed(N)
        x = (torch.randn(N, C, generator=gen) * 3).to(dev)
        labels = torch.randint(0, C, (N,), generator=gen)
        labels[torch.rand(N, generator=gen) < 0.75] = C              # mmdet samples about 1:3 positives
        labels = labels.to(dev)
        w = torch.ones(N, device=dev)
        m = CrossEntropyLoss(use_sigmoid=True)
        xf = x.clone().requires_grad_(True)
        xt = x.clone().requires_grad_(True)
        _, ticket, status = custom._workspace(x.device, 0, False)
        loss = torch.empty((), device=dev)
        d = torch.empty_like(x)
        rows = torch.empty(N, device=dev)
        tfocal = labels.clamp(max=C - 1)                              # the focal entry has no background label
        stream = _lib.stream_ptr()
        scale = 1.0 / (N * C)

        def module():
            xf.grad = None
            m(xf, labels, w).backward()

        def composed():
            xt.grad = None
            torch_bce(xt, labels, w, C).backward()

        def kernel():
            lib.iif_bce_det_fwd_bwd(_lib.ptr(x), 0, C, _lib.ptr(labels), _lib.ptr(w), -100, None, None, None, scale, N, C, None,
                                    _lib.ptr(loss), _lib.ptr(d), C, _lib.ptr(ticket), stream)

        def focal():
            lib.iif_sigmoid_focal_fwd_bwd(_lib.ptr(x), 0, C, _lib.ptr(tfocal), None, 1.0, None, 0.0, 0, 0.0, scale, N, C,
                                          _lib.ptr(rows), _lib.ptr(loss), _lib.ptr(d), C, _lib.ptr(status), _lib.ptr(ticket), stream)

        variants = (("module", module, 1), ("torch", composed, 1), ("kernel", kernel, K), ("focal", focal, K))
        module(); composed()
        diff = float((xf.grad - xt.grad).abs().max() / xt.grad.abs().max())
        for _, fn, _ in variants:
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _, _ in variants}
        for _ in range(ROUNDS):
            for name, fn, inner in variants:
                t[name].append(one_round(fn, inner))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        nbytes = 8.0 * N * C + 12.0 * N
        lines.append("[%d, %d]  max grad diff module vs torch %.1e" % (N, C, diff))
        for name, _, _ in variants:
            extra = ""
            if name in ("kernel", "focal"):
                extra = "   %.2f TB/s (%.1f MB)" % (nbytes / med[name] * 1e-6, nbytes * 1e-6)
            lines.append("    %-7s %9.1f  [%9.1f .. %9.1f]%s" % (name, med[name], min(t[name]), max(t[name]), extra))
        beats = med["module"] < med["torch"]
        level = med["kernel"] <= max(t["focal"])
        lines.append("    module vs torch (a): %.1fx faster: %s;  kernel vs focal (b): %.2fx its time, within (b)'s range of this call: %s"
                     % (med["torch"] / med["module"], beats, med["kernel"] / med["focal"], level))
        verdict.append((N, C, beats, level))
    lines.append("faster than the torch ops at every shape: %s;  level with the focal kernel (or faster) at every shape: %s"
                 % (all(v[2] for v in verdict), all(v[3] for v in verdict)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
