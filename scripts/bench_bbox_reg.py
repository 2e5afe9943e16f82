#!/usr/bin/env python3
"""Time the box-regression head (mmdet L1Loss / SmoothL1Loss, csrc/bbox_reg_head.hip) against the same math as torch ops, same
GPU, same process, the variants alternating round by round.

    python scripts/bench_bbox_reg.py [--out profiles/bbox_reg_head.txt]

Shapes, forward + backward through autograd:
  [1024, 4812] fp32, L1Loss          bbox_head_reg_loss, the LVIS box head (1203 classes, about one row in four positive)
  [1024, 4]    fp32, SmoothL1Loss    bbox_head_reg_loss, a class-agnostic (Cascade) head
  [434000, 4]  fp32, L1Loss          the module on a flat range, the RPN size
  fused    the native path: one launch forward, one backward
  torch    the ops of bbox_head.py:284-311 / smooth_l1_loss.py restated: pos_inds, .any(), three boolean indexings, abs / where /
           mul / sum / div, and autograd's index_put into a zero [N, 4C] tensor - what a user has without the native path
At the first shape also, K launches between two events each (report only, no gate):
  forward  iif_bbox_reg_fwd alone
  scatter  iif_bbox_reg_scatter_grad alone, with the bytes it stores per second
  zero_    torch's fill of the same [N, 4C] tensor: the floor of a 19.7 MB store stream
Every round times each variant (median of its iterations); the table gives the median over the rounds and their range, so
the spread of the baseline in this very call is next to the difference it is compared with.  Acceptance: at every shape
`fused` is faster than `torch` by more than the range of `torch`."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iif_amd import _lib, custom                                           # noqa: E402
from iif_amd.mmdet_bbox_loss import L1Loss, SmoothL1Loss, bbox_head_reg_loss  # noqa: E402

ROUNDS, ITERS, K = 7, 30, 20


def torch_loss(pred, target, weight, beta, avg_factor=None):
    diff = torch.abs(pred - target)
    loss = diff if beta == 0.0 else torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
    loss = loss * weight
    return loss.mean() if avg_factor is None else loss.sum() / avg_factor


def torch_head(bbox_pred, labels, targets, weights, num_classes, agnostic, beta):
    pos_inds = (labels >= 0) & (labels < num_classes)
    if pos_inds.any():
        if agnostic:
            pos_bbox_pred = bbox_pred.view(bbox_pred.size(0), 4)[pos_inds]
        else:
            pos_bbox_pred = bbox_pred.view(bbox_pred.size(0), -1, 4)[pos_inds, labels[pos_inds]]
        return torch_loss(pos_bbox_pred, targets[pos_inds], weights[pos_inds], beta, targets.size(0))
    return bbox_pred[pos_inds].sum()


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


def measure(variants):
    for _, fn, _ in variants:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _, _ in variants}
    for _ in range(ROUNDS):
        for name, fn, inner in variants:
            t[name].append(one_round(fn, inner))
    return t, {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    lib = _lib.lib()
    lines = ["box-regression head, fp32, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; per round the median of %d event pairs (forward / scatter / zero_: %d launches per "
             "pair); microseconds: median over the rounds [min .. max]" % (ROUNDS, ITERS, K)]
    verdict = []
    for N, C, num_classes, agnostic, beta in ((1024, 1203, 1203, False, 0.0), (1024, 1, 80, True, 1.0), (434000, 0, 0, False, 0.0)):
        gen = torch.Generator(device="cpu").manual_seed(N + C)
        plain = C == 0
        W = 4 if plain else 4 * C
        x = (torch.randn(N, W, generator=gen) * 0.5).to(dev)
        targets = (torch.randn(N, 4, generator=gen) * 0.5).to(dev)
        m = L1Loss() if beta == 0.0 else SmoothL1Loss(beta=beta)
        xf = x.clone().requires_grad_(True)
        xt = x.clone().requires_grad_(True)
        if plain:
            weights = (torch.rand(N, 4, generator=gen) < 0.5).float().to(dev)            # RPN: sampled anchors weigh 1
            avg = float(N // 4)

            def fused():
                xf.grad = None
                m(xf, targets, weights, avg_factor=avg).backward()

            def composed():
                xt.grad = None
                torch_loss(xt, targets, weights, beta, avg).backward()
            label = "[%d, 4] %s, the module" % (N, type(m).__name__)
        else:
            labels = torch.randint(0, num_classes, (N,), generator=gen)
            labels[torch.rand(N, generator=gen) < 0.75] = num_classes                    # mmdet samples about 1:3 positives
            weights = (labels < num_classes).float().view(N, 1).expand(N, 4).contiguous().to(dev)
            labels = labels.to(dev)

            def fused():
                xf.grad = None
                bbox_head_reg_loss(m, xf, labels, targets, weights, num_classes, reg_class_agnostic=agnostic).backward()

            def composed():
                xt.grad = None
                torch_head(xt, labels, targets, weights, num_classes, agnostic, beta).backward()
            label = "[%d, %d] %s, bbox_head_reg_loss" % (N, W, type(m).__name__)
        variants = [("fused", fused, 1), ("torch", composed, 1)]
        fused(); composed()
        diff = float((xf.grad - xt.grad).abs().max() / xt.grad.abs().max())
        same_zeros = bool(((xf.grad != 0) == (xt.grad != 0)).all())
        if not plain and not agnostic:
            _, ticket, _ = custom._workspace(x.device, 0, False)
            loss = torch.empty((), device=dev)
            dsel = torch.empty(N, 4, device=dev)
            d = torch.empty_like(x)
            g = torch.ones((), device=dev)
            stream = _lib.stream_ptr()

            def forward():
                lib.iif_bbox_reg_fwd(_lib.ptr(x), 0, W, _lib.ptr(labels), num_classes, C, _lib.ptr(targets), _lib.ptr(weights), beta,
                                     1.0 / N, 4 * N, N, None, _lib.ptr(loss), _lib.ptr(dsel), _lib.ptr(ticket), stream)

            def scatter():
                lib.iif_bbox_reg_scatter_grad(_lib.ptr(dsel), _lib.ptr(labels), num_classes, N, C, _lib.ptr(g), _lib.ptr(d), 0, W,
                                              stream)

            def zero():
                d.zero_()
            variants += [("forward", forward, K), ("scatter", scatter, K), ("zero_", zero, K)]
        t, med = measure(variants)
        lines.append("%s:  max grad diff fused vs torch %.1e, same zero positions: %s" % (label, diff, same_zeros))
        for name, _, _ in variants:
            extra = ""
            if name in ("scatter", "zero_"):
                extra = "   %.2f TB/s (%.1f MB stored)" % (4.0 * N * W / med[name] * 1e-6, 4.0 * N * W * 1e-6)
            lines.append("    %-8s %9.1f  [%9.1f .. %9.1f]%s" % (name, med[name], min(t[name]), max(t[name]), extra))
        spread = max(t["torch"]) - min(t["torch"])
        beats = med["torch"] - med["fused"] > spread
        lines.append("    fused vs torch: %.1fx faster, %.1f us less against a torch range of %.1f us in this call: %s"
                     % (med["torch"] / med["fused"], med["torch"] - med["fused"], spread, beats))
        if "scatter" in med:
            lines.append("    scatter vs zero_: %.2fx its time" % (med["scatter"] / med["zero_"]))
        verdict.append(beats)
    lines.append("faster than the torch ops by more than their spread at every shape: %s" % all(verdict))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
