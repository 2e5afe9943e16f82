"""HBM rate of the fused sigmoid BCE / focal loss kernel (iif_sigmoid_focal_fwd_bwd): algorithmic bytes (logits read
once, gradient written once in the logits' dtype, targets, per-row losses, class weights) over HIP-event time.
Prints one line per shape, dtype and gamma.  Needs the MI355X.

    python scripts/bench_focal_head.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iif_amd import custom  # noqa: E402

dev = "cuda:0"


def timed(fn, reps=50):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


SHAPES = ((256, 1000, torch.float32), (256, 1000, torch.bfloat16), (1024, 1204, torch.float32),
          (1024, 1204, torch.bfloat16), (65536, 1000, torch.float32), (65536, 1000, torch.bfloat16),
          (16384, 8142, torch.bfloat16))

for (B, C, dt) in SHAPES:
    counts = torch.tensor([max(int(1280 * (5 / 1280) ** (i / (C - 1.0))), 1) for i in range(C)])
    w = (counts.sum() / counts).float().to(dev)
    x = (torch.randn(B, C, device=dev) * 3).to(dt)
    y = torch.randint(0, C, (B,), device=dev)
    for gamma, alpha in ((0.0, None), (2.0, 0.25)):
        def k():
            custom._launch_focal(x, y, None, 1.0, w, gamma, alpha, 1.0 / (B * C), True)
        ms = timed(k)
        byt = B * C * 2 * x.element_size() + 8 * B + 4 * B + 4 * C
        print("iif_sigmoid_focal_fwd_bwd  B=%6d C=%5d %-8s gamma=%.1f %8.4f ms  %7.1f GB/s (algorithmic %7.1f MB)"
              % (B, C, str(dt).split(".")[-1], gamma, ms, byt / ms / 1e6, byt / 1e6))
