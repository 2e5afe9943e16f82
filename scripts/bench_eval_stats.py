"""Time of the fused evaluation-statistics launch (iif_eval_accumulate through EvalAccumulator.update) against
  * today's per-batch path of train.evaluate: iif_scale_logits + iif_topk_hits + two .item() (wall time, it syncs),
  * iif_topk_hits alone on the scaled logits (HIP-event time),
  * a torch composition of the same statistics (scale, softmax, max, argmax, bucketize, bincount; HIP-event time).
The fused launch reads the fp32 logits once with the IIF table applied in registers; GB/s is the logits' bytes over the
time, against the 8 TB/s HBM roof.  Prints one line per shape.  Needs the MI355X.

    python scripts/bench_eval_stats.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iif_amd import custom, utils  # noqa: E402
from iif_amd.eval_stats import EvalAccumulator  # noqa: E402

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
    return e0.elapsed_time(e1) / reps * 1e3


def wall(fn, reps=50):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


SHAPES = ((128, 100), (256, 1000), (1024, 1204), (64, 8142), (65536, 1000))

for (B, C) in SHAPES:
    x = torch.randn(B, C, device=dev) * 3
    t = torch.randint(0, C, (B,), device=dev)
    tab = torch.rand(C, device=dev) + 0.5
    acc = EvalAccumulator(C, topk=(1, 5), num_bins=10, table=tab, device=dev)
    edges = torch.linspace(0, 1, 11, device=dev, dtype=torch.float64)
    fused = timed(lambda: acc.update(x, t))

    def today():
        z = custom.scale_logits(x, tab)
        a1, a5 = utils.accuracy(z, t, topk=(1, 5))
        a1.item(), a5.item()
    now = wall(today)
    z = custom.scale_logits(x, tab)
    topk = timed(lambda: utils.topk_hit_counts(z, t, (1, 5)))

    def composed():
        zz = x * tab
        conf, pred = torch.softmax(zz, 1).max(1)
        b = torch.bucketize(conf.double(), edges, right=False) - 1
        hit = pred == t
        torch.bincount(b.clamp(0, 9), minlength=10), torch.bincount(b.clamp(0, 9)[hit], minlength=10)
        torch.bincount(t, minlength=C), torch.bincount(t[hit], minlength=C)
    comp = timed(composed)
    byt = B * C * 4
    print("B=%6d C=%5d  fused %8.2f us %7.1f GB/s (%4.1f %% of 8 TB/s) | topk_hits alone %8.2f us | today's path (scale + topk + "
          "2 x .item) %8.2f us | torch composition %8.2f us"
          % (B, C, fused, byt / fused / 1e3, byt / fused / 1e3 / 80, topk, now, comp))
