"""HBM rate of the fused RMSprop step (iif_rmsprop_step) over the ResNet-50 parameter arena, next to the fused SGD step.
Algorithmic bytes: p, g, square_avg read and p, square_avg written (20 B per parameter), + 8 B for the momentum buffer,
+ 8 B for grad_avg when centered; SGD: p, g, buf read and p, buf written (20 B).  HIP-event time over ``reps`` launches.
Prints one line per variant.  Needs the MI355X; kernel-only times come from running it under
``rocprofv3 --kernel-trace --stats -- python scripts/bench_rmsprop.py``.

    python scripts/bench_rmsprop.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iif_amd import ops, resnet_pytorch  # noqa: E402

dev = "cuda:0"


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


net = resnet_pytorch.resnet50(num_classes=1000, pretrained="None", device=dev)
n = net.param_arena.numel()
g = torch.Generator(device=dev).manual_seed(0)
p = net.param_arena.detach().clone()
grad = torch.randn(n, device=dev, generator=g) * 1e-3
sq, buf, ga = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
print("ResNet-50 arena: %d floats" % n)
for momentum, centered in ((0.9, False), (0.0, False), (0.0, True), (0.9, True)):
    nbytes = n * (20 + (8 if momentum > 0 else 0) + (8 if centered else 0))
    ms = timed(lambda: ops.rmsprop_step(p, grad, sq, 1e-4, 0.9, 0.0316, 1e-4, momentum, momentum_buf=buf,
                                        grad_avg=ga if centered else None))
    print("rmsprop momentum=%.1f centered=%d  %2d B/param  %8.1f us  %.2f TB/s"
          % (momentum, centered, nbytes // n, ms * 1e3, nbytes / (ms * 1e-3) / 1e12))
ms = timed(lambda: ops.sgd_step(p, grad, buf, 1e-4, 0.9, 1e-4))
print("sgd     momentum=0.9             20 B/param  %8.1f us  %.2f TB/s" % (ms * 1e3, n * 20 / (ms * 1e-3) / 1e12))
