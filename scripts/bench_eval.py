"""Time of the evaluation forward (model.eval() under torch.no_grad(), the engine's run_forward as evaluate() /
per_shot_acc drive it) per batch, with device events around windows of --batches forwards after --warmup forwards.
--fused switches NativeResNet.set_fused_eval on (eval-mode BN folded into the convolution epilogues); without it the
script also runs on a tree that predates the switch, which is how the parent commit is measured next to this one.
Prints one JSON line.  Needs the MI355X.

    python scripts/bench_eval.py --model resnet50 --batch 256 --size 224 [--fused] [--batches 50] [--windows 2]

Launches and HBM bytes per batch come from rocprofv3 runs of this script (scripts/rocpd_stats.py, scripts/rocpd_hbm.py:
divide by "forwards"); bytes_from_shapes is the activation traffic the route needs by a count from shapes alone.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iif_amd import resnet_cifar, resnet_pytorch  # noqa: E402


def build(name, classes):
    if hasattr(resnet_pytorch, name):
        return getattr(resnet_pytorch, name)(num_classes=classes, use_norm="None", pretrained="None", compute_dtype=torch.bfloat16)
    return getattr(resnet_cifar, name)(num_classes=classes, use_norm="None", compute_dtype=torch.bfloat16)


def bytes_from_shapes(net, n, h, w, fused):
    """Activation bytes (bf16) one eval forward moves after the stem, counted from shapes: per unit the convolution reads
    its source and writes its output; unfused, bn_apply reads that output (+ the residual) and writes the activation;
    fused, the residual is read by the convolution's epilogue and nothing is re-read.  Weights and ReLU bits not counted."""
    from iif_amd import ops
    c1 = net.conv1
    hh, ww = ops.conv_out_hw(h, w, c1.k, c1.k, c1.stride, c1.pad)
    if net.style == "imagenet":
        hh, ww = (hh + 2 - 3) // 2 + 1, (ww + 2 - 3) // 2 + 1
    total = 0
    for st in net._stages:
        for blk in st:
            hi, wi = hh, ww
            pairs = blk.units()
            for ui, (cv, _) in enumerate(pairs):
                oh, ow = ops.conv_out_hw(hi, wi, cv.k, cv.k, cv.stride, cv.pad)
                src, dst = n * hi * wi * cv.cin * 2, n * oh * ow * cv.cout * 2
                closing = ui == len(pairs) - 1
                unit_fused = fused and not (closing and blk.se is not None)
                total += src + dst + (dst if closing else 0)                # convolution (+ residual read somewhere)
                if not unit_fused:
                    total += 2 * dst                                         # bn_apply / se_apply: read raw, write activation
                hi, wi = oh, ow
            if blk.downsample is not None:
                dcv = blk.downsample[0]
                total += n * hh * ww * dcv.cin * 2 + n * hi * wi * dcv.cout * 2
            hh, ww = hi, wi
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--batches", type=int, default=50, help="forwards per timed window")
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval needs an MI355X: the native engine has no CPU path")
    torch.manual_seed(0)
    net = build(a.model, a.classes)
    if a.fused:
        net.set_fused_eval(True)
    net.eval()
    x = torch.randn(a.batch, 3, a.size, a.size, device="cuda")
    with torch.no_grad():
        for _ in range(a.warmup):
            net.run_forward(x, False)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.batches):
                net.run_forward(x, False)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / a.batches)
    best = min(ms)
    out = {"bench": "eval_forward", "tag": a.tag, "model": a.model, "batch": a.batch, "size": a.size,
           "route": "fused" if a.fused else "default", "ms_per_batch": round(best, 4), "images_per_s": round(a.batch / best * 1e3, 1),
           "windows_ms": [round(v, 4) for v in ms], "batches_per_window": a.batches,
           "forwards": a.warmup + a.windows * a.batches,
           "gb_from_shapes": round(bytes_from_shapes(net, a.batch, a.size, a.size, a.fused) / 1e9, 3)}
    if a.fused:
        route = net.eval_route(a.batch, a.size, a.size)
        out["fused_units"] = sum(r == "fused" for _, r in route)
        out["units"] = len(route)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
