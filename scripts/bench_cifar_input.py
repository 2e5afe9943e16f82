"""CIFAR input pipeline on one MI355X.

    python scripts/bench_cifar_input.py kernel [--iters 200]     # iif_cifar_augment at B = 128 / 512, CROP_FLIP and all stages
    python scripts/bench_cifar_input.py train [--steps 300]      # ResNet32 CIFAR100-LT bs 128 training img/s: the device
                                                                 # pipeline against the synthetic host DataLoader
    rocprofv3 --kernel-trace --stats -d out -o cifar -- python scripts/bench_cifar_input.py kernel
    python scripts/bench_cifar_input.py stats out/cifar_results.db   # per-case kernel times from that trace

``kernel`` prints one JSON line per case with the per-call time from device events over ``--iters`` back-to-back launches
(run it under ``rocprofv3 --kernel-trace --stats`` for the kernel time itself) and the bytes the call must move.
``train`` writes a fake full-size cifar-100-python tree (random pixels, 500 images per class) to a temporary directory and
times train.train_one_epoch over ``--steps`` iterations after a warm-up epoch, both input paths in the same process.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench_kernel(iters):
    from iif_amd import cifar
    n = 10847                                                 # CIFAR100-LT at imb 0.01
    rng = np.random.RandomState(0)
    data = torch.from_numpy(rng.randint(0, 256, size=(n, 3072)).astype(np.uint8)).cuda()
    labels = torch.from_numpy(rng.randint(0, 100, size=n)).cuda()
    idx = torch.from_numpy(rng.permutation(n)).cuda()
    pol = cifar.device_policy(None, "cuda")
    for B in (128, 512):
        for name, flags in (("crop_flip", cifar.CROP_FLIP), ("all", cifar.CROP_FLIP | cifar.POLICY | cifar.CUTOUT)):
            ix = idx[:B]
            for _ in range(10):
                cifar.augment_batch(data, labels, ix, flags, 0, 0, 0, 0, pol)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                cifar.augment_batch(data, labels, ix, flags, 0, 0, 0, i * B, pol)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / iters
            moved = B * (3072 + 3072 * 4 + 8 + 8)             # uint8 image in, fp32 image out, index, target
            print(json.dumps({"case": "kernel", "B": B, "stages": name, "us_per_call_events": round(us, 2),
                              "bytes": moved, "GB_per_s_at_event_time": round(moved / us / 1e3, 1)}), flush=True)


def bench_train(steps):
    from iif_amd import initialisers, train
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from cifar_cases import write_fake_cifar
    with tempfile.TemporaryDirectory() as root:
        write_fake_cifar(root, "cifar100", 500, 100, seed=1)
        for name, extra in (("device_pipeline", ["--data-path", root]),
                            ("device_pipeline_autoaugment", ["--data-path", root, "--auto-augment", "cifar"]),
                            ("synthetic_host_loader", ["-j", "4"])):
            args = train.get_args_parser().parse_args(["--model", "resnet32", "--dset_name", "cifar100", "--classif", "iif",
                                                       "-b", "128", "--print-freq", "100000", "--imb_factor", "0.01"] + extra)
            args.distributed = False
            _, C, loader, _, _ = initialisers.get_data(args)
            model = train.build_model(args, C)
            crit = initialisers.get_criterion(args, loader.dataset, model, C)
            args.max_iters = 20
            train.train_one_epoch(model, crit, loader, torch.device("cuda"), 0, args)           # warm-up
            torch.cuda.synchronize()
            args.max_iters = min(steps, len(loader))
            t0 = time.perf_counter()
            train.train_one_epoch(model, crit, loader, torch.device("cuda"), 1, args)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"case": "train", "input": name, "iters": args.max_iters, "batch": 128,
                              "img_per_s": round(args.max_iters * 128 / dt, 1), "ms_per_step": round(dt * 1e3 / args.max_iters, 3)}),
                  flush=True)


CASES = ("B=128 CROP_FLIP", "B=128 CROP_FLIP|POLICY|CUTOUT", "B=512 CROP_FLIP", "B=512 CROP_FLIP|POLICY|CUTOUT")


def kernel_stats(db_path, iters=200, warm=10):
    """The trace of ``kernel`` split into its four cases (launch order: ``warm`` + ``iters`` launches per case)."""
    import sqlite3
    import statistics
    rows = sqlite3.connect(db_path).execute("select grid_x / workgroup_x, end - start from kernels where name like "
                                            "'%cifar_augment%' order by start").fetchall()
    for i, label in enumerate(CASES):
        seg = rows[i * (warm + iters) + warm:(i + 1) * (warm + iters)]
        us = [d / 1e3 for _, d in seg]
        B, med = seg[0][0], statistics.median(us)
        moved = B * (3072 + 3072 * 4 + 8 + 8)
        print("%-30s %4d blocks  %d calls  median %.2f us  min %.2f  max %.2f  (%.0f GB/s over %d B)" % (
            label, B, len(us), med, min(us), max(us), moved / med / 1e3, moved))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "stats":
        kernel_stats(sys.argv[2])
        raise SystemExit(0)
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernel", "train"])
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--steps", type=int, default=300)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cifar_input.py needs the MI355X")
    bench_kernel(a.iters) if a.mode == "kernel" else bench_train(a.steps)
