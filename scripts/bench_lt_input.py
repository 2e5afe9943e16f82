"""List-dataset (ImageNet-LT / Places-LT / iNat18) input pipeline on one MI355X.

    python scripts/bench_lt_input.py kernel [--iters 100]    # iif_lt_augment at B = 256, S = 224: train without hue, train
                                                             # with hue, eval, and a 1200 x 900 large-image train case; then
                                                             # iif_lt_augment_policy with the imagenet and randaugment draws
    rocprofv3 --kernel-trace --stats -d out -o lt -- python scripts/bench_lt_input.py kernel
    python scripts/bench_lt_input.py stats out/lt_results.db # per-case kernel times from that trace
    python scripts/bench_lt_input.py loader [--batches 64] [--workers 16]
                                                             # steady-state loader img/s over pre-decoded .npy files, no
                                                             # model: TensorTransform in the DataLoader against DeviceLTLoader
                                                             # (--policy imagenet|randaugment: with that auto-augment policy,
                                                             # on the device through --device-policy)
    python scripts/bench_lt_input.py train [--steps 60] [--paths host|device] [--workers 16]
                                                             # ResNet50 training img/s on a Places-LT-shaped .npy tree, timed
                                                             # after the epoch's first 40 steps (one path per process;
                                                             # --policy as for loader)
    python scripts/bench_lt_input.py jpeg                    # PIL JPEG decode rate, when PIL imports

Sources are seeded synthetic uint8 images of ImageNet-like sizes (short side 256-500); training regions are the
RandomResizedCrop boxes the loader itself draws.  ``kernel`` also prints the bytes each launch must move (regions read,
fp32 batch written) and the rate at the device-event time; the trace gives the kernel time itself.
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

B, S = 256, 224
CASES = ("train, no hue", "train, hue (iNat18)", "eval", "train, 1200x900 sources", "train, imagenet policy",
         "train, randaugment")


def _image_shapes(n, seed):
    rng = np.random.RandomState(seed)
    short = rng.randint(256, 501, size=n)
    long_ = (short * rng.uniform(1.0, 1.5, size=n)).astype(int)
    port = rng.rand(n) < 0.3
    return [(int(l), int(s)) if p else (int(s), int(l)) for s, l, p in zip(short, long_, port)]


def _batch(shapes, train, dset, seed, policy=None):
    from iif_amd import augment, lt_device
    from iif_amd.imbalanced_dataset import mean_std_hue
    cj = augment.ColorJitter(0.4, 0.4, 0.4, mean_std_hue(dset)[2]) if (train and policy is None) else None
    base = np.random.RandomState(seed).randint(0, 256, size=(1300, 1300, 3), dtype=np.uint8)
    samples = []
    for pos, (h, w) in enumerate(shapes):
        img = base[pos % 50:pos % 50 + h, pos % 97:pos % 97 + w]
        if policy is not None:
            s = lt_device.train_sample(img, S, lt_device.uniforms(seed, 0, 0, pos))
            ops = lt_device.draw_policy(policy, lt_device.policy_uniforms(seed, 0, 0, pos))
            s = s + (0, lt_device.policy_record(ops, S))
        elif train:
            s = lt_device.train_sample(img, S, lt_device.uniforms(seed, 0, 0, pos), cj)
        else:
            s = lt_device.eval_sample(img, S)
        samples.append(s if policy is not None else s + (0,))
    return lt_device.pack(samples), sum(s[0].nbytes for s in samples)


def bench_kernel(iters):
    from iif_amd import lt_device
    from iif_amd.imbalanced_dataset import mean_std_hue
    cases = [("imagenet_lt", True, _image_shapes(B, 1)), ("inat18", True, _image_shapes(B, 2)),
             ("imagenet_lt", False, _image_shapes(B, 3)), ("imagenet_lt", True, [(900, 1200)] * B)]
    for label, (dset, train, shapes) in zip(CASES, cases):
        buf, region_bytes = _batch(shapes, train, dset, 7)
        dev = buf.cuda()
        pool, desc, jit, _ = lt_device.unpack(dev, B)
        mean, std, _ = mean_std_hue(dset)
        flags = lt_device.JITTER if train else 0
        out = torch.empty(B, 3, S, S, device="cuda")
        for _ in range(10):
            lt_device.lt_augment(pool, desc, jit if train else None, S, mean, std, flags, out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            lt_device.lt_augment(pool, desc, jit if train else None, S, mean, std, flags, out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / iters
        moved = region_bytes + B * 3 * S * S * 4
        print(json.dumps({"case": label, "B": B, "S": S, "us_per_call_events": round(us, 1), "region_bytes": region_bytes,
                          "bytes": moved, "GB_per_s_at_event_time": round(moved / us / 1e3, 1)}), flush=True)
    for label, policy in zip(CASES[4:], ("imagenet", "randaugment")):
        buf, region_bytes = _batch(_image_shapes(B, 1), True, "imagenet_lt", 7, policy)
        pool, desc, _, _, ops = lt_device.unpack(buf.cuda(), B, policy=True)
        mean, std, _ = mean_std_hue("imagenet_lt")
        out, work = torch.empty(B, 3, S, S, device="cuda"), torch.empty(B, 3, S, S, device="cuda")
        for _ in range(10):
            lt_device.lt_augment_policy(pool, desc, ops, S, mean, std, work, out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            lt_device.lt_augment_policy(pool, desc, ops, S, mean, std, work, out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / iters
        codes = ops[:, :, 0].cpu().numpy()
        swept = [lt_device.OPS.index(n) for n in lt_device.SWEEP_OPS]           # each one adds a sweep over its image
        print(json.dumps({"case": label, "B": B, "S": S, "us_per_call_events": round(us, 1), "region_bytes": region_bytes,
                          "applied_ops": int((codes != lt_device.OP_NONE).sum()),
                          "extra_sweeps": int(np.isin(codes, swept).sum())}), flush=True)


def kernel_stats(db_path, iters=100, warm=10):
    """The trace of ``kernel`` split into its cases (launch order: ``warm`` + ``iters`` launches per case)."""
    import sqlite3
    import statistics
    rows = sqlite3.connect(db_path).execute("select end - start from kernels where name like '%lt_augment%' "
                                            "or name like '%lt_policy%' order by start").fetchall()
    for i, label in enumerate(CASES):
        us = [d / 1e3 for (d,) in rows[i * (warm + iters) + warm:(i + 1) * (warm + iters)]]
        print("%-26s %d calls  median %.1f us  min %.1f  max %.1f" % (label, len(us), statistics.median(us), min(us), max(us)))


def _tree(root, n, classes, files=512, seed=0):
    """root/img/<i>.npy (``files`` arrays of ImageNet-like sizes) and root/train.txt, root/eval.txt of ``n`` lines cycling
    through them, with a long-tailed label profile."""
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    from iif_amd.imbalanced_dataset import lt_profile
    counts = lt_profile(classes, max(n // classes * 4, 2))
    labels = np.repeat(np.arange(classes), counts)[:n]
    labels = np.concatenate([labels, np.arange(n - len(labels)) % classes]) if len(labels) < n else labels
    for i, (h, w) in enumerate(_image_shapes(files, seed)):
        np.save(os.path.join(root, "img", "%d.npy" % i), np.random.RandomState(i).randint(0, 256, size=(h, w, 3), dtype=np.uint8))
    lines = ["img/%d.npy %d" % (i % files, labels[i]) for i in range(n)]
    for name in ("train.txt", "eval.txt"):
        with open(os.path.join(root, name), "w") as f:
            f.write("\n".join(lines) + "\n")


def _paths(policy):
    """(name, extra CLI flags) of the host and the device input path, with --auto-augment ``policy`` when given."""
    if policy is None:
        return (("host TensorTransform", []), ("device DeviceLTLoader", ["--device-augment"]))
    aa = ["--auto-augment", policy]
    return (("host TensorTransform", aa), ("device DeviceLTLoader", ["--device-augment", "--device-policy"] + aa))


def bench_loader(batches, workers, policy=None):
    """Steady-state loader rate: the first workers * prefetch_factor (+ 4) batches, which the DataLoader dispatches at once
    and builds in parallel before the clock could start, are drained untimed; then ``batches`` batches are timed, each
    moved to the device."""
    from iif_amd import initialisers, train
    warm = workers * 2 + 4                                        # DataLoader's default prefetch_factor is 2
    with tempfile.TemporaryDirectory() as root:
        _tree(root, B * (warm + batches + 2), 365)
        for name, extra in _paths(policy):
            args = train.get_args_parser().parse_args(["--dset_name", "places_lt", "--data-path", root, "--train-txt",
                                                       os.path.join(root, "train.txt"), "--eval-txt",
                                                       os.path.join(root, "eval.txt"), "-b", str(B), "-j", str(workers)]
                                                      + extra)
            args.distributed = False
            _, _, loader, _, _ = initialisers.get_data(args)
            it = iter(loader)
            for _ in range(warm):
                x, _ = next(it)
                x = x.cuda(non_blocking=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(batches):
                x, _ = next(it)
                x = x.cuda(non_blocking=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"case": "loader", "input": name, "policy": policy, "workers": workers, "batch": B, "untimed_batches": warm,
                              "timed_batches": batches, "img_per_s": round(batches * B / dt, 1)}), flush=True)
            del it


class _Timed(object):
    """A loader that synchronises the device and stamps the clock when it hands out batch ``skip``, so that a training run
    can be timed from there to its end without the epoch's worker start-up and first prefetch round."""

    def __init__(self, loader, skip):
        self.loader, self.skip, self.t = loader, skip, None

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for k, batch in enumerate(self.loader):
            if k == self.skip:
                torch.cuda.synchronize()
                self.t = time.perf_counter()
            yield batch


def bench_train(steps, paths, workers, skip=40, policy=None):
    from iif_amd import initialisers, train
    bs = 128
    with tempfile.TemporaryDirectory() as root:
        _tree(root, bs * (skip + steps + 8), 365)
        for name, extra in [c for c in _paths(policy) if c[0].split()[0] in paths]:
            args = train.get_args_parser().parse_args(["--model", "resnet50", "--dset_name", "places_lt", "--data-path", root,
                                                       "--train-txt", os.path.join(root, "train.txt"), "--eval-txt",
                                                       os.path.join(root, "eval.txt"), "-b", str(bs), "-j", str(workers),
                                                       "--print-freq", "100000"] + extra)
            args.distributed = False
            _, C, loader, _, _ = initialisers.get_data(args)
            model = train.build_model(args, C)
            crit = initialisers.get_criterion(args, loader.dataset, model, C)
            args.max_iters = 4
            train.train_one_epoch(model, crit, loader, torch.device("cuda"), 0, args)           # warm-up
            torch.cuda.synchronize()
            timed = _Timed(loader, skip)
            args.max_iters = skip + steps
            train.train_one_epoch(model, crit, timed, torch.device("cuda"), 1, args)
            torch.cuda.synchronize()
            dt = time.perf_counter() - timed.t
            print(json.dumps({"case": "train", "model": "resnet50", "input": name, "policy": policy, "workers": workers, "untimed_steps": skip,
                              "timed_steps": steps, "batch": bs, "img_per_s": round(steps * bs / dt, 1),
                              "ms_per_step": round(dt * 1e3 / steps, 2)}), flush=True)


def bench_jpeg():
    try:
        from PIL import Image
    except Exception:
        print(json.dumps({"case": "jpeg", "result": "not measured: PIL does not import"}))
        return
    import io
    img = Image.fromarray(np.random.RandomState(0).randint(0, 256, size=(375, 500, 3), dtype=np.uint8))
    b = io.BytesIO()
    img.save(b, format="JPEG", quality=90)
    data = b.getvalue()
    t0, n = time.perf_counter(), 200
    for _ in range(n):
        Image.open(io.BytesIO(data)).convert("RGB").load()
    print(json.dumps({"case": "jpeg", "size": "375x500", "img_per_s_one_core": round(n / (time.perf_counter() - t0), 1)}))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "stats":
        kernel_stats(sys.argv[2])
        raise SystemExit(0)
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernel", "loader", "train", "jpeg"])
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--batches", type=int, default=64)
    p.add_argument("--steps", type=int, default=60)
    p.add_argument("--paths", default="host,device", help="train: which input paths, in this order, in one process")
    p.add_argument("--workers", type=int, default=16)
    p.add_argument("--policy", default=None, choices=["imagenet", "randaugment"], help="loader / train: --auto-augment policy")
    a = p.parse_args()
    if a.mode == "jpeg":
        bench_jpeg()
        raise SystemExit(0)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lt_input.py needs the MI355X")
    {"kernel": lambda: bench_kernel(a.iters), "loader": lambda: bench_loader(a.batches, a.workers, a.policy),
     "train": lambda: bench_train(a.steps, a.paths.split(","), a.workers, policy=a.policy)}[a.mode]()
