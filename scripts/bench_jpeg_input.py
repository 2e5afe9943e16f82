"""Device JPEG decoding (--device-decode) on one MI355X, on seeded photo-like JPEG sources (tests/jpeg_ref.photo: smooth
shading, hard-edged shapes, mild texture).  Needs PIL to write the sources (in a temporary directory); each mode prints
JSON lines, collected in profiles/jpeg_input_rates.txt.

    python scripts/bench_jpeg_input.py pil                   # PIL decode rate on one core, and the sources' bytes per pixel
    python scripts/bench_jpeg_input.py worker                # worker time per image: read + parse + pack against a PIL decode
    python scripts/bench_jpeg_input.py kernel [--iters 50]   # iif_jpeg_decode at B = 256, training boxes (device-event
                                                             # times): 375x500 q90 4:2:0 sources, the same with a restart
                                                             # marker every MCU row, and 1200x900 sources
    rocprofv3 --kernel-trace --stats -d out -o jpeg -- python scripts/bench_jpeg_input.py kernel
    python scripts/bench_jpeg_input.py stats out/jpeg_results.db   # per-case kernel times of that trace
    python scripts/bench_jpeg_input.py loader [--batches 48] [--workers 16]   # DeviceLTLoader img/s, host against device decode
    python scripts/bench_jpeg_input.py train [--steps 60] [--paths host|device]  # ResNet50 bs 128 training img/s (the
                                                             # protocol of scripts/bench_lt_input.py train)
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

B = 256
CASES = ("375x500 q90 4:2:0", "375x500 q90 4:2:0 rst/row", "1200x900 q90 4:2:0")


def _source(h, w, seed, quality=90, subsampling=2, **opts):
    from tests.jpeg_ref import encode, photo
    return encode(photo(h, w, seed), quality=quality, subsampling=subsampling, **opts)


def _sources(shape, n, seed, **opts):
    return [_source(shape[0], shape[1], seed + k, **opts) for k in range(n)]


def bench_pil(n=200):
    from PIL import Image
    datas = _sources((375, 500), 16, 0)
    bpp = float(np.mean([len(d) for d in datas])) / (375 * 500)
    t0 = time.perf_counter()
    for k in range(n):
        Image.open(io.BytesIO(datas[k % len(datas)])).convert("RGB").load()
    print(json.dumps({"case": "pil", "size": "375x500", "quality": 90, "sampling": "4:2:0", "bytes_per_pixel": round(bpp, 3),
                      "img_per_s_one_core": round(n / (time.perf_counter() - t0), 1)}), flush=True)


def bench_worker(n=256):
    """Per image, in one process: what a --device-decode worker does (read the bytes, parse, draw, pack) against what a
    host-decode worker does with the same file (PIL decode, draw and cut the box, pack)."""
    from iif_amd import jpeg, lt_device
    from iif_amd.imbalanced_dataset import _default_loader
    with tempfile.TemporaryDirectory() as root:
        paths = []
        for k, d in enumerate(_sources((375, 500), 32, 100)):
            p = os.path.join(root, "%d.jpg" % k)
            with open(p, "wb") as f:
                f.write(d)
            paths.append(p)
        cj = lt_device.augment.ColorJitter(0.4, 0.4, 0.4, 0.0)
        for label in ("device decode: read + parse + pack", "host decode: PIL + cut + pack"):
            t0 = time.perf_counter()
            samples = []
            for k in range(n):
                u = lt_device.uniforms(0, 0, 0, k)
                if label.startswith("device"):
                    with open(paths[k % len(paths)], "rb") as f:
                        data = f.read()
                    samples.append(lt_device.train_job(data, jpeg.parse(data), 224, u, cj) + (0,))
                else:
                    samples.append(lt_device.train_sample(_default_loader(paths[k % len(paths)]), 224, u, cj) + (0,))
            buf = lt_device.pack_decode(samples) if label.startswith("device") else lt_device.pack(samples)
            dt = time.perf_counter() - t0
            print(json.dumps({"case": "worker", "path": label, "images": n, "us_per_image": round(dt * 1e6 / n, 1),
                              "upload_bytes_per_batch_of_256": int(buf.numel() * 256 // n)}), flush=True)


def _jobs(shape, seed, **opts):
    from iif_amd import jpeg, lt_device
    datas = _sources(shape, 32, seed, **opts)
    jobs = []
    for k in range(B):
        d = datas[k % len(datas)]
        hd = jpeg.parse(d)
        (top, left, ch, cw), _, _, _ = lt_device.draw(hd.h, hd.w, lt_device.uniforms(seed, 0, 0, k))
        jobs.append(jpeg.Job(d, hd, (top, left, ch, cw)))
    return jobs


def bench_kernel(iters):
    from iif_amd import jpeg
    for label, shape, opts in zip(CASES, ((375, 500), (375, 500), (900, 1200)), ({}, {"restart_marker_rows": 1}, {})):
        jobs = _jobs(shape, 7, **opts)
        sec, _, outs, out_bytes, scr_bytes = jpeg.layout(jobs, 0)
        data = torch.from_numpy(sec).cuda()
        rec = data[:B * jpeg.REC_WORDS * 8].view(torch.int64).view(B, jpeg.REC_WORDS)
        out = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(scr_bytes, dtype=torch.uint8, device="cuda")
        status = torch.empty(B, dtype=torch.int32, device="cuda")
        for _ in range(5):
            jpeg.launch(data, rec, B, scratch, out, status)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            jpeg.launch(data, rec, B, scratch, out, status)
        e1.record()
        torch.cuda.synchronize()
        scan = sum(len(j.data) - j.hd.scan_off for j in jobs)
        print(json.dumps({"case": label, "B": B, "us_per_batch_events": round(e0.elapsed_time(e1) * 1e3 / iters, 1),
                          "jpeg_bytes": scan, "region_bytes": int(out_bytes), "upload_bytes": int(sec.nbytes)}), flush=True)


def kernel_stats(db_path, iters=50, warm=5):
    """The trace of ``kernel`` split into its cases: per batch, the two launches of iif_jpeg_decode."""
    import sqlite3
    import statistics
    con = sqlite3.connect(db_path)
    rows = con.execute("select name, end - start from kernels where name like '%jpeg%' order by start").fetchall()
    per = 2 * (warm + iters)
    for i, label in enumerate(CASES):
        part = rows[i * per:(i + 1) * per][2 * warm:]
        scan = [d / 1e3 for n, d in part if "scan" in n]
        pix = [d / 1e3 for n, d in part if "pixel" in n]
        tot = [a + b for a, b in zip(scan, pix)]
        print("%-20s %d batches  median %.1f us (entropy + IDCT %.1f, pixels %.1f)  min %.1f  max %.1f"
              % (label, len(tot), statistics.median(tot), statistics.median(scan), statistics.median(pix), min(tot), max(tot)))


def _tree(root, n, files=256):
    """root/img/<i>.jpg (``files`` photo-like JPEGs of ImageNet-like sizes, q90 4:2:0) and train.txt / eval.txt of ``n``
    lines cycling through them, with a long-tailed label profile (scripts/bench_lt_input.py _tree's)."""
    from bench_lt_input import _image_shapes
    from iif_amd.imbalanced_dataset import lt_profile
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    for i, (h, w) in enumerate(_image_shapes(files, 0)):
        with open(os.path.join(root, "img", "%d.jpg" % i), "wb") as f:
            f.write(_source(h, w, 2000 + i))
    counts = lt_profile(365, max(n // 365 * 4, 2))
    labels = np.repeat(np.arange(365), counts)[:n]
    labels = np.concatenate([labels, np.arange(n - len(labels)) % 365]) if len(labels) < n else labels
    lines = ["img/%d.jpg %d" % (i % files, labels[i]) for i in range(n)]
    for name in ("train.txt", "eval.txt"):
        with open(os.path.join(root, name), "w") as f:
            f.write("\n".join(lines) + "\n")


PATHS = (("host decode (PIL in the workers)", ["--device-augment"]),
         ("device decode", ["--device-augment", "--device-decode"]))


def bench_loader(batches, workers):
    from iif_amd import initialisers, train
    warm = workers * 2 + 4
    with tempfile.TemporaryDirectory() as root:
        _tree(root, B * (warm + batches + 2))
        for name, extra in PATHS:
            args = train.get_args_parser().parse_args(["--dset_name", "places_lt", "--data-path", root, "--train-txt",
                                                       os.path.join(root, "train.txt"), "--eval-txt",
                                                       os.path.join(root, "eval.txt"), "-b", str(B), "-j", str(workers)] + extra)
            args.distributed = False
            _, _, loader, _, _ = initialisers.get_data(args)
            it = iter(loader)
            for _ in range(warm):
                next(it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(batches):
                next(it)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"case": "loader", "input": name, "workers": workers, "batch": B, "untimed_batches": warm,
                              "timed_batches": batches, "img_per_s": round(batches * B / dt, 1)}), flush=True)
            del it


def bench_train(steps, paths, workers, skip=40):
    from bench_lt_input import _Timed
    from iif_amd import initialisers, train
    bs = 128
    with tempfile.TemporaryDirectory() as root:
        _tree(root, bs * (skip + steps + 8))
        for name, extra in [c for c in PATHS if c[0].split()[0] in paths]:
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
            print(json.dumps({"case": "train", "model": "resnet50", "input": name, "workers": workers, "untimed_steps": skip,
                              "timed_steps": steps, "batch": bs, "img_per_s": round(steps * bs / dt, 1),
                              "ms_per_step": round(dt * 1e3 / steps, 2)}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "stats":
        kernel_stats(sys.argv[2])
        raise SystemExit(0)
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["pil", "worker", "kernel", "loader", "train"])
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--batches", type=int, default=48)
    p.add_argument("--steps", type=int, default=60)
    p.add_argument("--paths", default="host,device", help="train: which input paths, in this order, in one process")
    p.add_argument("--workers", type=int, default=16)
    a = p.parse_args()
    if a.mode in ("pil", "worker"):
        {"pil": bench_pil, "worker": bench_worker}[a.mode]()
        raise SystemExit(0)
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_input.py needs the MI355X")
    {"kernel": lambda: bench_kernel(a.iters), "loader": lambda: bench_loader(a.batches, a.workers),
     "train": lambda: bench_train(a.steps, a.paths.split(","), a.workers)}[a.mode]()
