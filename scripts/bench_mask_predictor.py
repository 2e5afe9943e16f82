#!/usr/bin/env python3
"""Measure the class-selected mask predictor (iif_amd/mmdet_mask_predictor.py) against the path the package offered before it,
``mask_cross_entropy(F.conv2d(x, w, b), t, labels)``, in one process; the output is profiles/mask_predictor.txt.

    python scripts/bench_mask_predictor.py [--out FILE] [--rounds 7] [--quick]

Method: results are compared first (loss and gradients of the two paths); every variant is warmed up; a round times `inner`
calls of each variant between two device events, the variants alternating inside a round; reported is the median over the
rounds [min .. max] per call.  Kernel times are the C entries called on their own against the bytes the algorithm must move (x
once per pass that reads it, dx once), timed twice: back to back as above - x (205 MB) then stays in the 256 MiB Infinity Cache
from call to call - and one call at a time behind a sweep that evicts it ("cold"): a READ of 1 GiB, which leaves clean lines, and
a FILL of 1 GiB, which leaves dirty lines that the kernel's misses have to write back first.  Peak memory is torch's
max_memory_allocated over one forward + backward, above what the inputs and parameters hold.  The error section runs the test cases of tests/mask_predictor_cases.py: the kernels' error
against the float64 restatement over the error of torch-CPU float32 conv2d + mask_cross_entropy against the same.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iif_amd import _lib                                                                  # noqa: E402
from iif_amd.mmdet_mask_loss import gather_class_masks, mask_cross_entropy               # noqa: E402
from iif_amd.mmdet_mask_predictor import class_mask_logits, class_mask_loss              # noqa: E402

DEV = "cuda:0"
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def make(n, c, cin=256, hw=28, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(n, cin, hw, hw, generator=g)).to(DEV)
    w = (torch.randn(c, cin, 1, 1, generator=g) * (8.0 / cin) ** 0.5).to(DEV)
    b = (torch.randn(c, generator=g) * 0.1).to(DEV)
    lb = torch.randint(0, c, (n,), generator=g).to(DEV)
    t = (torch.rand(n, hw, hw, generator=g) < 0.5).float().to(DEV)
    return x, w, b, lb, t


def timed(variants, rounds, inner):
    """{name: [ms per call, one per round]}; the variants alternate inside a round."""
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / inner)
    return out


def line(label, ms):
    return "    %-34s %9.1f us  [%9.1f .. %9.1f]" % (label, statistics.median(ms) * 1e3, min(ms) * 1e3, max(ms) * 1e3)


def cold(f, rounds, dirty):
    """ms of single calls, each behind a sweep over 1 GiB (larger than the last-level cache): a read, or (dirty) a fill."""
    junk = torch.ones(1 << 28, dtype=torch.float32, device=DEV)
    out = []
    for _ in range(rounds + 2):
        if dirty:
            junk.fill_(1.0)
        else:
            junk.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out[2:]


def peak(f, before_call=None):
    if before_call:
        before_call()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    f()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def train_shape(title, n, c, rounds, inner, kernels=False):
    x, w, b, lb, t = make(n, c)
    leaves = lambda: (x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True))   # noqa: E731

    def new(lv=None):
        xs, ws, bs = lv or (xg, wg, bg)
        xs.grad = ws.grad = bs.grad = None
        class_mask_loss(xs, ws, bs, lb, t).sum().backward()

    def old(lv=None):
        xs, ws, bs = lv or (xg, wg, bg)
        xs.grad = ws.grad = bs.grad = None
        mask_cross_entropy(F.conv2d(xs, ws, bs), t, lb).sum().backward()
    a, o = leaves(), leaves()
    new(a), old(o)
    with torch.no_grad():
        la = float(class_mask_loss(a[0], a[1], a[2], lb, t))
        lo = float(mask_cross_entropy(F.conv2d(o[0], o[1], o[2]), t, lb))
    rel = [float((p.grad - q.grad).abs().max() / q.grad.abs().max()) for p, q in zip(a, o)]
    agree = abs(la - lo) <= 2e-5 and max(rel) <= 2e-5
    say("%s: N = %d, C = %d, Cin = 256, 28 x 28; the two paths agree (loss %.1e, dx %.1e, dweight %.1e, dbias %.1e): %s"
        % (title, n, c, abs(la - lo), rel[0], rel[1], rel[2], agree))
    del a, o
    xg, wg, bg = leaves()
    r = timed({"new": new, "old": old}, rounds, inner)
    say(line("class_mask_loss fwd + bwd", r["new"]))
    say(line("conv2d + mask_cross_entropy", r["old"]))
    say("    class_mask_loss vs the full convolution: %.2fx its speed" % (statistics.median(r["old"]) / statistics.median(r["new"])))

    def drop():
        xg.grad = wg.grad = bg.grad = None
    say("    peak memory above the inputs and parameters, gradients included: class_mask_loss %.1f MB, full convolution %.1f MB"
        % (peak(new, drop), peak(old, drop)))
    drop()
    if kernels:
        kernel_times(x, w, b, lb, t, rounds, inner)
    return statistics.median(r["old"]) / statistics.median(r["new"]), agree


def kernel_times(x, w, b, lb, t, rounds, inner):
    n, cin, h, wd = x.shape
    c, hw = w.shape[0], h * wd
    L, st = _lib.lib(), _lib.stream_ptr()
    w2 = w.reshape(c, cin)
    g0 = torch.empty(n, hw, device=DEV)
    rows = torch.empty(n * ((hw + 63) // 64), device=DEV)
    loss, up = torch.empty(1, device=DEV), torch.ones(1, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    dx, scratch = torch.empty_like(x), torch.empty(n, cin + 1, device=DEV)
    dw, db = torch.empty(c, cin, device=DEV), torch.empty(c, device=DEV)
    p = _lib.ptr
    fwd = lambda: _lib.check(L.iif_mask_predict_fwd(p(x), 0, p(w2), cin, p(b), p(lb), p(t), n, c, cin, hw, 0, p(g0), p(rows), p(loss),     # noqa: E731
                                                    p(status), st), "fwd")
    dxk = lambda: _lib.check(L.iif_mask_predict_bwd_input(p(g0), p(up), p(w2), cin, p(lb), n, c, cin, hw, p(dx), 0, st), "dx")          # noqa: E731
    dwk = lambda: _lib.check(L.iif_mask_predict_bwd_weight(p(x), 0, p(g0), p(up), p(lb), n, c, cin, hw, p(scratch), p(dw), p(db), st),   # noqa: E731
                             "dw")
    r = timed({"fwd": fwd, "dx": dxk, "dw": dwk}, rounds, inner)
    xb = x.numel() * 4
    for k, f, label, nbytes in (("fwd", fwd, "iif_mask_predict_fwd (2 launches)", xb + 3 * n * hw * 4),
                                ("dx", dxk, "iif_mask_predict_bwd_input", xb + n * hw * 4),
                                ("dw", dwk, "iif_mask_predict_bwd_weight (2)", xb + n * hw * 4 + 2 * n * (cin + 1) * 4 + c * (cin + 1) * 4)):
        ms, mc, md = statistics.median(r[k]), statistics.median(cold(f, rounds, False)), statistics.median(cold(f, rounds, True))
        say("    %-33s %6.1f us for %6.2f MB that must move: %4.0f GB/s; cold behind a read %6.1f us: %4.0f GB/s, behind a fill %6.1f us: %4.0f GB/s"
            % (label, ms * 1e3, nbytes / 1e6, nbytes / ms / 1e6, mc * 1e3, nbytes / mc / 1e6, md * 1e3, nbytes / md / 1e6))


def test_shape(n, c, rounds, inner):
    x, w, b, lb, _ = make(n, c)
    with torch.no_grad():
        a, o = class_mask_logits(x, w, b, lb), gather_class_masks(F.conv2d(x, w, b), lb)
        err = float((a[:, 0] - o).abs().max())
        r = timed({"new": lambda: class_mask_logits(x, w, b, lb), "old": lambda: gather_class_masks(F.conv2d(x, w, b), lb)}, rounds, inner)
        say("test shape, forward only: N = %d, C = %d; largest difference of the selected logits %.1e" % (n, c, err))
        say(line("class_mask_logits", r["new"]))
        say(line("conv2d + gather_class_masks", r["old"]))
        say("    class_mask_logits vs the full convolution: %.2fx its speed; peak memory %.1f MB vs %.1f MB"
            % (statistics.median(r["old"]) / statistics.median(r["new"]), peak(lambda: class_mask_logits(x, w, b, lb)),
               peak(lambda: gather_class_masks(F.conv2d(x, w, b), lb))))


def error_ratios():
    from oracle import mmdet_iif as M
    from tests import mask_predictor_cases as mpc
    say("error against the float64 restatement, kernels / torch-CPU float32 reference (tests/mask_predictor_cases.py):")
    worst = 0.0
    for name in sorted(mpc.CASES):
        x, w, b, lb, t = mpc.inputs(name)
        c, cin = w.shape[:2]
        ref = mpc.reference64(name)
        rel = lambda d, k: float((d.double().reshape(ref[k].shape) - ref[k]).abs().max() / ref[k].abs().max())      # noqa: E731
        xs, ws = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        bs = None if b is None else b.clone().requires_grad_(True)
        M.mask_cross_entropy(F.conv2d(xs, ws, bs), t, lb).sum().backward()
        xd, wdv = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        bd = None if b is None else b.to(DEV).requires_grad_(True)
        class_mask_loss(xd, wdv, bd, lb.to(DEV), t.to(DEV)).sum().backward()
        parts = []
        for k, cpu, dev in (("dx", xs, xd), ("dweight", ws, wdv), ("dbias", bs, bd)):
            if cpu is None:
                continue
            e_ref, e_k = rel(cpu.grad, k), rel(dev.grad.cpu(), k)
            worst = max(worst, e_k / e_ref)
            parts.append("%s %.1e / %.1e = %.2f" % (k, e_k, e_ref, e_k / e_ref))
        say("    case %s  %s" % (name, "   ".join(parts)))
    say("    largest ratio: %.2f" % worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small N: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_predictor.py measures on the GPU; none found")
    n = 8 if a.quick else 256
    say("class-selected mask predictor, %s" % torch.cuda.get_device_name(0))
    inner = 20
    say("%d rounds, the variants alternating; per round %d calls between two device events; microseconds per call: median over the "
        "rounds [min .. max]" % (a.rounds, inner))
    ratio, agree = train_shape("LVIS training shape", n, 1203, a.rounds, inner, kernels=True)
    train_shape("COCO", n, 80, a.rounds, inner)
    train_shape("class-agnostic head", n, 1, a.rounds, inner)
    for nt in ((4, 6) if a.quick else (100, 300)):
        test_shape(nt, 1203, a.rounds, inner)
    error_ratios()
    say("required: at least 2x the speed of the full convolution end to end at the LVIS training shape: %s (%.2fx); results agree: %s"
        % ("MET" if ratio >= 2 else "NOT MET", ratio, agree))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
