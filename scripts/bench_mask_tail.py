#!/usr/bin/env python3
"""Measure the fused mask head tail (iif_amd/mmdet_mask_tail.py) against the composed path the package offered before it,
``class_mask_loss(relu(conv_transpose2d(f, up_weight, up_bias, stride=2)), weight, bias, labels, targets)``, in one process; the
output is profiles/mask_tail.txt.

    python scripts/bench_mask_tail.py [--out FILE] [--rounds 7] [--quick]

Method: results are compared first (loss and the five gradients of the two paths); every variant is warmed up; a round times
`inner` calls of each variant between two device events, the variants alternating inside a round; reported is the median over
the rounds [min .. max] per call.  Kernel times are the C entries called on their own, with the MFMA rate of the GEMM each one
contains (2 * N * hw * Ci * 4 Co flop).  Peak memory is torch's max_memory_allocated over one forward + backward, above what the
inputs and parameters hold, gradients included.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iif_amd import _lib                                                                          # noqa: E402
from iif_amd.mmdet_mask_predictor import class_mask_logits, class_mask_loss                       # noqa: E402
from iif_amd.mmdet_mask_tail import upsampled_class_mask_logits, upsampled_class_mask_loss        # noqa: E402

DEV = "cuda:0"
LINES = []
NAMES = ("df", "dup_weight", "dup_bias", "dweight", "dbias")


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def make(n, c, ci=256, co=256, hw=14, seed=0):
    g = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(n, ci, hw, hw, generator=g)).to(DEV)
    uw = (torch.randn(ci, co, 2, 2, generator=g) * (2.0 / ci) ** 0.5).to(DEV)
    ub = (torch.randn(co, generator=g) * 0.1).to(DEV)
    w = (torch.randn(c, co, 1, 1, generator=g) * (8.0 / co) ** 0.5).to(DEV)
    b = (torch.randn(c, generator=g) * 0.1).to(DEV)
    lb = torch.randint(0, c, (n,), generator=g).to(DEV)
    t = (torch.rand(n, 2 * hw, 2 * hw, generator=g) < 0.5).float().to(DEV)
    return f, uw, ub, w, b, lb, t


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
    return "    %-44s %9.1f us  [%9.1f .. %9.1f]" % (label, statistics.median(ms) * 1e3, min(ms) * 1e3, max(ms) * 1e3)


def peak(f, before_call):
    before_call()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    f()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def composed_loss(f, uw, ub, w, b, lb, t):
    return class_mask_loss(torch.relu_(F.conv_transpose2d(f, uw, ub, stride=2)), w, b, lb, t)


def train_shape(title, n, c, rounds, inner, kernels=False):
    f, uw, ub, w, b, lb, t = make(n, c)
    leaves = lambda: [x.clone().requires_grad_(True) for x in (f, uw, ub, w, b)]       # noqa: E731

    def run(fn, lv):
        for x in lv:
            x.grad = None
        fn(*lv, lb, t).sum().backward()
    a, o = leaves(), leaves()
    run(upsampled_class_mask_loss, a), run(composed_loss, o)
    with torch.no_grad():
        la, lo = float(upsampled_class_mask_loss(*a, lb, t)), float(composed_loss(*o, lb, t))
    rel = [float((p.grad - q.grad).abs().max() / q.grad.abs().max()) for p, q in zip(a, o)]
    agree = abs(la - lo) <= 2e-5 and max(rel) <= 2e-5
    say("%s: N = %d, C = %d, 256 -> 256 channels, 14 x 14 -> 28 x 28; the two paths agree (loss %.1e, %s): %s"
        % (title, n, c, abs(la - lo), ", ".join("%s %.1e" % kv for kv in zip(NAMES, rel)), agree))
    del a, o
    lv = leaves()
    r = timed({"new": lambda: run(upsampled_class_mask_loss, lv), "old": lambda: run(composed_loss, lv)}, rounds, inner)
    say(line("upsampled_class_mask_loss fwd + bwd", r["new"]))
    say(line("conv_transpose2d + relu + class_mask_loss", r["old"]))
    ratio = statistics.median(r["old"]) / statistics.median(r["new"])
    say("    fused vs composed: %.2fx its speed" % ratio)

    def drop():
        for x in lv:
            x.grad = None
    pn, po = peak(lambda: run(upsampled_class_mask_loss, lv), drop), peak(lambda: run(composed_loss, lv), drop)
    say("    peak memory above the inputs and parameters, gradients included: fused %.1f MB, composed %.1f MB (%.1f MB less)"
        % (pn, po, po - pn))
    drop()
    if kernels:
        kernel_times(f, uw, ub, w, b, lb, t, rounds, inner)
    return ratio, agree, po - pn


def kernel_times(f, uw, ub, w, b, lb, t, rounds, inner):
    n, ci, h, wd = f.shape
    co, c, hw = uw.shape[1], w.shape[0], h * wd
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    w2 = w.reshape(c, co)
    g0 = torch.empty(n, 4 * hw, device=DEV)
    rl = torch.empty(n * ((hw + 63) // 64), device=DEV)
    loss, up = torch.empty(1, device=DEV), torch.ones(1, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    signs = torch.empty(n * ((hw + 31) // 32) * 4 * co, dtype=torch.int32, device=DEV)
    rows = torch.empty(n, co + 1, device=DEV)
    df = torch.empty_like(f)
    splits = L.iif_mask_tail_splits(n, ci, co)
    partial = torch.empty(splits * (ci + 1) * 4 * co, device=DEV)
    duw, dub, dw, db = torch.empty_like(uw), torch.empty_like(ub), torch.empty(c, co, device=DEV), torch.empty(c, device=DEV)
    ks = {
        "iif_mask_tail_fwd (2 launches)": lambda: _lib.check(L.iif_mask_tail_fwd(
            p(f), 0, p(uw), p(ub), p(w2), co, p(b), p(lb), p(t), n, c, ci, co, h, wd, 0, p(g0), p(rl), p(loss), p(status), st), "fwd"),
        "iif_mask_tail_bwd_rows": lambda: _lib.check(L.iif_mask_tail_bwd_rows(
            p(f), 0, p(uw), p(ub), p(g0), p(up), p(lb), n, c, ci, co, h, wd, p(signs), p(rows), st), "rows"),
        "iif_mask_tail_bwd_input": lambda: _lib.check(L.iif_mask_tail_bwd_input(
            p(g0), p(up), p(uw), p(w2), co, p(lb), p(signs), n, c, ci, co, h, wd, p(df), 0, st), "df"),
        "iif_mask_tail_bwd_params (2, %d ranges)" % splits: lambda: _lib.check(L.iif_mask_tail_bwd_params(
            p(f), 0, p(g0), p(up), p(w2), co, p(lb), p(signs), n, c, ci, co, h, wd, p(partial), p(duw), p(dub), st), "dup"),
        "iif_mask_tail_bwd_classes": lambda: _lib.check(L.iif_mask_tail_bwd_classes(p(rows), p(lb), n, c, co, p(dw), p(db), st), "cls"),
    }
    r = timed(ks, rounds, inner)
    flop = 2.0 * n * hw * ci * 4 * co
    total = 0.0
    for k in ks:
        ms = statistics.median(r[k])
        total += ms
        rate = "" if k.endswith("classes") else "  %5.1f TF of the %.1f GFLOP GEMM inside" % (flop / ms / 1e9, flop / 1e9)
        say("    %-40s %8.1f us%s" % (k, ms * 1e3, rate))
    say("    sum of the kernels %.1f us" % (total * 1e3))


def test_shape(n, c, rounds, inner):
    f, uw, ub, w, b, lb, _ = make(n, c)
    composed = lambda: class_mask_logits(torch.relu_(F.conv_transpose2d(f, uw, ub, stride=2)), w, b, lb)      # noqa: E731
    fused = lambda: upsampled_class_mask_logits(f, uw, ub, w, b, lb)                                         # noqa: E731
    with torch.no_grad():
        err = float((fused() - composed()).abs().max())
        r = timed({"new": fused, "old": composed}, rounds, inner)
        say("test end, forward only: N = %d, C = %d; largest difference of the logits %.1e" % (n, c, err))
        say(line("upsampled_class_mask_logits", r["new"]))
        say(line("conv_transpose2d + relu + class_mask_logits", r["old"]))
        say("    fused vs composed: %.2fx its speed; peak memory %.1f MB vs %.1f MB"
            % (statistics.median(r["old"]) / statistics.median(r["new"]), peak(fused, lambda: None), peak(composed, lambda: None)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small N: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_tail.py measures on the GPU; none found")
    n = 8 if a.quick else 256
    say("fused mask head tail, %s" % torch.cuda.get_device_name(0))
    inner = 10
    say("%d rounds, the variants alternating; per round %d calls between two device events; microseconds per call: median over the "
        "rounds [min .. max]" % (a.rounds, inner))
    ratio, agree, saved = train_shape("LVIS training shape", n, 1203, a.rounds, inner, kernels=True)
    train_shape("COCO", n, 80, a.rounds, inner)
    train_shape("class-agnostic head", n, 1, a.rounds, inner)
    for nt in ((4, 6) if a.quick else (100, 300)):
        test_shape(nt, 1203, a.rounds, inner)
    say("aim: no slower than the composed path at the LVIS training shape: %s (%.2fx); peak cut by %.1f MB; results agree: %s"
        % ("MET" if ratio >= 1 else "NOT MET", ratio, saved, agree))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
