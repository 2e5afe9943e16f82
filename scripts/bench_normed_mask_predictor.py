#!/usr/bin/env python3
"""Measure the class-selected NormedConv2d mask predictor (iif_amd/mmdet_normed_mask_predictor.py) against the path the package
offered for the cos-norm mask head before it, the dense ``iif_amd.mmdet_normed_predictor.NormedConv2d`` followed by
``mask_cross_entropy``, in one process; the output is profiles/normed_mask_predictor.txt.

    python scripts/bench_normed_mask_predictor.py [--out FILE] [--rounds 7] [--quick]

Method (that of scripts/bench_mask_predictor.py): results are compared first (loss and gradients of the two paths); every
variant is warmed up; a round times `inner` calls of each variant between two device events, the variants alternating inside a
round; reported is the median over the rounds [min .. max] per call.  Kernel times are the C entries called on their own
against the bytes the algorithm must move (x once per pass that reads it, dx once, the compact [N, HW] arrays), timed back to
back - x (205 MB) then stays in the 256 MiB Infinity Cache from call to call - and one call at a time behind a 1 GiB read or
fill that evicts it.  Peak memory is torch's max_memory_allocated over one forward + backward, above what the inputs and
parameters hold.  The test end is the forward alone at 100 / 300 detections.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_mask_predictor import DEV, LINES, cold, line, make, peak, say, timed            # noqa: E402
from iif_amd import _lib                                                                  # noqa: E402
from iif_amd.mmdet_mask_loss import gather_class_masks, mask_cross_entropy               # noqa: E402
from iif_amd.mmdet_normed_mask_predictor import normed_class_mask_logits, normed_class_mask_loss        # noqa: E402
from iif_amd.mmdet_normed_predictor import NormedConv2d                                  # noqa: E402

TEMP, POWER, EPS = 20.0, 1.0, 1e-6


def dense(w, b):
    c, cin = w.shape[:2]
    conv = NormedConv2d(cin, c, 1, tempearture=TEMP, power=POWER, eps=EPS).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    return conv


def train_shape(title, n, c, rounds, inner, kernels=False):
    x, w, b, lb, t = make(n, c)
    conv = dense(w, b)
    xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xo = x.clone().requires_grad_(True)

    def new():
        xg.grad = wg.grad = bg.grad = None
        normed_class_mask_loss(xg, wg, bg, lb, t, TEMP, POWER, EPS).sum().backward()

    def old():
        xo.grad = conv.weight.grad = conv.bias.grad = None
        mask_cross_entropy(conv(xo), t, lb).sum().backward()
    new(), old()
    with torch.no_grad():
        la = float(normed_class_mask_loss(x, w, b, lb, t, TEMP, POWER, EPS))
        lo = float(mask_cross_entropy(conv(x), t, lb))
    rel = [float((p.grad - q.grad).abs().max() / q.grad.abs().max()) for p, q in ((xg, xo), (wg, conv.weight), (bg, conv.bias))]
    agree = abs(la - lo) <= 2e-5 and max(rel) <= 2e-5
    say("%s: N = %d, C = %d, Cin = 256, 28 x 28; the two paths agree (loss %.1e, dx %.1e, dweight %.1e, dbias %.1e): %s"
        % (title, n, c, abs(la - lo), rel[0], rel[1], rel[2], agree))
    r = timed({"new": new, "old": old}, rounds, inner)
    say(line("normed_class_mask_loss fwd + bwd", r["new"]))
    say(line("NormedConv2d + mask_cross_entropy", r["old"]))
    say("    normed_class_mask_loss vs the dense predictor: %.2fx its speed" % (statistics.median(r["old"]) / statistics.median(r["new"])))

    def drop():
        xg.grad = wg.grad = bg.grad = xo.grad = conv.weight.grad = conv.bias.grad = None
    say("    peak memory above the inputs and parameters, gradients included: normed_class_mask_loss %.1f MB, dense predictor %.1f MB"
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
    coef = torch.empty(3, n, hw, device=DEV)
    rows = torch.empty(n * ((hw + 63) // 64), device=DEV)
    loss, inv, up = torch.empty(1, device=DEV), torch.empty(1, device=DEV), torch.ones(1, device=DEV)
    dx, scratch = torch.empty_like(x), torch.empty(n, cin + 1, device=DEV)
    dw, db = torch.empty(c, cin, device=DEV), torch.empty(c, device=DEV)
    p = _lib.ptr
    g, ca, cb = coef[0], coef[1], coef[2]
    fwd = lambda: _lib.check(L.iif_normed_mask_predict_fwd(p(x), 0, p(w2), cin, p(b), p(lb), p(t), n, c, cin, hw, TEMP, POWER, EPS, 0,      # noqa: E731
                                                           0, p(g), p(ca), p(cb), p(rows), p(loss), p(inv), st), "fwd")
    dxk = lambda: _lib.check(L.iif_normed_mask_predict_bwd_input(p(x), 0, p(g), p(ca), p(cb), p(up), p(inv), p(w2), cin, p(lb), n, c,       # noqa: E731
                                                                 cin, hw, POWER, EPS, p(dx), st), "dx")
    dwk = lambda: _lib.check(L.iif_normed_mask_predict_bwd_weight(p(x), 0, p(g), p(ca), p(up), p(inv), p(w2), cin, p(lb), n, c, cin, hw,    # noqa: E731
                                                                  POWER, EPS, p(scratch), p(dw), p(db), st), "dw")
    r = timed({"fwd": fwd, "dx": dxk, "dw": dwk}, rounds, inner)
    xb, m = x.numel() * 4, n * hw * 4
    for k, f, label, nbytes in (("fwd", fwd, "iif_normed_mask_predict_fwd (2 launches)", xb + 4 * m),
                                ("dx", dxk, "iif_normed_mask_predict_bwd_input", 2 * xb + 3 * m),
                                ("dw", dwk, "iif_normed_mask_predict_bwd_weight (2)", xb + 2 * m + 2 * n * (cin + 1) * 4 + (c + min(n, c)) * (cin + 1) * 4)):
        ms, mc, md = statistics.median(r[k]), statistics.median(cold(f, rounds, False)), statistics.median(cold(f, rounds, True))
        say("    %-40s %6.1f us for %6.2f MB that must move: %4.0f GB/s; cold behind a read %6.1f us: %4.0f GB/s, behind a fill %6.1f us: %4.0f GB/s"
            % (label, ms * 1e3, nbytes / 1e6, nbytes / ms / 1e6, mc * 1e3, nbytes / mc / 1e6, md * 1e3, nbytes / md / 1e6))


def test_shape(n, c, rounds, inner):
    x, w, b, lb, _ = make(n, c)
    conv = dense(w, b)
    with torch.no_grad():
        new = lambda: normed_class_mask_logits(x, w, b, lb, TEMP, POWER, EPS)                # noqa: E731
        old = lambda: gather_class_masks(conv(x), lb)                                        # noqa: E731
        err = float((new()[:, 0] - old()).abs().max())
        r = timed({"new": new, "old": old}, rounds, inner)
        say("test shape, forward only: N = %d, C = %d; largest difference of the selected logits %.1e" % (n, c, err))
        say(line("normed_class_mask_logits", r["new"]))
        say(line("NormedConv2d + gather_class_masks", r["old"]))
        say("    normed_class_mask_logits vs the dense predictor: %.2fx its speed; peak memory %.1f MB vs %.1f MB"
            % (statistics.median(r["old"]) / statistics.median(r["new"]), peak(new), peak(old)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small N: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normed_mask_predictor.py measures on the GPU; none found")
    n = 8 if a.quick else 256
    say("class-selected NormedConv2d mask predictor (tempearture 20, power 1), %s" % torch.cuda.get_device_name(0))
    inner = 20
    say("%d rounds, the variants alternating; per round %d calls between two device events; microseconds per call: median over the "
        "rounds [min .. max]" % (a.rounds, inner))
    ratio, agree = train_shape("LVIS training shape", n, 1203, a.rounds, inner, kernels=True)
    agree = train_shape("COCO", n, 80, a.rounds, inner)[1] and agree
    agree = train_shape("class-agnostic head", n, 1, a.rounds, inner)[1] and agree
    for nt in ((4, 6) if a.quick else (100, 300)):
        test_shape(nt, 1203, a.rounds, inner)
    say("no speed-up is a condition; at the LVIS training shape forward + backward ran at %.2fx the dense predictor's speed; "
        "results agree: %s" % (ratio, agree))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
