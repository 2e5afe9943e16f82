#!/usr/bin/env python3
"""Measure ``valid_rows=True`` of the class-selected mask predictor (iif_amd/mmdet_mask_predictor.py) and of the fused mask head
tail (iif_amd/mmdet_mask_tail.py) on padded RoI rows against the chain the package offered before it: read the number of real
rows, compact ``x`` / ``f``, labels and targets with boolean indexing, call the existing loss.  One process; the output is
profiles/mask_valid_rows.txt.

    python scripts/bench_mask_valid_rows.py [--out FILE] [--rounds 7] [--quick]

Method (that of scripts/bench_mask_tail.py): results are compared first (loss and every gradient of the two paths, the gradient
of the padded ``x`` / ``f`` included); every variant is warmed up; a round times `inner` calls of each variant between two device
events, the variants alternating inside a round; reported is the median over the rounds [min .. max] per call.  The times are
end to end - host work, the chain's read of the count and its indexing kernels included - and the chain is measured twice
("chain", "chain again"): the distance between the two is the spread a difference has to exceed.  Kernel times are the C entries
called on their own: the new entries on all N padded rows against the existing entries on the K compacted rows.

The padded rows hold zeros (what SingleRoIExtractor and mask_targets_padded write) and the label C.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mask_tail import DEV, LINES, line, make, say, timed                                    # noqa: E402
from iif_amd import _lib                                                                          # noqa: E402
from iif_amd.mmdet_mask_predictor import class_mask_loss                                          # noqa: E402
from iif_amd.mmdet_mask_tail import upsampled_class_mask_loss                                     # noqa: E402

C = 1203


def padded(kind, n, k, seed):
    """(leaves, labels, targets): n rows of which a seeded random k are real.  kind 'predictor': x [n, 256, 28, 28], weight,
    bias; 'tail': f [n, 256, 14, 14] and the four parameters."""
    f, uw, ub, w, b, lb, t = make(n, C, seed=seed)
    real = torch.zeros(n, dtype=torch.bool)
    real[torch.randperm(n, generator=torch.Generator().manual_seed(seed + 1))[:k]] = True
    real = real.to(DEV)
    lb = torch.where(real, lb, torch.full_like(lb, C))
    t = t * real[:, None, None]
    if kind == "tail":
        return [f * real[:, None, None, None], uw, ub, w, b], lb, t
    x = torch.relu(torch.randn(n, 256, 28, 28, generator=torch.Generator().manual_seed(seed + 2))).to(DEV)
    return [x * real[:, None, None, None], w, b], lb, t


def chain(loss_fn, leaves, lb, t):
    """What a caller of the parent does: the count read, boolean indexing, the existing loss on the compacted rows."""
    keep = (lb >= 0) & (lb < C)
    if int(keep.sum()) == 0:                             # the read
        return leaves[0].sum() * 0
    return loss_fn(leaves[0][keep], *leaves[1:], lb[keep], t[keep])


def end_to_end(kind, n, k, rounds, inner):
    loss_fn = class_mask_loss if kind == "predictor" else upsampled_class_mask_loss
    base, lb, t = padded(kind, n, k, 10 * k)
    names = ("dx", "dweight", "dbias") if kind == "predictor" else ("df", "dup_weight", "dup_bias", "dweight", "dbias")
    leaves = lambda: [v.clone().requires_grad_(True) for v in base]                    # noqa: E731

    def run(new, lv):
        for v in lv:
            v.grad = None
        loss = loss_fn(*lv, lb, t, valid_rows=True) if new else chain(loss_fn, lv, lb, t)
        loss.sum().backward()
        return loss
    a, o = leaves(), leaves()
    la, lo = float(run(True, a).detach()), float(run(False, o).detach())
    rel = [float((p.grad - q.grad).abs().max() / q.grad.abs().max()) for p, q in zip(a, o)]
    agree = abs(la - lo) <= 2e-5 * max(1.0, abs(lo)) and max(rel) <= 2e-5
    say("%s, N = %d rows of which %d real, C = %d: the two paths agree (loss %.1e, %s): %s"
        % (kind, n, k, C, abs(la - lo), ", ".join("%s %.1e" % kv for kv in zip(names, rel)), agree))
    del a, o
    lv = leaves()
    r = timed({"new": lambda: run(True, lv), "chain": lambda: run(False, lv), "again": lambda: run(False, lv)}, rounds, inner)
    say(line("valid_rows=True on the padded rows, fwd + bwd", r["new"]))
    say(line("chain: count read, compact, existing loss", r["chain"]))
    say(line("chain again", r["again"]))
    med = {key: statistics.median(v) for key, v in r.items()}
    spread = abs(med["chain"] - med["again"]) / med["chain"]
    ratio = min(med["chain"], med["again"]) / med["new"]
    say("    padded vs chain: %.2fx its speed (the faster of the two chain runs; they differ by %.1f %%)" % (ratio, 100 * spread))
    return agree, ratio


def kernels(kind, n, k, rounds, inner):
    """The C entries alone: the new ones on the n padded rows, the existing ones on the k compacted rows."""
    base, lb, t = padded(kind, n, k, 10 * k)
    keep = lb < C
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    up = torch.ones(1, device=DEV)

    def entries(rows, new):
        x = (base[0] if new else base[0][keep]).contiguous()
        labels, tg = (lb, t) if new else (lb[keep].contiguous(), t[keep].contiguous())
        loss, inv, status = torch.empty(1, device=DEV), torch.empty(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        if kind == "predictor":
            w, b = base[1].reshape(C, -1), base[2]
            cin, hw = x.shape[1], x.shape[2] * x.shape[3]
            g, rl = torch.empty(rows, hw, device=DEV), torch.empty(rows * ((hw + 63) // 64), device=DEV)
            dx, scratch = torch.empty_like(x), torch.empty(rows, cin + 1, device=DEV)
            dw, db = torch.empty(C, cin, device=DEV), torch.empty(C, device=DEV)
            if new:
                return {
                    "fwd": lambda: _lib.check(L.iif_mask_predict_loss_fwd(p(x), 0, p(w), cin, p(b), p(labels), p(tg), rows, C, cin, hw, 1,
                                                                          p(g), p(rl), p(loss), p(inv), st), "fwd"),
                    "dx": lambda: _lib.check(L.iif_mask_predict_loss_bwd_input(p(g), p(up), p(inv), p(w), cin, p(labels), rows, C, cin,
                                                                               hw, p(dx), 0, st), "dx"),
                    "dweight": lambda: _lib.check(L.iif_mask_predict_loss_bwd_weight(p(x), 0, p(g), p(up), p(inv), p(labels), rows, C,
                                                                                     cin, hw, p(scratch), p(dw), p(db), st), "dw")}
            return {
                "fwd": lambda: _lib.check(L.iif_mask_predict_fwd(p(x), 0, p(w), cin, p(b), p(labels), p(tg), rows, C, cin, hw, 0, p(g),
                                                                 p(rl), p(loss), p(status), st), "fwd"),
                "dx": lambda: _lib.check(L.iif_mask_predict_bwd_input(p(g), p(up), p(w), cin, p(labels), rows, C, cin, hw, p(dx), 0, st),
                                         "dx"),
                "dweight": lambda: _lib.check(L.iif_mask_predict_bwd_weight(p(x), 0, p(g), p(up), p(labels), rows, C, cin, hw,
                                                                            p(scratch), p(dw), p(db), st), "dw")}
        uw, ub, w, b = base[1], base[2], base[3].reshape(C, -1), base[4]
        ci, co, h, wd = x.shape[1], uw.shape[1], x.shape[2], x.shape[3]
        hw = h * wd
        g, rl = torch.empty(rows, 4 * hw, device=DEV), torch.empty(rows * ((hw + 63) // 64), device=DEV)
        signs = torch.empty(rows * ((hw + 31) // 32) * 4 * co, dtype=torch.int32, device=DEV)
        rws, df = torch.empty(rows, co + 1, device=DEV), torch.empty_like(x)
        partial = torch.empty(L.iif_mask_tail_splits(rows, ci, co) * (ci + 1) * 4 * co, device=DEV)
        duw, dub = torch.empty_like(uw), torch.empty_like(ub)
        if new:
            return {
                "fwd": lambda: _lib.check(L.iif_mask_tail_loss_fwd(p(x), 0, p(uw), p(ub), p(w), co, p(b), p(labels), p(tg), rows, C, ci, co,
                                                                   h, wd, 1, p(g), p(rl), p(loss), p(inv), st), "fwd"),
                "rows": lambda: _lib.check(L.iif_mask_tail_loss_bwd_rows(p(x), 0, p(uw), p(ub), p(g), p(up), p(inv), p(labels), rows, C, ci,
                                                                         co, h, wd, p(signs), p(rws), st), "rows"),
                "df": lambda: _lib.check(L.iif_mask_tail_loss_bwd_input(p(g), p(up), p(inv), p(uw), p(w), co, p(labels), p(signs), rows, C,
                                                                        ci, co, h, wd, p(df), 0, st), "df"),
                "dup": lambda: _lib.check(L.iif_mask_tail_loss_bwd_params(p(x), 0, p(g), p(up), p(inv), p(w), co, p(labels), p(signs), rows,
                                                                          C, ci, co, h, wd, p(partial), p(duw), p(dub), st), "dup")}
        return {
            "fwd": lambda: _lib.check(L.iif_mask_tail_fwd(p(x), 0, p(uw), p(ub), p(w), co, p(b), p(labels), p(tg), rows, C, ci, co, h, wd,
                                                          0, p(g), p(rl), p(loss), p(status), st), "fwd"),
            "rows": lambda: _lib.check(L.iif_mask_tail_bwd_rows(p(x), 0, p(uw), p(ub), p(g), p(up), p(labels), rows, C, ci, co, h, wd,
                                                                p(signs), p(rws), st), "rows"),
            "df": lambda: _lib.check(L.iif_mask_tail_bwd_input(p(g), p(up), p(uw), p(w), co, p(labels), p(signs), rows, C, ci, co, h, wd,
                                                               p(df), 0, st), "df"),
            "dup": lambda: _lib.check(L.iif_mask_tail_bwd_params(p(x), 0, p(g), p(up), p(w), co, p(labels), p(signs), rows, C, ci, co, h,
                                                                 wd, p(partial), p(duw), p(dub), st), "dup")}
    new, old = entries(n, True), entries(k, False)
    variants = {}
    for key in new:                                      # forward first in either family: it fills g, the rows pass fills signs
        variants["new " + key], variants["old " + key] = new[key], old[key]
    r = timed(variants, rounds, inner)
    tot = {"new": 0.0, "old": 0.0}
    for key in new:
        a, b = statistics.median(r["new " + key]), statistics.median(r["old " + key])
        tot["new"] += a
        tot["old"] += b
        say("    %-8s padded rows %8.1f us   compacted rows, existing entry %8.1f us" % (key, a * 1e3, b * 1e3))
    why = ("dx writes the zero slices of the padded rows, which the chain's indexing backward writes instead" if kind == "predictor"
           else "dup cuts the rows into ranges by index, so the range with the most real rows sets its time")
    say("    kernels alone: padded %.1f us, compacted %.1f us (%+.1f %%): the grids cover all %d rows, the real ones first, and a"
        " block reads the labels to find its row; %s" % (tot["new"] * 1e3, tot["old"] * 1e3, 100 * (tot["new"] / tot["old"] - 1), n, why))
    return tot["new"] / tot["old"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small N: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_valid_rows.py measures on the GPU; none found")
    n = 16 if a.quick else 256
    inner = 10
    say("mask loss on padded RoI rows (valid_rows=True), %s" % torch.cuda.get_device_name(0))
    say("%d rounds, the variants alternating; per round %d calls between two device events; microseconds per call: median over the "
        "rounds [min .. max]" % (a.rounds, inner))
    ok = True
    for kind in ("predictor", "tail"):
        for k in (n // 2, n // 4):
            agree, _ = end_to_end(kind, n, k, a.rounds, inner)
            ok = ok and agree
            kernels(kind, n, k, a.rounds, inner)
    say("results agree in every configuration: %s" % ok)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
