#!/usr/bin/env python3
"""Time the sigmoid and Seesaw kinds of BBoxHead.loss's classification half without its host read
(iif_amd/mmdet_bbox_head_loss.py; csrc/head_loss.hip: iif_head_bce_loss_fwd; csrc/seesaw_head.hip: iif_seesaw_head_fwd / _bwd)
against the chain that existed before them, same GPU, same process, the variants alternating round by round.

    python scripts/bench_head_loss_kinds.py [--out profiles/head_loss_kinds.txt]

Shapes: [1024, 1203] fp32 scores with CrossEntropyLoss(use_sigmoid=True) and [1024, 1205] with SeesawLoss (1203 classes), one
row in four of weight 0 (padding), forward + backward through autograd, END TO END WITH THE HOST'S WORK: a host clock around
`inner` calls that end in a device synchronise (the old chain synchronises by itself, once per call).
  new      head_cls_loss(...) and backward(): sigmoid one launch forward, Seesaw two; one backward; nothing read back
  chain_a  torch.sum(label_weights > 0).float().item(), the module's own forward with that avg_factor, the accuracy launch
  chain_b  (iif_topk_hits / iif_seesaw_accuracy), autograd backward - measured TWICE, for the chain's own spread
The results are compared first (losses, gradient, avg_factor).  The Seesaw chain counts the padding rows into cum_samples, which
moves its loss, so for the comparison it gets the rows of weight != 0; it is timed on the padded batch, which is what a user
runs today.  Then, K launches between two device events each (report only):
  fwd_new  iif_head_bce_loss_fwd / iif_seesaw_head_fwd alone
  fwd_old  iif_bce_det_fwd_bwd / iif_seesaw_fwd_bwd + iif_seesaw_accuracy on the same inputs (avg_factor a host number)
Every round times each variant; the table gives the median over the rounds and their range.  No ratio is a gate."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iif_amd import _lib, custom                                           # noqa: E402
from iif_amd import mmdet_seesaw_loss as seesaw                            # noqa: E402
from iif_amd.mmdet_bbox_head_loss import SEESAW_HEAD_WORKSPACE_WORDS, head_cls_loss      # noqa: E402
from iif_amd.mmdet_ce_loss import CrossEntropyLoss                         # noqa: E402
from iif_amd.mmdet_seesaw_loss import SeesawLoss                           # noqa: E402
from iif_amd.utils import topk_hit_counts                                  # noqa: E402

ROUNDS, INNER, ITERS, K = 7, 200, 30, 20
N, CLASSES = 1024, 1203


def host_round(fn):
    """Microseconds per call: a host clock around INNER calls and the synchronise that ends them."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(INNER):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / INNER


def event_round(fn):
    """Median microseconds per launch of ITERS event pairs, each around K launches."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for a, b in ev:
        a.record()
        for _ in range(K):
            fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 / K for a, b in ev)
    return ts[len(ts) // 2]


def loss_keys(out):
    return sorted(k for k in out if k.startswith("loss"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X: no device, no number"
    dev = "cuda"
    lib = _lib.lib()
    lines = ["BBoxHead.loss classification half, sigmoid CrossEntropyLoss and SeesawLoss, fp32, %d rows, one in four of weight 0, %s"
             % (N, torch.cuda.get_device_name(0)),
             "%d rounds, the variants alternating; new / chain_*: host clock around %d forward + backward calls and a synchronise; fwd_*: "
             "median of %d event pairs around %d launches; microseconds per call: median over the rounds [min .. max]"
             % (ROUNDS, INNER, ITERS, K)]
    for kind in ("sigmoid", "seesaw"):
        C = CLASSES
        cols = C if kind == "sigmoid" else C + 2
        gen = torch.Generator(device="cpu").manual_seed(cols)
        x = (torch.randn(N, cols, generator=gen) * 2.0).to(dev)
        labels = torch.randint(0, C + 1, (N,), generator=gen)
        labels[torch.rand(N, generator=gen) < 0.5] = C                   # half of the rows are background, as a sampled batch is
        labels = labels.to(dev)
        w = (torch.rand(N, generator=gen) >= 0.25).float().to(dev)
        make = (lambda: CrossEntropyLoss(use_sigmoid=True)) if kind == "sigmoid" else (lambda: SeesawLoss(num_classes=C, device=dev))
        crit_new, crit_chain = make(), make()
        xn = x.clone().requires_grad_(True)
        xc = x.clone().requires_grad_(True)
        res = {}

        def new():
            xn.grad = None
            out = head_cls_loss(crit_new, xn, labels, w)
            sum(out[k] for k in loss_keys(out)).backward()
            res["new"] = out

        def chain(crit=crit_chain, xs=xc, lab=labels, wt=w):
            xs.grad = None
            avg = max(torch.sum(w > 0).float().item(), 1.)
            out = crit(xs, lab, wt, avg_factor=avg)
            out = out if isinstance(out, dict) else dict(loss_cls=out)
            if kind == "sigmoid":
                out["acc"] = topk_hit_counts(xs, lab, (1,)).to(torch.float32) * (100.0 / xs.size(0))
            else:
                out.update(crit.get_accuracy(xs, lab))
            sum(out[k] for k in loss_keys(out)).backward()
            res["chain"] = dict(out, avg_factor=avg)

        # ---- the results first: fresh modules, the chain on the rows the new path reads
        keep = w != 0
        x_keep = x[keep].clone().requires_grad_(True)
        new()
        chain(make(), x_keep, labels[keep], w[keep])
        torch.cuda.synchronize()
        a, b = res["new"], res["chain"]
        g_chain = torch.zeros_like(x)
        g_chain[keep] = x_keep.grad
        assert float(a["avg_factor"]) == b["avg_factor"]
        for k in loss_keys(a):
            la, lb = float(a[k].detach()), float(b[k].detach())
            lines.append("[%d, %d] %s: %s new %.7g chain %.7g (rel. diff %.1e)" % (N, cols, kind, k, la, lb, abs(la - lb) / abs(lb)))
            assert abs(la - lb) <= 1e-5 * abs(lb)
        gdiff = float((xn.grad - g_chain).abs().max() / g_chain.abs().max())
        lines.append("    avg_factor %g / %g; gradient max diff %.1e of the largest element" % (float(a["avg_factor"]), b["avg_factor"], gdiff))
        assert gdiff <= 1e-5
        avg = float(a["avg_factor"])

        # ---- each forward kernel alone, next to the kernel(s) it extends
        rows, ticket, status = custom._workspace(x.device, N, False)
        d = torch.empty_like(x)
        outs = torch.empty(8, device=dev)
        stream = _lib.stream_ptr()
        o = outs.data_ptr()
        if kind == "sigmoid":
            def fwd_new():
                lib.iif_head_bce_loss_fwd(_lib.ptr(x), 0, C, _lib.ptr(labels), _lib.ptr(w), None, -100, 1.0, N, C, _lib.ptr(d), C,
                                          o, o + 4, o + 8, _lib.ptr(ticket), stream)

            def fwd_old():
                lib.iif_bce_det_fwd_bwd(_lib.ptr(x), 0, C, _lib.ptr(labels), _lib.ptr(w), -100, None, None, None, 1.0 / avg, N, C, None,
                                        o, _lib.ptr(d), C, _lib.ptr(ticket), stream)
        else:
            ws = seesaw._workspace(x.device, stream)
            head_ws = torch.zeros(SEESAW_HEAD_WORKSPACE_WORDS, dtype=torch.int32, device=dev)
            cum_a, cum_b = torch.zeros(C + 1, device=dev), torch.zeros(C + 1, device=dev)
            lrows = torch.empty((2, N), device=dev)

            def fwd_new():
                lib.iif_seesaw_head_fwd(_lib.ptr(x), 0, cols, _lib.ptr(labels), _lib.ptr(w), _lib.ptr(cum_a), 0.8, 2.0, 1e-2, 1.0, N, C,
                                        _lib.ptr(d), cols, o, o + 12, o + 20, _lib.ptr(ws["status"]), _lib.ptr(head_ws), stream)

            def fwd_old():
                lib.iif_seesaw_fwd_bwd(_lib.ptr(x), 0, cols, _lib.ptr(labels), _lib.ptr(w), _lib.ptr(cum_b), 1, 0.8, 2.0, 1e-2, 1.0 / avg, 0,
                                       1.0 / avg, N, C, _lib.ptr(lrows[0]), _lib.ptr(lrows[1]), o, _lib.ptr(d), cols, _lib.ptr(ws["status"]),
                                       _lib.ptr(ws["loss"]), stream)
                lib.iif_seesaw_accuracy(_lib.ptr(x), 0, cols, _lib.ptr(labels), N, C, o + 12, _lib.ptr(ws["acc"]), stream)

        variants = [("new", new, host_round), ("chain_a", chain, host_round), ("chain_b", chain, host_round),
                    ("fwd_new", fwd_new, event_round), ("fwd_old", fwd_old, event_round)]
        for _, fn, _ in variants:
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _, _ in variants}
        for _ in range(ROUNDS):
            for name, fn, timer in variants:
                t[name].append(timer(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        for name, _, _ in variants:
            lines.append("    %-8s %9.1f  [%9.1f .. %9.1f]" % (name, med[name], min(t[name]), max(t[name])))
        chain_med = 0.5 * (med["chain_a"] + med["chain_b"])
        spread = max(max(t["chain_a"]), max(t["chain_b"])) - min(min(t["chain_a"]), min(t["chain_b"]))
        lines.append("    chain / new: %.2fx (%.1f us less per call; the chain's two measurements differ by %.1f us in the median and "
                     "range over %.1f us); fwd_new / fwd_old: %.2fx its time"
                     % (chain_med / med["new"], chain_med - med["new"], abs(med["chain_a"] - med["chain_b"]), spread,
                        med["fwd_new"] / med["fwd_old"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
