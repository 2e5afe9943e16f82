#!/usr/bin/env python3
"""Time the classification half of BBoxHead.loss without its host read (iif_amd/mmdet_bbox_head_loss.py, csrc/head_loss.hip)
against the chain that existed before it, same GPU, same process, the variants alternating round by round.

    python scripts/bench_bbox_head_loss.py [--out profiles/bbox_head_loss.txt]

Shapes: [1024, 1204] and [2048, 1204] fp32 scores, IIFLoss with the LVIS table, one row in four of weight 0 (padding),
forward + backward through autograd, END TO END WITH THE HOST'S WORK: a host clock around `inner` calls that end in a device
synchronise (the old chain synchronises by itself, once per call).
  new      head_cls_loss(...)['loss_cls'].backward(): one launch forward, one backward, nothing read back
  chain_a  torch.sum(label_weights > 0).float().item(), IIFLoss.forward (iif_ce_fwd_bwd), get_accuracy (a clear and
  chain_b  iif_topk_hits), autograd backward (iif_scale_by_device_scalar) - measured TWICE, for the chain's own spread
The results are compared first (loss, gradient, avg_factor; the accuracies differ by design on padded rows: the chain divides
by all rows).  Then, K launches between two device events each (report only):
  fwd_new  iif_head_loss_fwd alone
  fwd_ce   iif_ce_fwd_bwd alone at the same shape (loss + gradient, avg_factor a host number)
Every round times each variant; the table gives the median over the rounds and their range.  No ratio is a gate."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iif_amd import _lib, custom                                           # noqa: E402
from iif_amd.mmdet_bbox_head_loss import head_cls_loss                     # noqa: E402
from iif_amd.mmdet_iif_loss import IIFLoss                                 # noqa: E402

ROUNDS, INNER, ITERS, K = 7, 200, 30, 20
CSV = os.path.join(ROOT, "tests", "golden", "lvis_files", "idf_1204.csv")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X: no device, no number"
    dev = "cuda"
    lib = _lib.lib()
    lines = ["BBoxHead.loss classification half, IIFLoss (LVIS table), fp32, one row in four of weight 0, %s" % torch.cuda.get_device_name(0),
             "%d rounds, the variants alternating; new / chain_*: host clock around %d forward + backward calls and a synchronise; fwd_*: "
             "median of %d event pairs around %d launches; microseconds per call: median over the rounds [min .. max]"
             % (ROUNDS, INNER, ITERS, K)]
    for N in (1024, 2048):
        C = 1204
        gen = torch.Generator(device="cpu").manual_seed(N)
        x = (torch.randn(N, C, generator=gen) * 2.0).to(dev)
        labels = torch.randint(0, C, (N,), generator=gen).to(dev)
        w = (torch.rand(N, generator=gen) >= 0.25).float().to(dev)
        crit = IIFLoss(path=CSV, num_classes=C - 1, device=dev)
        xn = x.clone().requires_grad_(True)
        xc = x.clone().requires_grad_(True)
        res = {}

        def new():
            xn.grad = None
            out = head_cls_loss(crit, xn, labels, w)
            out["loss_cls"].backward()
            res["new"] = out

        def chain():
            xc.grad = None
            avg = max(torch.sum(w > 0).float().item(), 1.)
            loss = crit(xc, labels, w, avg_factor=avg)
            acc = crit.get_accuracy(xc, labels)
            loss.backward()
            res["chain"] = dict(loss_cls=loss, avg_factor=avg, **acc)

        new(); chain()
        torch.cuda.synchronize()
        a, b = ({k: v.detach() if torch.is_tensor(v) else v for k, v in res[n].items()} for n in ("new", "chain"))
        lines.append("[%d, %d]: loss new %.7g chain %.7g (rel. diff %.1e); avg_factor %g / %g; gradient max diff %.1e of the largest "
                     "element; acc over the rows that count %.4f, the chain's over all rows %.4f"
                     % (N, C, float(a["loss_cls"]), float(b["loss_cls"]),
                        abs(float(a["loss_cls"]) - float(b["loss_cls"])) / abs(float(b["loss_cls"])), float(a["avg_factor"]), b["avg_factor"],
                        float((xn.grad - xc.grad).abs().max() / xc.grad.abs().max()), float(a["acc_classes"]), float(b["acc_classes"])))
        assert float(a["avg_factor"]) == b["avg_factor"]
        assert abs(float(a["loss_cls"]) - float(b["loss_cls"])) <= 1e-5 * abs(float(b["loss_cls"]))

        rows, ticket, status = custom._workspace(x.device, N, False)
        tab = crit.iif_weights.reshape(-1).contiguous()
        d = torch.empty_like(x)
        outs = torch.empty(3, device=dev)
        stream = _lib.stream_ptr()
        scale = 1.0 / float(a["avg_factor"])

        def fwd_new():
            lib.iif_head_loss_fwd(_lib.ptr(x), 0, C, _lib.ptr(tab), _lib.ptr(labels), _lib.ptr(w), None, -100, 1.0, N, C, _lib.ptr(d), C,
                                  outs.data_ptr(), outs.data_ptr() + 4, outs.data_ptr() + 8, _lib.ptr(status), _lib.ptr(ticket), stream)

        def fwd_ce():
            lib.iif_ce_fwd_bwd(_lib.ptr(x), 0, C, _lib.ptr(tab), _lib.ptr(labels), None, 1.0, _lib.ptr(w), None, -100, scale, N, C,
                               _lib.ptr(rows), outs.data_ptr(), _lib.ptr(d), C, _lib.ptr(status), _lib.ptr(ticket), stream)

        variants = [("new", new, host_round), ("chain_a", chain, host_round), ("chain_b", chain, host_round),
                    ("fwd_new", fwd_new, event_round), ("fwd_ce", fwd_ce, event_round)]
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
                     "range over %.1f us); fwd_new / fwd_ce: %.2fx its time (at most %.0f MB moved - rows of weight 0 are written, not read: %.2f TB/s)"
                     % (chain_med / med["new"], chain_med - med["new"], abs(med["chain_a"] - med["chain_b"]), spread,
                        med["fwd_new"] / med["fwd_ce"], 8.0 * N * C * 1e-6, 8.0 * N * C / med["fwd_new"] * 1e-6))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
