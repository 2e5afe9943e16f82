#!/usr/bin/env python3
"""Time FasaBBoxHead.loss without a host read (iif_amd/mmdet_fasa_head_loss.py, csrc/fasa_head.hip) against the chain that
existed before it, same GPU, same process, the variants alternating round by round.

    python scripts/bench_fasa_head.py [--out profiles/fasa_head.txt]
    python scripts/bench_fasa_head.py --calls 50 --path new|chain      # nothing timed: that many calls, for a kernel trace

The LVIS head shape: 1 024 rows, one in four padded (label C, weight 0), about a quarter positive, D = 1024, 1 204 channels,
bbox_pred [1024, 4 * 1203], epoch >= 1, FasaIIFLoss (LVIS table) + L1Loss, fc_cls an nn.Linear, fresh draws every call.
Forward + backward through autograd, END TO END WITH THE HOST'S WORK: a host clock around `inner` calls that end in a device
synchronise (the old chain synchronises by itself, several times per call).
  new      fasa_bbox_head_loss(...), (loss_cls + loss_bbox).backward(): nothing read back
  chain_a  embedding[pos] / labels[pos] (boolean indexing), fa_update, bbox_head_loss, fa_generate with its read, fc_cls,
  chain_b  IIFLoss.forward with a host avg_factor, the sum, backward - measured TWICE, for the chain's own spread
The results are compared first, with the same given draws: both losses, both banks bit for bit, the three gradients.
Then the launches alone, between device events (report only), warm (K launches per event pair) and cold (one launch per pair
behind a 512 MB fill that empties the caches):
  upd_rows  iif_fasa_update_rows on the padded rows (two launches)      upd_old  iif_fasa_update on the compacted rows
  gen_pad   iif_fasa_generate_padded (one launch)                        gen_old  iif_fasa_generate (two launches)
Every round times each variant; the table gives the median over the rounds and their range.  The acceptance: `new` below the
faster of the chain's two medians by more than the chain's own spread."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iif_amd import _lib                                                            # noqa: E402
from iif_amd.mmdet_bbox_head_loss import bbox_head_loss                             # noqa: E402
from iif_amd.mmdet_bbox_loss import L1Loss                                          # noqa: E402
from iif_amd.mmdet_fasa import FasaFeatureBank, FasaIIFLoss                         # noqa: E402
from iif_amd.mmdet_fasa_head_loss import ENQUEUED_TRAIN, fasa_bbox_head_loss        # noqa: E402

ROUNDS, INNER, ITERS, K = 7, 100, 30, 20
N, D, C = 1024, 1024, 1203
CSV = os.path.join(ROOT, "tests", "golden", "lvis_files", "idf_1204.csv")
G13 = os.path.join(ROOT, "tests", "golden", "g13_mmdet_fasa.npz")


def host_round(fn):
    """Microseconds per call: a host clock around INNER calls and the synchronise that ends them."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(INNER):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / INNER


def event_round(fn):
    """Median microseconds per call of ITERS event pairs, each around K calls."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for a, b in ev:
        a.record()
        for _ in range(K):
            fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 / K for a, b in ev)
    return ts[len(ts) // 2]


_FLUSH = []


def cold_round(fn):
    """Median microseconds of ITERS single calls, each behind a fill of 512 MB (larger than the L2s and the Infinity Cache)."""
    if not _FLUSH:
        _FLUSH.append(torch.empty(128 << 20, dtype=torch.float32, device="cuda"))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for i, (a, b) in enumerate(ev):
        _FLUSH[0].fill_(float(i))
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return ts[len(ts) // 2]


class Setup:
    def __init__(self, dev):
        gen = torch.Generator(device="cpu").manual_seed(37)
        c1 = C + 1
        labels = torch.full((N,), C, dtype=torch.int64)
        real = 3 * N // 4
        npos = N // 4
        labels[:npos] = torch.randint(0, C, (npos,), generator=gen) // 6 * 6             # ~170 classes, a few rows each
        labels[:real] = labels[:real][torch.randperm(real, generator=gen)]
        w = torch.ones(N)
        w[real:] = 0.0
        pos = (labels >= 0) & (labels < C)
        bw = torch.zeros(N, 4)
        bw[pos] = 1.0
        self.labels, self.w, self.bw = labels.to(dev), w.to(dev), bw.to(dev)
        self.x = (torch.randn(N, c1, generator=gen) * 2.0).to(dev)
        self.bp = (torch.randn(N, 4 * C, generator=gen) / 4).to(dev)
        self.bt = (torch.randn(N, 4, generator=gen) / 8).to(dev)
        self.emb = (torch.randn(N, D, generator=gen) * 1.5 + 0.3).to(dev)
        self.rand = torch.rand(C, generator=gen).to(dev)
        self.normal = torch.randn(C, D, generator=gen).to(dev)
        self.counts = np.load(G13, allow_pickle=False)["instance_counts"]
        self.crit = FasaIIFLoss(path=CSV, num_classes=C, device=dev)
        self.reg = L1Loss()
        self.lin = torch.nn.Linear(D, c1).to(dev)
        self.dev = dev

    def bank(self):
        b = FasaFeatureBank(C, D, self.counts, dict(decay_ratio=0.1, loss_aug_weight=0.1, instance_prob_scale=1500.0), device=self.dev)
        b.epoch = 1
        return b


def make_paths(s, bank_new, bank_chain, res):
    xn, bn = s.x.clone().requires_grad_(True), s.bp.clone().requires_grad_(True)
    xc, bc = s.x.clone().requires_grad_(True), s.bp.clone().requires_grad_(True)

    def new(rand=None, normal=None):
        xn.grad = bn.grad = s.lin.weight.grad = s.lin.bias.grad = None
        losses = fasa_bbox_head_loss(bank_new, s.crit, s.reg, s.lin, xn, bn, None, s.labels, s.w, s.bt, s.bw, s.emb, C, rand=rand,
                                     normal=normal)
        (losses["loss_cls"] + losses["loss_bbox"]).backward()
        res["new"] = (losses, xn.grad, bn.grad, s.lin.weight.grad)

    def chain(rand=None, normal=None):
        xc.grad = bc.grad = s.lin.weight.grad = s.lin.bias.grad = None
        pos = (s.labels >= 0) & (s.labels < C)
        pos_embedding, pos_label = s.emb[pos], s.labels[pos]                         # two host reads
        if len(pos_embedding) > 0:
            bank_chain.fa_update(pos_embedding, pos_label)
        losses = bbox_head_loss(s.crit, s.reg, xc, bc, None, s.labels, s.w, s.bt, s.bw, C)
        e, l = bank_chain.fa_generate(rand, normal)                                  # one host read
        if len(e) > 0:
            aw = torch.ones(len(l), device=s.dev) * bank_chain.loss_aug_weight
            avg = max(torch.sum(aw > 0).float().item(), 1.)                          # one host read
            losses["loss_cls"] = losses["loss_cls"] + s.crit(s.lin(e), l, aw, avg_factor=avg)
        (losses["loss_cls"] + losses["loss_bbox"]).backward()
        res["chain"] = (losses, xc.grad, bc.grad, s.lin.weight.grad)

    return new, chain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--path", default="new", choices=("new", "chain"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X: no device, no number"
    dev = "cuda"
    lib = _lib.lib()
    s = Setup(dev)
    res = {}
    bank_new, bank_chain = s.bank(), s.bank()
    new, chain = make_paths(s, bank_new, bank_chain, res)
    if args.calls:
        fn = new if args.path == "new" else chain
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        print("%d calls of the %s path" % (args.calls, args.path))
        return

    # ---- the same values first, with given draws; two calls: first sight, then the moving average
    lines = ["FasaBBoxHead.loss, LVIS head shape: %d rows (one in four padded, %d positive over %d classes), D = %d, %d channels, epoch 1, fp32, %s"
             % (N, int(((s.labels >= 0) & (s.labels < C)).sum()), len(torch.unique(s.labels)) - 1, D, C + 1, torch.cuda.get_device_name(0)),
             "%d rounds, the variants alternating; new / chain_*: host clock around %d forward + backward calls and a synchronise; the others: "
             "median of %d event pairs around %d calls (warm) or around one call behind a 512 MB fill (cold); microseconds per call: "
             "median over the rounds [min .. max]" % (ROUNDS, INNER, ITERS, K)]
    for call in range(2):
        new(s.rand, s.normal)
        a = tuple(t.clone() if torch.is_tensor(t) else {k: v.detach().clone() for k, v in t.items()} for t in res["new"])
        chain(s.rand, s.normal)
        b = res["chain"]
        torch.cuda.synchronize()
        same_bank = all(torch.equal(p.data.view(torch.int32), q.data.view(torch.int32)) for p, q in
                        ((bank_new.feature_mean, bank_chain.feature_mean), (bank_new.feature_std, bank_chain.feature_std),
                         (bank_new.feature_used, bank_chain.feature_used)))
        rel = lambda u, v: float((u - v).abs().max() / v.abs().max().clamp_min(1e-30))      # noqa: E731
        lines.append("call %d: loss_cls new %.7g chain %.7g, loss_bbox new %.7g chain %.7g; banks bit-equal: %s (%d classes in use); "
                     "gradient max diff of the largest element: scores %.1e, bbox_pred %.1e, fc_cls %.1e"
                     % (call, float(a[0]["loss_cls"]), float(b[0]["loss_cls"]), float(a[0]["loss_bbox"]), float(b[0]["loss_bbox"]), same_bank,
                        int(bank_new.feature_used.sum()), rel(a[1], b[1]), rel(a[2], b[2]), rel(a[3], b[3])))
        assert same_bank
        assert abs(float(a[0]["loss_cls"]) - float(b[0]["loss_cls"])) <= 1e-5 * abs(float(b[0]["loss_cls"]))
        assert abs(float(a[0]["loss_bbox"]) - float(b[0]["loss_bbox"])) <= 1e-5 * abs(float(b[0]["loss_bbox"]))
        assert rel(a[1], b[1]) <= 1e-5 and rel(a[2], b[2]) <= 1e-5 and rel(a[3], b[3]) <= 1e-4
    e, l, wts, cnt = bank_new.fa_generate_padded(s.rand, s.normal)
    lines.append("virtual rows with the given draws: %d of %d padded rows" % (int(cnt), e.shape[0]))

    # ---- the launches alone
    pos = (s.labels >= 0) & (s.labels < C)
    pe, pl = s.emb[pos].contiguous(), s.labels[pos].contiguous()
    bank_k = s.bank()
    bank_k.fa_update(pe, pl)
    present = torch.zeros(C, dtype=torch.int32, device=dev)
    out = torch.empty(C, D, device=dev)
    out_l = torch.empty(C, dtype=torch.int64, device=dev)
    out_w = torch.empty(C, device=dev)
    slots = torch.zeros(C, dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr()
    fm, fv, fu, pr = (_lib.ptr(t.data) for t in (bank_k.feature_mean, bank_k.feature_std, bank_k.feature_used, bank_k.prob_list))

    def upd_rows():
        lib.iif_fasa_update_rows(_lib.ptr(s.emb), _lib.ptr(s.labels), N, D, D, C, 0.1, fm, fv, fu, _lib.ptr(present), stream)

    def upd_old():
        lib.iif_fasa_update(_lib.ptr(pe), _lib.ptr(pl), pe.shape[0], D, D, C, 0.1, fm, fv, fu, stream)

    def gen_pad():
        lib.iif_fasa_generate_padded(_lib.ptr(s.rand), pr, fu, fm, fv, _lib.ptr(s.normal), C, D, C, 0.1, _lib.ptr(out), _lib.ptr(out_l),
                                     _lib.ptr(out_w), _lib.ptr(count), stream)

    def gen_old():
        lib.iif_fasa_generate(_lib.ptr(s.rand), pr, fu, fm, fv, _lib.ptr(s.normal), C, D, _lib.ptr(slots), _lib.ptr(count), _lib.ptr(out),
                              _lib.ptr(out_l), stream)

    variants = [("new", new, host_round), ("chain_a", chain, host_round), ("chain_b", chain, host_round)]
    for name, fn in (("upd_rows", upd_rows), ("upd_old", upd_old), ("gen_pad", gen_pad), ("gen_old", gen_old)):
        variants += [(name, fn, event_round), (name + "_cold", fn, cold_round)]
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
        lines.append("    %-13s %9.1f  [%9.1f .. %9.1f]" % (name, med[name], min(t[name]), max(t[name])))
    fast = min(med["chain_a"], med["chain_b"])
    spread = max(abs(med["chain_a"] - med["chain_b"]),
                 max(max(t["chain_a"]) - min(t["chain_a"]), max(t["chain_b"]) - min(t["chain_b"])))
    lines.append("    faster chain median / new: %.2fx (%.1f us less per call; the chain's two medians differ by %.1f us, its rounds range "
                 "over %.1f us): %s" % (fast / med["new"], fast - med["new"], abs(med["chain_a"] - med["chain_b"]), spread,
                                        "new is below the chain by more than the chain's spread" if fast - med["new"] > spread
                                        else "NOT below the chain by more than the chain's spread"))
    lines.append("    update: rows / old %.2fx its time warm, %.2fx cold; generate: padded / old %.2fx warm, %.2fx cold"
                 % (med["upd_rows"] / med["upd_old"], med["upd_rows_cold"] / med["upd_old_cold"], med["gen_pad"] / med["gen_old"],
                    med["gen_pad_cold"] / med["gen_old_cold"]))
    lines.append("    operations enqueued forward by the new path, by construction (mmdet_fasa_head_loss.ENQUEUED_TRAIN): %d, whatever the "
                 "data holds; the chain's number depends on the draw (no aug rows: five fewer)" % ENQUEUED_TRAIN)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
