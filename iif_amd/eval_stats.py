"""Evaluation statistics on the device: top-k accuracy, the many / median / low-shot split of
``per_shot_acc.shot_acc`` and the reliability bins of ``calibration.compute_calibration``, from one
launch of ``iif_eval_accumulate`` per batch into one int64 buffer.  The host reads that buffer once,
in ``result()``; ``synchronize_between_processes()`` is one all-reduce of it.

    acc = EvalAccumulator(num_classes, topk=(1, 5), num_bins=10)
    for image, target in loader:
        acc.update(model(image), target)
    acc.synchronize_between_processes()
    r = acc.result(train_targets=dataset.targets)
"""
import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .calibration import summarise

MAX_TOPK = 4
MAX_BINS = 256
_CONF_ONE = float(2 ** 32)          # bin_conf holds llrint(conf * 2^32)


class EvalAccumulator(object):
    """Counts of one evaluation; ``table`` ([C] or [1, C]) scales the logits as IIFLoss(..., infer=True) does,
    without materialising the product.  ``num_bins=0`` turns calibration off (the bins are still
    accumulated into one unused bin).  ``keep_rows`` also keeps each batch's predictions and confidences."""

    def __init__(self, num_classes, topk=(1, 5), num_bins=10, table=None, device="cuda", keep_rows=False):
        C = int(num_classes)
        if C <= 0:
            raise ValueError("num_classes must be positive, got %d" % C)
        ks = tuple(min(int(k), C) for k in topk)
        if not 1 <= len(ks) <= MAX_TOPK or min(ks) < 1:
            raise ValueError("topk takes 1 to %d values >= 1, got %r" % (MAX_TOPK, tuple(topk)))
        nb = int(num_bins)
        if not 0 <= nb <= MAX_BINS:
            raise ValueError("num_bins must be in [0, %d], got %d" % (MAX_BINS, nb))
        if table is not None:
            table = torch.as_tensor(table)
            if table.numel() != C:
                raise ValueError("IIF table has %d classes, the accumulator %d" % (table.numel(), C))
        self.num_classes, self.topk, self.num_bins, self.keep_rows = C, ks, nb, keep_rows
        self.device = torch.device(device)
        self.bins = np.linspace(0.0, 1.0, max(nb, 1) + 1)
        self._k = torch.tensor(ks, dtype=torch.int32)
        self.table = None if table is None else table.reshape(-1).to(self.device, torch.float32).contiguous()
        self._edges = torch.tensor(self.bins, dtype=torch.float64, device=self.device)
        self.acc = torch.zeros(self.size(C, len(ks), max(nb, 1)), dtype=torch.int64, device=self.device)
        self.preds, self.confs, self.targets = [], [], []

    @staticmethod
    def size(C, nk, nb):
        return 2 + nk + 2 * C + 3 * nb

    def reset(self):
        self.acc.zero_()
        self.preds, self.confs, self.targets = [], [], []

    def update(self, output, target):
        """One launch over ``output`` [B, C] (fp32 / bf16, rows may be strided) and ``target`` [B]; no host sync."""
        _lib.require_gpu(output, target, self.acc)
        x = output.detach()
        if x.dim() != 2 or x.shape[1] != self.num_classes:
            raise ValueError("logits must be [B, %d], got %s" % (self.num_classes, tuple(x.shape)))
        if x.stride(-1) != 1:
            x = x.contiguous()
        B, C = x.shape
        tgt = target.detach().reshape(-1).to(torch.int64).contiguous()
        if tgt.numel() != B:
            raise ValueError("%d targets for %d rows" % (tgt.numel(), B))
        pred = conf = None
        if self.keep_rows:
            pred = torch.empty(B, dtype=torch.int64, device=x.device)
            conf = torch.empty(B, dtype=torch.float32, device=x.device)
        rc = _lib.lib().iif_eval_accumulate(_lib.ptr(x), _lib.dtype_code(x), x.stride(0) if B else C, _lib.ptr(self.table),
                                            _lib.ptr(tgt), B, C, self._k.data_ptr(), len(self.topk), _lib.ptr(self._edges),
                                            len(self.bins) - 1, _lib.ptr(self.acc), _lib.ptr(pred), _lib.ptr(conf),
                                            _lib.stream_ptr())
        _lib.check(rc, "iif_eval_accumulate")
        if self.keep_rows:
            self.preds.append(pred)
            self.confs.append(conf)
            self.targets.append(tgt)

    def synchronize_between_processes(self):
        """Sum ``acc`` over the ranks (one all-reduce; over gloo through a host copy)."""
        if not (dist.is_available() and dist.is_initialized()):
            return
        if dist.get_backend() == "nccl":
            dist.all_reduce(self.acc)
        else:
            host = self.acc.cpu()
            dist.all_reduce(host)
            self.acc.copy_(host)

    def counts(self):
        """The buffer on the host (one device-to-host copy)."""
        return self.acc.cpu().numpy()

    def rows(self):
        """(preds, confidences, targets) of every update so far as numpy arrays (``keep_rows`` only)."""
        if not self.keep_rows:
            raise RuntimeError("EvalAccumulator(keep_rows=True) keeps the per-row outputs")
        cat = (lambda v, dt: torch.cat(v).cpu().numpy() if v else np.zeros(0, dt))
        return cat(self.preds, np.int64), cat(self.confs, np.float32), cat(self.targets, np.int64)

    def result(self, train_targets=None, many_shot_thr=100, low_shot_thr=20):
        return counts_to_result(self.counts(), self.num_classes, self.topk, len(self.bins) - 1,
                                train_targets=train_targets, many_shot_thr=many_shot_thr, low_shot_thr=low_shot_thr,
                                calibration=self.num_bins > 0)


def split_counts(acc, C, nk, nb):
    """The named parts of the ``iif_eval_accumulate`` buffer."""
    acc = np.asarray(acc, dtype=np.int64)
    if acc.shape != (EvalAccumulator.size(C, nk, nb),):
        raise ValueError("buffer of %d values, expected %d" % (acc.size, EvalAccumulator.size(C, nk, nb)))
    o = 2 + nk
    return {"rows": int(acc[0]), "out_of_range": int(acc[1]), "hits": acc[2:o], "n_test": acc[o:o + C],
            "n_hit": acc[o + C:o + 2 * C], "bin_count": acc[o + 2 * C:o + 2 * C + nb],
            "bin_hit": acc[o + 2 * C + nb:o + 2 * C + 2 * nb], "bin_conf": acc[o + 2 * C + 2 * nb:]}


def shot_split(n_test, n_hit, train_targets, many_shot_thr=100, low_shot_thr=20):
    """``shot_acc`` from per-class counts: the same float64 operations on the same classes in the same order, so the
    triple is bit-equal to ``shot_acc(preds, labels, train_targets)``."""
    seen = np.asarray(train_targets.detach().cpu().numpy() if isinstance(train_targets, torch.Tensor) else train_targets)
    seen = seen.astype(np.int64).reshape(-1)
    C = len(n_test)
    n_train = np.bincount(seen, minlength=C)[:C]
    present = n_test > 0
    acc = n_hit[present] / n_test[present]
    freq = n_train[present]
    splits = (freq > many_shot_thr, (freq <= many_shot_thr) & (freq >= low_shot_thr), freq < low_shot_thr)
    return tuple(acc[sel].mean() if sel.any() else np.float64(0) for sel in splits)


def calibration_from_counts(bin_count, bin_hit, bin_conf, bins):
    """``compute_calibration``'s dictionary from the bin counts (the confidence sums in units of 2^-32)."""
    counts = np.asarray(bin_count, dtype=np.int64)
    nz = counts > 0
    accs = np.zeros(len(counts), dtype=np.float64)
    confs = np.zeros(len(counts), dtype=np.float64)
    accs[nz] = np.asarray(bin_hit)[nz] / counts[nz]
    confs[nz] = np.asarray(bin_conf)[nz] / _CONF_ONE / counts[nz]
    return summarise(accs, confs, counts, np.asarray(bins, dtype=np.float64))


def counts_to_result(acc, C, topk, nb, train_targets=None, many_shot_thr=100, low_shot_thr=20, calibration=True):
    """Counts -> {"rows", "out_of_range", "topk": {k: percent}, "shot": (many, median, low) or None,
    "calibration": compute_calibration's dict or None}."""
    p = split_counts(acc, C, len(topk), nb)
    rows = p["rows"]
    out = {"rows": rows, "out_of_range": p["out_of_range"],
           "topk": {k: (100.0 * int(h) / rows if rows else 0.0) for k, h in zip(topk, p["hits"])},
           "shot": None, "calibration": None}
    if train_targets is not None:
        if p["out_of_range"]:
            raise ValueError("%d targets outside [0, %d): their classes have no slot, the shot split is undefined"
                             % (p["out_of_range"], C))
        out["shot"] = shot_split(p["n_test"], p["n_hit"], train_targets, many_shot_thr, low_shot_thr)
    if calibration:
        out["calibration"] = calibration_from_counts(p["bin_count"], p["bin_hit"], p["bin_conf"], np.linspace(0.0, 1.0, nb + 1))
    return out
