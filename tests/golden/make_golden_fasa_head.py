#!/usr/bin/env python3
"""Generate tests/golden/g37_fasa_head.npz by RUNNING THE REFERENCE's ConvFCFASABBoxHead.loss with its own FasaIIFLoss and
L1Loss on the CPU, in float32 and in float64.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fasa_head.py

The placeholder-module loader is make_golden_mmdet.py's (imported, unchanged): the reference's files are executed from where
they lie, ``ConvFCBBoxHead`` is the stand-in that records num_classes / cls_last_dim, 'cuda' means the CPU while the
reference's code runs.  On the head the attributes ``loss`` reads are set by hand: loss_cls, loss_bbox, fc_cls, with_cls,
custom_activation, reg_class_agnostic, reg_decoded_bbox, epoch, training.  ``torch.rand`` and ``torch.normal`` are wrapped
while ``loss`` runs so that the draws fa_generate consumes are recorded (the wrappers call the real functions).

The sequence and the inputs are tests/fasa_head_cases.py's.  The fixture holds the reference's outputs after every call (each
loss key, the accuracy on the rows that count, the bank state at the classes in use, the accumulators), the recorded
rand [STEPS, C] and the recorded normals of the selected classes - no inputs, and nothing of the reference's program text.
The generator asserts that the float32 and float64 restatements of the cases file reproduce the two runs.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_golden_mmdet as mg                       # noqa: E402  (the loader; its module-level code sets the placeholders up)
from tests import fasa_head_cases as fc              # noqa: E402

REF = mg.REF
SL = mg._load("mmdet.models.losses.smooth_l1_loss", "mmdet/models/losses/smooth_l1_loss.py")


class _Recorder:
    """torch.rand / torch.normal with their results kept."""

    def __enter__(self):
        self.rand, self.normal = [], []
        self._rand, self._normal = torch.rand, torch.normal

        def rand(*a, **k):
            r = self._rand(*a, **k)
            self.rand.append(r.clone())
            return r

        def normal(*a, **k):
            r = self._normal(*a, **k)
            self.normal.append(r.clone())
            return r
        torch.rand, torch.normal = rand, normal
        return self

    def __exit__(self, *exc):
        torch.rand, torch.normal = self._rand, self._normal


def run(dtype):
    with mg._cuda_is_cpu():
        head = REF["fh"].ConvFCFASABBoxHead(num_classes=fc.C, cls_last_dim=fc.D, fasa_cfg=dict(fc.CFG))
        crit = REF["fiif"].FasaIIFLoss(num_classes=fc.C, path=mg.LVIS_CSV, variant="raw", loss_weight=fc.CLS_LOSS_WEIGHT)
    assert np.array_equal(head.instance_count_list.numpy(), fc.instance_counts())
    assert torch.equal(head.prob_list.data, fc.prob_list())
    assert torch.equal(crit.iif_weights, fc.table())
    lin = nn.Linear(fc.D, fc.C1)
    w, b = fc.fc_cls_params()
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    head.loss_cls, head.loss_bbox, head.fc_cls, head.with_cls = crit, SL.L1Loss(loss_weight=fc.BBOX_LOSS_WEIGHT), lin, True
    head.custom_activation, head.reg_class_agnostic, head.reg_decoded_bbox = True, True, False
    head.epoch = fc.EPOCH
    head.to(dtype)                                   # the bank, the probabilities (float32 values) and fc_cls
    out, rands = {}, []

    def call(i, tag, embedding):
        args = [i[k].to(dtype) for k in ("cls_score", "bbox_pred")]
        torch.manual_seed(9100 + len(rands))
        with mg._cuda_is_cpu(), _Recorder() as rec:
            losses = head.loss(args[0], args[1], None, i["labels"], i["label_weights"].to(dtype), i["bbox_targets"].to(dtype),
                               i["bbox_weights"].to(dtype), embedding=embedding)
        assert set(losses) == {"loss_bbox", "loss_cls", "acc_classes"}, sorted(losses)
        for k, v in losses.items():
            out["%s_%s" % (tag, k)] = v.detach().numpy().copy()
        out[tag + "_acc_valid"] = fc.accuracy_valid(i["cls_score"], i["labels"], i["label_weights"]).numpy()
        return rec

    head.train()
    for step in range(fc.STEPS):
        i = fc.step_inputs(step)
        rec = call(i, "s%d" % step, i["embedding"].to(dtype))
        assert len(rec.rand) == 1 and tuple(rec.rand[0].shape) == (fc.C,)
        rands.append(rec.rand[0])
        # the classes fa_generate drew, in its order: selected and in use (:152-159)
        drawn = [int(c) for c in torch.where(rec.rand[0] < head.prob_list.data)[0] if head.feature_used.data[int(c)] > 0]
        assert len(rec.normal) == len(drawn)
        out["s%d_aug_labels" % step] = np.array(drawn, dtype=np.int64)
        out["s%d_aug_normals" % step] = (torch.stack(rec.normal).float().numpy() if drawn else np.zeros((0, fc.D), np.float32))
        used = torch.nonzero(head.feature_used.data > 0).reshape(-1)
        out["s%d_used" % step] = used.numpy()
        out["s%d_mean" % step] = head.feature_mean.data[used].numpy().copy()
        out["s%d_var" % step] = head.feature_std.data[used].numpy().copy()
    head.eval()
    with mg._cuda_is_cpu():
        crit.open_cums()
    crit.cum_losses = crit.cum_losses.to(dtype)      # the accumulator in the run's own precision
    i = fc.step_inputs(fc.STEPS)
    rec = call(i, "val", None)
    assert not rec.rand and not rec.normal
    out["val_cum_losses"] = crit.cum_losses.detach().numpy().copy()
    out["val_cum_labels"] = crit.cum_labels.detach().numpy().copy()
    out["rand"] = torch.stack(rands).numpy()
    return out


def main():
    r32, r64 = run(torch.float32), run(torch.float64)
    assert np.array_equal(r32["rand"], r64["rand"])
    out = {"rand": r32["rand"]}
    n_aug = []
    for s in range(fc.STEPS):
        for k in ("aug_labels", "aug_normals", "used"):
            assert np.array_equal(r32["s%d_%s" % (s, k)], r64["s%d_%s" % (s, k)]), (s, k)
            out["s%d_%s" % (s, k)] = r32["s%d_%s" % (s, k)]
        n_aug.append(len(out["s%d_aug_labels" % s]))
        used = set(out["s%d_used" % s].tolist())
        assert len(used - set(out["s%d_aug_labels" % s].tolist())) >= 1, "every class in use was drawn: nothing pins the selection"
    assert min(n_aug) >= 3, n_aug
    labels = [fc.step_inputs(s)["labels"] for s in range(fc.STEPS)]
    pos = [set(l[(l >= 0) & (l < fc.C)].tolist()) for l in labels]
    assert not pos[1] and len(pos[0] & pos[2]) >= 4 and len(pos[2] - pos[0]) >= 4      # no positives; revisited and new classes
    assert np.array_equal(out["s0_used"], out["s1_used"])
    for key in sorted(r32):
        if key == "rand" or key.endswith(("aug_labels", "aug_normals", "used")):
            continue
        if key.endswith(("acc_valid", "cum_labels")):
            assert np.array_equal(r32[key], r64[key].astype(np.float32)), key
            out[key] = r32[key].astype(np.float32)
            continue
        if key.endswith("acc_classes"):
            out[key] = r32[key].astype(np.float32)
            continue
        out[key + "32"], out[key + "64"] = r32[key].astype(np.float32), r64[key].astype(np.float64)
    # the restatements of the cases file against the two runs
    draws = fc.fixture_draws(out)
    worst = 0.0
    for dtype, run_, tol in ((torch.float32, r32, 2.0 ** -23), (torch.float64, r64, 1e-12)):
        rs = fc.restate(dtype, *draws)
        for key, v in rs.items():
            if key.endswith(("aug_emb", "loss_main")):
                continue
            want = np.asarray(run_[key], dtype=np.float64)
            got = np.asarray(v, dtype=np.float64)
            assert got.shape == want.shape, (key, got.shape, want.shape)
            if key.endswith(("used", "aug_labels", "acc_valid", "cum_labels")):
                assert np.array_equal(got, want), key
                continue
            err = np.abs(got - want)
            assert (err <= tol * np.abs(want)).all(), (str(dtype), key, float(err.max()))
            if want.size and np.abs(want).max() > 0:
                worst = max(worst, float((err / np.maximum(np.abs(want), 1e-300)).max())) if dtype == torch.float32 else worst
    path = os.path.join(HERE, "g37_fasa_head.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %.1f KB; virtual rows per step %s; float32 restatement within %.2e of the float32 run"
          % (path, len(out), os.path.getsize(path) / 1024.0, n_aug, worst))


if __name__ == "__main__":
    main()
