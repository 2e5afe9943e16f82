#!/usr/bin/env python3
"""Generate tests/golden/g38_head_loss_kinds.npz by RUNNING THE REFERENCE's BBoxHead.loss on the CPU, in float32 and in
float64, with its own CrossEntropyLoss(use_sigmoid=True) and its own SeesawLoss.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_head_loss_kinds.py <reference checkout>

``instance_segmentation/mmdet/models/losses/{utils,accuracy,cross_entropy_loss,seesaw_loss}.py`` and
``roi_heads/bbox_heads/bbox_head.py`` are imported as they are, under the placeholder mmcv / mmdet modules of
make_golden_bbox_head_loss.py; ``BBoxHead.loss`` is called unbound on a ``SimpleNamespace`` with the attributes it reads.
Nothing from the reference is written to the repository except inputs' sums and outputs (data).

The contract of the native kinds has two parts (tests/head_loss_kinds_cases.py): without rows of weight zero the result is
BBoxHead.loss's; with them it is BBoxHead.loss's on the batch WITHOUT those rows.  So the reference runs on the compacted
rows (and its gradient is scattered back to the rows it came from); on a padded case it runs once more on the padded batch,
to record the accuracy it dilutes and the cum_samples it inflates.  A batch whose every weight is zero has no rows left:
the reference returns no classification key for an empty cls_score, and the fixture records zeros.

Per case (g36's layout): the losses of the float32 and of the float64 run; avg_factor (recomputed the reference's way); the
reference's accuracies on the compacted rows, on the rows with weight > 0 (the rows the native accuracy counts - they
differ from the compacted rows only by rows of negative weight) and on the padded batch; the float32 and float64 gradient
at the rows and columns head_loss_kinds_cases.kept() lists; the largest gradient element and the largest
float32-vs-float64 gradient difference over the WHOLE tensor; for Seesaw, cum_samples after the call (compacted and
padded).  The generator asserts that the float64 restatement of the cases file reproduces the float64 run (losses and the
whole gradient to 1e-12; accuracies, avg_factor and cum_samples exactly).
"""
import contextlib
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import head_loss_kinds_cases as kc          # noqa: E402

torch.set_num_threads(8)


def _identity_decorator(*a, **kw):
    if len(a) == 1 and callable(a[0]) and not kw:
        return a[0]
    return lambda f: f


class _Registry:
    def register_module(self, name=None, force=False, module=None):
        if module is not None:
            return module
        return lambda cls: cls


def _pkg(name, path=None, **names):
    m = types.ModuleType(name)
    m.__path__ = [path] if path else []
    for k, v in names.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


@contextlib.contextmanager
def _float_means(dtype):
    """The reference casts targets and weights with ``.float()`` (cross_entropy_loss.py:104-106, seesaw_loss.py:52-73), and
    torch gives the loss of a float32 target in float32 whatever the scores are: during the float64 run ``.float()`` means
    float64, so that the run is float64 throughout (make_golden_bbox_head_loss.py does the same for 'cuda')."""
    real = torch.Tensor.float
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.Tensor.float = real


def reference_classes(ref_root):
    models = os.path.join(ref_root, "instance_segmentation", "mmdet", "models")
    _pkg("mmcv", jit=_identity_decorator)
    _pkg("mmcv.runner", BaseModule=nn.Module, auto_fp16=_identity_decorator, force_fp32=_identity_decorator)
    _pkg("mmdet")
    _pkg("mmdet.core", build_bbox_coder=None, multi_apply=None, multiclass_nms=None)
    _pkg("mmdet.models")
    _pkg("mmdet.models.builder", LOSSES=_Registry(), HEADS=_Registry(), build_loss=None)
    _pkg("mmdet.models.utils", build_linear_layer=None)
    losses = _pkg("mmdet.models.losses", os.path.join(models, "losses"))
    acc = importlib.import_module("mmdet.models.losses.accuracy")
    ce = importlib.import_module("mmdet.models.losses.cross_entropy_loss")
    ss = importlib.import_module("mmdet.models.losses.seesaw_loss")
    losses.accuracy = acc.accuracy                         # what `from mmdet.models.losses import accuracy` must find
    spec = importlib.util.spec_from_file_location("ref_bbox_head", os.path.join(models, "roi_heads", "bbox_heads", "bbox_head.py"))
    bh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bh)
    return ce.CrossEntropyLoss, ss.SeesawLoss, bh.BBoxHead, acc.accuracy


def main():
    CrossEntropyLoss, SeesawLoss, BBoxHead, accuracy = reference_classes(sys.argv[1])

    def loss_module(name, dtype):
        c = kc.CASES[name]
        if c["kind"] == "sig":
            cw = kc.class_weight(name)
            return CrossEntropyLoss(use_sigmoid=True, loss_weight=c["lw"], ignore_index=c["ignore"],
                                    class_weight=None if cw is None else cw.tolist())
        m = SeesawLoss(p=c["p"], q=c["q"], num_classes=c["C"], eps=kc.EPS, loss_weight=c["lw"])
        m.cum_samples = torch.from_numpy(kc.cum_before(name)).to(dtype)      # (the buffer of the float64 run is float64 too)
        return m

    def run(name, x, labels, w, dtype):
        """BBoxHead.loss on these rows: dict of arrays (losses, accuracies, gradient, cum_samples)."""
        c = kc.CASES[name]
        crit = loss_module(name, dtype)
        head = types.SimpleNamespace(loss_cls=crit, custom_activation=getattr(crit, "custom_activation", False),
                                     num_classes=c["C"], reg_decoded_bbox=False, reg_class_agnostic=False, loss_bbox=None)
        xs = torch.from_numpy(x).to(dtype).requires_grad_(True)
        see = c["kind"] == "see"
        with _float_means(dtype):
            losses = BBoxHead.loss(head, xs, None, None, torch.from_numpy(labels), torch.from_numpy(w).to(dtype), None, None)
            if x.shape[0]:
                sum(losses[k] for k in losses if k.startswith("loss")).backward()
        cum = crit.cum_samples.numpy().astype(np.float32) if see else None
        if x.shape[0] == 0:
            assert losses == {}, (name, sorted(losses))
            z, z1 = np.zeros(()), np.zeros(1, dtype=np.float32)
            k = 2 if see else 1
            return dict(loss=(z,) * k, acc=(z1,) * k, grad=np.zeros(x.shape), cum=cum)
        if see:
            assert set(losses) == {"loss_cls_classes", "loss_cls_objectness", "acc_classes", "acc_objectness"}, sorted(losses)
            ls = (losses["loss_cls_classes"], losses["loss_cls_objectness"])
            ac = (losses["acc_classes"], losses["acc_objectness"])
        else:
            assert set(losses) == {"loss_cls", "acc"}, sorted(losses)
            ls, ac = (losses["loss_cls"],), (losses["acc"],)
        return dict(loss=tuple(v.detach().numpy() for v in ls), acc=tuple(v.detach().numpy().reshape(-1).astype(np.float32) for v in ac),
                    grad=xs.grad.numpy() if xs.grad is not None else np.zeros(x.shape), cum=cum)

    out = dict(kc.input_sums())
    worst = {"loss": 0.0, "grad": 0.0, "restate_loss": 0.0, "restate_grad": 0.0}
    for name, c in kc.CASES.items():
        x, labels, w = kc.inputs(name)
        see = c["kind"] == "see"
        keep = w != 0
        res = {}
        for dtype in (torch.float32, torch.float64):
            r = run(name, x[keep], labels[keep], w[keep], dtype)
            full = np.zeros(x.shape, dtype=r["grad"].dtype)
            full[keep] = r["grad"]
            r["grad"] = full
            res[dtype] = r
        r32, r64 = res[torch.float32], res[torch.float64]
        wt = torch.from_numpy(w)
        avg = max(torch.sum(wt > 0).float().item(), 1.)
        cnt = w > 0
        # the reference's accuracy on the rows that count, and on the padded batch
        padded = run(name, x, labels, w, torch.float32)
        valid = run(name, x[cnt], labels[cnt], w[cnt], torch.float32)["acc"]
        rs = kc.restate_case(name)
        want = (rs["loss_cls"], rs["loss_obj"]) if see else (rs["loss"],)
        racc = (rs["acc_cls"], rs["acc_obj"]) if see else (rs["acc"],)
        gmax = float(np.abs(r64["grad"]).max())
        e_l = max(abs(a - float(b)) / max(abs(float(b)), 1e-300) if float(b) else abs(a) for a, b in zip(want, r64["loss"]))
        e_g = float(np.abs(rs["grad"] - r64["grad"]).max()) / gmax if gmax else float(np.abs(rs["grad"]).max())
        assert e_l <= 1e-12 and e_g <= 1e-12, (name, e_l, e_g)
        assert rs["avg"] == avg, (name, rs["avg"], avg)
        for a, b in zip(racc, valid):
            assert np.array_equal(a, b), (name, a, b)
        if not (w < 0).any():
            for a, b in zip(valid, r32["acc"]):
                assert np.array_equal(a, b), name
        if see:
            assert np.array_equal(rs["cum"], r32["cum"]) and np.array_equal(r32["cum"], r64["cum"]), name
            assert np.array_equal(rs["cum"], kc.cum_after(name)), name
        worst["restate_loss"], worst["restate_grad"] = max(worst["restate_loss"], e_l), max(worst["restate_grad"], e_g)
        e32_g = float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())
        for a, b in zip(r32["loss"], r64["loss"]):
            if float(b):
                worst["loss"] = max(worst["loss"], abs(float(a) - float(b)) / abs(float(b)))
        if gmax:
            worst["grad"] = max(worst["grad"], e32_g / gmax)
        rows, cols = kc.kept(name)
        out[name + "_loss32"] = np.array([float(v) for v in r32["loss"]], dtype=np.float32)
        out[name + "_loss64"] = np.array([float(v) for v in r64["loss"]], dtype=np.float64)
        out[name + "_avg"] = np.float32(avg)
        out[name + "_acc_compact"] = np.concatenate(r32["acc"])
        out[name + "_acc_valid"] = np.concatenate(valid)
        out[name + "_acc_padded"] = np.concatenate(padded["acc"])
        out[name + "_grad32"] = r32["grad"][np.ix_(rows, cols)].astype(np.float32)
        out[name + "_grad64"] = r64["grad"][np.ix_(rows, cols)]
        out[name + "_gmax64"] = np.float64(gmax)
        out[name + "_e32_grad"] = np.float64(e32_g)
        if see:
            out[name + "_cum"] = r32["cum"].astype(np.float32)
            out[name + "_cum_padded"] = padded["cum"].astype(np.float32)
    out["worst"] = np.array([worst["loss"], worst["grad"], worst["restate_loss"], worst["restate_grad"]])
    path = os.path.join(HERE, "g38_head_loss_kinds.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d cases, %.1f KB; float32 run vs float64 run: loss %.2e, gradient %.2e (of the largest element); "
          "float64 restatement vs float64 run: loss %.2e, gradient %.2e"
          % (path, len(kc.CASES), os.path.getsize(path) / 1024.0, worst["loss"], worst["grad"], worst["restate_loss"], worst["restate_grad"]))


if __name__ == "__main__":
    main()
