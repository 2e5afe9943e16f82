#!/usr/bin/env python3
"""Generate tests/golden/g36_bbox_head_loss.npz by RUNNING THE REFERENCE's BBoxHead.loss on the CPU, in float32 and in float64,
with its own IIFLoss and CrossEntropyLoss (and, for the case with both halves, its L1Loss).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bbox_head_loss.py <reference checkout>

``instance_segmentation/mmdet/models/losses/{utils,accuracy,cross_entropy_loss,iif_loss,smooth_l1_loss}.py`` and
``roi_heads/bbox_heads/bbox_head.py`` are imported as they are.  mmcv / mmdet are not needed: the process gets placeholder
modules, the way make_golden_bbox_reg.py does (``mmcv.jit`` / ``force_fp32`` / ``auto_fp16`` as the identity decorator, a
registry whose ``register_module`` returns the class, ``BaseModule = nn.Module``, the names ``bbox_head.py`` imports).
``IIFLoss`` hard-codes ``device='cuda'`` for its table (iif_loss.py:50); while it is constructed 'cuda' means the CPU.  Its
table comes from ``lvis_files/idf_1204.csv`` (C = 1204) or from a synthetic one-column CSV written to a temporary directory
from tests/bbox_head_loss_cases.py (every other C).  ``BBoxHead.loss`` is called unbound on a ``SimpleNamespace`` with the
attributes it reads.  Nothing from the reference is written to the repository except inputs' sums and outputs (data).

Per case the fixture keeps: the loss of the float32 and of the float64 run; avg_factor (recomputed the reference's way);
the reference's accuracy over all rows (what BBoxHead.loss returns) and ``accuracy`` on the rows with weight > 0 (the
padded-row semantics); the float32 and float64 gradient at the rows and columns bbox_head_loss_cases.kept() lists and at
each kept row's label column; the largest gradient element and the largest float32-vs-float64 gradient difference over the
WHOLE tensor.  The generator asserts that the float64 restatement of the cases file reproduces the float64 run (loss and
the whole gradient to 1e-12, accuracy and avg_factor exactly), so the tests may use the restatement for the elements the
fixture leaves out.
"""
import contextlib
import importlib
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import bbox_head_loss_cases as hc          # noqa: E402

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
def _cuda_is_cpu():
    real = torch.tensor

    def tensor(*a, **k):
        if str(k.get("device", "")).startswith("cuda"):
            k["device"] = "cpu"
        return real(*a, **k)
    torch.tensor = tensor
    try:
        yield
    finally:
        torch.tensor = real


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
    iif = importlib.import_module("mmdet.models.losses.iif_loss")
    sl = importlib.import_module("mmdet.models.losses.smooth_l1_loss")
    losses.accuracy = acc.accuracy                         # what `from mmdet.models.losses import accuracy` must find
    spec = importlib.util.spec_from_file_location("ref_bbox_head", os.path.join(models, "roi_heads", "bbox_heads", "bbox_head.py"))
    bh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bh)
    return iif.IIFLoss, ce.CrossEntropyLoss, sl.L1Loss, bh.BBoxHead, acc.accuracy


def main():
    ref_root = sys.argv[1]
    IIFLoss, CrossEntropyLoss, L1Loss, BBoxHead, accuracy = reference_classes(ref_root)
    lvis_csv = os.path.join(ref_root, "instance_segmentation", "lvis_files", "idf_1204.csv")
    tmp = tempfile.TemporaryDirectory()

    def loss_module(name):
        N, C, kind, bf, pad, cwf, lw, ignore, neg = hc.CASES[name]
        cw = hc.class_weight(name)
        kw = dict(loss_weight=lw, ignore_index=ignore, class_weight=None if cw is None else cw.tolist())
        if kind == "ce":
            return CrossEntropyLoss(**kw)
        if C == 1204:
            path = lvis_csv
        else:
            path = os.path.join(tmp.name, name + ".csv")
            with open(path, "w") as f:                       # the first data row is the placeholder iif_loss.py:49 drops
                f.write("raw\n1.0\n" + "".join("%r\n" % float(v) for v in hc.table(name)[:-1]))
        with _cuda_is_cpu():
            m = IIFLoss(num_classes=C - 1, path=path, **kw)
        assert np.array_equal(m.iif_weights.numpy().reshape(-1), hc.table(name)), name
        return m

    out = dict(hc.input_sums())
    worst = {"loss": 0.0, "grad": 0.0, "restate_loss": 0.0, "restate_grad": 0.0}
    for name, (N, C, kind, bf, pad, cwf, lw, ignore, neg) in hc.CASES.items():
        x, labels, w = hc.inputs(name)
        both = name == hc.BOTH
        res = {}
        for dtype in (torch.float32, torch.float64):
            crit = loss_module(name)
            head = types.SimpleNamespace(loss_cls=crit, custom_activation=getattr(crit, "custom_activation", False),
                                         num_classes=hc.BBOX_CLASSES if both else C - 1, reg_decoded_bbox=False,
                                         reg_class_agnostic=False, loss_bbox=L1Loss(loss_weight=hc.BBOX_LOSS_WEIGHT))
            xs = torch.from_numpy(x).to(dtype).requires_grad_(True)
            bp = None
            args = (None, None)
            if both:
                p, t, bw = hc.bbox_inputs()
                bp = torch.from_numpy(p).to(dtype).requires_grad_(True)
                args = (torch.from_numpy(t).to(dtype), torch.from_numpy(bw).to(dtype))
            losses = BBoxHead.loss(head, xs, bp, None, torch.from_numpy(labels), torch.from_numpy(w).to(dtype), *args)
            key = "acc_classes" if kind == "iif" else "acc"
            assert set(losses) == {"loss_cls", key} | ({"loss_bbox"} if both else set()), (name, sorted(losses))
            total = losses["loss_cls"] + (losses["loss_bbox"] if both else 0.0)
            total.backward()
            res[dtype] = dict(loss=losses["loss_cls"].detach().numpy(), grad=xs.grad.numpy(), acc=losses[key].detach().numpy(),
                              loss_bbox=losses["loss_bbox"].detach().numpy() if both else None,
                              bgrad=bp.grad.numpy() if both else None)
        r32, r64 = res[torch.float32], res[torch.float64]
        # the reference's avg_factor and its accuracy on the rows that count
        wt = torch.from_numpy(w)
        avg = max(torch.sum(wt > 0).float().item(), 1.)
        keep = wt > 0
        acc_valid = accuracy(torch.from_numpy(x)[keep], torch.from_numpy(labels)[keep]).numpy().reshape(-1).astype(np.float32)
        assert tuple(r32["acc"].shape) == (1,)
        # the restatement against the float64 run
        rs = hc.restate_case(name)
        gmax = float(np.abs(r64["grad"]).max())
        e_l = abs(rs["loss"] - float(r64["loss"])) / max(abs(float(r64["loss"])), 1e-300) if float(r64["loss"]) else abs(rs["loss"])
        e_g = float(np.abs(rs["grad"] - r64["grad"]).max()) / gmax if gmax else float(np.abs(rs["grad"]).max())
        assert e_l <= 1e-12 and e_g <= 1e-12, (name, e_l, e_g)
        assert rs["avg"] == avg and np.array_equal(np.float32(rs["acc"]).reshape(1), acc_valid), (name, rs["acc"], acc_valid, avg)
        if pad == hc.PAD_NONE:
            assert np.array_equal(acc_valid, r32["acc"]), name
        assert np.array_equal(r32["acc"], r64["acc"].astype(np.float32)), name
        worst["restate_loss"], worst["restate_grad"] = max(worst["restate_loss"], e_l), max(worst["restate_grad"], e_g)
        e32_l = abs(float(r32["loss"]) - float(r64["loss"]))
        e32_g = float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())
        if float(r64["loss"]):
            worst["loss"] = max(worst["loss"], e32_l / abs(float(r64["loss"])))
        if gmax:
            worst["grad"] = max(worst["grad"], e32_g / gmax)
        rows, cols = hc.kept(name)
        lab_cols = np.clip(labels[rows], 0, C - 1)
        out[name + "_loss32"] = np.float32(r32["loss"])
        out[name + "_loss64"] = np.float64(r64["loss"])
        out[name + "_avg"] = np.float32(avg)
        out[name + "_acc_all"] = r32["acc"].astype(np.float32)
        out[name + "_acc_valid"] = acc_valid
        out[name + "_grad32"] = r32["grad"][np.ix_(rows, cols)].astype(np.float32)
        out[name + "_grad64"] = r64["grad"][np.ix_(rows, cols)]
        out[name + "_gradlab32"] = r32["grad"][rows, lab_cols].astype(np.float32)
        out[name + "_gradlab64"] = r64["grad"][rows, lab_cols]
        out[name + "_gmax64"] = np.float64(gmax)
        out[name + "_e32_grad"] = np.float64(e32_g)
        if both:
            out["bbox_loss32"], out["bbox_loss64"] = np.float32(r32["loss_bbox"]), np.float64(r64["loss_bbox"])
            nz = np.nonzero(r64["bgrad"])
            assert np.array_equal(np.nonzero(r32["bgrad"])[0], nz[0]) and np.array_equal(np.nonzero(r32["bgrad"])[1], nz[1])
            out["bbox_grad_rows"], out["bbox_grad_cols"] = nz[0].astype(np.int64), nz[1].astype(np.int64)
            out["bbox_grad32"], out["bbox_grad64"] = r32["bgrad"][nz].astype(np.float32), r64["bgrad"][nz]
    out["worst"] = np.array([worst["loss"], worst["grad"], worst["restate_loss"], worst["restate_grad"]])
    path = os.path.join(HERE, "g36_bbox_head_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d cases, %.1f KB; float32 run vs float64 run: loss %.2e, gradient %.2e (of the largest element); "
          "float64 restatement vs float64 run: loss %.2e, gradient %.2e"
          % (path, len(hc.CASES), os.path.getsize(path) / 1024.0, worst["loss"], worst["grad"], worst["restate_loss"], worst["restate_grad"]))
    tmp.cleanup()


if __name__ == "__main__":
    main()
