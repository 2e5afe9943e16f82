#!/usr/bin/env python3
"""Generate tests/golden/gNN_mask_head.npz (the next free number) by RUNNING THE REFERENCE's two ends of the mask branch on the
CPU, once in float64 and once in float32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mask_head.py <reference checkout>

Training end: ``core/mask/mask_target.py`` and ``core/mask/structures.py`` are imported as they are, under placeholder modules:
``mmcv``, ``cv2`` and ``pycocotools`` are empty packages, ``mmcv.ops.roi_align.roi_align`` is the torch RoIAlign of
make_golden_roi_extract.py (mmcv's definition, evaluated with torch gathers in the input's precision), the helpers are those of
make_golden_targets.py.  ``mask_target`` runs per case on the rows the reference can take (a valid image and gt index); the
other rows are zero rows by the contract in include/iif_amd.h.  Test end: ``fcn_mask_head.py`` is imported under placeholders and
its ``_do_paste_mask(..., skip_empty=False)`` (the device branch of ``get_seg_masks``) runs on the sigmoid of the class channel,
followed by the thresholding line ``(masks_chunk >= threshold).to(dtype=torch.bool)``.

The float64 run needs two shims, because the reference narrows on the way: ``Tensor.float()`` (mask_target.py:123) and the
``torch.float32`` that ``_do_paste_mask`` casts to are replaced, for that run only, by the identity and ``torch.float64``.

Asserted before anything is stored:
  * the numpy restatements of tests/mask_cases.py agree with the reference in float64 to 1e-12;
  * the float32 and the float64 reference runs give IDENTICAL binary outputs, for every case and threshold;
  * no float64 value lies within mask_cases.MARGIN of its threshold - except the deliberate exact ties, which are EQUAL to the
    threshold in both precisions (the 0.5 bins of TIE_ROW, the 0.5 interior of PASTE_TIE, and every pixel at threshold 0);
    no pixel is excluded from any comparison;
  * the deliberate ties are there: TIE_ROW has bins of exactly 0.5 that come out as 1, the tie detection's interior is true.
Stored: the rois / boxes / labels, input checksums, the binary outputs bit-packed, checksums of the float64 values (the array
for mask_cases.FULL_TARGET_CASE) and ``ref_f32_err``: the float32 run's largest error against float64.
"""
import contextlib
import glob
import importlib
import importlib.util
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from tests import mask_cases as mc                                           # noqa: E402
from make_golden_roi_extract import RoIAlign                                 # noqa: E402
from make_golden_targets import _Registry, _identity_decorator, _pkg        # noqa: E402

torch.set_num_threads(8)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def roi_align(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True):
    return RoIAlign(output_size, spatial_scale, sampling_ratio, pool_mode, aligned)(input, rois)


def reference(ref_root):
    mm = os.path.join(ref_root, "instance_segmentation", "mmdet")
    _pkg("cv2")
    _pkg("pycocotools")
    _pkg("pycocotools.mask")
    _pkg("mmcv")
    _pkg("mmcv.ops")
    _pkg("mmcv.ops.roi_align", roi_align=roi_align)
    _pkg("mmcv.ops.carafe", CARAFEPack=None)
    _pkg("mmcv.cnn", ConvModule=None, build_conv_layer=None, build_upsample_layer=None)
    _pkg("mmcv.runner", BaseModule=torch.nn.Module, ModuleList=torch.nn.ModuleList, auto_fp16=_identity_decorator,
         force_fp32=_identity_decorator)
    _pkg("mmdet")
    core = _pkg("mmdet.core")
    _pkg("mmdet.core.mask", os.path.join(mm, "core", "mask"))
    structures = importlib.import_module("mmdet.core.mask.structures")
    mt = importlib.import_module("mmdet.core.mask.mask_target")
    core.mask_target = mt.mask_target
    _pkg("mmdet.models")
    _pkg("mmdet.models.builder", HEADS=_Registry(), build_loss=None)
    spec = importlib.util.spec_from_file_location("ref_fcn_mask_head", os.path.join(mm, "models", "roi_heads", "mask_heads", "fcn_mask_head.py"))
    head = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(head)
    return structures, mt, head


@contextlib.contextmanager
def keep_float64():
    """The two shims of the float64 run (see the module docstring)."""
    f32, to_float = torch.float32, torch.Tensor.float
    torch.float32, torch.Tensor.float = torch.float64, lambda self, *a, **kw: self
    try:
        yield
    finally:
        torch.float32, torch.Tensor.float = f32, to_float


def run_targets(structures, mt, name, dt, binarize):
    """[K, MH, MW] of the reference's mask_target in precision dt (zero rows where the reference cannot run), as numpy."""
    _, size, images = mc.TARGET_CASES[name]
    rows, mlist = mc.target_rows(name), mc.case_masks(name)
    out = np.zeros((len(rows),) + size, dtype=np.float64 if dt == torch.float64 else np.float32)
    valid = np.array([mc.target_row_valid(r, images) for r in rows])
    sel = [np.nonzero(valid & (rows[:, 0] == i))[0] for i in range(len(images))]
    props = [torch.from_numpy(rows[s, 2:6].copy()).to(dt) for s in sel]
    inds = [torch.from_numpy(rows[s, 1].astype(np.int64)) for s in sel]
    gts = [structures.BitmapMasks(m.copy(), m.shape[1], m.shape[2]) for m in mlist]
    cfg = Cfg(mask_size=size if size[0] != size[1] else size[0], soft_mask_target=not binarize)
    ctx = keep_float64() if dt == torch.float64 else contextlib.nullcontext()
    with ctx:
        res = mt.mask_target(props, inds, gts, cfg)
    res = res.numpy()
    if binarize and res.dtype == np.bool_:          # the float64 run's identity .float() leaves the thresholded booleans
        res = res.astype(out.dtype)
    assert res.dtype == out.dtype and res.shape[0] == sum(len(s) for s in sel), (res.dtype, res.shape)
    out[np.concatenate(sel)] = res
    return out


def run_paste(head, name, dt):
    """[N, img_h, img_w] pasted values of the reference in precision dt, as numpy."""
    C, agnostic, activated = mc.PASTE_CASES[name]
    pred = torch.from_numpy(mc.paste_pred(name).copy()).to(dt)
    boxes = torch.from_numpy(mc.paste_boxes().copy()).to(dt)[:, :4]
    labels = torch.from_numpy(mc.paste_labels())
    N = pred.size(0)
    ctx = keep_float64() if dt == torch.float64 else contextlib.nullcontext()
    with ctx:
        if not activated:
            pred = pred.sigmoid()
        if not agnostic:
            pred = pred[range(N), labels][:, None]
        vals, _ = head._do_paste_mask(pred, boxes, mc.IMG_H, mc.IMG_W, skip_empty=False)
    assert vals.dtype == dt
    return vals.numpy()


def threshold_line(vals, threshold):
    return (torch.from_numpy(vals) >= threshold).to(dtype=torch.bool).numpy()


def check_margin(v64, v32, thr, what):
    """No value within MARGIN of the threshold unless it EQUALS it in both precisions; returns the number of exact ties."""
    d = np.abs(v64 - thr)
    tie = d == 0
    assert np.all(tie | (d >= mc.MARGIN)), (what, float(d[~tie].min()))
    assert np.all(v32[tie] == np.float32(thr)), what
    return int(tie.sum())


def main():
    structures, mt, head = reference(sys.argv[1])
    store = dict(mc.input_checksums())
    for name in mc.TARGET_CASES:
        soft64 = run_targets(structures, mt, name, torch.float64, False)
        soft32 = run_targets(structures, mt, name, torch.float32, False)
        bin64 = run_targets(structures, mt, name, torch.float64, True)
        bin32 = run_targets(structures, mt, name, torch.float32, True)
        assert soft64.dtype == np.float64 and soft32.dtype == np.float32
        assert np.array_equal(bin32, bin64), name
        assert np.array_equal(bin64, (soft64 >= 0.5).astype(np.float64)), name
        assert set(np.unique(bin32).tolist()) <= {0.0, 1.0}
        mine = mc.target_reference64(name)
        assert np.abs(mine - soft64).max() <= 1e-12, (name, np.abs(mine - soft64).max())
        ties = check_margin(soft64, soft32, 0.5, name)
        if mc.TARGET_CASES[name] == mc.TARGET_CASES["kinds_28"]:
            t = soft64[mc.TIE_ROW]
            assert ties == int((t == 0.5).sum()) and ties >= 20 and bin32[mc.TIE_ROW][t == 0.5].all(), (name, ties)
        else:
            assert ties == 0, (name, ties)
        err = float(np.abs(soft32.astype(np.float64) - soft64).max())
        store["t_%s_bits" % name] = mc.pack(bin32)
        store["t_%s_soft_sum" % name] = mc.checksum(soft64)
        store["t_%s_ref_f32_err" % name] = np.array(err)
        if name == mc.FULL_TARGET_CASE:
            store["t_%s_soft" % name] = soft64
        print("targets %-12s K %2d  ones %5d  exact ties %3d  ref f32 err %.2e" % (name, soft64.shape[0], int(bin32.sum()), ties, err))
    for name in mc.PASTE_CASES:
        v64, v32 = run_paste(head, name, torch.float64), run_paste(head, name, torch.float32)
        mine = mc.paste_reference64(name)
        assert np.abs(mine - v64).max() <= 1e-12, (name, np.abs(mine - v64).max())
        b64, b32 = threshold_line(v64, 0.5), threshold_line(v32, 0.5)
        assert np.array_equal(b32, b64), name
        ties = check_margin(v64, v32, 0.5, name)
        activated = mc.PASTE_CASES[name][2]
        if activated:
            assert ties == 0
        else:
            t = v64[mc.PASTE_TIE]
            assert ties == int((t == 0.5).sum()) and ties >= 400 and b32[mc.PASTE_TIE][t == 0.5].all(), (name, ties)
        assert threshold_line(v64, 0.0).all() and threshold_line(v32, 0.0).all(), name        # threshold 0: every pixel, padding included
        assert (v64 >= 0).all() and (v32 >= 0).all()
        err = float(np.abs(v32.astype(np.float64) - v64).max())
        store["p_%s_bits" % name] = mc.pack(b32)
        store["p_%s_val_sum" % name] = mc.checksum(v64)
        store["p_%s_ref_f32_err" % name] = np.array(err)
        print("paste   %-12s N %2d  true %5d  exact ties %3d  ref f32 err %.2e" % (name, v64.shape[0], int(b32.sum()), ties, err))
    taken = [int(m.group(1)) for f in glob.glob(os.path.join(HERE, "g*.npz")) for m in [re.match(r"g(\d+)_", os.path.basename(f))] if m]
    mine = glob.glob(os.path.join(HERE, "g*_mask_head.npz"))
    path = mine[0] if mine else os.path.join(HERE, "g%d_mask_head.npz" % (max(taken) + 1))
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
