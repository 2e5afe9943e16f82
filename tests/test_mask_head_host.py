"""The two ends of the mask branch (iif_amd.mmdet_mask_target, iif_amd.mmdet_mask_loss, csrc/mask_ops.hip), the part that needs
no device: the fixture tests/golden/g30_mask_head.npz against the input generators and the numpy restatements of
tests/mask_cases.py, the two C entry points in header, library and ctypes table with their argument checks (by status code),
and the Python side's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from . import mask_cases as mc
from iif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_mask_targets", "iif_paste_masks")
FIXTURE = "g30_mask_head"


def close(a, b, tol=1e-12):
    return bool(np.all(np.abs(np.asarray(a) - np.asarray(b)) <= tol * max(1.0, float(np.asarray(b).ravel()[1]))))


def test_fixture_inputs_regenerate(golden):
    mc.check_generator(golden(FIXTURE))


@pytest.mark.parametrize("name", list(mc.TARGET_CASES))
def test_target_restatement_reproduces_the_fixture(golden, name):
    """Binary outputs exactly, float64 values to 1e-12 (the array where stored, checksums elsewhere), the float32 evaluation
    within the float32 reference's own error and with the same bits."""
    g = golden(FIXTURE)
    v64 = mc.target_reference64(name)
    assert np.array_equal(mc.pack(v64 >= 0.5), g["t_%s_bits" % name])
    assert close(mc.checksum(v64), g["t_%s_soft_sum" % name])
    if name == mc.FULL_TARGET_CASE:
        assert np.abs(v64 - g["t_%s_soft" % name]).max() <= 1e-12
    v32 = mc.targets_np(mc.target_rows(name), mc.case_masks(name), mc.TARGET_CASES[name][1], mc.F32)
    assert v32.dtype == np.float32
    assert np.array_equal(mc.pack(v32 >= np.float32(0.5)), g["t_%s_bits" % name])
    err, ref = float(np.abs(v32.astype(np.float64) - v64).max()), float(g["t_%s_ref_f32_err" % name])
    assert 0 < ref < 1e-4 and err <= 4 * ref, (err, ref)


@pytest.mark.parametrize("name", list(mc.PASTE_CASES))
def test_paste_restatement_reproduces_the_fixture(golden, name):
    g = golden(FIXTURE)
    v64 = mc.paste_reference64(name)
    assert np.array_equal(mc.pack(v64 >= 0.5), g["p_%s_bits" % name])
    assert close(mc.checksum(v64), g["p_%s_val_sum" % name])
    assert (v64 >= 0.0).all()                                   # threshold 0: every pixel, padding included
    C, agnostic, activated = mc.PASTE_CASES[name]
    v32 = mc.paste_values_np(mc.paste_pred(name), None if agnostic else mc.paste_labels(), mc.paste_boxes(), mc.IMG_H, mc.IMG_W,
                             mc.F32, activated)
    assert np.array_equal(mc.pack(v32 >= np.float32(0.5)), g["p_%s_bits" % name])
    assert 0 < float(g["p_%s_ref_f32_err" % name]) < 1e-5


def test_cases_are_what_they_are_there_for(golden):
    g = golden(FIXTURE)
    rows = mc.target_rows("kinds_28")
    assert rows.shape == (len(mc.KINDS) + mc.N_RANDOM, 6)
    v = mc.target_reference64("kinds_28")
    for k in (7, 8, 9, 14, 15, 16, 17, 18):                    # outside twice, zero width, padding, image N, gt G twice, gt -1
        assert not v[k].any(), k
    assert all(v[k].any() for k in range(len(mc.KINDS)) if k not in (7, 8, 9, 14, 15, 16, 17, 18))
    tie = v[mc.TIE_ROW]
    assert (tie == 0.5).sum() >= 20
    d = np.abs(v - 0.5)
    assert ((d == 0) | (d >= mc.MARGIN)).all() and not (np.delete(d, mc.TIE_ROW, axis=0) == 0).any()
    bits = np.unpackbits(g["t_kinds_28_bits"])[:v.size].reshape(v.shape).astype(bool)
    assert bits[mc.TIE_ROW][tie == 0.5].all()                   # an average of exactly 0.5 comes out as 1
    # the whole 200 x 272 image at 28 x 28: grids of 8 and 10 samples
    H, W, _ = mc.BIG_IMAGE
    dec = mc.rc.decisions(mc.clipped_roi(mc.target_rows("big_28")[0], H, W), mc.F32, **mc._geo(H, W, (28, 28)))
    assert (dec[2], dec[3]) == (8, 10)
    # sub-pixel bins: the three-pixel box has grid 1 on both axes
    H, W, _ = mc.IMAGES[0]
    dec = mc.rc.decisions(mc.clipped_roi(rows[19], H, W), mc.F32, **mc._geo(H, W, (28, 28)))
    assert (dec[2], dec[3]) == (1, 1)
    # paste: logits exact in bf16, the tie detection's interior is exactly 0.5, nothing else is near it
    for name, (C, agnostic, activated) in mc.PASTE_CASES.items():
        assert mc.bf16_exact(mc.paste_pred(name))
        p = mc.paste_reference64(name)
        d = np.abs(p - 0.5)
        assert ((d == 0) | (d >= mc.MARGIN)).all()
        if not activated:
            assert (p[mc.PASTE_TIE] == 0.5).sum() >= 400 and not (np.delete(d, mc.PASTE_TIE, axis=0) == 0).any()
        assert not p[3].any()                                   # the box outside the image
        assert (p[4] > 0).any(axis=0).all()                     # zero width: the tile's centre column in every image column


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_entry_points_in_header_library_and_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name])
    fields = re.search(r"typedef struct iif_mask_image \{(.*?)\}", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", fields).strip() == "const uint8_t* ptr; int32_t G, H, W; int64_t ld_row, ld_mask;"
    assert [f[0] for f in _lib.MaskImage._fields_] == ["ptr", "G", "H", "W", "ld_row", "ld_mask"] and ctypes.sizeof(_lib.MaskImage) == 40


def test_mask_targets_checks_arguments_before_launching():
    L = _lib.lib()
    one = 64            # a non-null, aligned stand-in: the checks fail before any pointer is used

    def images(n=2, ptr=one, G=3, H=67, W=83, ld_row=None, ld_mask=None):
        arr = (_lib.MaskImage * max(n, 1))()
        for m in arr:
            m.ptr, m.G, m.H, m.W = ptr, G, H, W
            m.ld_row = W if ld_row is None else ld_row
            m.ld_mask = H * m.ld_row if ld_mask is None else ld_mask
        return arr

    def call(**kw):
        return L.iif_mask_targets(kw.get("images", images()), kw.get("n", 2), kw.get("rois", one), kw.get("ld", 5), kw.get("gt", one),
                                  kw.get("K", 3), kw.get("mh", 28), kw.get("mw", 28), 1, kw.get("out", one), None)
    assert call(images=None) == -1 and call(rois=None) == -1 and call(gt=None) == -1 and call(out=None) == -1
    assert call(rois=66) == -1 and call(out=66) == -1 and call(gt=68) == -1
    assert call(n=0) == -1 and call(n=17) == -1 and call(K=-1) == -1 and call(ld=4) == -1
    assert call(mh=0) == -1 and call(mw=-2) == -1
    assert call(images=images(ptr=None)) == -1 and call(images=images(G=-1)) == -1
    assert call(images=images(H=0)) == -1 and call(images=images(W=0)) == -1
    assert call(images=images(ld_row=82)) == -1                            # a pitch below the width
    assert call(images=images(ld_mask=66 * 83 + 82)) == -1                 # masks that overlap
    assert call(mh=65) == -2 and call(mw=65) == -2 and call(images=images(W=4097)) == -2
    assert call(K=0, rois=None, gt=None, out=None) == 0
    assert call(K=0, images=images(G=0, ptr=None), rois=None, gt=None, out=None) == 0


def test_paste_masks_checks_arguments_before_launching():
    L = _lib.lib()
    one = 64

    def call(**kw):
        return L.iif_paste_masks(kw.get("pred", one), kw.get("dtype", 0), 0, kw.get("labels", one), kw.get("boxes", one), kw.get("ld", 5),
                                 kw.get("N", 3), kw.get("C", 5), kw.get("h", 28), kw.get("w", 28), kw.get("img_h", 61),
                                 kw.get("img_w", 93), kw.get("thr", 0.5), kw.get("out", one), None)
    assert call(pred=None) == -1 and call(boxes=None) == -1 and call(out=None) == -1
    assert call(pred=66) == -1 and call(boxes=66) == -1 and call(labels=68) == -1 and call(pred=65, dtype=1) == -1
    assert call(dtype=2) == -1 and call(N=-1) == -1 and call(N=65536) == -1 and call(C=0) == -1 and call(ld=3) == -1
    assert call(h=0) == -1 and call(w=0) == -1 and call(img_h=0) == -1 and call(img_w=-1) == -1
    assert call(thr=-0.5) == -1 and call(thr=float("nan")) == -1           # the uint8 visualisation branch is not offered
    assert call(h=65) == -2 and call(w=65) == -2 and call(img_h=65536, img_w=32768) == -2
    assert call(N=0, pred=None, boxes=None, out=None, labels=None) == 0


# ------------------------------------------------------------------------------------------------------------ Python surface
def test_python_side_refusals():
    from iif_amd import mmdet_mask_loss as ML
    from iif_amd import mmdet_mask_target as MT
    cfg = dict(mask_size=28)
    props, inds = torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64)
    masks = np.zeros((1, 8, 8), dtype=np.uint8)
    assert MT.mask_target([], [], [], cfg) == []
    assert MT.mask_target_single(props[:0], inds[:0], masks, dict(mask_size=(7, 11))).shape == (0, 7, 11)
    assert MT.mask_target([props[:0], props[:0]], [inds[:0], inds[:0]], [masks, masks], cfg).shape == (0, 28, 28)
    with pytest.raises(_lib.IIFNativeError):                    # CPU tensors are rejected, not emulated
        MT.mask_target_single(props, inds, masks, cfg)
    with pytest.raises(_lib.IIFNativeError):
        MT.mask_targets_padded(torch.zeros(2, 5), inds, [masks], 28)
    with pytest.raises(NotImplementedError):
        MT.mask_target_single(props.double(), inds, masks, cfg)
    with pytest.raises(NotImplementedError):
        MT.mask_targets_padded(torch.zeros(2, 5), inds, [masks], 65)
    with pytest.raises(ValueError):
        MT.mask_targets_padded(torch.zeros(2, 5), inds, [masks] * 17, 28)

    class PolygonMasks:
        masks, height, width = [[np.zeros(6)]], 8, 8
    with pytest.raises(NotImplementedError):
        MT._resolve(PolygonMasks(), "cpu")
    with pytest.raises(NotImplementedError):
        MT.DeviceBitmapMasks([[np.zeros(6)]], 8, 8)
    with pytest.raises(NotImplementedError):
        MT._resolve(object(), "cpu")
    with pytest.raises(NotImplementedError):
        MT._resolve(torch.zeros(1, 8, 8), "cpu")                # a float mask tensor
    d = MT.DeviceBitmapMasks(np.ones((3, 8, 8), dtype=bool), 8, 8)
    assert len(d) == 3 and (d.height, d.width) == (8, 8) and d.masks.dtype == np.uint8 and len(d[1]) == 1 and len(d[[0, 2]]) == 2
    assert len(MT.DeviceBitmapMasks([], 8, 8)) == 0
    with pytest.raises(NotImplementedError):
        d.crop_and_resize(np.zeros((1, 4), dtype=np.float32), (28, 28), np.zeros(1, dtype=np.int64), device="cpu", interpolation="nearest")
    for word in ("PolygonMasks", "bilinear", "float32", "4 096", "above 64"):
        assert word in MT.__doc__, word

    pred, boxes, labels = torch.zeros(2, 3, 28, 28), torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(NotImplementedError):
        ML.paste_masks(pred, boxes, labels, 20, 30, -1)         # the uint8 visualisation branch
    with pytest.raises(NotImplementedError):
        ML.paste_masks(pred.half(), boxes, labels, 20, 30, 0.5)
    with pytest.raises(NotImplementedError):
        ML.paste_masks(torch.zeros(2, 3, 65, 28), boxes, labels, 20, 30, 0.5)
    with pytest.raises(ValueError):
        ML.paste_masks(pred, boxes[:, :3], labels, 20, 30, 0.5)
    with pytest.raises(_lib.IIFNativeError):
        ML.paste_masks(pred, boxes, labels, 20, 30, 0.5)
    for word in ("mask_thr_binary < 0", "NaN", "64 x 64"):
        assert word in ML.__doc__, word
