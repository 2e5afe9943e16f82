"""CPU-side checks of the native NMS / RPN proposals (csrc/nms.hip, iif_amd/mmdet_nms.py): the numpy restatement of
tests/nms_cases.py against the fixture that the reference produced (tests/golden/make_golden_nms.py), the workspace formula,
the argument checks of the two C entries (they return before anything is launched) and the Python refusals.  No device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from iif_amd import _lib
from iif_amd import mmdet_nms as mn

from . import nms_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden):
    return golden("g28_nms")


def test_inputs_reproduce_the_fixture_checksums(g):
    sums = nc.input_checksums()
    assert sums
    for k, v in sums.items():
        assert np.array_equal(g[k], v), k


@pytest.mark.parametrize("name", list(nc.PLAIN_CASES))
def test_restatement_reproduces_plain_case(g, name):
    assert np.array_equal(nc.run_plain(name), g["p_%s_keep" % name])


@pytest.mark.parametrize("name", list(nc.BATCHED_CASES))
def test_restatement_reproduces_batched_case(g, name):
    assert np.array_equal(nc.run_batched(name), g["b_%s_keep" % name])


@pytest.mark.parametrize("name", list(nc.RPN_CASES))
def test_restatement_reproduces_rpn_case(g, name):
    """Candidate order, levels, valid counts and kept positions exactly; the boxes and scores of the kept proposals within the
    reference's own measured error and the same again (numpy's exp is not torch's; the fixture stores no value that went
    through exp)."""
    cls, reg, anchors = nc.rpn_inputs(name)
    c = nc.RPN_CASES[name]
    assert bool(g["r_%s_from_ref" % name]) == (name not in nc.RPN_TIE_CASES)
    for b in range(len(c["shapes"])):
        r = nc.rpn_np(name, b, cls, reg, anchors)
        pre = "r_%s_%d_" % (name, b)
        assert np.array_equal(r["index"], g[pre + "index"]) and np.array_equal(r["level"], g[pre + "level"])
        assert int(r["valid"].sum()) == int(g[pre + "nvalid"]) and np.array_equal(r["keep"], g[pre + "keep"])
        k = r["keep"]
        if k.size:
            ok, kinds, err = nc.tc.decode_check(r["boxes"][k], r["anchors"][k], r["deltas"][k], *nc.decode_args(c["shapes"][b]))
            assert ok and kinds and err <= 2 * float(g["ref_decode_ulps"])
            assert nc.sigmoid_ulps(r["scores"][k], r["logits"][k]) <= 2 * float(g["ref_sigmoid_ulps"])


def test_long_rpn_cases_say_what_they_should():
    """The first level is longer than one grid-stride step of the select, both levels are cut, and the tie variant's cut at
    nms_pre splits a run of equal logits (the distinct variant's does not)."""
    for name, c in nc.RPN_LONG_CASES.items():
        cls, reg, _ = nc.rpn_inputs(name)
        assert c["min_size"] < 0 and c["nms_pre"] == 256
        for b in range(len(c["shapes"])):
            (x0, _), (x1, _) = nc.rpn_flat(cls, reg, b)
            assert x0.size == 17280 > 16 * 1024 and x0.size - 16 * 1024 == 896 and x1.size == 288
            top = np.sort(x0)[::-1]
            assert (top[c["nms_pre"] - 1] == top[c["nms_pre"]]) == c["tie"]
            assert np.unique(x1).size == x1.size


def test_chain_and_zero_area_cases_say_what_they_should(g):
    assert g["p_chain_keep"].tolist() == [0, 2]                       # c survives: only the suppressed b overlaps it
    assert {3, 5} <= set(g["p_zero_area_keep"].tolist())              # 0 / 0 does not suppress


def test_workspace_formula_matches_the_header():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    m = re.search(r"#define IIF_NMS_WORKSPACE_BYTES\(B, N\) (.+)", text)
    assert m
    expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
    for B, N in ((1, 0), (1, 1), (1, 64), (1, 65), (2, 858), (2, 8768), (16, 16384)):
        assert mn.workspace_bytes(B, N) == eval(expr, {"B": B, "N": N}), (B, N)
    assert re.search(r"#define IIF_NMS_MAX_BOXES %d\b" % mn.MAX_BOXES, text)
    # what the kernels lay out: header, per image histograms and states, 60 bytes per padded box, the bit matrix
    n64 = 8768 // 64 * 64
    assert mn.workspace_bytes(2, 8768) >= 4096 + 2 * (8 * 5 * 4096 * 4 + 4096 + n64 * 60 + n64 * (n64 // 64) * 8)


def _aligned(nbytes):
    raw = (ctypes.c_char * (nbytes + 16))()
    return raw, (ctypes.addressof(raw) + 15) // 16 * 16


def test_iif_nms_rejects_bad_arguments():
    L = _lib.lib()
    raw, p = _aligned(4096)
    big = mn.workspace_bytes(1, 64)
    ok = dict(boxes=p, ld=4, scores=p, ids=None, N=64, mode=0, thr=0.5, off=0, st=0.0, mx=-1, keep=p, dets=p, count=p, ws=p, wsb=big)

    def call(**kw):
        a = dict(ok, **kw)
        return L.iif_nms(a["boxes"], a["ld"], a["scores"], a["ids"], a["N"], a["mode"], a["thr"], a["off"], a["st"], a["mx"], a["keep"],
                         a["dets"], a["count"], a["ws"], a["wsb"], None)
    assert call(boxes=None) == -1 and call(scores=None) == -1 and call(keep=None) == -1 and call(count=None) == -1
    assert call(N=mn.MAX_BOXES + 1, wsb=1 << 40) == -1 and call(N=-1) == -1
    assert call(ld=3) == -1
    assert call(mode=3) == -1 and call(mode=-1) == -1
    assert call(mode=1, ids=None) == -1                                # ids are needed with an id mode
    assert call(off=2) == -1
    assert call(thr=float("nan")) == -1
    assert call(ws=None) == -1 and call(ws=p + 8) == -1 and call(wsb=big - 1) == -1
    assert call(count=p + 4) == -1


def test_iif_rpn_proposals_rejects_bad_arguments():
    L = _lib.lib()
    raw, p = _aligned(4096)
    f4 = (ctypes.c_float * 4)(0, 0, 0, 0)
    hw = (ctypes.c_float * 64)(*([100.0] * 64))

    def levels(n, **kw):
        arr = (_lib.RpnLevel * max(n, 1))()
        for lv in arr:
            lv.scores = lv.deltas = lv.anchors = p
            lv.score_strides = (ctypes.c_int64 * 4)(48, 16, 4, 1)
            lv.delta_strides = (ctypes.c_int64 * 4)(192, 16, 4, 1)
            lv.ld_anchors, lv.A, lv.H, lv.W = 4, 3, 4, 4
            for k, v in kw.items():
                setattr(lv, k, v)
        return arr
    ws_ok = mn.workspace_bytes(2, 48)
    ok = dict(lv=levels(1), L=1, B=2, hw=hw, pre=1000, mpi=10, ms=0.0, thr=0.7, off=0, means=f4, stds=f4, dets=p, counts=p, ws=p, wsb=ws_ok)

    def call(**kw):
        a = dict(ok, **kw)
        return L.iif_rpn_proposals(a["lv"], a["L"], a["B"], a["hw"], a["pre"], a["mpi"], a["ms"], a["thr"], a["off"], a["means"], a["stds"],
                                   4.135, 0, 32.0, 1, a["dets"], a["counts"], None, None, None, None, None, a["ws"], a["wsb"], None)
    assert call(lv=None) == -1 and call(hw=None) == -1 and call(means=None) == -1 and call(dets=None) == -1 and call(counts=None) == -1
    assert call(B=17, wsb=1 << 40) == -1 and call(B=0) == -1
    assert call(lv=levels(9), L=9, wsb=1 << 40) == -1 and call(L=0) == -1
    assert call(lv=levels(1, scores=None)) == -1 and call(lv=levels(1, anchors=None)) == -1
    assert call(lv=levels(1, A=0)) == -1 and call(lv=levels(1, ld_anchors=3)) == -1
    assert call(lv=levels(1, H=128, W=128), pre=0, wsb=1 << 40) == -1        # 49 152 candidates: above the cap
    assert call(mpi=0) == -1 and call(off=2) == -1 and call(thr=float("nan")) == -1
    assert call(ws=None) == -1 and call(ws=p + 8) == -1 and call(wsb=ws_ok - 1) == -1
    # the workspace is sized by the candidates, not by the anchors
    assert call(lv=levels(1), pre=10, wsb=mn.workspace_bytes(2, 10) - 1) == -1


class _Coder:
    means, stds, clip_border, add_ctr_clamp, ctr_clamp = (0., 0., 0., 0.), (1., 1., 1., 1.), True, False, 32


def test_python_refusals_on_cpu_tensors():
    """Every refusal raises before any kernel could run; CPU tensors are rejected, not emulated."""
    b, s = torch.zeros(10, 4), torch.zeros(10)
    ids = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(_lib.IIFNativeError):
        mn.nms(b, s, 0.5)
    with pytest.raises(_lib.IIFNativeError):
        mn.batched_nms(b, s, ids, dict(type="nms", iou_threshold=0.5))
    with pytest.raises(ValueError):
        mn.nms(torch.zeros(mn.MAX_BOXES + 1, 4), torch.zeros(mn.MAX_BOXES + 1), 0.5)
    with pytest.raises(NotImplementedError):
        mn.nms(b.double(), s.double(), 0.5)
    with pytest.raises(NotImplementedError):
        mn.nms(b.half(), s.half(), 0.5)
    with pytest.raises(NotImplementedError):
        mn.batched_nms(b, s, ids, dict(type="soft_nms", iou_threshold=0.5))
    cfg = dict(nms_pre=100, max_per_img=10, min_bbox_size=0, nms=dict(type="nms", iou_threshold=0.7))
    cls, reg, anc = [torch.zeros(1, 3, 2, 2)], [torch.zeros(1, 12, 2, 2)], [torch.zeros(12, 4)]
    metas = [dict(img_shape=(8, 8, 3))]
    with pytest.raises(_lib.IIFNativeError):
        mn.rpn_get_bboxes(cls, reg, anc, metas, cfg, _Coder())
    with pytest.raises(NotImplementedError):                           # two score channels per anchor: the softmax RPN
        mn.rpn_get_bboxes([torch.zeros(1, 6, 2, 2)], reg, anc, metas, cfg, _Coder())
    with pytest.raises(NotImplementedError):
        mn.rpn_get_bboxes(cls, reg, anc, metas, cfg, _Coder(), rescale=True)
    with pytest.raises(ValueError):
        mn.rpn_get_bboxes(cls, reg, anc, metas, cfg, _Coder(), with_nms=False)
    with pytest.raises(NotImplementedError):
        mn.rpn_proposals_padded(cls, reg, anc, [torch.tensor([8, 8])], cfg, _Coder())
    with pytest.raises(NotImplementedError):
        mn.rpn_get_bboxes([x.double() for x in cls], reg, anc, metas, cfg, _Coder())
    with pytest.raises(NotImplementedError):
        mn.rpn_get_bboxes(cls, reg, anc, metas, dict(cfg, nms=dict(type="soft_nms", iou_threshold=0.7)), _Coder())
    with pytest.raises(NotImplementedError):                           # 12 candidates reach split_thr: the reference may go per level
        mn.rpn_get_bboxes(cls, reg, anc, metas, dict(cfg, nms=dict(type="nms", iou_threshold=0.7, split_thr=12)), _Coder())
    with pytest.raises(ValueError):                                    # 5 x 4096 candidates
        mn.rpn_get_bboxes([torch.zeros(1, 3, 40, 40)] * 5, [torch.zeros(1, 12, 40, 40)] * 5, [torch.zeros(4800, 4)] * 5, metas,
                          dict(cfg, nms_pre=4096), _Coder())
