"""CPU-side checks of the native multiclass_nms (csrc/multiclass_nms.hip, iif_amd/mmdet_multiclass_nms.py): the numpy restatement
of tests/multiclass_cases.py against the fixture that the reference produced (tests/golden/make_golden_multiclass_nms.py), the
workspace formula, the argument checks of the C entry (it returns before anything is launched) and the Python refusals.  No
device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from iif_amd import _lib
from iif_amd import mmdet_multiclass_nms as mm

from . import multiclass_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden):
    return golden("g29_multiclass_nms")


def test_inputs_reproduce_the_fixture_checksums(g):
    sums = mc.input_checksums()
    assert len(sums) == len(mc.CASES) + len(mc.GB_CASES)
    for k, v in sums.items():
        assert np.array_equal(g[k], v), k


def _same(g, name, res):
    dets, labels, inds, M = res
    assert M == int(g[name + "_M"]) and inds.size == int(g[name + "_count"])
    assert np.array_equal(inds, g[name + "_inds"]) and np.array_equal(labels, g[name + "_labels"])


@pytest.mark.parametrize("name", list(mc.CASES))
def test_restatement_reproduces_case(g, name):
    c = mc.CASES[name]
    assert bool(g[name + "_from_ref"]) == (name not in mc.TIE_CASES)
    res = mc.run(name)
    _same(g, name, res)
    assert np.array_equal(mc.bits(res[0]), mc.bits(mc.dets_from_inds(*mc.inputs(name), res[2])))
    assert np.array_equal(res[1], res[2] % c["C"])
    assert res[2].size <= mc.cap(name)


@pytest.mark.parametrize("name", list(mc.GB_CASES))
def test_restatement_reproduces_get_bboxes_case(g, name):
    """Identities only: numpy's exp is not torch's, and the generator proved the case's kept pairs independent of that rounding."""
    _same(g, name, mc.gb_run(name))


def test_fixture_cases_say_what_they_should(g):
    m = int(g["bnd_below_M"])
    assert m == int(g["bnd_at_M"]) == int(g["bnd_above_M"])
    assert mc.split_thr("bnd_below") == m + 1 and mc.split_thr("bnd_at") == m and mc.split_thr("bnd_above") < m
    assert int(g["lvis_M"]) >= 10000 and "split_thr" not in mc.nms_cfg("lvis")
    assert int(g["none_count"]) == 0 and int(g["none_M"]) == 0
    assert not np.array_equal(g["negative_inds"], g["negative_split_inds"])        # suppression across classes below -1
    for name in mc.TRUNCATED:
        assert int(g[name + "_count"]) == mc.cap(name)


def test_long_kept_case_says_what_it_should():
    """Without the cut every one of the 64 * 512 candidates is kept (the per-class regime), and the cut at 100 falls between two
    equal scores, so the flat index decides it."""
    name = "long_kept"
    c = mc.LONG_CASES[name]
    dets, labels, inds, M = mc.run(name, max_num=-1)
    assert M == 32768 >= mc.split_thr(name) and inds.size == 32768 == 2 * 16 * 1024
    assert c["max_num"] == mc.cap(name) == 100 and dets[99, 4] == dets[100, 4]
    assert inds[99] < inds[100]
    cut = mc.run(name)
    assert np.array_equal(cut[2], inds[:100]) and np.array_equal(mc.bits(cut[0]), mc.bits(dets[:100]))


def test_workspace_formula_matches_the_header():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    m = re.search(r"#define IIF_MULTICLASS_NMS_WORKSPACE_BYTES\(B, R, C, cap\) (.+)", text)
    assert m
    expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
    for B, R, C, cap in ((1, 0, 1, 1), (1, 1, 1, 1), (1, 130, 3, 300), (2, 256, 1203, 300), (16, 1000, 1230, 300), (16, 1024, 4096, 4096)):
        assert mm.workspace_bytes(B, R, C, cap) == eval(expr, {"B": B, "R": R, "C": C, "cap": cap}), (B, R, C, cap)
    for k, v in (("ROWS", mm.MAX_ROWS), ("CLASSES", mm.MAX_CLASSES), ("CAP", mm.MAX_CAP)):
        assert re.search(r"#define IIF_MULTICLASS_NMS_MAX_%s %d\b" % (k, v), text)
    # what the kernels lay out: header, histograms, class counters, the ranked flat list, segments and list, the selection
    assert mm.workspace_bytes(2, 256, 1203, 300) >= 4096 + 2 * (5 * 4096 * 4 + 4 * 1204 + 16384 * 8 + 2 * 8 * 256 * 1203 + 8 * 300)


def _aligned(nbytes):
    raw = (ctypes.c_char * (nbytes + 16))()
    return raw, (ctypes.addressof(raw) + 15) // 16 * 16


def test_iif_multiclass_nms_rejects_bad_arguments():
    L = _lib.lib()
    raw, p = _aligned(4096)
    big = mm.workspace_bytes(2, 64, 3, 10)
    ok = dict(boxes=p, ldb=12, pc=1, scores=p, lds=4, fac=None, rc=None, B=2, R=64, C=3, st=0.05, thr=0.5, off=0, split=10000, cap=10,
              dets=p, labels=p, inds=p, counts=p, ncand=p, ws=p, wsb=big)

    def call(**kw):
        a = dict(ok, **kw)
        return L.iif_multiclass_nms(a["boxes"], a["ldb"], a["pc"], a["scores"], a["lds"], a["fac"], a["rc"], a["B"], a["R"], a["C"], a["st"],
                                    a["thr"], a["off"], a["split"], a["cap"], a["dets"], a["labels"], a["inds"], a["counts"], a["ncand"],
                                    a["ws"], a["wsb"], None)
    for k in ("boxes", "scores", "dets", "labels", "inds", "counts"):
        assert call(**{k: None}) == -1, k
    assert call(B=0) == -1 and call(B=17, wsb=1 << 40) == -1
    assert call(R=-1) == -1 and call(R=mm.MAX_ROWS + 1, wsb=1 << 40) == -1
    assert call(C=0) == -1 and call(C=mm.MAX_CLASSES + 1, lds=mm.MAX_CLASSES + 2, ldb=4, pc=0, wsb=1 << 40) == -1
    assert mm.MAX_ROWS * mm.MAX_CLASSES < 1 << 24                                    # the candidate index has 24 bits
    assert call(cap=0) == -1 and call(cap=mm.MAX_CAP + 1, wsb=1 << 40) == -1
    assert call(off=2) == -1 and call(thr=float("nan")) == -1 and call(st=float("nan")) == -1
    assert call(lds=3) == -1 and call(ldb=11) == -1 and call(ldb=3, pc=0) == -1
    assert call(R=1024, C=80, lds=81, ldb=320, split=20000, wsb=1 << 40) == -1       # all pairs could hold 81 920 candidates
    assert call(ws=None) == -1 and call(ws=p + 8) == -1 and call(wsb=big - 1) == -1
    assert call(counts=p + 4) == -1 and call(rc=p + 4) == -1


NMS = dict(type="nms", iou_threshold=0.5)


def test_python_refusals_on_cpu_tensors():
    """Every refusal raises before any kernel could run; CPU tensors are rejected, not emulated."""
    b, s = torch.zeros(10, 12), torch.zeros(10, 4)
    with pytest.raises(_lib.IIFNativeError):
        mm.multiclass_nms(b, s, 0.05, NMS, 100)
    with pytest.raises(_lib.IIFNativeError):
        mm.multiclass_nms_padded(b[None], s[None], 0.05, NMS, 100)
    with pytest.raises(NotImplementedError, match="max_num"):
        mm.multiclass_nms(b, s, 0.05, NMS)                                        # no bound at all
    with pytest.raises(NotImplementedError, match="max_num"):
        mm.multiclass_nms(b, s, 0.05, dict(NMS, max_num=-1), 0)
    with pytest.raises(NotImplementedError, match="type"):
        mm.multiclass_nms(b, s, 0.05, dict(NMS, type="soft_nms"), 100)
    with pytest.raises(NotImplementedError, match="score_threshold"):
        mm.multiclass_nms(b, s, 0.05, dict(NMS, score_threshold=0.1), 100)
    with pytest.raises(NotImplementedError, match="class_agnostic"):
        mm.multiclass_nms(b, s, 0.05, dict(NMS, class_agnostic=True), 100)
    with pytest.raises(ValueError, match="split_thr"):
        mm.multiclass_nms(torch.zeros(1000, 4), torch.zeros(1000, 81), 0.05, dict(NMS, split_thr=20000), 100)
    with pytest.raises(NotImplementedError, match="float32"):
        mm.multiclass_nms(b.double(), s.double(), 0.05, NMS, 100)
    with pytest.raises(NotImplementedError, match="float32"):
        mm.multiclass_nms(b.half(), s.half(), 0.05, NMS, 100)
    with pytest.raises(NotImplementedError, match="float32"):
        mm.multiclass_nms(b, s, 0.05, NMS, 100, score_factors=torch.zeros(10, dtype=torch.float64))
    with pytest.raises(ValueError):
        mm.multiclass_nms(b, s, 0.05, NMS, mm.MAX_CAP + 1)
    with pytest.raises(ValueError):
        mm.multiclass_nms(torch.zeros(mm.MAX_ROWS + 1, 4), torch.zeros(mm.MAX_ROWS + 1, 4), 0.05, NMS, 100)
    with pytest.raises(ValueError):
        mm.multiclass_nms(torch.zeros(10, 8), s, 0.05, NMS, 100)                   # 8 columns for 3 classes
    with pytest.raises(TypeError):
        mm.multiclass_nms(b, s, 0.05, dict(NMS, sigma=0.5), 100)
    # a split_thr above MAX_BOXES is fine while all candidates fit the all-pairs regime; the refusal left is the device's
    with pytest.raises(_lib.IIFNativeError):
        mm.multiclass_nms(b, s, 0.05, dict(NMS, split_thr=20000), 100)


def test_onnx_export_is_refused(monkeypatch):
    monkeypatch.setattr(torch.onnx, "is_in_onnx_export", lambda: True)
    with pytest.raises(NotImplementedError, match="ONNX"):
        mm.multiclass_nms(torch.zeros(10, 12), torch.zeros(10, 4), 0.05, NMS, 100)


def test_get_bboxes_without_cfg_returns_boxes_and_scores():
    """cfg=None with no deltas needs no kernel: the rois' boxes as they are (the reference's clamp acts on copies), divided under
    rescale."""
    rois, scores, _ = mc.gb_inputs("gb_nopred")
    out, s = mm.bbox_head_get_bboxes(torch.from_numpy(rois), torch.from_numpy(scores), None, mc.GB_SHAPE, mc.GB_SCALE, True, None, None)
    assert s.shape == scores.shape
    assert np.array_equal(mc.bits(out.numpy()), mc.bits(mc.gb_boxes_np("gb_nopred")))
