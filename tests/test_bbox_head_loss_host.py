"""Host-side checks of BBoxHead.loss without a host read (iif_amd/mmdet_bbox_head_loss.py, csrc/head_loss.hip): no device.

  * the header declares the new entries, the library exports them and the ctypes table lists them;
  * the float64 restatement of tests/bbox_head_loss_cases.py reproduces the REFERENCE's own BBoxHead.loss
    (tests/golden/g36_bbox_head_loss.npz, written by tests/golden/make_golden_bbox_head_loss.py): the float64 loss and the kept
    gradient elements to 1e-12, avg_factor and both accuracies exactly;
  * CPU tensors, wrong shapes and wrong dtypes raise; the C entries reject bad arguments before any launch;
  * a loss module that is not native takes the reference's lines through its own forward / get_accuracy.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from iif_amd import _lib
from tests import bbox_head_loss_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_head_loss_fwd", "iif_head_loss_bwd")


def test_header_library_and_ctypes_table_have_the_entries():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "include/iif_amd.h does not declare " + name
        assert hasattr(lib, name), "libiif_amd.so does not export " + name
        assert name in _lib.SIGNATURES
        # one ctypes argument per declared parameter
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name]) == len(params.split(",")), name
    m = re.search(r"#define\s+IIF_HEAD_LOSS_WORKSPACE_BYTES\s+\((.*?)\)\s*$", code, flags=re.M)
    assert m, "no workspace-size macro"
    from iif_amd.loss_reduction import CE_WORKSPACE_WORDS
    assert eval(m.group(1)) <= 4 * CE_WORKSPACE_WORDS           # the per-stream workspace of custom._workspace serves this head
    from iif_amd import mmdet_bbox_head_loss as hl
    assert re.search(r"#define\s+IIF_HEAD_LOSS_MAX_CLASSES\s+%d\b" % hl.MAX_CLASSES, code)
    assert re.search(r"#define\s+IIF_HEAD_LOSS_MAX_ROWS\s+%d\b" % hl.MAX_ROWS, code)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_restatement_reproduces_the_reference(golden, name):
    g = golden("g36_bbox_head_loss")
    hc.check_generator(g)
    N, C, kind, bf, pad = hc.CASES[name][:5]
    x, labels, w = hc.inputs(name)
    r = hc.restate_case(name)
    l64 = float(g[name + "_loss64"])
    assert abs(r["loss"] - l64) <= 1e-12 * abs(l64)
    assert r["avg"] == float(g[name + "_avg"])
    assert np.array_equal(np.float32(r["acc"]).reshape(1), g[name + "_acc_valid"])
    if pad == hc.PAD_NONE:
        assert np.array_equal(g[name + "_acc_valid"], g[name + "_acc_all"])
    elif pad == hc.PAD_MIXED and N >= 63:
        assert not np.array_equal(g[name + "_acc_valid"], g[name + "_acc_all"])       # the reference dilutes it by the padding
    rows, cols = hc.kept(name)
    gmax = float(g[name + "_gmax64"])
    assert np.abs(r["grad"]).max() == pytest.approx(gmax, rel=1e-12, abs=0.0)
    assert np.abs(r["grad"][np.ix_(rows, cols)] - g[name + "_grad64"]).max() <= 1e-12 * max(gmax, 1e-300)
    lab_cols = np.clip(labels[rows], 0, C - 1)
    assert np.abs(r["grad"][rows, lab_cols] - g[name + "_gradlab64"]).max() <= 1e-12 * max(gmax, 1e-300)
    # rows of weight zero, ignored rows: exact zeros in the reference too
    dead = (w[rows] == 0) | (labels[rows] < 0)
    assert not g[name + "_grad32"][dead].any() and not g[name + "_grad64"][dead].any()
    if bf:
        assert np.array_equal(hc.bf16_round(x), x)


def test_cases_hold_the_forced_rows():
    """Ties and flat rows behave as the cases file says, under the reference's topk as the generator asserted."""
    x, labels, w = hc.inputs("c257x81")
    one = lambda r: hc.restate64(x[r:r + 1], None, labels[r:r + 1], w[r:r + 1], None, None, 1.0)["hits"]        # noqa: E731
    assert (one(hc.TIE_LOWER), one(hc.TIE_HIGHER), one(hc.FLAT_FIRST), one(hc.FLAT_OTHER)) == (0, 1, 1, 0)
    assert (w < 0).any() and (w == 0).any() and (labels == -100).any() and (labels == 80).any()
    r = hc.restate_case("z5x5")
    assert (r["loss"], r["avg"], float(r["acc"])) == (0.0, 1.0, 0.0) and not r["grad"].any()
    r = hc.restate_case("o64x81")
    assert (r["valid"], r["hits"], float(r["acc"])) == (1, 1, 100.0)
    # a NaN in a row of weight zero is never touched
    xn = x.copy()
    xn[w == 0] = np.nan
    a, b = hc.restate_case("c257x81"), hc.restate64(xn, None, labels, w, None, None, 1.0)
    assert a["loss"] == b["loss"] and np.array_equal(a["grad"], b["grad"]) and a["acc"] == b["acc"]


def _iif(**kw):
    from iif_amd.mmdet_iif_loss import IIFLoss
    return IIFLoss(path=hc.LVIS_CSV, num_classes=1203, device="cpu", **kw)


def test_cpu_tensors_shapes_and_dtypes_raise(monkeypatch):
    from iif_amd import mmdet_bbox_head_loss as hl
    from iif_amd.mmdet_bbox_loss import L1Loss
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    x = torch.zeros(4, 1204)
    lab = torch.zeros(4, dtype=torch.int64)
    w = torch.ones(4)
    ce = CrossEntropyLoss()
    for crit in (_iif(), ce):
        with pytest.raises(_lib.IIFNativeError):
            hl.head_cls_loss(crit, x, lab, w)
    with pytest.raises(_lib.IIFNativeError):
        hl.bbox_head_loss(ce, L1Loss(), x, None, None, lab, w, None, None, 1203)
    with pytest.raises(_lib.IIFNativeError):
        hl.bbox_head_loss(ce, L1Loss(), None, torch.zeros(4, 8), None, lab, w, torch.zeros(4, 4), torch.zeros(4, 4), 2)
    assert hl.bbox_head_loss(ce, L1Loss(), None, None, None, lab, w, None, None, 2) == {}
    # shapes and dtypes, with the device check out of the way
    monkeypatch.setattr(_lib, "require_gpu", lambda *a: None)
    for bad in ((x[0], lab, w), (x.reshape(4, 2, 602), lab, w), (x, lab[:3], w), (x, lab, w[:3]), (x[:, :1], lab, w)):
        with pytest.raises(ValueError):
            hl._prep(ce, *bad)
    with pytest.raises(ValueError):
        hl._prep(_iif(), x[:, :81], lab, w)                        # the table has 1204 classes
    with pytest.raises(ValueError):
        hl._prep(CrossEntropyLoss(class_weight=[1.0, 2.0]), x, lab, w)
    for bad in ((x.double(), lab, w), (x.half(), lab, w), (x, lab.float(), w), (x, lab, w.double()), (torch.zeros(4, 2049), lab, w),
                (torch.zeros(65536, 2), torch.zeros(65536, dtype=torch.int64), torch.ones(65536))):
        with pytest.raises(NotImplementedError, match=r"loss_cls\.forward"):
            hl._prep(ce, *bad)
    wide = torch.zeros(4, 1300, dtype=torch.bfloat16)[:, :1204]                          # a row-strided view is read in place
    out = hl._prep(_iif(ignore_index=7, class_weight=[0.5] * 1204), wide, lab.int(), w.bfloat16())
    assert out[0].stride(0) == 1300 and out[1].numel() == 1204 and out[2].dtype == torch.int64 and out[3].dtype == torch.float32
    assert out[4].shape == (1204,) and out[5] == 7
    assert hl._prep(ce, x.t().contiguous().t(), lab, w)[0].is_contiguous() and hl._prep(ce, x, lab, w)[1] is None


def test_which_modules_are_native():
    from iif_amd import mmdet_bbox_head_loss as hl
    from iif_amd.mmdet_ce_loss import CrossEntropyCounterLoss, CrossEntropyLoss
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    assert hl._is_native(_iif(), None) and hl._is_native(CrossEntropyLoss(), None) and hl._is_native(CrossEntropyLoss(reduction="sum"), "mean")
    assert not hl._is_native(_iif(), "none") and not hl._is_native(_iif(), "sum") and not hl._is_native(_iif(reduction="sum"), None)
    assert not hl._is_native(CrossEntropyLoss(use_sigmoid=True), None) and not hl._is_native(CrossEntropyLoss(use_mask=True), None)
    assert not hl._is_native(CrossEntropyCounterLoss(device="cpu"), None)
    assert not hl._is_native(SeesawLoss(num_classes=5, device="cpu"), None)
    assert not hl._is_native(nn.CrossEntropyLoss(), None)


class _Stub(nn.Module):
    """A loss module that is not ours: records what it was called with."""

    def __init__(self, as_dict=False):
        super().__init__()
        self.custom_activation = True
        self.as_dict = as_dict
        self.calls = []

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None):
        self.calls.append((avg_factor, reduction_override))
        loss = (cls_score.sum(1) * weight).sum() / avg_factor
        return dict(loss_cls_objectness=loss, loss_cls_classes=2 * loss) if self.as_dict else loss

    def get_accuracy(self, cls_score, labels):
        return dict(acc_classes=cls_score.new_tensor([12.5]))


def test_a_module_that_is_not_native_takes_the_references_lines():
    from iif_amd import mmdet_bbox_head_loss as hl
    x = torch.arange(12, dtype=torch.float32).reshape(4, 3).requires_grad_(True)
    lab = torch.tensor([0, 1, 2, 0])
    w = torch.tensor([1.0, 0.0, 2.0, -1.0])
    stub = _Stub()
    out = hl.head_cls_loss(stub, x, lab, w, reduction_override="sum")
    assert stub.calls == [(2.0, "sum")] and out["avg_factor"] == 2.0 and isinstance(out["avg_factor"], float)
    assert set(out) == {"loss_cls", "acc_classes", "avg_factor"} and float(out["acc_classes"]) == 12.5
    assert float(out["loss_cls"].detach()) == float(((x.detach().sum(1) * w).sum() / 2.0))
    out["loss_cls"].backward()
    assert torch.equal(x.grad, (w / 2.0)[:, None].expand(4, 3))
    both = hl.bbox_head_loss(_Stub(as_dict=True), None, x, None, None, lab, torch.zeros(4), None, None, 3)
    assert set(both) == {"loss_cls_objectness", "loss_cls_classes", "acc_classes"}               # the reference's keys: no avg_factor
    assert hl.head_cls_loss(stub, x[:0], lab[:0], w[:0]) == {"avg_factor": 1.0}                    # bbox_head.py:268: nothing for an empty batch
    assert hl.bbox_head_loss(stub, None, x[:0], None, None, lab[:0], w[:0], None, None, 3) == {}


def test_c_entries_reject_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory: nothing may be launched."""
    L = _lib.lib()
    raw = (ctypes.c_float * 64)()
    p = ctypes.addressof(raw)
    p += (-p) % 16
    call = lambda fn, spec: (lambda **k: fn(*[k.get(a, d) for a, d in spec]))        # noqa: E731
    fwd = call(L.iif_head_loss_fwd, (("scores", p), ("dtype", _lib.IIF_F32), ("ld", 8), ("table", None), ("labels", p), ("weights", p),
                                     ("cw", None), ("ignore", -100), ("lw", 1.0), ("n", 2), ("c", 8), ("dscores", p), ("ld_d", 8),
                                     ("loss", p), ("acc", p), ("avg", p), ("status", None), ("ws", p), ("stream", None)))
    for name in ("scores", "labels", "loss", "acc", "avg", "ws"):
        assert fwd(**{name: None}) == -1, name
    assert fwd(n=-1) == -1 and fwd(n=65536) == -1
    assert fwd(c=1) == -1 and fwd(c=0) == -1 and fwd(c=-5) == -1
    assert fwd(dtype=7) == -1
    assert fwd(ld=7) == -1 and fwd(ld_d=7) == -1                     # rows that overlap
    assert fwd(scores=p + 2) == -1 and fwd(dscores=p + 2) == -1 and fwd(ws=p + 2) == -1       # not element-aligned
    assert fwd(c=2049, ld=2049, ld_d=2049) == -2                    # IIF_EUNSUPPORTED
    bwd = call(L.iif_head_loss_bwd, (("d", p), ("dtype", _lib.IIF_F32), ("n", 16), ("g", p), ("avg", p), ("lw", 1.0), ("out", p),
                                     ("stream", None)))
    for name in ("d", "g", "avg", "out"):
        assert bwd(**{name: None}) == -1, name
    assert bwd(n=-1) == -1 and bwd(dtype=7) == -1 and bwd(d=p + 2) == -1 and bwd(out=p + 1) == -1
    assert bwd(n=0) == 0                                             # nothing to do: IIF_OK, nothing enqueued
