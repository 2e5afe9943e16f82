"""mmdet CrossEntropyLoss family, the part that needs no device: the fixture tests/golden/g23_mmdet_ce.npz against the
input generator and the float64 closed forms of tests/ce_cases.py, the module's constructors, attributes and error
conventions, the CPU-tensor rejection, and the new C entry point in header, library and ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

from . import ce_cases as cc
from iif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_fixture_inputs_regenerate(golden):
    cc.check_generator(golden("g23_mmdet_ce"))


def test_float32_float64_and_closed_form_agree(golden):
    """The reference's float32 run (what the GPU tests compare with) sits <= 1e-5 from its float64 run and, its gradient, from
    the closed form (measured 4.0e-6, on the single element of the [1, 1] shape, whose gradient torch forms as sigmoid(x) - 1 in
    float32; 2.9e-7 on the other shapes), and the float64 closed form <= 5e-7 from the float64 run (measured 1.6e-7: binary_cross_entropy casts
    the targets to float32, and torch then returns float32 element losses for float64 logits too, so that run carries one
    float32 rounding).  On the [1024, 1204] mean loss the two runs agree to the last float32 bit."""
    g = golden("g23_mmdet_ce")
    worst32 = worst_cf = 0.0
    for prefix, cases in (("sig_", cc.sig_cases()), ("dense_", cc.dense_cases()), ("soft_", cc.soft_cases())):
        l32, l64, g32 = (cc.unpack(g, prefix + k) for k in ("loss", "loss64", "grad"))
        assert len(cases) == len(l32) == len(l64) == len(g32)
        for i, case in enumerate(cases):
            worst32 = max(worst32, _rel(l32[i], l64[i]))
            red = case[4]
            if prefix == "sig_":
                si, wf, cwf, af, _, ign, bf = case
                name, N, C, keep = cc.SIG_SHAPES[si]
                x, labels, weights, cw = cc.sig_inputs(si, bf)
                c_l, c_g = cc.closed_form_labels(x, labels, weights if wf else None, cw if cwf else None, ign, red,
                                                 cc.AVG_FACTOR if af else None)
            elif prefix == "dense_":
                si, ewf, cwf, af, _ = case
                name, N, C, keep = cc.SIG_SHAPES[si]
                x, t, w, cw = cc.dense_inputs(si)
                c_l, c_g = cc.closed_form_dense(x, t, w if ewf else None, cw if cwf else None, red,
                                                cc.AVG_FACTOR if af else None)
            else:
                continue
            if red == "none":
                c_l = c_l[list(keep)]
            worst_cf = max(worst_cf, _rel(c_l, l64[i]))
            worst32 = max(worst32, _rel(g32[i], c_g[list(keep)]))
    assert worst32 <= 1e-5, worst32
    assert worst_cf <= 5e-7, worst_cf
    assert g["worst"][2] == 0.0


def test_fixture_edge_batches(golden):
    g = golden("g23_mmdet_ce")
    assert float(g["allignored_mean_loss"]) == 0.0 and not g["allignored_mean_grad"].any()
    x, _, weights, cw = cc.sig_inputs(cc.shape_index("m64x81"))
    for sp in cc.SPECIALS:
        for red in ("mean", "none"):
            c_l, c_g = cc.closed_form_labels(x, cc.special_labels(sp), weights, cw, None, red)
            assert _rel(c_l, g["%s_%s_loss" % (sp, red)]) <= 2e-6 and _rel(c_g, g["%s_%s_grad" % (sp, red)]) <= 2e-6
    for mode in ("sig", "soft"):
        assert np.isnan(g["empty_" + mode][0]) and g["empty_" + mode][1] == 0.0 and float(g["empty_%s_avg" % mode]) == 0.0
    for mode in ("softmax", "sigmoid"):
        total = np.zeros(cc.COUNTER_CLASSES + 1)
        for k in range(cc.COUNTER_CALLS):
            _, labels, _ = cc.counter_inputs(mode, k)
            total += np.bincount(labels, minlength=cc.COUNTER_CLASSES + 1)
            assert np.array_equal(g["cnt_%s%d_cum_labels" % (mode, k)], total.astype(np.float32))


def test_module_imports_without_a_device_and_mirrors_the_constructors():
    from iif_amd import mmdet_ce_loss as M
    from iif_amd.mmdet_mask_loss import mask_cross_entropy
    assert M.mask_cross_entropy is mask_cross_entropy
    m = M.CrossEntropyLoss()
    assert (m.use_sigmoid, m.use_mask, m.reduction, m.class_weight, m.ignore_index, m.loss_weight) == (
        False, False, "mean", None, None, 1.0)
    assert m.cls_criterion is M.cross_entropy
    assert M.CrossEntropyLoss(use_sigmoid=True).cls_criterion is M.binary_cross_entropy
    assert M.CrossEntropyLoss(use_mask=True).cls_criterion is M.mask_cross_entropy
    m = M.CrossEntropyLoss(True, False, "sum", [1.0, 2.0], 3, 0.5)                    # the reference's positional order
    assert (m.use_sigmoid, m.reduction, m.class_weight, m.ignore_index, m.loss_weight) == (True, "sum", [1.0, 2.0], 3, 0.5)
    c = M.CrossEntropyCounterLoss(device="cpu")
    assert (c.use_sigmoid, c.use_mask, c.reduction, c.class_weight, c.loss_weight, c.use_cums, c.num_classes) == (
        False, False, "mean", None, 1.0, False, 1203)
    assert not hasattr(c, "cum_losses")
    assert M.CrossEntropyCounterLoss(use_sigmoid=True, device="cpu").cls_criterion is M.binary_cross_entropy
    assert M.CrossEntropyCounterLoss(use_mask=True, device="cpu").cls_criterion is M.mask_cross_entropy
    assert M.register_into_mmdet() is False                                          # no mmdet here: no error either


def test_counters_open_and_close():
    from iif_amd.mmdet_ce_loss import CrossEntropyCounterLoss
    c = CrossEntropyCounterLoss(reduction="sum", use_cums=True, num_classes=7, device="cpu")
    assert c.use_cums and c.reduction == "none" and c.reduction_old == "sum"
    assert c.cum_losses.shape == (8,) and c.cum_labels.shape == (8,) and c.cum_losses.dtype == torch.float32
    c.cum_losses += 1.0
    c.close_cums()
    assert not c.use_cums and c.reduction == "sum" and not c.cum_losses.any() and not c.cum_labels.any()
    c.open_cums()
    assert c.use_cums and c.reduction == "none" and c.reduction_old == "sum"


def test_error_conventions():
    from iif_amd import mmdet_ce_loss as M
    for cls, kw in ((M.CrossEntropyLoss, {}), (M.CrossEntropyCounterLoss, dict(device="cpu"))):
        with pytest.raises(AssertionError):
            cls(use_sigmoid=True, use_mask=True, **kw)
        x, lab = torch.zeros(2, 3), torch.tensor([0, 1])
        for mode in (dict(), dict(use_sigmoid=True)):
            m = cls(**mode, **kw)
            with pytest.raises(AssertionError):
                m(x, lab, reduction_override="max")
            with pytest.raises(ValueError):
                m(x, lab, avg_factor=2.0, reduction_override="sum")
    # the mask mode's asserts (cross_entropy_loss.py:155-157)
    m = M.CrossEntropyLoss(use_mask=True)
    pred, target, label = torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4), torch.tensor([0, 1])
    with pytest.raises(AssertionError):
        m(pred, target, label, reduction_override="sum")
    with pytest.raises(AssertionError):
        m(pred, target, label, avg_factor=2.0)
    with pytest.raises(AssertionError):
        m(pred, target, label, ignore_index=1)
    with pytest.raises(AssertionError):
        M.CrossEntropyLoss(use_mask=True, ignore_index=255)(pred, target, label)


def test_cpu_tensor_is_rejected_not_emulated():
    from iif_amd import mmdet_ce_loss as M
    x, lab = torch.zeros(2, 3), torch.tensor([0, 1])
    for m in (M.CrossEntropyLoss(), M.CrossEntropyLoss(use_sigmoid=True), M.CrossEntropyCounterLoss(use_sigmoid=True, device="cpu")):
        with pytest.raises(_lib.IIFNativeError):
            m(x, lab)
    with pytest.raises(_lib.IIFNativeError):
        M.binary_cross_entropy(x, torch.zeros(2, 3))


def test_fasa_iif_loss_constructs_with_either_switch(tmp_path):
    from iif_amd import mmdet_ce_loss as M
    from iif_amd.mmdet_fasa import FasaIIFLoss
    path = tmp_path / "idf.csv"
    path.write_text("raw\n" + "\n".join("1.0" for _ in range(5)) + "\n")
    m = FasaIIFLoss(use_sigmoid=True, num_classes=4, path=str(path), device="cpu", use_cums=True)
    assert m.use_sigmoid is True and m.use_mask is False and m.cls_criterion is M.binary_cross_entropy
    assert m.reduction == "none" and m.cum_losses.shape == (5,)
    m = FasaIIFLoss(use_mask=True, num_classes=4, path=str(path), device="cpu")
    assert m.use_mask is True and m.cls_criterion is M.mask_cross_entropy
    with pytest.raises(AssertionError):
        FasaIIFLoss(use_sigmoid=True, use_mask=True, num_classes=4, path=str(path), device="cpu")
    m = FasaIIFLoss(num_classes=4, path=str(path), device="cpu")                      # the IIF path is what it was
    assert m.use_sigmoid is False and m.cls_criterion == m.cross_entropy


def test_entry_point_in_header_library_and_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\biif_bce_det_fwd_bwd\s*\(", code)
    assert "iif_bce_det_fwd_bwd" in _lib.SIGNATURES and hasattr(_lib.lib(), "iif_bce_det_fwd_bwd")
    proto = re.search(r"int\s+iif_bce_det_fwd_bwd\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES["iif_bce_det_fwd_bwd"])


def test_entry_point_checks_arguments_before_launching():
    """Bad arguments return before anything touches the device."""
    f = _lib.lib().iif_bce_det_fwd_bwd
    one = 16            # a non-null stand-in: the checks below fail before any pointer is used

    def args(**kw):
        return [kw.get("x", one), kw.get("dtype", 0), kw.get("ld", 3), kw.get("labels", one), kw.get("rw", None), -100,
                kw.get("tgt", None), kw.get("ew", None), None, 1.0, kw.get("N", 4), kw.get("C", 3), None, kw.get("out", one),
                kw.get("d", None), kw.get("ldd", 3), kw.get("ws", one), None]
    assert f(*args(dtype=2)) == -1
    assert f(*args(N=-1)) == -1 and f(*args(C=0)) == -1
    assert f(*args(labels=None)) == -1                       # neither mode
    assert f(*args(tgt=one)) == -1                           # both modes
    assert f(*args(ew=one)) == -1                            # an elementwise weight belongs to the dense mode
    assert f(*args(labels=None, tgt=one, rw=one)) == -1      # a row weight belongs to the label mode
    assert f(*args(ws=None)) == -1                           # a scalar loss needs the workspace
    assert f(*args(ld=2)) == -1 and f(*args(d=one, ldd=2)) == -1
    assert f(*args(x=None)) == -1
    assert f(*args(x=18)) == -1                              # fp32 logits on a 2-byte boundary
    assert f(*args(N=0, out=None, ws=None)) == 0             # nothing to do
