"""Host-side checks of the sigmoid and Seesaw kinds of BBoxHead.loss without a host read (iif_amd/mmdet_bbox_head_loss.py,
csrc/head_loss.hip, csrc/seesaw_head.hip): no device.

  * the header declares the three entries, the library exports them and the ctypes table lists them;
  * the float64 restatement of tests/head_loss_kinds_cases.py reproduces the REFERENCE's own BBoxHead.loss
    (tests/golden/g38_head_loss_kinds.npz, written by tests/golden/make_golden_head_loss_kinds.py): the float64 losses and the
    kept gradient elements to 1e-12, avg_factor, the accuracies and cum_samples exactly;
  * which loss modules are which native kind;
  * a sigmoid or Seesaw call outside the kernels' limits reaches the module's own forward with a host avg_factor;
  * the C entries reject bad arguments before any launch.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from iif_amd import _lib
from tests import head_loss_kinds_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_head_bce_loss_fwd", "iif_seesaw_head_fwd", "iif_seesaw_head_bwd")


def test_header_library_and_ctypes_table_have_the_entries():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "include/iif_amd.h does not declare " + name
        assert hasattr(lib, name), "libiif_amd.so does not export " + name
        assert name in _lib.SIGNATURES
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name]) == len(params.split(",")), name
    m = re.search(r"#define\s+IIF_SEESAW_HEAD_WORKSPACE_BYTES\s+\((.*?)\)\s*$", code, flags=re.M)
    assert m, "no workspace-size macro of its own"
    from iif_amd import mmdet_bbox_head_loss as hl
    assert eval(m.group(1)) == 4 * hl.SEESAW_HEAD_WORKSPACE_WORDS


def test_the_cases_cover_what_they_should():
    ns = [c["N"] for c in kc.CASES.values()]
    for n in (1, 3, 4, 5, 63, 64, 65, 257):
        assert ns.count(n) >= 2, n
    for kind, cs in (("sig", (1, 2, 5, 80, 1203, 2048)), ("see", (2, 5, 80, 1203, 2046))):
        have = [c["C"] for c in kc.CASES.values() if c["kind"] == kind]
        assert sorted(set(have)) == sorted(cs)
        for v in cs:
            assert have.count(v) >= 2, (kind, v)
    assert {(c["p"], c["q"]) for c in kc.CASES.values() if c["kind"] == "see"} == {(0.8, 2.0), (0.0, 2.0), (0.8, 0.0)}
    for name, c in kc.CASES.items():
        x, labels, w = kc.inputs(name)
        if c["pad"] == kc.PAD_MIXED and c["N"] >= 63:
            assert 0.15 < float((w == 0).mean()) < 0.35, name                  # one row in four is padding
        if c["pad"] == kc.PAD_ALL:
            assert not w.any()
        if c["pad"] == kc.PAD_ONE:
            assert int((w != 0).sum()) == 1
        if c["neg"]:
            assert (w < 0).any(), name
        if c["bf"]:
            assert np.array_equal(kc.bf16_round(x), x) and c["kind"] == "sig"
    x, labels, w = kc.inputs("g63x1203")
    live = w != 0
    assert (labels[live] == 11).any() and (labels[live] == -1).any() and (labels[live] >= 1203).any()      # ignored, background
    assert (kc.inputs("s63x5bg")[1] == 5).all() and (kc.inputs("s65x5pos")[1] < 5).all()
    assert kc.cum_before(kc.STATE[0]).any() and np.array_equal(kc.cum_before(kc.STATE[2]), kc.cum_after(kc.STATE[1]))


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_restatement_reproduces_the_reference(golden, name):
    g = golden("g38_head_loss_kinds")
    kc.check_generator(g)
    c = kc.CASES[name]
    see = c["kind"] == "see"
    x, labels, w = kc.inputs(name)
    r = kc.restate_case(name)
    want = (r["loss_cls"], r["loss_obj"]) if see else (r["loss"],)
    for a, b in zip(want, g[name + "_loss64"]):
        assert abs(a - float(b)) <= 1e-12 * abs(float(b)), (name, a, b)
    assert r["avg"] == float(g[name + "_avg"])
    acc = np.concatenate([r["acc_cls"], r["acc_obj"]] if see else [r["acc"]])
    assert np.array_equal(acc, g[name + "_acc_valid"])
    if not (w < 0).any():
        assert np.array_equal(g[name + "_acc_valid"], g[name + "_acc_compact"])
    if c["pad"] == kc.PAD_NONE:
        assert np.array_equal(g[name + "_acc_valid"], g[name + "_acc_padded"])
    elif c["pad"] == kc.PAD_MIXED and c["N"] >= 63 and c["labels"] is None:
        assert not np.array_equal(g[name + "_acc_valid"], g[name + "_acc_padded"])        # the reference dilutes it by the padding
    rows, cols = kc.kept(name)
    gmax = float(g[name + "_gmax64"])
    assert np.abs(r["grad"]).max() == pytest.approx(gmax, rel=1e-12, abs=0.0)
    assert np.abs(r["grad"][np.ix_(rows, cols)] - g[name + "_grad64"]).max() <= 1e-12 * max(gmax, 1e-300)
    dead = w[rows] == 0
    assert not g[name + "_grad32"][dead].any() and not g[name + "_grad64"][dead].any()
    if see:
        assert np.array_equal(r["cum"], g[name + "_cum"]) and np.array_equal(r["cum"], kc.cum_after(name))
        if (w == 0).any():            # the reference counts every padding row into its label's class
            assert g[name + "_cum_padded"].sum() - g[name + "_cum"].sum() == float((w == 0).sum())
    # a NaN in a row of weight zero is never touched
    xn, ln = x.copy(), labels.copy()
    xn[w == 0], ln[w == 0] = np.nan, -12345
    if see:
        b = kc.restate_seesaw(xn, ln, w, kc.cum_before(name), c["C"], c["p"], c["q"], c["lw"])
        assert (b["loss_cls"], b["loss_obj"]) == want and np.array_equal(b["cum"], r["cum"])
    else:
        b = kc.restate_sigmoid(xn, ln, w, kc.class_weight(name), c["ignore"], c["lw"])
        assert b["loss"] == r["loss"]
    assert np.array_equal(b["grad"], r["grad"])


def _iif(**kw):
    from iif_amd.mmdet_iif_loss import IIFLoss
    from tests.bbox_head_loss_cases import LVIS_CSV
    return IIFLoss(path=LVIS_CSV, num_classes=1203, device="cpu", **kw)


def test_which_modules_are_which_kind():
    from iif_amd import mmdet_bbox_head_loss as hl
    from iif_amd.mmdet_ce_loss import CrossEntropyCounterLoss, CrossEntropyLoss
    from iif_amd.mmdet_fasa import FasaIIFLoss
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    kind = hl._native_kind
    see = SeesawLoss(num_classes=5, device="cpu")
    assert kind(_iif(), None) == "softmax" and kind(CrossEntropyLoss(), None) == "softmax"
    assert kind(CrossEntropyLoss(use_sigmoid=True), None) == "sigmoid" and kind(CrossEntropyLoss(use_sigmoid=True, reduction="sum"), "mean") == "sigmoid"
    assert kind(see, None) == "seesaw" and kind(SeesawLoss(num_classes=5, device="cpu", return_dict=False), "mean") == "seesaw"
    for red in ("none", "sum"):
        assert kind(CrossEntropyLoss(use_sigmoid=True), red) is None and kind(see, red) is None and kind(_iif(), red) is None
    assert kind(CrossEntropyLoss(use_sigmoid=True, reduction="sum"), None) is None
    assert kind(CrossEntropyLoss(use_mask=True), None) is None
    assert kind(CrossEntropyCounterLoss(device="cpu"), None) is None and kind(CrossEntropyCounterLoss(use_sigmoid=True, device="cpu"), None) is None
    assert kind(nn.CrossEntropyLoss(), None) is None and kind(nn.BCEWithLogitsLoss(), None) is None
    # every IIFLoss instance keeps today's route, whatever flags a subclass carries: never the sigmoid kernel
    fasa = FasaIIFLoss(use_sigmoid=True, path=kc_lvis(), num_classes=1203, device="cpu")
    assert kind(fasa, None) != "sigmoid" and (kind(fasa, None) == "softmax") == hl._is_native(fasa, None)
    # _is_native keeps its meaning: the softmax kind, and nothing else
    for m in (_iif(), CrossEntropyLoss(), CrossEntropyLoss(use_sigmoid=True), see, CrossEntropyCounterLoss(device="cpu"), nn.CrossEntropyLoss()):
        for red in (None, "mean", "sum"):
            assert hl._is_native(m, red) == (kind(m, red) == "softmax")


def kc_lvis():
    from tests.bbox_head_loss_cases import LVIS_CSV
    return LVIS_CSV


def test_a_call_outside_the_limits_takes_the_modules_own_forward(monkeypatch):
    """More than 2048 columns, more than 65535 rows, float16 / float64 scores, floating-point labels: today's behaviour, the
    reference's lines with a host avg_factor - and no exception from the native path."""
    from iif_amd import mmdet_bbox_head_loss as hl
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    calls = []

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, **kw):
        calls.append((type(self).__name__, avg_factor, reduction_override))
        loss = cls_score.float().sum() * 0.0
        return dict(loss_cls_objectness=loss, loss_cls_classes=loss) if getattr(self, "return_dict", False) else loss

    monkeypatch.setattr(CrossEntropyLoss, "forward", forward)
    monkeypatch.setattr(SeesawLoss, "forward", forward)
    monkeypatch.setattr(SeesawLoss, "get_accuracy", lambda self, s, l: dict(acc_objectness=s.new_zeros(1), acc_classes=s.new_zeros(1)))
    monkeypatch.setattr(hl, "topk_hit_counts", lambda s, l, k: torch.zeros(1))
    sig = CrossEntropyLoss(use_sigmoid=True)
    lab4, w4 = torch.zeros(4, dtype=torch.int64), torch.tensor([1.0, 0.0, 2.0, -1.0])
    big = 65536
    sig_calls = ((torch.zeros(4, 2049), lab4, w4), (torch.zeros(4, 8, dtype=torch.float64), lab4, w4),
                 (torch.zeros(4, 8, dtype=torch.float16), lab4, w4), (torch.zeros(4, 8), lab4.float(), w4),
                 (torch.zeros(big, 1), torch.zeros(big, dtype=torch.int64), torch.ones(big)))
    for args in sig_calls:
        out = hl.head_cls_loss(sig, *args)
        assert set(out) == {"loss_cls", "acc", "avg_factor"} and isinstance(out["avg_factor"], float)
        assert out["avg_factor"] == (2.0 if args[0].shape[0] == 4 else float(big))
    assert calls == [("CrossEntropyLoss", a, None) for a in (2.0, 2.0, 2.0, 2.0, float(big))]
    del calls[:]
    see_calls = ((SeesawLoss(num_classes=2047, device="cpu"), torch.zeros(4, 2049), lab4, w4),
                 (SeesawLoss(num_classes=6, device="cpu"), torch.zeros(4, 8, dtype=torch.bfloat16), lab4, w4),
                 (SeesawLoss(num_classes=6, device="cpu"), torch.zeros(4, 8), lab4.double(), w4),
                 (SeesawLoss(num_classes=1, device="cpu", return_dict=False), torch.zeros(big, 3), torch.zeros(big, dtype=torch.int64), torch.ones(big)))
    for crit, *args in see_calls:
        out = hl.head_cls_loss(crit, *args)
        keys = {"loss_cls_objectness", "loss_cls_classes"} if crit.return_dict else {"loss_cls"}
        assert set(out) == keys | {"acc_objectness", "acc_classes", "avg_factor"} and isinstance(out["avg_factor"], float)
    assert calls == [("SeesawLoss", a, None) for a in (2.0, 2.0, 2.0, float(big))]
    # inside the limits the native path is taken: it wants the device and says so
    for crit, x in ((sig, torch.zeros(4, 8)), (SeesawLoss(num_classes=6, device="cpu"), torch.zeros(4, 8))):
        with pytest.raises(_lib.IIFNativeError):
            hl.head_cls_loss(crit, x, lab4, w4)
        with pytest.raises(_lib.IIFNativeError):
            hl.head_cls_loss(crit, x, lab4, None)                      # label_weights=None: all ones, natively
    monkeypatch.setattr(_lib, "require_gpu", lambda *a: None)
    with pytest.raises(ValueError):
        hl.head_cls_loss(sig, torch.zeros(4, 8), lab4[:3], w4)
    with pytest.raises(ValueError):
        hl.head_cls_loss(CrossEntropyLoss(use_sigmoid=True, class_weight=[1.0, 2.0]), torch.zeros(4, 8), lab4, w4)


def test_c_entries_reject_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory: nothing may be launched."""
    L = _lib.lib()
    raw = (ctypes.c_float * 64)()
    p = ctypes.addressof(raw)
    p += (-p) % 16
    call = lambda fn, spec: (lambda **k: fn(*[k.get(a, d) for a, d in spec]))        # noqa: E731
    bce = call(L.iif_head_bce_loss_fwd, (("scores", p), ("dtype", _lib.IIF_F32), ("ld", 8), ("labels", p), ("weights", p), ("cw", None),
                                         ("ignore", -100), ("lw", 1.0), ("n", 2), ("c", 8), ("dscores", p), ("ld_d", 8), ("loss", p),
                                         ("acc", p), ("avg", p), ("ws", p), ("stream", None)))
    for name in ("scores", "labels", "loss", "acc", "avg", "ws"):
        assert bce(**{name: None}) == -1, name
    assert bce(n=-1) == -1 and bce(n=65536) == -1
    assert bce(c=0) == -1 and bce(c=-5) == -1
    assert bce(dtype=7) == -1
    assert bce(ld=7) == -1 and bce(ld_d=7) == -1                     # rows that overlap
    assert bce(scores=p + 2) == -1 and bce(dscores=p + 2) == -1 and bce(ws=p + 2) == -1       # not element-aligned
    assert bce(c=2049, ld=2049, ld_d=2049) == -2                    # IIF_EUNSUPPORTED
    see = call(L.iif_seesaw_head_fwd, (("scores", p), ("dtype", _lib.IIF_F32), ("ld", 8), ("labels", p), ("weights", p), ("cum", p),
                                       ("p", 0.8), ("q", 2.0), ("eps", 1e-2), ("lw", 1.0), ("n", 2), ("c", 6), ("dscore", p), ("ld_d", 8),
                                       ("loss", p), ("acc", p), ("avg", p), ("status", None), ("ws", p), ("stream", None)))
    for name in ("scores", "labels", "cum", "loss", "acc", "avg", "ws"):
        assert see(**{name: None}) == -1, name
    assert see(n=-1) == -1 and see(n=65536) == -1 and see(c=0) == -1
    assert see(dtype=_lib.IIF_BF16) == -1 and see(dtype=7) == -1
    assert see(p=-0.5) == -1 and see(q=-1.0) == -1 and see(eps=0.0) == -1 and see(p=float("nan")) == -1
    assert see(ld=7) == -1 and see(ld_d=7) == -1                     # a pitch below C + 2
    assert see(scores=p + 2) == -1 and see(dscore=p + 2) == -1 and see(ws=p + 2) == -1
    assert see(c=2047, ld=2049, ld_d=2049) == -2                    # C + 2 > 2048: IIF_EUNSUPPORTED
    bwd = call(L.iif_seesaw_head_bwd, (("d", p), ("ld", 8), ("n", 2), ("c", 6), ("gc", p), ("go", p), ("avg", p), ("lw", 1.0), ("out", p),
                                       ("ld_o", 8), ("stream", None)))
    for name in ("d", "gc", "go", "avg", "out"):
        assert bwd(**{name: None}) == -1, name
    assert bwd(n=-1) == -1 and bwd(c=0) == -1 and bwd(ld=7) == -1 and bwd(ld_o=7) == -1 and bwd(d=p + 2) == -1 and bwd(out=p + 1) == -1
    assert bwd(n=0) == 0                                             # nothing to do: IIF_OK, nothing enqueued
