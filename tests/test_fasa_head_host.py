"""Host-side checks of FasaBBoxHead.loss without a host read (iif_amd/mmdet_fasa_head_loss.py, csrc/fasa_head.hip,
csrc/head_loss.hip): no device.

  * the header declares the three new entries, the library exports them and the ctypes table lists them;
  * the float32 restatement of tests/fasa_head_cases.py (torch CPU operations plus oracle.mmdet_iif's fasa_update /
    fasa_generate / fasa_accumulate) reproduces the REFERENCE's own ConvFCFASABBoxHead.loss over the whole sequence
    (tests/golden/g37_fasa_head.npz): integers exactly, floats within one float32 rounding of the float32 run; the float64
    restatement reproduces the float64 run to 1e-12;
  * the argument checks raise as documented: the limits of fa_update_rows, a capacity below 1, the sigmoid and mask modes of
    FasaIIFLoss; the C entries reject bad arguments before any launch.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from iif_amd import _lib
from tests import fasa_head_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_fasa_update_rows", "iif_fasa_generate_padded", "iif_head_loss_cums_fwd")
INTEGERS = ("used", "aug_labels", "acc_valid", "cum_labels")


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
    from iif_amd.mmdet_fasa import FasaFeatureBank
    assert re.search(r"#define\s+IIF_FASA_ROWS_MAX_ROWS\s+%d\b" % FasaFeatureBank.MAX_ROWS, code)
    assert re.search(r"#define\s+IIF_FASA_ROWS_MAX_CLASSES\s+%d\b" % FasaFeatureBank.MAX_CLASSES, code)


def test_both_update_kernels_use_the_one_arithmetic_function():
    """The bit equality of fa_update_rows and fa_update is a property of the source: one __device__ function, called by both."""
    csrc = os.path.join(ROOT, "iif_amd", "csrc")
    header = open(os.path.join(csrc, "fasa_stats.h")).read()
    assert len(re.findall(r"void\s+fasa_class_feature\s*\(", header)) == 1 and "fmaf(t, t, ss)" in header
    for name in ("fasa.hip", "fasa_head.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "fasa_stats.h"' in text and "fasa_class_feature(" in text and "fasa_virtual_sample(" in text, name
        assert "fmaf(" not in text, name                                 # no second copy of the arithmetic
    assert "-ffp-contract=off" in open(os.path.join(csrc, "Makefile")).read()


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("g37_fasa_head")


@pytest.fixture(scope="module")
def restated(fixture):
    draws = fc.fixture_draws(fixture)
    return {32: fc.restate(torch.float32, *draws), 64: fc.restate(torch.float64, *draws)}


def test_the_cases_are_what_the_issue_asks_for(fixture):
    labels = [fc.step_inputs(s)["labels"] for s in range(fc.STEPS + 1)]
    pos = [set(l[(l >= 0) & (l < fc.C)].tolist()) for l in labels]
    assert pos[0] and not pos[1] and len(pos[0] & pos[2]) >= 4 and len(pos[2] - pos[0]) >= 4
    for s in range(fc.STEPS):
        w = fc.step_inputs(s)["label_weights"]
        assert (w == 0).sum() == fc.N - fc.PAD_FROM and (labels[s][fc.PAD_FROM:] == fc.C).all()
        drawn, used = fixture["s%d_aug_labels" % s], fixture["s%d_used" % s]
        assert 3 <= len(drawn) < len(used) and set(drawn.tolist()) <= set(used.tolist())
        assert fixture["s%d_aug_normals" % s].shape == (len(drawn), fc.D)
    assert (fc.step_inputs(fc.STEPS)["label_weights"] == 1).all()
    assert fixture["rand"].shape == (fc.STEPS, fc.C)
    assert float(fixture["s1_loss_bbox32"]) == 0.0 and float(fixture["s0_loss_bbox32"]) > 0.0
    # the fixture holds outputs and draws only
    assert not [k for k in fixture.files if "score" in k or "embedding" in k or "pred" in k]


def test_restatement_reproduces_the_reference(fixture, restated):
    checked = 0
    for bits, tol in ((32, 2.0 ** -23), (64, 1e-12)):
        for key, got in restated[bits].items():
            if key.endswith(("aug_emb", "loss_main")):
                continue
            if key.endswith(INTEGERS):
                assert np.array_equal(np.asarray(got, dtype=np.float64), fixture[key].astype(np.float64)), key
            else:
                want = fixture[key + str(bits)].astype(np.float64)
                err = np.abs(np.asarray(got, dtype=np.float64) - want)
                assert got.shape == want.shape and (err <= tol * np.abs(want)).all(), (bits, key, float(err.max()))
            checked += 1
    assert checked == 2 * (7 * fc.STEPS + 5)
    # the reference's own accuracy is over ALL rows, padding included; without padding the two agree
    assert not np.array_equal(fixture["s0_acc_classes"], fixture["s0_acc_valid"])
    assert np.array_equal(fixture["val_acc_classes"], fixture["val_acc_valid"])
    assert fixture["val_cum_labels"].sum() == fc.N


def test_cums_restatement_against_the_sequence_restatement(restated):
    """cums_restate (the float64 reference of the GPU tests) gives the validation call of the sequence."""
    i = fc.step_inputs(fc.STEPS)
    r = fc.cums_restate(i["cls_score"].numpy(), fc.table().numpy().reshape(-1), i["labels"].numpy(), i["label_weights"].numpy(),
                        fc.CLS_LOSS_WEIGHT)
    want = restated[64]
    assert abs(r["loss"] - float(want["val_loss_cls"])) <= 1e-12 * abs(float(want["val_loss_cls"]))
    assert np.array_equal(r["cum_labels"], want["val_cum_labels"]) and r["avg"] == fc.N
    assert np.abs(r["cum_losses"] - want["val_cum_losses"]).max() <= 1e-12 * np.abs(want["val_cum_losses"]).max()
    assert np.array_equal(np.float32(r["acc"]).reshape(1), want["val_acc_valid"])
    # rows of weight zero holding NaN are never touched, and leave every figure alone
    x, lab, w = i["cls_score"].numpy().copy(), i["labels"].numpy(), i["label_weights"].numpy().copy()
    w[::3] = 0.0
    a = fc.cums_restate(x, fc.table().numpy().reshape(-1), lab, w, fc.CLS_LOSS_WEIGHT)
    x[::3] = np.nan
    b = fc.cums_restate(x, fc.table().numpy().reshape(-1), lab, w, fc.CLS_LOSS_WEIGHT)
    assert a["loss"] == b["loss"] and np.array_equal(a["cum_losses"], b["cum_losses"]) and a["avg"] == fc.N - len(w[::3])


# ---------------------------------------------------------------------------------------- argument checks
def _bank(c=8, d=4):
    from iif_amd.mmdet_fasa import FasaFeatureBank
    return FasaFeatureBank(c, d, [10] * c, device="cpu")


def _fasa_loss(**kw):
    from iif_amd.mmdet_fasa import FasaIIFLoss
    return FasaIIFLoss(path=fc.LVIS_CSV, num_classes=fc.C, device="cpu", **kw)


def test_update_rows_limits_name_fa_update():
    bank = _bank()
    with pytest.raises(ValueError, match="fa_update"):
        bank.fa_update_rows(torch.zeros(65536, 4), torch.zeros(65536, dtype=torch.int64))
    with pytest.raises(ValueError, match="fa_update"):
        _bank(c=4097).fa_update_rows(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        bank.fa_update_rows(torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64))             # not the bank's D
    with pytest.raises(ValueError):
        bank.fa_update_rows(torch.zeros(3, 4), torch.zeros(2, dtype=torch.int64))             # one label per row
    with pytest.raises(_lib.IIFNativeError):
        bank.fa_update_rows(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64))             # within the limits: GPU only
    bank.fa_update_rows(torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64))                  # nothing to do
    assert not bank.feature_used.any()


def test_generate_padded_capacity_and_shapes():
    bank = _bank()
    for bad in (0, -3):
        with pytest.raises(ValueError, match="capacity"):
            bank.fa_generate_padded(capacity=bad)
    with pytest.raises(ValueError):
        bank.fa_generate_padded(rand=torch.zeros(7), normal=torch.zeros(8, 4))
    with pytest.raises(ValueError):
        bank.fa_generate_padded(rand=torch.zeros(8), normal=torch.zeros(8, 5))
    with pytest.raises(_lib.IIFNativeError):
        bank.fa_generate_padded(rand=torch.zeros(8), normal=torch.zeros(8, 4), capacity=2)


def test_sigmoid_and_mask_modes_never_reach_the_softmax_path(monkeypatch):
    from iif_amd import mmdet_fasa_head_loss as fh
    from iif_amd.mmdet_iif_loss import IIFLoss
    x = torch.zeros(4, fc.C1)
    lab = torch.zeros(4, dtype=torch.int64)
    w = torch.tensor([1.0, 0.0, 2.0, 1.0])
    monkeypatch.setattr(fh, "head_cls_loss", lambda *a, **k: pytest.fail("head_cls_loss was asked"))
    monkeypatch.setattr(fh, "head_cls_loss_cums", lambda *a, **k: pytest.fail("head_cls_loss_cums was asked"))
    for kw in (dict(use_sigmoid=True), dict(use_mask=True), dict(use_sigmoid=True, use_cums=True)):
        crit = _fasa_loss(**kw)
        assert isinstance(crit, IIFLoss)                                    # which is why head_cls_loss would take it for a softmax loss
        calls = []

        def forward(cls_score, label, weight=None, avg_factor=None, reduction_override=None, _calls=calls):
            _calls.append((avg_factor, reduction_override))
            return cls_score.sum()
        monkeypatch.setattr(crit, "forward", forward)
        monkeypatch.setattr(crit, "get_accuracy", lambda s, l: dict(acc_classes=s.new_tensor([50.0])))
        out = fh.fasa_cls_loss(crit, x, lab, w)
        assert calls == [(3.0, None)] and out["avg_factor"] == 3.0 and set(out) == {"loss_cls", "acc_classes", "avg_factor"}
    monkeypatch.undo()
    for kw in (dict(use_sigmoid=True, use_cums=True), dict(use_mask=True, use_cums=True)):
        with pytest.raises(ValueError, match="use_sigmoid"):
            fh.head_cls_loss_cums(_fasa_loss(**kw), x, lab, w)


def test_cums_path_argument_checks(monkeypatch):
    from iif_amd import mmdet_fasa_head_loss as fh
    from iif_amd.mmdet_iif_loss import IIFLoss
    x = torch.zeros(4, fc.C1)
    lab = torch.zeros(4, dtype=torch.int64)
    w = torch.ones(4)
    with pytest.raises(ValueError, match="FasaIIFLoss"):
        fh.head_cls_loss_cums(IIFLoss(path=fc.LVIS_CSV, num_classes=fc.C, device="cpu"), x, lab, w)
    with pytest.raises(ValueError, match="closed"):
        fh.head_cls_loss_cums(_fasa_loss(), x, lab, w)
    opened = _fasa_loss(use_cums=True)
    for red in ("mean", "sum"):
        with pytest.raises(ValueError, match="reduction_override"):
            fh.head_cls_loss_cums(opened, x, lab, w, reduction_override=red)
    with pytest.raises(_lib.IIFNativeError):
        fh.head_cls_loss_cums(opened, x, lab, w)                            # all checks passed: GPU only
    # the router: closed accumulators go to head_cls_loss, open ones to head_cls_loss_cums
    seen = []
    monkeypatch.setattr(fh, "head_cls_loss", lambda *a, **k: seen.append("closed") or {"avg_factor": 1.0})
    monkeypatch.setattr(fh, "head_cls_loss_cums", lambda *a, **k: seen.append("open") or {"avg_factor": 1.0, "rows": None})
    fh.fasa_cls_loss(_fasa_loss(), x, lab, w)
    fh.fasa_cls_loss(opened, x, lab, w)
    fh.fasa_cls_loss(opened, x, lab, w, reduction_override="mean")          # the reference cannot index a reduced loss: its lines
    assert seen == ["closed", "open", "closed"]
    with pytest.raises(ValueError, match="num_classes"):
        fh.fasa_bbox_head_loss(_bank(), opened, None, None, x, None, None, lab, w, None, None, None, fc.C)


def test_c_entries_reject_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory: nothing may be launched."""
    L = _lib.lib()
    raw = (ctypes.c_float * 64)()
    p = ctypes.addressof(raw)
    p += (-p) % 16
    call = lambda fn, spec: (lambda **k: fn(*[k.get(a, d) for a, d in spec]))        # noqa: E731
    upd = call(L.iif_fasa_update_rows, (("emb", p), ("labels", p), ("n", 2), ("d", 4), ("ld", 4), ("c", 8), ("decay", 0.1), ("mean", p),
                                        ("var", p), ("used", p), ("present", p), ("stream", None)))
    for name in ("emb", "labels", "mean", "var", "used", "present"):
        assert upd(**{name: None}) == -1, name
    assert upd(n=-1) == -1 and upd(d=0) == -1 and upd(c=0) == -1 and upd(ld=3) == -1
    assert upd(n=65536) == -2 and upd(c=4097) == -2                  # IIF_EUNSUPPORTED: the documented limits
    assert upd(n=0) == 0                                             # nothing to do: IIF_OK, nothing enqueued
    gen = call(L.iif_fasa_generate_padded, (("rnd", p), ("prob", p), ("used", p), ("mean", p), ("var", p), ("normal", p), ("c", 8),
                                            ("d", 4), ("cap", 8), ("w", 0.1), ("out", p), ("labels", p), ("weights", p), ("count", p),
                                            ("stream", None)))
    for name in ("rnd", "prob", "used", "mean", "var", "normal", "out", "labels", "weights", "count"):
        assert gen(**{name: None}) == -1, name
    assert gen(c=0) == -1 and gen(d=0) == -1 and gen(cap=0) == -1 and gen(cap=-1) == -1
    fwd = call(L.iif_head_loss_cums_fwd, (("scores", p), ("dtype", _lib.IIF_F32), ("ld", 8), ("table", None), ("labels", p),
                                          ("weights", p), ("cw", None), ("ignore", -100), ("lw", 1.0), ("n", 2), ("c", 8), ("dscores", p),
                                          ("ld_d", 8), ("rows", p), ("cl", p), ("cn", p), ("loss", p), ("acc", p), ("avg", p),
                                          ("status", None), ("ws", p), ("stream", None)))
    for name in ("scores", "labels", "rows", "cl", "cn", "loss", "acc", "avg", "ws"):
        assert fwd(**{name: None}) == -1, name
    assert fwd(n=-1) == -1 and fwd(n=65536) == -1 and fwd(c=1) == -1 and fwd(dtype=7) == -1
    assert fwd(ld=7) == -1 and fwd(ld_d=7) == -1 and fwd(scores=p + 2) == -1 and fwd(ws=p + 2) == -1
    assert fwd(c=2049, ld=2049, ld_d=2049) == -2
