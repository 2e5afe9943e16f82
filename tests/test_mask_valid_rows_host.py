"""Host-side checks of ``valid_rows`` on the plain class-selected mask predictor and the fused mask head tail, and of
``mask_head_loss`` (iif_amd/mmdet_mask_head_loss.py): no device.

  * ``valid_rows`` is a keyword of the four loss entry points, default ``False``;
  * the new C entries are declared in include/iif_amd.h and in the ctypes table (tests/test_cabi.py compares the two), and they
    refuse bad arguments before any launch;
  * ``mask_head_loss`` rejects what ``mask_targets_padded`` rejects, with the same errors;
  * the two contracts agree: ``restate64`` on the compacted rows equals ``restate64(..., valid=mask)`` on the padded batch
    rescaled by ``N / K``, to 1e-12 - the reference of the GPU tests is the one the existing label tests already use;
  * the label mapping of the ``class_agnostic`` modules.
"""
import inspect
import os
import re

import pytest
import torch

from iif_amd import _lib
from tests import mask_predictor_cases as mpc
from tests import mask_tail_cases as mtc
from tests import mask_valid_rows_cases as vc

EINVAL, OK = -1, 0

NEW_ENTRIES = ("iif_mask_predict_loss_fwd", "iif_mask_predict_loss_bwd_input", "iif_mask_predict_loss_bwd_weight",
               "iif_mask_tail_loss_fwd", "iif_mask_tail_loss_bwd_rows", "iif_mask_tail_loss_bwd_input",
               "iif_mask_tail_loss_bwd_params")


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def test_valid_rows_is_a_keyword_with_default_false():
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor, class_mask_loss
    from iif_amd.mmdet_mask_tail import FusedMaskHeadTail, upsampled_class_mask_loss
    for fn in (class_mask_loss, ClassSelectedMaskPredictor.loss, upsampled_class_mask_loss, FusedMaskHeadTail.loss):
        p = inspect.signature(fn).parameters
        assert "valid_rows" in p and p["valid_rows"].default is False, fn
        assert list(p)[-1] == "valid_rows", fn                                  # behind every existing parameter


def test_new_entries_are_in_the_header_and_in_the_ctypes_table():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iif_amd.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name


def test_new_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    one = 8                                                                     # a non-null pointer that is never followed
    fwd = lambda **k: L.iif_mask_predict_loss_fwd(one, 0, one, 4, 0, one, k.get("t", one), k.get("n", 2), 3, k.get("cin", 4), 4, 1,   # noqa: E731
                                                  0, one, one, k.get("inv", one), 0)
    assert fwd(t=0) == EINVAL and fwd(inv=0) == EINVAL and fwd(n=-1) == EINVAL
    assert fwd(cin=4096) == EINVAL and fwd(n=0) == OK
    assert L.iif_mask_predict_loss_bwd_input(0, 0, 0, one, 4, one, 2, 3, 4, 4, one, 0, 0) == EINVAL
    assert L.iif_mask_predict_loss_bwd_weight(one, 0, one, 0, 0, one, 2, 3, 4, 4, 0, one, one, 0) == EINVAL
    tail = lambda **k: L.iif_mask_tail_loss_fwd(one, 0, one, 0, one, 4, 0, one, k.get("t", one), k.get("n", 2), 3, 4, 4, 2, 2, 1, 0,  # noqa: E731
                                                one, one, k.get("inv", one), 0)
    assert tail(t=0) == EINVAL and tail(inv=0) == EINVAL and tail(n=0) == OK
    assert L.iif_mask_tail_loss_bwd_rows(one, 0, one, 0, 0, 0, 0, one, 2, 3, 4, 4, 2, 2, one, 0, 0) == EINVAL
    assert L.iif_mask_tail_loss_bwd_input(0, 0, 0, 16, one, 4, one, one, 2, 3, 4, 4, 2, 2, one, 0, 0) == EINVAL
    assert L.iif_mask_tail_loss_bwd_params(one, 0, one, 0, 0, one, 4, one, one, 2, 3, 4, 4, 2, 2, 0, one, one, 0) == EINVAL


def test_mask_head_loss_rejects_what_mask_targets_padded_rejects():
    from iif_amd.mmdet_mask_head_loss import mask_head_loss
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor
    from iif_amd.mmdet_mask_target import mask_targets_padded
    m = ClassSelectedMaskPredictor(4, 3)
    feats, gt, lb = torch.zeros(2, 4, 6, 6), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    rois = torch.zeros(2, 5)
    masks = [torch.zeros(1, 8, 8, dtype=torch.uint8)]
    bad = [
        (rois[:, :4], gt, masks, 6),                                            # rois [K, 4]
        (rois.double(), gt, masks, 6),                                          # not float32
        (rois, gt, [], 6),                                                      # no image
        (rois, gt, masks * 17, 6),                                              # too many images
        (rois, gt, masks, 65),                                                  # a mask size without a kernel
    ]
    for r, g, ms, size in bad:
        with pytest.raises((ValueError, NotImplementedError)) as want:
            mask_targets_padded(r, g, ms, size)
        with pytest.raises(type(want.value)) as got:
            mask_head_loss(m, feats, r, g, lb, ms, size)
        assert str(got.value) == str(want.value)


@pytest.mark.parametrize("name", vc.PREDICTOR_CASES)
def test_predictor_compacted_rows_equal_the_valid_mask_contract_rescaled(name):
    x, w, b, lb, t, valid = vc.predictor_batch(name, 0.0)                       # finite contents: restate64 multiplies them by 0
    n, k = valid.numel(), int(valid.sum())
    masked = mpc.restate64(x, w, b, lb, t, 1.0, valid)
    compact = mpc.reference64(name)
    assert abs(float(masked["loss"]) * n / k - float(compact["loss"])) <= 1e-12 * abs(float(compact["loss"]))
    assert _rel(masked["dx"][valid] * n / k, compact["dx"]) <= 1e-12 and not masked["dx"][~valid].any()
    assert _rel(masked["dweight"] * n / k, compact["dweight"]) <= 1e-12
    assert _rel(masked["dbias"] * n / k, compact["dbias"]) <= 1e-12 or not compact["dbias"].any()


@pytest.mark.parametrize("name", vc.TAIL_CASES)
def test_tail_compacted_rows_equal_the_valid_mask_contract_rescaled(name):
    f, uw, ub, w, b, lb, t, valid = vc.tail_batch(name, 0.0)
    n, k = valid.numel(), int(valid.sum())
    masked = mtc.restate64(f, uw, ub, w, b, lb, t, 1.0, valid)
    compact = mtc.reference64(name)
    assert abs(float(masked["loss"]) * n / k - float(compact["loss"])) <= 1e-12 * abs(float(compact["loss"]))
    assert _rel(masked["df"][valid] * n / k, compact["df"]) <= 1e-12 and not masked["df"][~valid].any()
    for key in ("dup_weight", "dup_bias", "dweight"):
        assert _rel(masked[key] * n / k, compact[key]) <= 1e-12, key
    assert _rel(masked["dbias"] * n / k, compact["dbias"]) <= 1e-12 or not compact["dbias"].any()


def test_padded_batches_have_the_layout_the_cases_promise():
    for name in vc.PREDICTOR_CASES:
        x, w, _, lb, t, valid = vc.predictor_batch(name)
        c, n = w.shape[0], mpc.CASES[name][0]
        assert valid.numel() == n + 4 and not valid[0] and not valid[-1] and int((~valid).sum()) == 4
        assert sorted(lb[~valid].tolist()) == sorted(vc.invalid_labels(c))
        assert torch.isnan(x[~valid]).all() and torch.isnan(t[~valid]).all() and torch.equal(x[valid], mpc.inputs(name)[0])
        mid = (~valid).nonzero().flatten()[1:3]
        assert 0 < int(mid[0]) and int(mid[1]) < n + 3
    for count, (n, where) in vc.COUNT_CASES.items():
        valid = vc.predictor_count_batch(count)[5]
        assert valid.numel() == n and int(valid.sum()) == len(where)


def test_class_agnostic_label_mapping():
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor
    from iif_amd.mmdet_mask_tail import FusedMaskHeadTail
    from iif_amd.mmdet_normed_mask_predictor import ClassSelectedNormedMaskPredictor
    lb = torch.tensor([0, 4, 5, -1, 2, 10, 2 ** 40])
    for m in (ClassSelectedMaskPredictor(4, 5, class_agnostic=True), ClassSelectedNormedMaskPredictor(4, 5, class_agnostic=True),
              FusedMaskHeadTail(4, 4, 5, class_agnostic=True)):
        assert m._labels(lb).tolist() == [0] * 7                                # as today
        assert m._labels(lb, True).tolist() == [0, 0, -1, -1, 0, -1, -1]
    for m in (ClassSelectedMaskPredictor(4, 5), ClassSelectedNormedMaskPredictor(4, 5), FusedMaskHeadTail(4, 4, 5)):
        assert m._labels(lb, True) is lb and m._labels(lb) is lb
