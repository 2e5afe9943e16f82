"""The native multiclass_nms (csrc/multiclass_nms.hip, iif_amd/mmdet_multiclass_nms.py) on the MI355X against
tests/golden/g29_multiclass_nms.npz, which the reference's multiclass_nms and BBoxHead.get_bboxes produced on the CPU
(tests/golden/make_golden_multiclass_nms.py).

  * every case: counts, num_candidates, inds, labels, the padding and the bits of dets EXACTLY.  The overlap test is single
    float32 operations in mmcv's order, the rank is a total order and no exp is involved, so there is nothing to tolerate.
  * get_bboxes: the composition is exact against multiclass_nms_padded on the native coder's own output (the rounding of exp does
    not enter); the kept (row, class) pairs equal the reference's for the cases whose inputs the generator proved robust against
    that rounding.
"""
import types

import numpy as np
import pytest
import torch

from . import multiclass_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g29_multiclass_nms")


@pytest.fixture(scope="module")
def mm():
    from iif_amd import mmdet_multiclass_nms
    return mmdet_multiclass_nms


def _t(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None for a in arrays]


def _call(mm, dev, name, **kw):
    c = mc.case(name)
    boxes, scores, factors = _t(dev, *mc.inputs(name))
    rc = torch.tensor([c["rows"]], dtype=torch.int64, device=dev) if c["rows"] is not None else None
    return mm.multiclass_nms_padded(boxes, scores, c["score_thr"], mc.nms_cfg(name), c["max_num"], score_factors=factors,
                                    row_counts=rc, **kw)


def _check(g, name, dets, labels, inds, count, ncand):
    """One image's padded result against the fixture, exactly."""
    dets, labels, inds = dets.cpu().numpy(), labels.cpu().numpy(), inds.cpu().numpy()
    cap, want = mc.cap(name), g[name + "_inds"].astype(np.int64)
    k = int(count)
    print(name, "M", int(ncand), "expected", int(g[name + "_M"]), "kept", k, "expected", want.size)
    assert dets.shape == (cap, 5) and labels.shape == (cap,) and inds.shape == (cap,)
    assert labels.dtype == np.int64 and inds.dtype == np.int64
    assert int(ncand) == int(g[name + "_M"])
    assert k == int(g[name + "_count"]) == want.size
    assert np.array_equal(inds[:k], want)
    assert np.array_equal(labels[:k], g[name + "_labels"])
    assert (inds[k:] == -1).all() and (labels[k:] == -1).all() and not mc.bits(dets[k:]).any()
    assert np.array_equal(mc.bits(dets[:k]), mc.bits(mc.dets_from_inds(*mc.inputs(name), want)))


@pytest.mark.parametrize("name", list(mc.CASES))
def test_padded_result_is_exact(dev, g, mm, name):
    dets, labels, inds, counts, ncand = _call(mm, dev, name)
    assert counts.shape == (1,) and ncand.shape == (1,)
    _check(g, name, dets, labels, inds, counts[0].item(), ncand[0].item())


def test_select_takes_two_full_stride_steps(dev, mm):
    """32 768 kept keys in the per-class regime, cut to 100 among equal scores: the padded result against the restatement."""
    name = "long_kept"
    dets, labels, inds, M = mc.run(name)
    want = {name + "_inds": inds, name + "_labels": labels, name + "_M": M, name + "_count": inds.size}
    assert M == 32768 >= mc.split_thr(name) and inds.size == mc.cap(name) == 100
    got = _call(mm, dev, name)
    _check(want, name, got[0], got[1], got[2], got[3][0].item(), got[4][0].item())


@pytest.mark.parametrize("name", ["n130_c3", "n130_c80_split", "none", "none_split", "factors"])
def test_multiclass_nms_returns_the_reference_shapes(dev, g, mm, name):
    c = mc.CASES[name]
    boxes, scores, factors = _t(dev, *mc.inputs(name))
    want = g[name + "_inds"].astype(np.int64)
    dets, labels, inds = mm.multiclass_nms(boxes, scores, c["score_thr"], mc.nms_cfg(name), c["max_num"], score_factors=factors,
                                           return_inds=True)
    assert dets.shape == (want.size, 5) and labels.shape == (want.size,) and inds.shape == (want.size,)
    assert dets.dtype == torch.float32 and labels.dtype == torch.int64
    assert np.array_equal(inds.cpu().numpy(), want) and np.array_equal(labels.cpu().numpy(), g[name + "_labels"])
    two = mm.multiclass_nms(boxes, scores, c["score_thr"], mc.nms_cfg(name), c["max_num"], score_factors=factors)
    assert len(two) == 2 and two[0].shape == (want.size, 5) and two[1].shape == (want.size,)
    if name.startswith("none"):
        assert dets.shape == (0, 5) and labels.shape == (0,)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", ["n130_c80", "max_num_split", "ties_split"])
def test_result_is_deterministic_and_ignores_the_workspace_contents(dev, mm, name):
    c = mc.CASES[name]
    first = _call(mm, dev, name)
    ws = torch.full((mm.workspace_bytes(1, c["n"], c["C"], mc.cap(name)),), 0xFF, dtype=torch.uint8, device=dev)
    for again in (_call(mm, dev, name), _call(mm, dev, name, workspace=ws), _call(mm, dev, name, workspace=ws)):
        for a, b in zip(first, again):
            assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("batch", list(mc.BATCHES))
def test_row_counts_run_equals_the_run_on_the_truncated_inputs(dev, g, mm, batch):
    """B = 2 with row_counts shorter than R; the rows that take no part hold the highest scores."""
    names = mc.BATCHES[batch]
    c = mc.CASES[names[0]]
    ins = [mc.inputs(k) for k in names]
    boxes, scores = _t(dev, np.stack([i[0] for i in ins]), np.stack([i[1] for i in ins]))
    rows = [mc.CASES[k]["rows"] for k in names]
    assert all(mc.nms_cfg(k) == mc.nms_cfg(names[0]) and r < c["n"] for k, r in zip(names, rows))
    rc = torch.tensor(rows, dtype=torch.int64, device=dev)
    dets, labels, inds, counts, ncand = mm.multiclass_nms_padded(boxes, scores, c["score_thr"], mc.nms_cfg(names[0]), c["max_num"],
                                                                 row_counts=rc)
    assert dets.shape[0] == 2 and counts.shape == (2,)
    for i, k in enumerate(names):
        _check(g, k, dets[i], labels[i], inds[i], counts[i].item(), ncand[i].item())
        cut = mm.multiclass_nms_padded(boxes[i, :rows[i]].contiguous(), scores[i, :rows[i]].contiguous(), c["score_thr"],
                                       mc.nms_cfg(k), c["max_num"])
        for a, b in zip((dets[i], labels[i], inds[i], counts[i:i + 1], ncand[i:i + 1]), cut):
            assert torch.equal(_bits(a), _bits(b))
    # without the counts the padding rows win
    full = mm.multiclass_nms_padded(boxes, scores, c["score_thr"], mc.nms_cfg(names[0]), c["max_num"])
    assert (full[2][0, 0] // c["C"]).item() >= rows[0]


def _coder():
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder
    return DeltaXYWHBBoxCoder(mc.MEANS, mc.STDS)


@pytest.mark.parametrize("name", list(mc.GB_CASES))
def test_get_bboxes_is_the_composition_and_keeps_what_the_reference_keeps(dev, g, mm, name):
    c = mc.GB_CASES[name]
    rois, scores, pred = _t(dev, *mc.gb_inputs(name))
    cfg = types.SimpleNamespace(**mc.GB_CFG)
    coder = _coder()
    got = mm.bbox_head_get_bboxes(rois, scores, pred, mc.GB_SHAPE, mc.GB_SCALE, c["rescale"], cfg, coder, padded=True)
    # the composition, bit for bit: the native coder's own output through the padded entry
    boxes = coder.decode(rois[:, 1:], pred, max_shape=mc.GB_SHAPE) if pred is not None else rois[:, 1:].clone()
    if c["rescale"]:
        boxes = (boxes.view(boxes.size(0), -1, 4) / boxes.new_tensor(mc.GB_SCALE)).view(boxes.size(0), -1)
    want = mm.multiclass_nms_padded(boxes, scores, cfg.score_thr, cfg.nms, cfg.max_per_img)
    for a, b in zip(got, want):
        assert torch.equal(_bits(a), _bits(b))
    raw_boxes, raw_scores = mm.bbox_head_get_bboxes(rois, scores, pred, mc.GB_SHAPE, mc.GB_SCALE, c["rescale"], None, coder)
    assert torch.equal(_bits(raw_boxes), _bits(boxes)) and raw_scores is scores
    # the reference's kept (row, class) pairs (the generator proved them independent of the rounding of exp)
    k = int(got[3].item())
    ref = g[name + "_inds"].astype(np.int64)
    assert int(got[4].item()) == int(g[name + "_M"]) and k == ref.size
    assert np.array_equal(got[2].cpu().numpy()[:k], ref) and np.array_equal(got[1].cpu().numpy()[:k], g[name + "_labels"])
    det, lab = mm.bbox_head_get_bboxes(rois, scores, pred, mc.GB_SHAPE, mc.GB_SCALE, c["rescale"], cfg, coder)
    assert det.shape == (k, 5) and lab.shape == (k,) and torch.equal(_bits(det), _bits(got[0][:k]))
    if pred is None:
        assert np.array_equal(mc.bits(det.cpu().numpy()), mc.bits(mc.gb_run(name)[0]))    # no exp on this path: exact
