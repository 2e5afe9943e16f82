#!/usr/bin/env python3
"""Generate tests/golden/g29_multiclass_nms.npz by RUNNING THE REFERENCE's multiclass_nms
(instance_segmentation/mmdet/core/post_processing/bbox_nms.py) and BBoxHead.get_bboxes
(models/roi_heads/bbox_heads/bbox_head.py) on the CPU in float32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_multiclass_nms.py <reference checkout>

The reference is imported under the placeholder modules of make_golden_targets.py; ``mmcv.ops.nms.batched_nms`` is the placeholder
stated in make_golden_nms.py (mmcv 1.3.8's definition as a small torch function).  get_bboxes is called unbound on a stand-in
``self`` whose ``loss_cls.get_activation`` is the identity (the scores of the cases are already activated) and whose coder is
the reference's.  Nothing from the reference is written to the repository except results.

Stored: identities (``inds``, ``labels``), counts, ``M`` and input checksums.  Nothing that went through exp is stored.

Before storing anything the generator asserts:
  * the numpy restatement (tests/multiclass_cases.py) equals the reference exactly - ``inds``, ``labels`` and the bits of ``dets``
    - on every case whose scores are distinct; tie cases are stored from the restatement only and marked;
  * each case's ``M`` lies on the intended side of its ``split_thr``, and the three boundary cases sit at M = split_thr - 1,
    M = split_thr and M > split_thr on the same inputs; the truncating cases truncate;
  * in every random case the greedy result differs from "any higher-ranked box suppresses";
  * in the ``negative`` case the all-pairs and the per-class results differ;
  * for the get_bboxes cases that decode: the kept (row, class) pairs do not change when the NMS is rerun on the float64
    continuation of the decode, or on eight copies whose coordinates are moved by random whole numbers of float32 ulps in
    [-4, 4] and clipped again (a coordinate the clip replaced is not moved), and no pair of candidates that take part has an IoU
    within 1e-4 of the threshold on the float64 shifted boxes.  The seed of these cases is chosen so that this holds: a
    condition on the inputs that makes the comparison independent of the rounding of exp, not a tolerance on the result.
"""
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_golden_targets as mgt              # noqa: E402
import make_golden_nms as mgn                  # noqa: E402
from tests import multiclass_cases as mc       # noqa: E402
from tests import nms_cases as nc              # noqa: E402
from tests import targets_cases as tc          # noqa: E402

torch.set_num_threads(1)
T = torch.from_numpy


def reference(ref_root):
    R = mgn.reference(ref_root)
    mm = os.path.join(ref_root, "instance_segmentation", "mmdet")
    mgt._pkg("mmcv.ops.nms", batched_nms=mgn.batched_nms, nms=mgn.nms)
    mgt._pkg("mmdet.core.bbox.iou_calculators", bbox_overlaps=None)
    mgt._pkg("mmdet.core.post_processing", os.path.join(mm, "core", "post_processing"))
    bn = importlib.import_module("mmdet.core.post_processing.bbox_nms")
    assert os.path.samefile(bn.__file__, os.path.join(mm, "core", "post_processing", "bbox_nms.py"))
    sys.modules[R.BBoxHead.__module__].multiclass_nms = bn.multiclass_nms      # bbox_head imported it by name
    R.multiclass_nms = bn.multiclass_nms
    return R


def distinct(a):
    return np.unique(nc.bits(a)).size == np.asarray(a).size


def greedy_differs(name):
    """Does the greedy walk differ from 'any higher-ranked box suppresses' on the case's ranked shifted boxes (per class in the
    per-class regime)?"""
    c = mc.CASES[name]
    boxes, scores, factors = mc.inputs(name)
    n, C = c["n"], c["C"]
    b = boxes.reshape(n, C, 4).reshape(-1, 4)
    s = scores[:, :C].reshape(-1)
    inds = np.nonzero(s > np.float32(c["score_thr"]))[0]
    lab = inds % C
    sh = nc.shifted_np(b[inds], lab)
    order = nc.rank_np(s[inds])
    if inds.size < mc.split_thr(name):
        return not np.array_equal(nc.greedy_np(sh[order], c["thr"], c["offset"]), nc.any_higher_np(sh[order], c["thr"], c["offset"]))
    for k in np.unique(lab):
        o = order[lab[order] == k]
        if not np.array_equal(nc.greedy_np(sh[o], c["thr"], c["offset"]), nc.any_higher_np(sh[o], c["thr"], c["offset"])):
            return True
    return False


# ---------------------------------------------------------------------------------------------- get_bboxes robustness
def decode64(rois, pred):
    """The float64 continuation of the decode (from the bit-exact float32 intermediates) [n, 4 C], clipped; and unclipped."""
    gx, gy, pw, ph, dw, dh = tc.decode_parts_np(rois[:, 1:], pred, mc.MEANS, mc.STDS, tc.WH_RATIO_CLIP, False, 32)
    gw = pw.astype(np.float64) * np.exp(dw.astype(np.float64))
    gh = ph.astype(np.float64) * np.exp(dh.astype(np.float64))
    gx, gy = gx.astype(np.float64), gy.astype(np.float64)
    raw = np.stack([gx - 0.5 * gw, gy - 0.5 * gh, gx + 0.5 * gw, gy + 0.5 * gh], axis=-1).reshape(rois.shape[0], -1)
    return tc._clip_np(raw, mc.GB_SHAPE, raw.shape[1] // 4), raw


def gb_problems(name):
    c = mc.GB_CASES[name]
    rois, scores, pred = mc.gb_inputs(name)
    C = c["C"]
    base = mc.gb_run(name)
    b64, raw = decode64(rois, pred)
    problems = []
    if not np.array_equal(mc.gb_run(name, boxes=b64.astype(np.float32))[2], base[2]):
        problems.append("float64 decode changes the result")
    b32 = tc.delta2bbox_np(rois[:, 1:], pred, *mc.decode_args())
    rng = np.random.RandomState(1000 * c["seed"] + 17)
    free = b64 == raw
    for t in range(8):
        moved = b32 + np.where(free, rng.randint(-4, 5, size=b32.shape), 0).astype(np.float32) * np.spacing(np.abs(b32))
        if not np.array_equal(mc.gb_run(name, boxes=tc._clip_np(moved.astype(np.float32), mc.GB_SHAPE, C))[2], base[2]):
            problems.append("ulp perturbation %d changes the result" % t)
    f64 = b64.reshape(-1, C, 4) / mc.GB_SCALE.astype(np.float64) if c["rescale"] else b64.reshape(-1, C, 4)
    inds = np.nonzero(scores[:, :C].reshape(-1) > np.float32(mc.GB_CFG["score_thr"]))[0]
    v = f64.reshape(-1, 4)[inds]
    v = v + ((inds % C).astype(np.float64) * (v.max() + 1.0))[:, None]
    iou = mgn.iou64(v)
    np.fill_diagonal(iou, np.nan)
    near = np.abs(iou - mc.GB_CFG["nms"]["iou_threshold"]) < 1e-4
    if near.any():
        problems.append("%d pairs with an IoU within 1e-4 of the threshold" % (int(near.sum()) // 2))
    return problems


def store(out, name, res, from_ref):
    dets, labels, inds, M = res
    out[name + "_inds"] = inds.astype(np.int32)
    out[name + "_labels"] = labels.astype(np.int16)
    out[name + "_count"] = np.array(inds.size, dtype=np.int32)
    out[name + "_M"] = np.array(M, dtype=np.int32)
    out[name + "_from_ref"] = np.array(bool(from_ref))


def main():
    if len(sys.argv) > 2 and sys.argv[2] == "--scan-seeds":
        for name in sys.argv[3:]:
            for seed in range(12):
                mc.GB_CASES[name]["seed"] = seed
                print(name, "seed", seed, gb_problems(name) or "ok")
        return
    R = reference(sys.argv[1])
    warnings.simplefilter("ignore")
    out = dict(mc.input_checksums())

    for name, c in mc.CASES.items():
        boxes, scores, factors = mc.inputs(name)
        mine = mc.run(name)
        dets, labels, inds, M = mine
        split = mc.split_thr(name)
        tie = name in mc.TIE_CASES
        rows = c["rows"] if c["rows"] is not None else c["n"]
        valid_scores = scores[:rows, :c["C"]][scores[:rows, :c["C"]] > np.float32(c["score_thr"])]
        assert M == mc.candidates(name) == valid_scores.size
        assert tie == (not distinct(valid_scores)), name
        # the intended regime
        if name.startswith("none"):
            assert M == 0
        elif name == "n1_c1_split":
            assert M == 1 < split                                   # one candidate: below any split_thr >= 2
        elif name.endswith("_split") or name in ("dense", "dense_cut", "lvis", "bnd_at", "bnd_above"):
            assert M >= split, (name, M, split)
        else:
            assert 0 < M < split, (name, M, split)
        if name == "lvis":
            assert M >= 10000 and "split_thr" not in mc.nms_cfg(name)
        if name == "flat_full":
            assert 15 * 1024 < M < split == 16384 and 1024 < inds.size < mc.cap(name)      # every slot of the walk holds a box
        if name == "dense":
            assert M == 2048 and inds.size > 0
        if name in mc.TRUNCATED:
            full = mc.run(name, nms_max_num=-1, max_num=-1)[2]
            assert inds.size == mc.cap(name) < full.size, (name, inds.size, full.size)
            if name.startswith("nms_max"):
                assert c["nms_max"] < c["max_num"]
        if c["kind"] == "pad_high":
            assert scores[c["rows"]:, :c["C"]].min() > scores[:c["rows"]].max()
        if name in mc.RANDOM_CASES:
            assert greedy_differs(name), (name, "the greedy scan and 'any higher-ranked box' agree")
        if not tie:
            f = T(factors[:rows].copy()) if factors is not None else None
            rd, rl, ri = R.multiclass_nms(T(boxes[:rows].copy()), T(scores[:rows].copy()), c["score_thr"], mc.nms_cfg(name), c["max_num"],
                                          score_factors=f, return_inds=True)
            assert rd.shape == (inds.size, 5) and rl.shape == (inds.size,), (name, rd.shape, inds.size)
            assert np.array_equal(ri.numpy(), inds) and np.array_equal(rl.numpy(), labels), name
            assert np.array_equal(nc.bits(rd.numpy()), nc.bits(dets)), name
        store(out, name, mine, not tie)
        print("%-20s n %4d C %4d: M %6d split_thr %6d, %4d kept%s" % (name, c["n"], c["C"], M, split, inds.size,
                                                                      " (restatement only)" if tie else ""))
    m = [mc.candidates(k) for k in ("bnd_below", "bnd_at", "bnd_above")]
    assert m[0] == m[1] == m[2] and mc.split_thr("bnd_below") == m[0] + 1 and mc.split_thr("bnd_at") == m[0] and mc.split_thr("bnd_above") < m[0]
    assert np.array_equal(out["in_bnd_below"], out["in_bnd_at"]) and np.array_equal(out["in_bnd_at"], out["in_bnd_above"])
    neg, per = mc.run("negative"), mc.per_class_np(*mc.inputs("negative")[:2], mc.CASES["negative"]["score_thr"], mc.CASES["negative"]["thr"],
                                                   max_num=mc.CASES["negative"]["max_num"])
    assert not np.array_equal(neg[2], per[2]), "no suppression between different classes in the negative case"
    assert np.array_equal(per[2], mc.run("negative_split")[2])

    # ---- BBoxHead.get_bboxes
    cfg = types.SimpleNamespace(**mc.GB_CFG)
    for name, c in mc.GB_CASES.items():
        rois, scores, pred = mc.gb_inputs(name)
        me = types.SimpleNamespace(custom_cls_channels=True, loss_cls=types.SimpleNamespace(get_activation=lambda x: x),
                                   bbox_coder=R.Coder(mc.MEANS, mc.STDS))
        args = (T(rois.copy()), T(scores.copy()), T(pred.copy()) if pred is not None else None, mc.GB_SHAPE, mc.GB_SCALE)
        det, lab = R.BBoxHead.get_bboxes(me, *args, rescale=c["rescale"], cfg=cfg)
        rb, rs = R.BBoxHead.get_bboxes(me, *args, rescale=c["rescale"], cfg=None)
        mine = mc.gb_run(name)
        assert distinct(scores) and rs.numpy().shape == scores.shape
        # the reference's detections carry no indices: the scores are distinct and untouched, so they name the (row, class) pair
        flat = scores[:, :c["C"]].reshape(-1)
        lookup = {int(k): i for i, k in enumerate(nc.bits(flat))}
        ref_inds = np.array([lookup[int(k)] for k in nc.bits(det.numpy()[:, 4])], dtype=np.int64)
        assert np.array_equal(ref_inds % c["C"], lab.numpy())
        if pred is not None:
            problems = gb_problems(name)
            assert not problems, (name, problems, "choose another seed (--scan-seeds)")
        else:
            # no exp on this path: the reference's boxes are the restatement's, bit for bit - and they are NOT clamped
            assert np.array_equal(nc.bits(rb.numpy()), nc.bits(mc.gb_boxes_np(name)))
            assert np.array_equal(nc.bits(det.numpy()), nc.bits(mine[0]))
            assert (rois[:, 1:] < 0).any() and (rois[:, 4] > mc.GB_SHAPE[0]).any()
        assert np.array_equal(ref_inds, mine[2]), (name, "kept pairs differ from the reference's")
        assert 0 < mine[3] < 10000
        store(out, name, mine, True)
        print("%-20s n %4d C %4d: M %6d, %4d kept" % (name, c["n"], c["C"], mine[3], mine[2].size))
    path = os.path.join(HERE, "g29_multiclass_nms.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %.1f KB" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
