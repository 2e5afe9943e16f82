#!/usr/bin/env python3
"""Generate tests/golden/g28_nms.npz by RUNNING THE REFERENCE's RPNHead.get_bboxes / _get_bboxes_single
(instance_segmentation/mmdet/models/dense_heads/rpn_head.py) with its AnchorGenerator and DeltaXYWHBBoxCoder on the CPU in
float32, and mmcv 1.3.8's nms / batched_nms as restated below.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nms.py <reference checkout>

The reference is imported under the placeholder modules of make_golden_targets.py.  It has no NMS of its own: it calls
``mmcv.ops.batched_nms``.  The placeholder given to it here is a small torch function that states mmcv 1.3.8's definition
(ops/nms.py: the coordinate offset per id, ``split_thr``, ``score_threshold`` / ``max_num``, and for the compiled operator a
stable descending sort and the greedy loop).  The reference's call into it, the per-level sort, the gathers, the decode, the
min-size filter and the truncation are its own code.  Nothing from the reference is written to the repository except results.

Before storing anything the generator asserts:
  * the placeholder and the numpy restatement (tests/nms_cases.py) agree exactly on every case; the numpy anchors equal the
    reference's;
  * in every case compared with the reference all scores that take part are distinct in float32, and for the RPN cases the order
    of the sigmoid values equals the order of the logits (cases with ties are stored from the restatement only and marked);
  * in every random case the greedy result differs from "suppressed if any higher-ranked box overlaps";
  * the id case with coordinates below -1 has a suppression between different ids;
  * for the RPN cases compared with the reference: the kept anchors do not change when the NMS stage is rerun on the
    float64-decoded candidates, or on eight copies whose coordinates are moved by random whole numbers of float32 ulps in [-4, 4]
    and clipped again (a coordinate that the clip replaced is the border in every implementation and is not moved); no pair of candidates that take part has an IoU within 1e-4 of the threshold, and no side lies within
    1e-3 of min_bbox_size - except a side of exactly 0 whose two coordinates were both replaced by the same border of the clip,
    which is 0 in every implementation.  The seed of each case (nms_cases.RPN_CASES) is chosen so that this holds; it makes
    the comparison independent of the rounding of exp.  A condition on the inputs, not a tolerance on the result.
It records ``ref_decode_ulps`` / ``ref_sigmoid_ulps``: the reference's float32 decode and sigmoid against the float64
continuation (targets_cases.decode_check, nms_cases.sigmoid_ulps).

The fixture stores NO value that went through exp: identities, levels, counts, kept positions, checksums and the two ulp maxima.
torch's CPU exp is vectorised and rounds a handful of elements differently depending on how the tensor is split over threads
(1 to 32 units in the last place were seen between two environments), so the reference's float32 dets are compared with the
restatement inside this run and not stored; the run is single-threaded so that the ulp maxima do not depend on the core count.
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
from tests import nms_cases as nc              # noqa: E402
from tests import targets_cases as tc          # noqa: E402

torch.set_num_threads(1)                        # torch's vectorised CPU exp rounds a few elements differently per chunking
T = torch.from_numpy
CALLS = []                                      # what the reference handed to batched_nms


# ---------------------------------------------------------------------------------------------- mmcv 1.3.8 ops/nms.py, restated
def nms(boxes, scores, iou_threshold, offset=0, score_threshold=0, max_num=-1):
    assert boxes.size(1) == 4 and boxes.size(0) == scores.size(0) and offset in (0, 1)
    valid_inds = None
    b, s = boxes, scores
    if score_threshold > 0:
        valid_mask = scores > score_threshold
        b, s = boxes[valid_mask], scores[valid_mask]
        valid_inds = torch.nonzero(valid_mask, as_tuple=False).squeeze(dim=1)
    # the compiled operator: sort by score, descending; walk the list, a kept box removes what it overlaps by more than the threshold
    order = torch.sort(s, descending=True, stable=True)[1]
    r = b[order]
    off = torch.tensor(float(offset), dtype=torch.float32)
    area = (r[:, 2] - r[:, 0] + off) * (r[:, 3] - r[:, 1] + off)
    removed = torch.zeros(r.shape[0], dtype=torch.bool)
    keep = []
    for i in range(r.shape[0]):
        if removed[i]:
            continue
        keep.append(i)
        q = r[i + 1:]
        w = torch.clamp(torch.min(r[i, 2], q[:, 2]) - torch.max(r[i, 0], q[:, 0]) + off, min=0)
        h = torch.clamp(torch.min(r[i, 3], q[:, 3]) - torch.max(r[i, 1], q[:, 1]) + off, min=0)
        inter = w * h
        removed[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > iou_threshold
    inds = order[torch.tensor(keep, dtype=torch.long)]
    if max_num > 0:
        inds = inds[:max_num]
    if valid_inds is not None:
        inds = valid_inds[inds]
    return torch.cat((boxes[inds], scores[inds].reshape(-1, 1)), dim=1), inds


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    CALLS.append((boxes.numpy().copy(), scores.numpy().copy(), idxs.numpy().copy()))
    nms_cfg_ = nms_cfg.copy()
    class_agnostic = nms_cfg_.pop("class_agnostic", class_agnostic)
    if class_agnostic:
        boxes_for_nms = boxes
    else:
        max_coordinate = boxes.max()
        offsets = idxs.to(boxes) * (max_coordinate + torch.tensor(1).to(boxes))
        boxes_for_nms = boxes + offsets[:, None]
    nms_type = nms_cfg_.pop("type", "nms")
    assert nms_type == "nms"
    split_thr = nms_cfg_.pop("split_thr", 10000)
    if boxes_for_nms.shape[0] < split_thr:
        dets, keep = nms(boxes_for_nms, scores, **nms_cfg_)
        boxes = boxes[keep]
        scores = dets[:, -1]
    else:
        max_num = nms_cfg_.pop("max_num", -1)
        total_mask = scores.new_zeros(scores.size(), dtype=torch.bool)
        scores_after_nms = scores.new_zeros(scores.size())
        for id in torch.unique(idxs):
            mask = (idxs == id).nonzero(as_tuple=False).view(-1)
            dets, keep = nms(boxes_for_nms[mask], scores[mask], **nms_cfg_)
            total_mask[mask[keep]] = True
            scores_after_nms[mask[keep]] = dets[:, -1]
        keep = total_mask.nonzero(as_tuple=False).view(-1)
        scores, inds = torch.sort(scores_after_nms[keep], descending=True, stable=True)
        keep = keep[inds]
        boxes = boxes[keep]
        if max_num > 0:
            keep, boxes, scores = keep[:max_num], boxes[:max_num], scores[:max_num]
    return torch.cat([boxes, scores[:, None]], -1), keep


def reference(ref_root):
    R = mgt.reference(ref_root)
    mm = os.path.join(ref_root, "instance_segmentation", "mmdet")
    sys.modules["mmcv"].is_tuple_of = lambda seq, t: isinstance(seq, tuple) and all(isinstance(x, t) for x in seq)
    mgt._pkg("mmcv.ops", batched_nms=batched_nms, nms=nms)
    mgt._pkg("mmdet.core.anchor.builder", PRIOR_GENERATORS=mgt._Registry(), ANCHOR_GENERATORS=mgt._Registry())
    ag = importlib.import_module("mmdet.core.anchor.anchor_generator")
    rh = importlib.import_module("mmdet.models.dense_heads.rpn_head")
    assert os.path.samefile(os.path.dirname(rh.__file__), os.path.join(mm, "models", "dense_heads"))
    R.AnchorGenerator, R.RPNHead = ag.AnchorGenerator, rh.RPNHead
    return R


def distinct(a):
    return np.unique(nc.bits(a)).size == np.asarray(a).size


# ---------------------------------------------------------------------------------------------- RPN robustness
def decode64(anc, d, shape):
    """The float64 continuation of the decode (from the bit-exact float32 intermediates), clipped; and which coordinates the clip
    replaced."""
    gx, gy, pw, ph, dw, dh = tc.decode_parts_np(anc, d, nc.MEANS, nc.STDS, tc.WH_RATIO_CLIP, False, 32)
    gw = pw.astype(np.float64) * np.exp(dw.astype(np.float64))
    gh = ph.astype(np.float64) * np.exp(dh.astype(np.float64))
    gx, gy = gx.astype(np.float64), gy.astype(np.float64)
    raw = np.stack([gx - 0.5 * gw, gy - 0.5 * gh, gx + 0.5 * gw, gy + 0.5 * gh], axis=-1).reshape(-1, 4)
    return tc._clip_np(raw, shape, 1), raw


def iou64(b, off=0.0):
    area = (b[:, 2] - b[:, 0] + off) * (b[:, 3] - b[:, 1] + off)
    w = np.maximum(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]) + off, 0)
    h = np.maximum(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]) + off, 0)
    inter = w * h
    with np.errstate(all="ignore"):
        return inter / (area[:, None] + area[None, :] - inter)


def side_problems(c, b64, raw):
    """(problems, which candidates take part) from the float64 decode: no side within 1e-3 of min_bbox_size, except a side of
    exactly 0 between two coordinates that the clip replaced by the same border."""
    ms = c["min_size"]
    problems, valid = [], np.ones(b64.shape[0], dtype=bool)
    if ms >= 0:
        for lo, hi in ((0, 2), (1, 3)):
            side = b64[:, hi] - b64[:, lo]
            both_clipped = (b64[:, hi] != raw[:, hi]) & (b64[:, lo] != raw[:, lo]) & (side == 0)
            if (np.abs(side - ms) < 1e-3)[~both_clipped].any():
                problems.append("a side within 1e-3 of min_bbox_size")
            valid &= side > ms
    return problems, valid


def robustness_problems(name, b, cls, reg, anchors):
    c = nc.RPN_CASES[name]
    shape = c["shapes"][b]
    base = nc.rpn_np(name, b, cls, reg, anchors)
    kept = base["index"][base["keep"]]
    idx, lvl, logits, anc, d = nc.rpn_candidates_np(name, b, cls, reg, anchors)
    b64, raw = decode64(anc, d, shape)
    problems = []
    alt = nc.rpn_np(name, b, cls, reg, anchors, boxes=b64.astype(np.float32))
    if not np.array_equal(alt["index"][alt["keep"]], kept):
        problems.append("float64 decode changes the result")
    b32 = tc.delta2bbox_np(anc, d, *nc.decode_args(shape))
    rng = np.random.RandomState(1000 * c["seed"] + b)
    for t in range(8):
        free = b64 == raw                                       # a coordinate the clip replaced is the border itself everywhere
        moved = b32 + np.where(free, rng.randint(-4, 5, size=b32.shape), 0).astype(np.float32) * np.spacing(np.abs(b32))
        alt = nc.rpn_np(name, b, cls, reg, anchors, boxes=tc._clip_np(moved.astype(np.float32), shape, 1))
        if not np.array_equal(alt["index"][alt["keep"]], kept):
            problems.append("ulp perturbation %d changes the result" % t)
    side, valid = side_problems(c, b64, raw)
    problems += side
    v = b64[valid] + (lvl[valid].astype(np.float64) * (b64[valid].max() + 1.0))[:, None] if valid.any() else b64[valid]
    iou = iou64(v)
    np.fill_diagonal(iou, np.nan)
    near = np.abs(iou - c["thr"]) < 1e-4
    if near.any():
        problems.append("%d pairs with an IoU within 1e-4 of the threshold" % (int(near.sum()) // 2))
    return problems


def main():
    if len(sys.argv) > 2 and sys.argv[2] == "--scan-seeds":
        for name in sys.argv[3:]:
            for seed in range(12):
                nc.RPN_CASES[name]["seed"] = seed
                cls, reg, anchors = nc.rpn_inputs(name)
                p = [q for b in range(len(nc.RPN_CASES[name]["shapes"])) for q in robustness_problems(name, b, cls, reg, anchors)]
                print(name, "seed", seed, p or "ok")
        return
    R = reference(sys.argv[1])
    warnings.simplefilter("ignore")
    out = dict(nc.input_checksums())

    # ---- plain and batched NMS: the placeholder (what the reference calls) against the restatement
    for name, c in nc.PLAIN_CASES.items():
        boxes, scores = nc.plain_inputs(name)
        mine = nc.run_plain(name)
        dets, inds = nms(T(boxes.copy()), T(scores.copy()), c["thr"], c["offset"], c["score_threshold"], c["max_num"])
        assert np.array_equal(inds.numpy(), mine), name
        assert np.array_equal(nc.bits(dets.numpy()), nc.bits(nc.dets_np(boxes, scores, mine))), name
        assert (name in nc.TIE_CASES) == (not distinct(scores)), name
        if name in nc.RANDOM_PLAIN:
            order = nc.rank_np(scores, c["score_threshold"])
            full = nc.greedy_np(boxes[order], c["thr"], c["offset"])
            wrong = nc.any_higher_np(boxes[order], c["thr"], c["offset"])
            assert not np.array_equal(full, wrong), (name, "the greedy scan and 'any higher-ranked box' agree")
        if c["max_num"] > 0:
            assert mine.size == c["max_num"] < nc.nms_np(boxes, scores, c["thr"], c["offset"], c["score_threshold"]).size
        out["p_%s_keep" % name] = mine.astype(np.int32)
        print("nms %-12s N %5d: %4d kept" % (name, c["n"], mine.size))
    assert np.array_equal(nc.run_plain("chain"), [0, 2])
    b, s = nc.plain_inputs("zero_area")
    assert {3, 5} <= set(nc.run_plain("zero_area").tolist())
    for name, c in nc.BATCHED_CASES.items():
        boxes, scores, ids = nc.batched_inputs(name)
        mine = nc.run_batched(name)
        cfg = nc.nms_cfg(name)
        dets, keep = batched_nms(T(boxes.copy()), T(scores.copy()), T(ids.copy()), cfg, class_agnostic=c["class_agnostic"])
        assert np.array_equal(keep.numpy(), mine), name
        assert np.array_equal(nc.bits(dets.numpy()), nc.bits(nc.dets_np(boxes, scores, mine))), name
        assert distinct(scores)
        if c["kind"] == "random":
            order = nc.rank_np(scores)
            s_ = boxes if c["class_agnostic"] else nc.shifted_np(boxes, ids)
            assert not np.array_equal(nc.greedy_np(s_[order], c["thr"]), nc.any_higher_np(s_[order], c["thr"])), name
        if c["kind"] == "negative":
            per_id = np.sort(np.concatenate([np.nonzero(ids == i)[0][nc.nms_np(boxes[ids == i], scores[ids == i], c["thr"])]
                                             for i in np.unique(ids)]))
            assert not np.array_equal(per_id, np.sort(mine)), "no suppression between different ids in the negative case"
        out["b_%s_keep" % name] = mine.astype(np.int32)
        print("batched %-9s N %5d: %4d kept" % (name, c["n"], mine.size))

    # ---- RPN: the reference's get_bboxes
    worst_dec, worst_sig = 0.0, 0.0
    for name, c in nc.RPN_CASES.items():
        cls, reg, anchors = nc.rpn_inputs(name)
        gen = R.AnchorGenerator(strides=list(c["strides"]), ratios=[0.5, 1.0, 2.0], scales=[8])
        ref_anchors = gen.grid_anchors([tuple(s) for s in c["sizes"]], device="cpu")
        for a, r in zip(anchors, ref_anchors):
            assert np.array_equal(nc.bits(a), nc.bits(r.numpy())), "numpy anchors != the reference's"
        me = types.SimpleNamespace(test_cfg=None, use_sigmoid_cls=True, bbox_coder=R.Coder(nc.MEANS, nc.STDS), anchor_generator=gen)
        me._get_bboxes_single = types.MethodType(R.RPNHead._get_bboxes_single, me)
        cfg = types.SimpleNamespace(nms_pre=c["nms_pre"], max_per_img=c["max_per_img"], min_bbox_size=c["min_size"],
                                    nms=dict(type="nms", iou_threshold=c["thr"]))
        tcls = [T(x.copy()) for x in cls]
        treg = [T(x.copy()) for x in reg]
        if c["channels_last"]:
            tcls = [x.contiguous(memory_format=torch.channels_last) for x in tcls]
            treg = [x.contiguous(memory_format=torch.channels_last) for x in treg]
        metas = [dict(img_shape=s, scale_factor=np.ones(4, dtype=np.float32)) for s in c["shapes"]]
        del CALLS[:]
        results = R.RPNHead.get_bboxes(me, tcls, treg, metas, cfg)
        calls = list(CALLS)
        tie = name in nc.RPN_TIE_CASES
        out["r_%s_from_ref" % name] = np.array(not tie)
        for b, res in enumerate(results):
            mine = nc.rpn_np(name, b, cls, reg, anchors)
            nv = int(mine["valid"].sum())
            res = res.numpy()
            assert (name == "none") == (nv == 0)
            if nv == 0:
                assert res.shape == (0, 5)
            if not tie:
                # tie the reference's candidates to anchors: same concatenation order, its scores and boxes bit for bit
                idx, lvl, logits, anc, d = nc.rpn_candidates_np(name, b, cls, reg, anchors)
                sig = np.concatenate([torch.sigmoid(T(x.copy())).numpy() for x, _ in nc.rpn_flat(cls, reg, b)])[idx]   # per level, as the reference
                assert distinct(sig) and np.array_equal(np.argsort(-sig.astype(np.float64), kind="stable"),
                                                        np.argsort(-logits.astype(np.float64), kind="stable")), name
                ref_boxes = R.delta2bbox(T(anc.copy()), T(d.copy()), *nc.decode_args(c["shapes"][b])).numpy()
                v = nc.valid_np(ref_boxes, c["min_size"])
                assert np.array_equal(v, nc.valid_np(tc.delta2bbox_np(anc, d, *nc.decode_args(c["shapes"][b])), c["min_size"])), name
                if nv:
                    cb, cs, ci = calls.pop(0)
                    assert np.array_equal(nc.bits(cs), nc.bits(sig[v])) and np.array_equal(ci, lvl[v]), name
                    assert np.array_equal(nc.bits(cb), nc.bits(ref_boxes[v])), name
                ok, kinds, err = tc.decode_check(ref_boxes, anc, d, *nc.decode_args(c["shapes"][b]))
                assert ok and kinds
                worst_dec, worst_sig = max(worst_dec, err), max(worst_sig, nc.sigmoid_ulps(sig, logits))
                problems = robustness_problems(name, b, cls, reg, anchors)
                assert not problems, (name, b, problems, "choose another seed (--scan-seeds)")
                # the reference's result: the same anchors, its own float32 numbers
                assert res.shape[0] == mine["keep"].size, (name, b, res.shape, mine["keep"].size)
                order = nc.rpn_rank_np(idx, logits, v)
                ref_ranked = np.concatenate([ref_boxes, sig[:, None]], axis=1)[order]
                assert np.array_equal(nc.bits(res), nc.bits(ref_ranked[mine["keep"]])), (name, b)
                if nv:
                    full = nc.greedy_np(nc.shifted_np(mine["boxes"][:nv], mine["level"][:nv]), c["thr"])
                    wrong = nc.any_higher_np(nc.shifted_np(mine["boxes"][:nv], mine["level"][:nv]), c["thr"])
                    assert not np.array_equal(full, wrong), name
            else:
                # equal logits: nothing is compared with the reference, but the stored order and valid flags are compared with the
                # device exactly, so the flags must not hang on the rounding of exp either
                assert not distinct(mine["logits"])
                idx, lvl, logits, anc, d = nc.rpn_candidates_np(name, b, cls, reg, anchors)
                problems, v64 = side_problems(c, *decode64(anc, d, c["shapes"][b]))
                assert not problems and int(v64.sum()) == nv, (name, b, problems)
            out["r_%s_%d_index" % (name, b)] = mine["index"].astype(np.int32)
            out["r_%s_%d_level" % (name, b)] = mine["level"].astype(np.int8)
            out["r_%s_%d_nvalid" % (name, b)] = np.array(nv, dtype=np.int32)
            out["r_%s_%d_keep" % (name, b)] = mine["keep"].astype(np.int32)
            print("rpn %-8s image %d: %4d candidates, %4d take part, %4d kept%s" % (name, b, mine["index"].size, nv, mine["keep"].size,
                                                                                    " (restatement only)" if tie else ""))
        if name == "ties":
            x = nc.rpn_flat(cls, reg, 0)[0][0]
            cut = np.sort(x)[::-1][c["nms_pre"] - 1]
            assert (x == cut).sum() > 1 and (x > cut).sum() < c["nms_pre"] < (x >= cut).sum(), "no equal logits across the cut"
    out["ref_decode_ulps"] = np.array(worst_dec)
    out["ref_sigmoid_ulps"] = np.array(worst_sig)
    print("the reference's own maximum error against the float64 continuation: decode %.4f ulp, sigmoid %.4f ulp" % (worst_dec, worst_sig))
    path = os.path.join(HERE, "g28_nms.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %.1f KB" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
