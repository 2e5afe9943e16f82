#!/usr/bin/env python3
"""Generate tests/golden/g34_rpn_stage.npz by RUNNING THE REFERENCE's AnchorGenerator, RPNHead (get_anchors, get_targets, loss),
MaxIoUAssigner, RandomSampler, DeltaXYWHBBoxCoder, CrossEntropyLoss and L1Loss / SmoothL1Loss on the CPU in float32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rpn_stage.py <reference checkout>

The reference's files are imported as they are under the placeholder mmcv / mmdet modules of make_golden_targets.py and
make_golden_nms.py; the head is a subclass of the reference's ``RPNHead`` whose constructor only sets the attributes the three
methods read.  Nothing from the reference is written to the repository except outputs (data).

``torch.randperm`` is wrapped to record the permutations ``get_targets`` drew; tests/targets_cases.ranks_from_perms /
keys_from_ranks turn them into per-anchor keys under which "keep the k smallest (key, index) pairs" selects the reference's
sample, and ``loss`` is then run with the same permutations replayed.  Recorded per case: the reference's index lists (compact
indices mapped through its inside flags), counts, assigned gts, encoded targets and ``num_total_samples``; per loss kind the
per-level losses and the autograd gradients of every score and delta map at the sampled positions (asserted zero elsewhere), in
float32 and from a float64 rerun of the reference's loss code on the same float32 inputs.

The generator asserts on the CPU that tests/rpn_stage_cases.py's numpy restatement reproduces the reference and that the cases
hold what they are there for (see the asserts at the end of ``main``).
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_golden_nms as mgn                   # noqa: E402
import make_golden_targets as mgt               # noqa: E402
from tests import assign_cases as ac            # noqa: E402
from tests import rpn_stage_cases as rc         # noqa: E402
from tests import targets_cases as tc           # noqa: E402

torch.set_num_threads(8)
T = torch.from_numpy


def reference(ref_root):
    R = mgn.reference(ref_root)
    mm = os.path.join(ref_root, "instance_segmentation", "mmdet")
    bbox = os.path.join(mm, "core", "bbox")
    ic = mgt._pkg("mmdet.core.bbox.iou_calculators", os.path.join(bbox, "iou_calculators"))
    mgt._pkg("mmdet.core.bbox.iou_calculators.builder", IOU_CALCULATORS=mgt._Registry())
    calc = importlib.import_module("mmdet.core.bbox.iou_calculators.iou2d_calculator")
    ic.build_iou_calculator = lambda cfg: calc.BboxOverlaps2D()
    R.MaxIoUAssigner = importlib.import_module("mmdet.core.bbox.assigners.max_iou_assigner").MaxIoUAssigner
    sys.modules["mmdet.models.builder"].LOSSES = mgt._Registry()
    mgt._pkg("mmdet.models.losses", os.path.join(mm, "models", "losses"), accuracy=None)
    R.CrossEntropyLoss = importlib.import_module("mmdet.models.losses.cross_entropy_loss").CrossEntropyLoss
    sl = importlib.import_module("mmdet.models.losses.smooth_l1_loss")
    R.L1Loss, R.SmoothL1Loss = sl.L1Loss, sl.SmoothL1Loss
    return R


def make_head(R, name, kind):
    c = rc.CASES[name]
    pos, neg, min_pos, assign_all, ign, ign_wrt, mlq = rc.run_of(name)

    class Head(R.RPNHead):
        def __init__(self):
            torch.nn.Module.__init__(self)

    h = Head()
    h.anchor_generator = R.AnchorGenerator(**rc.GEN_CASES[rc.FPN][0])
    h.assigner = R.MaxIoUAssigner(pos, neg, min_pos_iou=min_pos, gt_max_assign_all=assign_all, ignore_iof_thr=ign,
                                  ignore_wrt_candidates=ign_wrt, match_low_quality=mlq)
    h.sampler = R.RandomSampler(rc.NUM, rc.FRAC, neg_pos_ub=rc.UB, add_gt_as_proposals=False)
    h.bbox_coder = R.Coder(rc.MEANS, rc.STDS)
    h.train_cfg = types.SimpleNamespace(allowed_border=c["border"], pos_weight=c["pos_weight"])
    h.sampling, h.num_classes, h.cls_out_channels, h.use_sigmoid_cls, h.reg_decoded_bbox = True, 1, 1, True, False
    h.loss_cls = R.CrossEntropyLoss(use_sigmoid=True, loss_weight=1.0)
    h.loss_bbox = R.L1Loss(loss_weight=1.0) if kind == "l1" else R.SmoothL1Loss(beta=rc.BETA, loss_weight=1.0)
    return h


class Replay:
    """torch.randperm returns the recorded permutations, in order."""

    def __init__(self, perms):
        self.perms = [p.copy() for p in perms]

    def __enter__(self):
        self._orig = torch.randperm

        def randperm(n, *a, **kw):
            p = self.perms.pop(0)
            assert p.size == n
            return T(p.copy())
        torch.randperm = randperm
        return self

    def __exit__(self, *exc):
        torch.randperm = self._orig
        assert not self.perms


class CastTargets:
    """binary_cross_entropy_with_logits with the target and weight cast to the input's dtype (the float64 rerun)."""

    def __enter__(self):
        import torch.nn.functional as Fn
        self.Fn, self._orig = Fn, Fn.binary_cross_entropy_with_logits

        def bce(input, target, weight=None, *a, **kw):
            return self._orig(input, target.to(input.dtype), None if weight is None else weight.to(input.dtype), *a, **kw)
        Fn.binary_cross_entropy_with_logits = bce
        return self

    def __exit__(self, *exc):
        self.Fn.binary_cross_entropy_with_logits = self._orig


def run_loss(head, perms, scores, deltas, gts, metas, dtype):
    s = [T(x.copy()).to(dtype).requires_grad_(True) for x in scores]
    d = [T(x.copy()).to(dtype).requires_grad_(True) for x in deltas]
    with Replay(perms), CastTargets():
        out = head.loss(s, d, [T(g.copy()) for g in gts], metas, gt_bboxes_ignore=None)
    cls, box = out["loss_rpn_cls"], out["loss_rpn_bbox"]
    (sum(cls) + sum(box)).backward()
    return (np.array([[float(v) for v in cls], [float(v) for v in box]], dtype=np.float64),
            [x.grad.numpy().copy() for x in s], [x.grad.numpy().copy() for x in d])


def main():
    R = reference(sys.argv[1])
    torch.manual_seed(20261019)
    out = dict(rc.input_checksums())

    # ---- generators
    for name, (kw, featmaps) in rc.GEN_CASES.items():
        gen = R.AnchorGenerator(**kw)
        base = rc.base_anchors_np(**kw)
        for l, (b, mine) in enumerate(zip(gen.base_anchors, base)):
            assert mgt.same_bits(b.numpy(), mine), (name, l)
            out["gen_%s_base%d" % (name, l)] = b.numpy()
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            anchors = np.concatenate([a.numpy() for a in gen.grid_anchors(featmaps, device="cpu")])
        priors = np.concatenate([a.numpy() for a in gen.grid_priors(featmaps, device="cpu")])
        assert mgt.same_bits(anchors, priors)
        assert mgt.same_bits(anchors, np.concatenate(rc.grid_anchors_np(base, kw["strides"], featmaps))), name
        out["gen_%s_anchors" % name] = anchors
        for k, pad in enumerate(rc.GEN_PAD_SHAPES):
            flags = np.concatenate([f.numpy() for f in gen.valid_flags(featmaps, pad, device="cpu")])
            mine = np.concatenate(rc.valid_flags_np(kw["strides"], featmaps, gen.num_base_anchors, pad))
            assert np.array_equal(flags, mine), (name, pad)
            out["gen_%s_flags%d" % (name, k)] = np.packbits(flags)
        print("generator %-11s: %5d anchors, base anchors %s" % (name, anchors.shape[0], gen.num_base_anchors))

    # ---- targets and losses
    ulps = np.load(os.path.join(HERE, "g26_targets.npz"))["coder_ref_ulps"]
    _, per_level, flat = rc.fpn_anchors()
    level_counts = [a.shape[0] for a in per_level]
    metas = [dict(pad_shape=rc.PAD_SHAPES[b], img_shape=rc.IMG_SHAPES[b]) for b in range(2)]
    seen = dict(more=False, fewer=False, nogt=False, masked_lq=False, tie_all=False, tie_first=False)
    for name, c in rc.CASES.items():
        gts = rc.case_gts(name)
        scores, deltas = rc.maps(name)
        head = make_head(R, name, "l1")
        anchor_list, valid_list = head.get_anchors(rc.FEATMAPS, metas, device="cpu")
        with mgt.PermRecorder() as rec:
            res = head.get_targets(anchor_list, valid_list, [T(g.copy()) for g in gts], metas, return_sampling_results=True)
        labels_l, lw_l, bt_l, bw_l, n_pos, n_neg, samplings = res
        perms = list(rec.perms)
        queue = list(perms)
        per_image, pos_pad, neg_pad = [], np.full((2, rc.NEP), -1, np.int64), np.full((2, rc.NUM), -1, np.int64)
        gt_pad, bt_pad, counts = np.full((2, rc.NEP), -1, np.int64), np.zeros((2, rc.NEP, 4), np.float32), np.zeros((2, 2), np.int64)
        for b in range(2):
            inside = rc.fpn_inside(b, c["border"])
            assert np.array_equal(inside, R.inside_flags(T(flat.copy()), torch.cat(valid_list[b]), rc.IMG_SHAPES[b][:2], c["border"]).numpy())
            sel = np.nonzero(inside)[0]
            gi = ac.assign_np(flat[sel], gts[b], None, None, rc.run_of(name))[0]
            P, Q = int((gi > 0).sum()), int((gi == 0).sum())
            mine = {0: None, 1: None}
            if P > rc.NEP:
                mine[0] = queue.pop(0)
            if Q > rc.NUM - min(P, rc.NEP):
                mine[1] = queue.pop(0)
            ranks = tc.ranks_from_perms(gi, mine)
            kc = tc.keys_from_ranks(gi, ranks, rc.key_salt(name, b))
            keys = tc.free_keys(inside.size, rc.key_salt(name, b) + 3)
            keys[inside] = kc
            sr = samplings[b]
            pos, neg, pos_gt, bt, _ = rc.targets_np(flat, inside, gts[b], keys, rc.run_of(name))
            assert np.array_equal(pos, sel[sr.pos_inds.numpy()]) and np.array_equal(neg, sel[sr.neg_inds.numpy()]), (name, b)
            assert np.array_equal(pos_gt, sr.pos_assigned_gt_inds.numpy()), (name, b)
            ref_bt = head.bbox_coder.encode(sr.pos_bboxes, sr.pos_gt_bboxes).numpy() if pos.size else np.zeros((0, 4), np.float32)
            assert mgt.same_bits(bt[:, :2], ref_bt[:, :2]), (name, b)
            if pos.size and not mgt.same_bits(bt, ref_bt):
                e = tc.encode_check(bt, flat[pos], gts[b][pos_gt], rc.MEANS, rc.STDS)
                assert e[0] and e[1] and e[2] <= 2 * ulps[0], (name, b, e)
            out["t_%s_%d_rank0" % (name, b)], out["t_%s_%d_rank1" % (name, b)] = ranks[0], ranks[1]
            pos_pad[b, :pos.size], neg_pad[b, :neg.size] = pos, neg
            gt_pad[b, :pos.size], bt_pad[b, :pos.size], counts[b] = pos_gt, ref_bt, (pos.size, neg.size)
            per_image.append((pos, neg, ref_bt))
            seen["more"] |= P > rc.NEP
            seen["fewer"] |= 0 < P < rc.NEP
            seen["nogt"] |= gts[b].shape[0] == 0
            if gts[b].shape[0]:
                ov = ac.overlaps_np(gts[b], flat)                              # [G, A], all anchors
                best_all = ov.argmax(axis=1)
                ov_in = np.where(inside[None, :], ov, np.float32(-1))
                for g in range(gts[b].shape[0]):
                    mx = ov_in[g].max()
                    if not inside[best_all[g]] and ov[g, best_all[g]] > mx >= np.float32(0.3) and mx < np.float32(0.7) and \
                            (gi[np.nonzero(ov_in[g][sel] == mx)[0]] == g + 1).any():
                        seen["masked_lq"] = True
                    if np.float32(0.3) <= mx < np.float32(0.7) and (ov_in[g] == mx).sum() >= 2:
                        hit = gi[np.nonzero(ov_in[g][sel] == mx)[0]] == g + 1
                        if c["assign_all"] and hit.all():
                            seen["tie_all"] = True
                        if not c["assign_all"] and hit[0] and not hit[1:].any():
                            seen["tie_first"] = True
        assert not queue
        nts = n_pos + n_neg
        assert nts == sum(max(int(counts[b, 0]), 1) + max(int(counts[b, 1]), 1) for b in range(2))
        dense = rc.dense_np(level_counts, per_image, c["pos_weight"])
        for mine, theirs in zip(dense, (labels_l, lw_l, bt_l, bw_l)):
            for m, t in zip(mine, theirs):
                assert m.shape == tuple(t.shape) and np.array_equal(m.view(np.int32 if m.dtype == np.float32 else m.dtype),
                                                                    t.numpy().view(np.int32 if m.dtype == np.float32 else m.dtype)), name
        pre = "t_%s_" % name
        out[pre + "pos"], out[pre + "neg"], out[pre + "counts"] = pos_pad.astype(np.int32), neg_pad.astype(np.int32), counts
        out[pre + "pos_gt"], out[pre + "pos_bt"], out[pre + "nts"] = gt_pad.astype(np.int32), bt_pad, np.array(nts, dtype=np.int64)

        # ---- the losses of both kinds and their gradients
        entry = np.concatenate([pos_pad, neg_pad], axis=1)                     # [B, nep + num] flat indices, -1 unused
        for kind, beta in (("l1", 0.0), ("sl1", rc.BETA)):
            head = make_head(R, name, kind)
            l32, gs32, gd32 = run_loss(head, perms, scores, deltas, gts, metas, torch.float32)
            l64, gs64, gd64 = run_loss(head, perms, scores, deltas, gts, metas, torch.float64)
            cls_t, box_t, nts2 = rc.loss_terms_np(scores, deltas, per_image, level_counts, c["pos_weight"], beta)
            assert nts2 == nts
            mine = np.array([[t.sum() / nts for t in cls_t], [t.sum() / nts for t in box_t]])
            assert np.allclose(mine, l64, rtol=1e-12, atol=1e-15), (name, kind, mine, l64)
            packs = {}
            for tag, gs, gd in (("32", gs32, gd32), ("64", gs64, gd64)):
                fs, fd = rc.flat_maps(gs, gd)
                g_cls = np.zeros(entry.shape, dtype=fs.dtype)
                g_box = np.zeros((2, rc.NEP, 4), dtype=fd.dtype)
                for b in range(2):
                    live = entry[b] >= 0
                    g_cls[b, live] = fs[b, entry[b, live]]
                    g_box[b, :counts[b, 0]] = fd[b, pos_pad[b, :counts[b, 0]]]
                    rest_s, rest_d = fs[b].copy(), fd[b].copy()
                    rest_s[entry[b, live]] = 0
                    rest_d[pos_pad[b, :counts[b, 0]]] = 0
                    assert not rest_s.any() and not rest_d.any(), (name, kind, tag)          # exactly zero where nothing was sampled
                packs[tag] = (g_cls, g_box)
            pre = "l_%s_%s_" % (name, kind)
            out[pre + "loss32"], out[pre + "loss64"] = l32.astype(np.float32), l64
            out[pre + "gcls32"], out[pre + "gbox32"] = packs["32"][0].astype(np.float32), packs["32"][1].astype(np.float32)
            out[pre + "gcls64"], out[pre + "gbox64"] = packs["64"]
            err = np.abs(l32 - l64).max()
            print("case %-9s %-3s: positives %s negatives %s, num_total_samples %d, max |loss32 - loss64| %.3g"
                  % (name, kind, counts[:, 0].tolist(), counts[:, 1].tolist(), nts, err))

    assert all(seen.values()), seen
    assert {c["border"] for c in rc.CASES.values()} == {-1, 0} and {c["pos_weight"] for c in rc.CASES.values()} == {-1.0, 2.0}
    assert {"offset", "ratio_major", "octave", "nonsquare"} <= set(rc.GEN_CASES)
    path = os.path.join(HERE, "g34_rpn_stage.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %.1f KB" % (path, os.path.getsize(path) / 1024.0))
    assert os.path.getsize(path) <= 308 * 1024


if __name__ == "__main__":
    main()
