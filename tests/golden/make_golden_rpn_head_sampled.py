#!/usr/bin/env python3
"""Generate tests/golden/g39_rpn_head_sampled.npz by RUNNING THE REFERENCE's RPNHead (``_init_layers``, ``forward_single``,
``loss``) with its AnchorGenerator, MaxIoUAssigner, RandomSampler, DeltaXYWHBBoxCoder, CrossEntropyLoss and L1Loss / SmoothL1Loss on
the CPU, in float32 and in float64.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rpn_head_sampled.py <reference checkout>

The reference's files are imported as they are under the placeholder mmcv / mmdet modules of make_golden_rpn_stage.py; the head
is a subclass of the reference's ``RPNHead`` whose constructor only sets the attributes the methods read and then calls the
reference's ``_init_layers``.  Nothing from the reference is written to the repository except outputs (data).

Inputs (features, parameters, ground truth) are tests/rpn_head_cases.py's closed formulas; ``torch.randperm`` is recorded during
``get_targets`` and replayed in both ``loss`` runs so that float32 and float64 see the sample that is recorded.  Per case: the
sample (flat indices through the reference's inside flags, ascending, padded with -1; counts; encoded targets;
``num_total_samples``), the per-level losses, the six parameter gradients and ``d feats``, each in both precisions.

Asserted here: the ReLU's input is the same number in float32 and float64 (the dyadic grid), so no sign can disagree; ``d feats``
is non-zero exactly within the 3x3 neighbourhoods of the sampled pixels, in both precisions; tests/rpn_head_cases.py's decode and
owner rule agree with where the reference's gradient maps are non-zero; some pixel holds two sampled anchors; an image has
counts that do not fill the sampler; an image has no ground truth.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_golden_rpn_stage as mgr             # noqa: E402
import make_golden_targets as mgt               # noqa: E402
from tests import rpn_head_cases as hc          # noqa: E402

torch.set_num_threads(8)
T = torch.from_numpy
A = 3


def make_head(R, name):
    c = hc.CASES[name]
    pos, neg, min_pos, assign_all, ign, ign_wrt, mlq = hc.RUN

    class Head(R.RPNHead):
        def __init__(self):
            torch.nn.Module.__init__(self)

    h = Head()
    h.anchor_generator = R.AnchorGenerator(**hc.GEN)
    h.assigner = R.MaxIoUAssigner(pos, neg, min_pos_iou=min_pos, gt_max_assign_all=assign_all, ignore_iof_thr=ign,
                                  ignore_wrt_candidates=ign_wrt, match_low_quality=mlq)
    h.sampler = R.RandomSampler(hc.NUM, hc.FRAC, neg_pos_ub=hc.UB, add_gt_as_proposals=False)
    h.bbox_coder = R.Coder(hc.MEANS, hc.STDS)
    h.train_cfg = types.SimpleNamespace(allowed_border=c["border"], pos_weight=c["pos_weight"])
    h.sampling, h.num_classes, h.cls_out_channels, h.use_sigmoid_cls, h.reg_decoded_bbox = True, 1, 1, True, False
    h.loss_cls = R.CrossEntropyLoss(use_sigmoid=True, loss_weight=1.0)
    h.loss_bbox = R.L1Loss(loss_weight=1.0) if c["kind"] == "l1" else R.SmoothL1Loss(beta=hc.BETA, loss_weight=1.0)
    h.in_channels, h.feat_channels, h.num_anchors = c["ci"], c["co"], h.anchor_generator.num_base_anchors[0]
    assert h.num_anchors == A
    h._init_layers()
    params = hc.parameters(c["ci"], c["co"], A, c["salt"])
    with torch.no_grad():
        for p, v in zip((h.rpn_conv.weight, h.rpn_conv.bias, h.rpn_cls.weight, h.rpn_cls.bias, h.rpn_reg.weight, h.rpn_reg.bias), params):
            assert tuple(p.shape) == v.shape
            p.copy_(T(v.copy()))
    return h


def run(head, perms, feats, gts, metas, dtype):
    head = copy.deepcopy(head).to(dtype)
    xs = [T(x.copy()).to(dtype).requires_grad_(True) for x in feats]
    pre = [head.rpn_conv(x).detach() for x in xs]
    outs = [head.forward_single(x) for x in xs]
    scores, deltas = [o[0] for o in outs], [o[1] for o in outs]
    for m in scores + deltas:
        m.retain_grad()
    with mgr.Replay(perms), mgr.CastTargets():
        out = head.loss(scores, deltas, [T(g.copy()) for g in gts], metas, gt_bboxes_ignore=None)
    cls, box = out["loss_rpn_cls"], out["loss_rpn_bbox"]
    (sum(cls) + sum(box)).backward()
    params = (head.rpn_conv.weight, head.rpn_conv.bias, head.rpn_cls.weight, head.rpn_cls.bias, head.rpn_reg.weight, head.rpn_reg.bias)
    return dict(loss=np.array([[float(v.detach()) for v in cls], [float(v.detach()) for v in box]], dtype=np.float64),
                params=[p.grad.numpy().copy() for p in params], dfeat=[x.grad.numpy().copy() for x in xs],
                pre=[p.numpy() for p in pre], maps=[m.detach().numpy() for m in scores + deltas],
                gmaps=[m.grad.numpy().copy() for m in scores + deltas])


def main():
    R = mgr.reference(sys.argv[1])
    torch.manual_seed(20261021)
    out = dict(hc.input_checksums())
    metas = [dict(pad_shape=hc.PAD_SHAPES[b], img_shape=hc.IMG_SHAPES[b]) for b in range(hc.B)]
    seen = dict(shared_pixel=False, short_image=False, no_gt=False)
    L = len(hc.FEATMAPS)
    for name, c in hc.CASES.items():
        gts = hc.case_gts(name)
        feats = hc.features(c["ci"], c["salt"])
        head = make_head(R, name)
        anchor_list, valid_list = head.get_anchors(hc.FEATMAPS, metas, device="cpu")
        with mgt.PermRecorder() as rec:
            res = head.get_targets(anchor_list, valid_list, [T(g.copy()) for g in gts], metas, return_sampling_results=True)
        perms, samplings = list(rec.perms), res[-1]
        n_pos, n_neg = res[4], res[5]
        pos_pad, neg_pad = np.full((hc.B, hc.NEP), -1, np.int64), np.full((hc.B, hc.NUM), -1, np.int64)
        bt_pad, counts = np.zeros((hc.B, hc.NEP, 4), np.float32), np.zeros((hc.B, 2), np.int64)
        for b in range(hc.B):
            flat = torch.cat(anchor_list[b])
            inside = R.inside_flags(flat, torch.cat(valid_list[b]), hc.IMG_SHAPES[b][:2], c["border"]).numpy()
            sel = np.nonzero(inside)[0]
            sr = samplings[b]
            pos, neg = sel[sr.pos_inds.numpy()], sel[sr.neg_inds.numpy()]
            bt = head.bbox_coder.encode(sr.pos_bboxes, sr.pos_gt_bboxes).numpy() if pos.size else np.zeros((0, 4), np.float32)
            order = np.argsort(pos, kind="stable")
            pos, bt, neg = pos[order], bt[order], np.sort(neg)
            assert np.unique(pos).size == pos.size and np.unique(neg).size == neg.size
            pos_pad[b, :pos.size], neg_pad[b, :neg.size], bt_pad[b, :pos.size], counts[b] = pos, neg, bt, (pos.size, neg.size)
            seen["short_image"] |= pos.size + neg.size < hc.NUM
            seen["no_gt"] |= gts[b].shape[0] == 0
        nts = n_pos + n_neg
        assert nts == sum(max(int(counts[b, 0]), 1) + max(int(counts[b, 1]), 1) for b in range(hc.B))
        r32 = run(head, perms, feats, gts, metas, torch.float32)
        r64 = run(head, perms, feats, gts, metas, torch.float64)
        for a, b in zip(r32["pre"], r64["pre"]):
            assert np.array_equal(a.astype(np.float64), b), name             # exact: no sign of the ReLU's input can disagree
        # the decode and the owner rule against where the reference's gradient maps are non-zero
        slots, owner = hc.sample_slots(pos_pad, neg_pad, counts, A)
        active = slots[slots[:, 1] >= 0]
        sampled = int(counts.sum())
        assert active.shape[0] == int((owner >= 0).sum()) <= sampled
        seen["shared_pixel"] |= active.shape[0] < sampled
        pix0 = np.concatenate([[0], np.cumsum([h * w for h, w in hc.FEATMAPS])])
        for l, (H, W) in enumerate(hc.FEATMAPS):
            hit = (np.abs(r64["gmaps"][l]).sum(axis=1) + np.abs(r64["gmaps"][L + l]).sum(axis=1)) > 0          # [B, H, W]
            own = owner[:, pix0[l]:pix0[l + 1]].reshape(hc.B, H, W) >= 0
            assert np.array_equal(hit, own), (name, l)
            near = np.zeros((hc.B, H, W), dtype=bool)                        # d feats is 0 exactly where no owned pixel reaches
            for b, y, x in zip(*np.nonzero(own)):
                near[b, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
            for r in (r32, r64):
                assert np.array_equal(r["dfeat"][l] != 0, np.broadcast_to(near[:, None], r["dfeat"][l].shape)), (name, l)
        pre = "%s_" % name
        out[pre + "pos"], out[pre + "neg"], out[pre + "counts"] = pos_pad.astype(np.int32), neg_pad.astype(np.int32), counts
        out[pre + "pos_bt"], out[pre + "nts"] = bt_pad, np.array(nts, dtype=np.int64)
        for tag, r in (("32", r32), ("64", r64)):
            dt = np.float32 if tag == "32" else np.float64
            out[pre + "loss" + tag] = r["loss"].astype(dt)
            for pn, g in zip(hc.PARAM_NAMES, r["params"]):
                out[pre + "d_" + pn + tag] = g.astype(dt)
            out[pre + "dfeat" + tag] = np.concatenate([g.reshape(-1) for g in r["dfeat"]]).astype(dt)
        err = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32["params"] + r32["dfeat"], r64["params"] + r64["dfeat"]))
        print("case %-10s: positives %s negatives %s, active pixels %d of %d sampled, max |g32 - g64| %.3g"
              % (name, counts[:, 0].tolist(), counts[:, 1].tolist(), active.shape[0], sampled, err))
    assert all(seen.values()), seen
    path = os.path.join(HERE, "g39_rpn_head_sampled.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %.1f KB" % (path, os.path.getsize(path) / 1024.0))
    assert os.path.getsize(path) <= 1000 * 1024


if __name__ == "__main__":
    main()
