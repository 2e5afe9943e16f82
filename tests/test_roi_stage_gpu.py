"""The RoI stage in one launch (csrc/roi_stage.hip, iif_amd/mmdet_roi_stage.py) on the MI355X.

  * against the existing per-image chain - ``MaxIoUAssigner.assign`` on ``proposals[b, :n_b]``, ``RandomSampler.sample_padded``
    with the same keys, ``bbox_targets`` -: every output as BIT PATTERNS, the ``log`` columns included (both sides run the same
    device functions), and ``counts`` / ``pos_is_gt`` / the ``pos_*`` rows against what the chain's tensors imply;
  * against the reference's own runs (tests/golden/g33_roi_stage.npz): integers, weights and rois exactly, the encoded
    ``dw, dh`` within 2 x ``coder_ref_ulps`` of the float64 continuation, as test_targets_gpu.test_roi_targets does;
  * the proposal counts are honoured, colliding keys, empty inputs, ``refine_bboxes`` and host synchronisation.
"""
import numpy as np
import pytest
import torch

from . import assign_cases as ac
from . import roi_stage_cases as rc
from . import targets_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("labels", "label_weights", "bbox_targets", "bbox_weights", "rois", "pos_assigned_gt_inds")


def T(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV, dtype=dtype)                 # a copy: the case arrays are read-only


def N_(t):
    return t.cpu().numpy()


def raw(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def ref(golden):
    g = golden("g33_roi_stage")
    rc.check_generator(g)
    return g


@pytest.fixture(scope="module")
def ulps(golden):
    return golden("g26_targets")["coder_ref_ulps"]


def parts(run, num, frac, ub=-1, add_gt=True, means=tc.MEANS[0], stds=tc.STDS[1]):
    from iif_amd.mmdet_assigner import MaxIoUAssigner
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler
    pos, neg, min_pos, assign_all, _, _, mlq = run
    return (MaxIoUAssigner(pos, neg, min_pos_iou=min_pos, gt_max_assign_all=assign_all, match_low_quality=mlq),
            RandomSampler(num, frac, neg_pos_ub=ub, add_gt_as_proposals=add_gt), DeltaXYWHBBoxCoder(means, stds))


def case_parts(name):
    c = rc.CASES[name]
    return parts(c["run"], c["num"], c["frac"], c["ub"], c["add_gt"], c["means"], c["stds"])


def stage(props, counts, gts, labs, asg, smp, coder, keys, pos_weight=-1, decoded=False):
    from iif_amd.mmdet_roi_stage import roi_stage_targets_padded
    return roi_stage_targets_padded(props, counts, gts, labs, asg, smp, coder, rc.NUM_CLASSES, pos_weight=pos_weight,
                                    reg_decoded_bbox=decoded, keys=keys)


def assert_equals_chain(out, props, ns, gts, labs, asg, smp, coder, keys, pos_weight=-1, decoded=False):
    """``out`` against the per-image chain of the existing entries on ``props[b, :ns[b]]`` with the same keys."""
    from iif_amd.mmdet_targets import bbox_targets
    B, num, nep = len(ns), int(smp.num), int(smp.num * smp.pos_fraction)
    ps, fronts = [], []
    for b in range(B):
        p = props[b, :ns[b]]
        front = gts[b].shape[0] if smp.add_gt_as_proposals and gts[b].shape[0] > 0 else 0
        ar = asg.assign(p, gts[b], None, labs[b])
        ps.append(smp.sample_padded(ar, p, gts[b], labs[b], keys=keys[b, :front + ns[b]].contiguous()))
        fronts.append(front)
    want = bbox_targets(ps, gts, labs, coder, rc.NUM_CLASSES, pos_weight=pos_weight, reg_decoded_bbox=decoded)
    for f, w in zip(FIELDS, want):
        got = getattr(out, f)
        assert got.shape == w.shape and got.dtype == w.dtype, f
        bad = (raw(got) != raw(w)).reshape(got.shape[0], -1).any(1).nonzero().flatten()
        assert bad.numel() == 0, (f, bad[:8].tolist())
    counts = torch.stack([p.counts for p in ps])
    assert out.counts.dtype == torch.int64 and torch.equal(out.counts, counts)
    labels, _, _, _, rois, pos_gt = want
    for b in range(B):
        kp = int(counts[b, 0])
        is_gt = torch.zeros(num, dtype=torch.uint8, device=DEV)
        is_gt[:kp] = (ps[b].pos_inds[:kp] < fronts[b]).to(torch.uint8)
        assert out.pos_is_gt.dtype == torch.uint8 and torch.equal(out.pos_is_gt[b * num:(b + 1) * num], is_gt), b
        s, d = slice(b * nep, (b + 1) * nep), slice(b * num, b * num + nep)
        live = (torch.arange(nep, device=DEV) < kp)
        w_rois = torch.where(live[:, None], rois[d], torch.tensor([-1.0, 0, 0, 0, 0], device=DEV)[None, :])
        assert torch.equal(raw(out.pos_rois[s]), raw(w_rois)), b
        assert torch.equal(out.pos_gt_inds[s], torch.where(live, pos_gt[d], torch.full_like(pos_gt[d], -1))), b
        assert torch.equal(out.pos_labels[s], torch.where(live, labels[d], torch.full_like(labels[d], rc.NUM_CLASSES))), b
    return counts


def case_tensors(name):
    props, counts, gts, labs = rc.inputs(name)
    return T(props), T(counts), [T(g) for g in gts], [T(l) for l in labs], [int(n) for n in counts]


def fixture_batch_keys(ref, name):
    return rc.batch_keys(name, [rc.fixture_keys(ref, name, b) for b in range(len(rc.CASES[name]["images"]))])


# ------------------------------------------------------------------------------------------------------------ 1. the chain
@pytest.mark.parametrize("name", list(rc.CASES))
def test_fixture_cases_equal_the_chain_bit_for_bit(ref, name):
    c = rc.CASES[name]
    props, counts, gts, labs, ns = case_tensors(name)
    asg, smp, coder = case_parts(name)
    keys = T(fixture_batch_keys(ref, name))
    out = stage(props, counts, gts, labs, asg, smp, coder, keys, c["pos_weight"], c["decoded"])
    assert_equals_chain(out, props, ns, gts, labs, asg, smp, coder, keys, c["pos_weight"], c["decoded"])


@pytest.mark.parametrize("G", rc.SWEEP_G)
def test_sweep_of_sizes_equals_the_chain_bit_for_bit(G):
    """M_b in {1, 63, 64, 65, 1023, 1024, 1025, 4096} candidates (one image each) with G ground-truth boxes, under the R-CNN
    thresholds without and the RPN thresholds with low-quality matching; hash keys, so the select has work to do."""
    props, ns, gts, labs = rc.sweep_inputs(G)
    B, P = props.shape[:2]
    dp, dn, dg, dl = T(props), T(ns), [T(g) for g in gts], [T(l) for l in labs]
    keys = T(tc.free_keys(B * (G + P), 8900 + G).reshape(B, G + P))
    seen = set()
    for run in (rc.RCNN, rc.LOWQ, ac._with(rc.LOWQ, assign_all=False)):
        asg, smp, coder = parts(run, 512, 0.25)
        out = stage(dp, dn, dg, dl, asg, smp, coder, keys)
        counts = assert_equals_chain(out, dp, [int(n) for n in ns], dg, dl, asg, smp, coder, keys)
        seen.update(map(tuple, N_(counts).tolist()))
    assert len(seen) > 1


# ------------------------------------------------------------------------------------------------------------ 2. the fixture
@pytest.mark.parametrize("name", list(rc.CASES))
def test_fixture_cases_equal_the_reference(ref, ulps, name):
    c = rc.CASES[name]
    num, nep = c["num"], int(c["num"] * c["frac"])
    props, counts, gts, labs, ns = case_tensors(name)
    np_gts = rc.inputs(name)[2]
    out = stage(props, counts, gts, labs, *case_parts(name), T(fixture_batch_keys(ref, name)), c["pos_weight"], c["decoded"])
    allowed = 2 * float(ulps[0])
    for b in range(len(ns)):
        pre = "%s_%d_" % (name, b)
        rois, labels, lw, bt, bw, pg, pos, neg, is_gt = rc.chain_np(name, b, rc.fixture_keys(ref, name, b))
        assert np.array_equal(pos, ref[pre + "pos"]) and np.array_equal(neg, ref[pre + "neg"])
        kp, k = pos.size, pos.size + neg.size
        s = slice(b * num, (b + 1) * num)
        assert N_(out.counts)[b].tolist() == [kp, neg.size], (b, N_(out.counts)[b])
        assert np.array_equal(tc.bits(N_(out.rois)[s]), tc.bits(rois)) and np.array_equal(N_(out.labels)[s], labels)
        assert np.array_equal(N_(out.labels)[s][:k], ref[pre + "labels"])
        assert np.array_equal(tc.bits(N_(out.label_weights)[s]), tc.bits(lw)) and np.array_equal(tc.bits(N_(out.label_weights)[s][:k]), tc.bits(ref[pre + "lw"]))
        assert np.array_equal(tc.bits(N_(out.bbox_weights)[s]), tc.bits(bw)) and np.array_equal(N_(out.pos_assigned_gt_inds)[s], pg)
        assert np.array_equal(N_(out.pos_is_gt)[s], is_gt)
        got = N_(out.bbox_targets)[s]
        assert not tc.bits(got[kp:]).any()
        if c["decoded"]:
            assert np.array_equal(tc.bits(got[:kp]), tc.bits(ref[pre + "bt_pos"]))
        elif kp:
            gi = ref[pre + "gt_inds"].astype(np.int64)
            exact, kinds, err = tc.encode_check(got[:kp], rois[:kp, 1:], np_gts[b][gi[pos] - 1], c["means"], c["stds"])
            print("%s image %d: encode max error %.4f ulp (allowed %.4f)" % (name, b, err, allowed))
            assert exact and kinds and err <= allowed, (b, exact, kinds, err)
            assert np.array_equal(tc.bits(got[:kp, :2]), tc.bits(ref[pre + "bt_pos"][:, :2]))
        ps = slice(b * nep, (b + 1) * nep)
        assert np.array_equal(tc.bits(N_(out.pos_rois)[ps][:kp]), tc.bits(rois[:kp])) and (N_(out.pos_rois)[ps][kp:, 0] == -1).all()
        assert np.array_equal(N_(out.pos_gt_inds)[ps][:kp], pg[:kp]) and (N_(out.pos_gt_inds)[ps][kp:] == -1).all()
        assert np.array_equal(N_(out.pos_labels)[ps][:kp], labels[:kp]) and (N_(out.pos_labels)[ps][kp:] == rc.NUM_CLASSES).all()


# ------------------------------------------------------------------------------------------------------------ 3. counts
def assert_same(a, b):
    for f in a._fields:
        assert torch.equal(raw(getattr(a, f)), raw(getattr(b, f))), f


def test_rows_beyond_the_counts_are_not_read(ref):
    """The rows at or beyond n_b hold copies of a ground-truth box: read, they would be positives."""
    name = "rcnn"
    props, counts, gts, labs, ns = case_tensors(name)
    asg, smp, coder = case_parts(name)
    keys = T(fixture_batch_keys(ref, name))
    clean = stage(props, counts, gts, labs, asg, smp, coder, keys)
    dirty = props.clone()
    for b, n in enumerate(ns):
        box = gts[b][0] if gts[b].shape[0] else gts[0][0]
        dirty[b, n:, :4] = box
    assert ns[1] < props.shape[1]
    got = stage(dirty, counts, gts, labs, asg, smp, coder, keys)
    assert_same(got, clean)
    assert_same(got, stage([props[b, :n] for b, n in enumerate(ns)], None, gts, labs, asg, smp, coder, keys))     # the sliced tensors
    # without counts every row is read: the dirty rows of image 1 now are positives
    full = torch.full_like(counts, props.shape[1])
    assert_same(stage(dirty, None, gts, labs, asg, smp, coder, keys), stage(dirty, full, gts, labs, asg, smp, coder, keys))
    assert int(stage(dirty, None, gts, labs, asg, smp, coder, keys).counts[1, 0]) > int(clean.counts[1, 0])


# ------------------------------------------------------------------------------------------------------------ 4. colliding keys
@pytest.mark.parametrize("kind", ["equal", "four"])
def test_colliding_keys_equal_the_restatement(kind):
    name = "rcnn"
    c = rc.CASES[name]
    props, counts, gts, labs, ns = case_tensors(name)
    B, width = len(ns), 9 + c["P"]
    keys = np.full((B, width), 12345, dtype=np.int32)
    if kind == "four":
        keys = (np.array([7, 2 ** 31 - 1, 0, 1 << 23], dtype=np.int64)[rc._u(B * width, 8950, 4)]).astype(np.int32).reshape(B, width)
    out = stage(props, counts, gts, labs, *case_parts(name), T(keys))
    assert_same(out, stage(props, counts, gts, labs, *case_parts(name), T(keys)))
    for b in range(B):
        gi, boxes, _, front = rc.assign_front_np(name, b)
        pos, neg = tc.sample_np(gi, keys[b, :gi.size], c["num"], c["frac"], c["ub"])
        assert N_(out.counts)[b].tolist() == [pos.size, neg.size]
        rows = N_(out.rois)[b * c["num"]:(b + 1) * c["num"]]
        assert np.array_equal(tc.bits(rows[:pos.size, 1:]), tc.bits(boxes[pos]))
        assert np.array_equal(tc.bits(rows[pos.size:pos.size + neg.size, 1:]), tc.bits(boxes[neg]))
        assert np.array_equal(N_(out.pos_assigned_gt_inds)[b * c["num"]:][:pos.size], gi[pos] - 1)


# ------------------------------------------------------------------------------------------------------------ 5. empty inputs
def test_images_without_proposals():
    asg, smp, coder = parts(rc.RCNN, 64, 0.25)
    _, g = rc.image_boxes(0, 3, 8990)
    gts, labs = [T(g), torch.zeros((0, 4), device=DEV)], [T(np.array([5, 6, 7])), torch.zeros((0,), dtype=torch.int64, device=DEV)]
    keys = T(tc.free_keys(2 * 11, 8991).reshape(2, 11))
    props = T(np.tile(g[0], (2, 8, 1)))                          # never read
    zero = torch.zeros(2, dtype=torch.int64, device=DEV)
    out = stage(props, zero, gts, labs, asg, smp, coder, keys)
    assert N_(out.counts).tolist() == [[3, 0], [0, 0]]
    assert N_(out.pos_is_gt)[:4].tolist() == [1, 1, 1, 0] and not N_(out.pos_is_gt)[4:].any()
    assert N_(out.labels)[:4].tolist() == [5, 6, 7, rc.NUM_CLASSES] and not N_(out.label_weights)[3:].any()
    assert np.array_equal(N_(out.rois)[:3, 1:], g) and not N_(out.rois)[3:, 1:].any() and (N_(out.rois)[64:, 0] == 1).all()
    assert_equals_chain(out, props, [0, 0], gts, labs, asg, smp, coder, keys)
    empty = stage(props[:, :0], None, gts, labs, asg, smp, coder, keys[:, :3].contiguous())     # P = 0
    assert_same(empty, out)


# ------------------------------------------------------------------------------------------------------------ 6. refine
@pytest.mark.parametrize("name", rc.REFINE_CASES)
@pytest.mark.parametrize("agnostic", [False, True])
def test_refine_bboxes(ref, ulps, name, agnostic):
    from iif_amd.mmdet_roi_stage import refine_bboxes, refine_bboxes_padded
    from iif_amd.mmdet_targets import delta2bbox
    c = rc.CASES[name]
    num, B = c["num"], len(c["images"])
    props, counts, gts, labs, ns = case_tensors(name)
    asg, smp, coder = case_parts(name)
    out = stage(props, counts, gts, labs, asg, smp, coder, T(fixture_batch_keys(ref, name)))
    r_lab, r_pred = rc.refine_inputs(name, agnostic)
    d_lab, d_pred = T(r_lab), T(r_pred)
    boxes, kept = refine_bboxes_padded(out.rois, d_lab, d_pred, out.pos_is_gt, out.counts, [rc.IMG + (3,)] * B, coder, agnostic)
    assert boxes.shape == (B, num, 4) and kept.dtype == torch.int64 and kept.shape == (B,)
    allowed = 2 * float(ulps[1])
    exact_rois, exact_lab, exact_pred, is_gts = [], [], [], []
    for b in range(B):
        want = ref["refine_%s_%d_%d" % (name, int(agnostic), b)]
        k = int(out.counts[b].sum())
        s = slice(b * num, b * num + k)
        assert int(kept[b]) == want.shape[0] and not raw(boxes[b, want.shape[0]:]).any()
        got = boxes[b, :want.shape[0]]
        # the decode rule of test_targets_gpu.test_decode, on the kept rows in their order
        keep = N_(out.pos_is_gt)[s] == 0
        d = r_pred[s] if agnostic else np.stack([r_pred[s][np.arange(k), 4 * r_lab[s] + j] for j in range(4)], 1)
        ok, kinds, err = tc.decode_check(N_(got), N_(out.rois)[s][keep, 1:], np.ascontiguousarray(d[keep]), c["means"], c["stds"], rc.IMG,
                                         tc.WH_RATIO_CLIP, True, False, 32)
        print("refine %s image %d: max error %.4f ulp (allowed %.4f)" % (name, b, err, allowed))
        assert ok and kinds and err <= allowed, (b, ok, kinds, err)
        same_order = np.abs(N_(got) - want).max(initial=0.0) <= 1e-2                 # a swapped pair would be pixels apart
        assert same_order
        # the native delta2bbox with torch's gather and boolean indexing, bit for bit
        lab4 = (d_lab[s] * 4)[:, None] + torch.arange(4, device=DEV)[None, :]
        dd = d_pred[s] if agnostic else torch.gather(d_pred[s], 1, lab4)
        tb = delta2bbox(out.rois[s][:, 1:].contiguous(), dd.contiguous(), c["means"], c["stds"], rc.IMG + (3,), tc.WH_RATIO_CLIP)
        assert torch.equal(raw(tb[out.pos_is_gt[s] == 0]), raw(got)), b
        exact_rois.append(out.rois[s]); exact_lab.append(d_lab[s]); exact_pred.append(d_pred[s])
        is_gts.append(out.pos_is_gt[b * num:b * num + int(out.counts[b, 0])])
    lists = refine_bboxes(torch.cat(exact_rois), torch.cat(exact_lab), torch.cat(exact_pred), is_gts,
                          [dict(img_shape=rc.IMG + (3,))] * B, coder, agnostic)
    assert len(lists) == B
    for b in range(B):
        assert torch.equal(raw(lists[b]), raw(boxes[b, :int(kept[b])])), b


def test_refine_decodes_an_out_of_range_label_with_zero_deltas():
    from iif_amd.mmdet_roi_stage import refine_bboxes_padded
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder
    rois = T(np.array([[0, 10, 10, 50, 60], [0, 20, 20, 40, 40], [0, 5, 5, 9, 9], [0, 0, 0, 0, 0]], dtype=np.float32))
    labels = T(np.array([7, -1, 1, 0], dtype=np.int64))
    preds = torch.full((4, 8), 0.25, device=DEV)
    boxes, kept = refine_bboxes_padded(rois, labels, preds, torch.zeros(4, dtype=torch.uint8, device=DEV),
                                       T(np.array([[1, 2]], dtype=np.int64)), [(100, 100)], DeltaXYWHBBoxCoder())
    assert int(kept[0]) == 3 and torch.equal(boxes[0, :2], rois[:2, 1:]) and not torch.equal(boxes[0, 2], rois[2, 1:])
    assert not boxes[0, 3].any()


# ------------------------------------------------------------------------------------------------------------ 7. synchronisation
def test_nothing_synchronises_the_host():
    """rpn_proposals_padded's outputs through roi_stage_targets_padded, then three cascade rounds of (seeded bbox_pred,
    refine_bboxes_padded, roi_stage_targets_padded), under torch's sync debug mode ('error'); mirrors
    test_targets_gpu.test_nothing_but_sample_synchronises_the_host."""
    import types
    from iif_amd import mmdet_nms
    from iif_amd.mmdet_roi_stage import refine_bboxes_padded, roi_stage_targets_padded
    from . import nms_cases as nc
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    c = nc.RPN_CASES["fpn5"]
    cls, reg, anchors = nc.rpn_inputs("fpn5")
    tcls, treg, tanc = ([T(x) for x in v] for v in (cls, reg, anchors))
    cfg = types.SimpleNamespace(nms_pre=c["nms_pre"], max_per_img=c["max_per_img"], min_bbox_size=c["min_size"],
                                nms=dict(type="nms", iou_threshold=c["thr"]))
    rpn_coder = types.SimpleNamespace(means=nc.MEANS, stds=nc.STDS, clip_border=True, add_ctr_clamp=False, ctr_clamp=32)
    B = len(c["shapes"])
    gts = [T(ac.proposals(5, 8970 + b, 120, 100, 8, 60)) for b in range(B)]
    labs = [T(rc._u(5, 8980 + b, rc.REFINE_CLASSES)) for b in range(B)]
    asg, smp, coder = parts(rc.RCNN, 64, 0.25)
    stages = [parts(ac._with(rc.RCNN, pos=t, neg=t, min_pos=t), 64, 0.25) for t in (0.5, 0.6, 0.7)]
    preds = [T(rc.refine_inputs("rcnn", False)[1][:B * 64]) for _ in range(3)]
    mmdet_nms.rpn_proposals_padded(tcls, treg, tanc, c["shapes"], cfg, rpn_coder)         # the library is loaded before the mode is on
    roi_stage_targets_padded(torch.zeros(B, 4, 4, device=DEV), None, gts, labs, asg, smp, coder, rc.REFINE_CLASSES)
    torch.cuda.synchronize()
    outs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        dets, counts = mmdet_nms.rpn_proposals_padded(tcls, treg, tanc, c["shapes"], cfg, rpn_coder)
        t = roi_stage_targets_padded(dets, counts, gts, labs, *stages[0], rc.REFINE_CLASSES)
        outs.append(t)
        for i in range(3):
            labels = torch.where(t.labels < rc.REFINE_CLASSES, t.labels, torch.zeros_like(t.labels))      # stands for the argmax
            boxes, kept = refine_bboxes_padded(t.rois, labels, preds[i], t.pos_is_gt, t.counts, c["shapes"], coder)
            t = roi_stage_targets_padded(boxes, kept, gts, labs, *stages[min(i + 1, 2)], rc.REFINE_CLASSES)
            outs.append(t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert len(outs) == 4
    for t in outs:
        assert all(torch.isfinite(x.float()).all().item() for x in t)
        assert int(t.counts.sum()) > 0 and (t.counts.sum(1) <= 64).all()
