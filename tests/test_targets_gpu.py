"""Box sampling, the delta coder and the target builders on the MI355X: iif_amd.mmdet_targets against the reference's own runs
(tests/golden/g26_targets.npz) and the numpy restatements that the fixture's generator and tests/test_targets_host.py tie to
the reference.

The sampler, the labels, the weights, the gathers and every coder column made of ``+ - * /`` alone are compared EXACTLY (floats
as bit patterns).  The ``log`` / ``exp`` columns are measured in float32 ulps against a float64 continuation from the last
bit-exact float32 intermediate (targets_cases.encode_check / decode_check); the kernel is allowed the reference's own maximum on
that scale (``coder_ref_ulps`` in the fixture, measured by its generator) plus the same amount again: the device's logf / expf
and the CPU's are each near one rounding of the true value, but not the same rounding."""
import numpy as np
import pytest
import torch

from . import targets_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = "g26_targets"


def T(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def N_(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def ref(golden):
    g = golden(FIXTURE)
    tc.check_generator(g)
    return g


def assign_result(gi, labels=None, num_gts=tc.G_DEFAULT):
    from iif_amd.mmdet_assigner import AssignResult
    return AssignResult(num_gts, T(gi), torch.zeros(gi.size, device=DEV), None if labels is None else T(labels))


def sampler_setup(name):
    """(gt_inds before add_gt, gt_inds after, bboxes [n, 4] whose first column is the index, gts, gt labels or None)."""
    N, P, I, num, frac, ub, front = tc.SAMPLER_CASES[name]
    gi = tc.sampler_gt_inds(name)
    bboxes = np.zeros((gi.size, 4), dtype=np.float32)
    bboxes[:, 0] = np.arange(gi.size)
    gts = np.zeros((tc.G_DEFAULT, 4), dtype=np.float32)
    gts[:, 2] = 1000 + np.arange(tc.G_DEFAULT)
    return gi, tc.with_gts_in_front(gi, front), bboxes, gts, (np.arange(tc.G_DEFAULT, dtype=np.int64) if front else None)


def check_padded(p, N, pos, neg, nep, num):
    c = N_(p.counts)
    assert p.counts.dtype == torch.int64 and c.tolist() == [pos.size, neg.size], c
    pi, ni = N_(p.pos_inds), N_(p.neg_inds)
    assert pi.shape == (nep,) and ni.shape == (num,) and p.pos_inds.dtype == torch.int64
    assert np.array_equal(pi[:pos.size], pos), (pi[:8], pos[:8])
    assert np.array_equal(ni[:neg.size], neg), (ni[:8], neg[:8])
    assert (pi[pos.size:] == -1).all() and (ni[neg.size:] == -1).all()
    f = N_(p.flags)
    assert f.dtype == np.int8 and f.shape == (N,)
    bad = np.nonzero(f != tc.flags_np(N, pos, neg))[0]
    assert bad.size == 0, (bad[:8], f[bad[:8]])


@pytest.mark.parametrize("name", list(tc.SAMPLER_CASES))
def test_sampler_equals_the_reference(ref, name):
    """Every fixture case with the fixture's keys: the padded lists, counts, tails and flags, then SamplingResult's fields."""
    from iif_amd.mmdet_targets import RandomSampler
    N, P, I, num, frac, ub, front = tc.SAMPLER_CASES[name]
    gi, gi2, bboxes, gts, glab = sampler_setup(name)
    keys = tc.fixture_keys(ref, "s", name, gi2)
    pos, neg = ref["s_%s_pos" % name].astype(np.int64), ref["s_%s_neg" % name].astype(np.int64)
    smp = RandomSampler(num, frac, neg_pos_ub=ub, add_gt_as_proposals=bool(front))
    b5 = torch.cat([T(bboxes), torch.full((gi.size, 1), 0.5, device=DEV)], dim=1)          # a score column, as the RPN's proposals
    p = smp.sample_padded(assign_result(gi), b5, T(gts), T(glab), keys=T(keys))
    check_padded(p, N, pos, neg, int(num * frac), num)
    res = smp.sample(assign_result(gi), b5, T(gts), T(glab), keys=T(keys))
    allb = np.concatenate([gts, bboxes]) if front else bboxes
    assert np.array_equal(N_(res.pos_inds), pos) and np.array_equal(N_(res.neg_inds), neg)
    assert np.array_equal(N_(res.pos_bboxes), allb[pos]) and np.array_equal(N_(res.neg_bboxes), allb[neg])
    assert np.array_equal(N_(res.pos_is_gt), (pos < front).astype(np.uint8)) and res.num_gts == tc.G_DEFAULT
    assert np.array_equal(N_(res.pos_assigned_gt_inds), gi2[pos] - 1)
    assert np.array_equal(N_(res.pos_gt_bboxes), gts[gi2[pos] - 1]) and res.pos_gt_labels is None
    assert np.array_equal(N_(res.bboxes), allb[np.concatenate([pos, neg])])


@pytest.mark.parametrize("kind", ["equal", "four", "equal_rpn"])
def test_sampler_with_colliding_keys_equals_the_restatement(kind):
    """All keys equal (the boundary list is every candidate: ties go to the lower index) and keys in {0..3}; the first also at
    a size that spans several blocks."""
    from iif_amd.mmdet_targets import RandomSampler
    case = "rpn" if kind == "equal_rpn" else "many_pos"
    gi = tc.sampler_gt_inds(case)
    N = gi.size
    keys = np.full(N, 0x12345678, dtype=np.int32) if kind != "four" else (tc.free_keys(N, 99) & 3).astype(np.int32)
    bboxes = torch.zeros((N, 4), device=DEV)
    gts = torch.zeros((tc.G_DEFAULT, 4), device=DEV)
    for num, frac, ub in ((256, 0.5, -1), (512, 0.25, -1), (7, 0.5, 2), (3000, 0.5, -1)):
        pos, neg = tc.sample_np(gi, keys, num, frac, ub)
        p = RandomSampler(num, frac, neg_pos_ub=ub, add_gt_as_proposals=False).sample_padded(assign_result(gi), bboxes, gts, keys=T(keys))
        check_padded(p, N, pos, neg, int(num * frac), num)


def test_sampler_with_every_key_in_one_bin_equals_the_restatement():
    """tc.one_bin_keys: two sweep tiles, every candidate a boundary candidate, the threshold key found by the two low-digit
    histograms and tied (test_targets_host.py checks that the selection cuts through the tie)."""
    from iif_amd.mmdet_targets import RandomSampler
    keys, gi = tc.one_bin_keys(), tc.one_bin_gt_inds()
    N = gi.size
    bboxes = torch.zeros((N, 4), device=DEV)
    gts = torch.zeros((tc.G_DEFAULT, 4), device=DEV)
    for num, frac, ub in tc.ONE_BIN_BUDGETS:
        pos, neg = tc.sample_np(gi, keys, num, frac, ub)
        p = RandomSampler(num, frac, neg_pos_ub=ub, add_gt_as_proposals=False).sample_padded(assign_result(gi), bboxes, gts, keys=T(keys))
        check_padded(p, N, pos, neg, int(num * frac), num)


def test_sampler_edge_sizes():
    """No candidates at all, a zero budget, and a budget of everything."""
    from iif_amd.mmdet_targets import RandomSampler
    gts = torch.zeros((tc.G_DEFAULT, 4), device=DEV)
    p = RandomSampler(8, 0.5, add_gt_as_proposals=False).sample_padded(assign_result(np.zeros(0, dtype=np.int64)), torch.zeros((0, 4), device=DEV), gts)
    assert N_(p.counts).tolist() == [0, 0] and (N_(p.pos_inds) == -1).all() and (N_(p.neg_inds) == -1).all() and p.flags.numel() == 0
    gi = tc.sampler_gt_inds("wave")
    keys = tc.free_keys(gi.size, 7)
    for num, frac in ((0, 0.5), (4, 0.0), (4, 1.0), (100, 0.5)):
        pos, neg = tc.sample_np(gi, keys, num, frac)
        p = RandomSampler(num, frac, add_gt_as_proposals=False).sample_padded(assign_result(gi), torch.zeros((gi.size, 4), device=DEV), gts, keys=T(keys))
        check_padded(p, gi.size, pos, neg, int(num * frac), num)


# ------------------------------------------------------------------------------------------------------------ coder
@pytest.mark.parametrize("name", list(tc.ENCODE_CASES))
def test_encode(ref, name):
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, bbox2delta
    n, means, stds = tc.ENCODE_CASES[name]
    p5, g = tc.encode_inputs(name)
    allowed = 2 * float(ref["coder_ref_ulps"][0])
    dp5, dg = T(p5), T(g)
    out = bbox2delta(dp5, dg, means, stds)                                     # the 5-column tensor read in place
    assert out.shape == (n, 4) and out.dtype == torch.float32
    exact, kinds, err = tc.encode_check(N_(out), p5[:, :4], g, means, stds)
    print("encode %s: max error %.4f ulp (allowed %.4f)" % (name, err, allowed))
    assert exact, "dx / dy differ from the reference's bits"
    assert kinds, "non-finite entries differ in kind or position"
    assert err <= allowed, (err, allowed)
    via = DeltaXYWHBBoxCoder(means, stds).encode(dp5[:, :4], dg)               # a [:, :4] view of pitch 5; and a compact copy
    assert torch.equal(via.view(torch.int32), out.view(torch.int32))
    assert torch.equal(bbox2delta(dp5[:, :4].contiguous(), dg, means, stds).view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize("name", list(tc.DECODE_CASES))
def test_decode(ref, name):
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, delta2bbox
    n, K, means, stds, max_shape, clip_border, ctr, ctr_clamp = tc.DECODE_CASES[name]
    rois, d = tc.decode_inputs(name)
    allowed = 2 * float(ref["coder_ref_ulps"][1])
    out = DeltaXYWHBBoxCoder(means, stds, clip_border, ctr, ctr_clamp).decode(T(rois), T(d), max_shape, tc.WH_RATIO_CLIP)
    assert out.shape == (n, 4 * K) and out.dtype == torch.float32
    args = (means, stds, max_shape, tc.WH_RATIO_CLIP, clip_border, ctr, ctr_clamp)
    ok, kinds, err = tc.decode_check(N_(out), rois, d, *args)
    print("decode %s: max error %.4f ulp (allowed %.4f)" % (name, err, allowed))
    assert ok, "entries the clip replaced differ from the bound's bits"
    assert kinds, "non-finite entries differ in kind or position"
    assert err <= allowed, (err, allowed)
    r5 = torch.cat([T(rois), torch.rand((n, 1), device=DEV)], dim=1)
    wide = torch.cat([T(d), torch.rand((n, 3), device=DEV)], dim=1)            # rois of pitch 5, deltas of pitch 4 K + 3
    again = delta2bbox(r5, wide[:, :4 * K], *args)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))


def test_decode_passes_nan_through_clamp_and_clip():
    from iif_amd.mmdet_targets import delta2bbox
    rois = torch.tensor([[0., 0., 10., 10.], [0., 0., 10., 10.]], device=DEV)
    d = torch.tensor([[float("nan"), 0., 0., float("nan")], [0., 0., 100., -100.]], device=DEV)
    out = N_(delta2bbox(rois, d, max_shape=(20, 20)))
    assert np.isnan(out[0, 0]) and np.isnan(out[0, 2]) and np.isnan(out[0, 1]) and np.isnan(out[0, 3])
    assert out[1].tolist()[0] == 0.0 and out[1, 2] == 20.0 and abs(out[1, 1] - (5 - 0.5 * 10 * 0.016)) < 1e-5


# ------------------------------------------------------------------------------------------------------------ targets
class FixedAssigner:
    """Stands in for the assigner: the case's prepared gt_inds for whatever candidates it is given."""

    def __init__(self, gi):
        self.gi = gi

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        assert bboxes.shape[0] == self.gi.size and gt_labels is None
        return assign_result(self.gi, num_gts=gt_bboxes.shape[0])


def fixed_keys_sampler(keys, *a, **kw):
    """A RandomSampler whose draw is the fixture's keys."""
    from iif_amd.mmdet_targets import RandomSampler

    class FixedKeys(RandomSampler):
        def sample_padded(self, assign_result, bboxes, gt_bboxes, gt_labels=None, keys=None):
            return RandomSampler.sample_padded(self, assign_result, bboxes, gt_bboxes, gt_labels, keys=self.fixed)
    s = FixedKeys(*a, **kw)
    s.fixed = keys
    return s


def check_encoded_rows(got, want_np, boxes, gts, means, stds, allowed, decoded=False):
    if decoded or got.shape[0] == 0:
        assert np.array_equal(tc.bits(got), tc.bits(want_np))
        return
    exact, kinds, err = tc.encode_check(got, boxes, gts, means, stds)
    assert exact and kinds and err <= allowed, (exact, kinds, err, allowed)


@pytest.mark.parametrize("name", list(tc.ANCHOR_CASES))
def test_anchor_targets(ref, name):
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, anchor_inside_flags, anchor_targets_single
    with_labels, pos_weight, decoded, masked, means, stds = tc.ANCHOR_CASES[name]
    anchors, gts, glab, gi_full, inside = tc.anchor_inputs()
    gi = gi_full[inside] if masked else gi_full
    keys = tc.fixture_keys(ref, "a", name, gi)
    w_lab, w_lw, w_bt, w_bw, pos, neg = tc.anchor_targets_np(anchors, gts, glab if with_labels else None, gi_full, keys,
                                                             inside if masked else None, tc.ANCHOR_CLASSES, pos_weight, decoded, means, stds)
    assert np.array_equal(pos, ref["a_%s_pos" % name]) and np.array_equal(neg, ref["a_%s_neg" % name])
    da = T(anchors)
    flags = None
    if masked:
        flags = anchor_inside_flags(da, torch.ones(tc.A_TARGETS, dtype=torch.bool, device=DEV), tc.IMG_SHAPE + (3,), 0)
        assert np.array_equal(N_(flags), inside)
    num, frac, ub = tc.ANCHOR_SAMPLER
    smp = fixed_keys_sampler(T(keys), num, frac, neg_pos_ub=ub, add_gt_as_proposals=False)
    labels, lw, bt, bw, counts = anchor_targets_single(da, T(gts), None, T(glab) if with_labels else None, FixedAssigner(gi), smp,
                                                       DeltaXYWHBBoxCoder(means, stds), tc.ANCHOR_CLASSES, pos_weight=pos_weight,
                                                       inside_flags=flags, reg_decoded_bbox=decoded)
    assert N_(counts).tolist() == [pos.size, neg.size]
    assert labels.dtype == torch.int64 and np.array_equal(N_(labels), w_lab)
    assert np.array_equal(tc.bits(N_(lw)), tc.bits(w_lw)) and np.array_equal(tc.bits(N_(bw)), tc.bits(w_bw))
    sel = (np.nonzero(inside)[0] if masked else np.arange(tc.A_TARGETS))[pos]
    assert np.array_equal(N_(labels)[sel], ref["a_%s_labels_pos" % name])
    got = N_(bt)
    rest = np.ones(tc.A_TARGETS, dtype=bool)
    rest[sel] = False
    assert not tc.bits(got[rest]).any()
    check_encoded_rows(got[sel], w_bt[sel], anchors[sel], gts[gi[pos] - 1], means, stds, 2 * float(ref["coder_ref_ulps"][0]), decoded)
    sums = ref["a_%s_sums" % name]
    assert tc.bit_sum(N_(lw)) == sums[0] and tc.bit_sum(N_(bw)) == sums[1]


def test_anchor_targets_with_an_empty_mask_return_none():
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler, anchor_targets_single
    anchors, gts, _, gi, _ = tc.anchor_inputs()
    out = anchor_targets_single(T(anchors), T(gts), None, None, FixedAssigner(gi), RandomSampler(256, 0.5, add_gt_as_proposals=False),
                                DeltaXYWHBBoxCoder(), 1, inside_flags=torch.zeros(tc.A_TARGETS, dtype=torch.bool, device=DEV))
    assert out == (None,) * 5


@pytest.mark.parametrize("name", list(tc.ROI_CASES))
def test_roi_targets(ref, name):
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler, bbox_targets
    case, means, stds, pos_weight = tc.ROI_CASES[name]
    b, gts, lab, gi, cand_lab, (num, frac, ub, front) = tc.roi_inputs(name)
    gi2 = tc.with_gts_in_front(gi, front)
    allb = np.concatenate([gts, b]) if front else b
    alll = np.concatenate([lab, cand_lab]) if front else cand_lab
    keys = tc.fixture_keys(ref, "r", name, gi2)
    pos, neg = ref["r_%s_pos" % name].astype(np.int64), ref["r_%s_neg" % name].astype(np.int64)
    want = tc.roi_targets_np(allb, gts, gi2, alll, pos, neg, num, tc.ROI_CLASSES, pos_weight, means, stds, img=1)
    smp = RandomSampler(num, frac, neg_pos_ub=ub, add_gt_as_proposals=bool(front))
    coder = DeltaXYWHBBoxCoder(means, stds)
    allowed = 2 * float(ref["coder_ref_ulps"][0])
    k = pos.size + neg.size
    # two images with the same content: the second one's rows carry image index 1
    ps = [smp.sample_padded(assign_result(gi, cand_lab), T(b), T(gts), T(lab), keys=T(keys)) for _ in range(2)]
    labels, lw, bt, bw, rois, pg = bbox_targets(ps, [T(gts)] * 2, [T(lab)] * 2, coder, tc.ROI_CLASSES, pos_weight=pos_weight)
    assert labels.shape == (2 * num,) and rois.shape == (2 * num, 5) and bt.shape == (2 * num, 4)
    assert np.array_equal(N_(rois)[:num, 0], np.zeros(num)) and np.array_equal(tc.bits(N_(rois)[num:]), tc.bits(want[0]))
    for img in (0, 1):
        s = slice(img * num, (img + 1) * num)
        assert np.array_equal(N_(labels)[s], want[1]) and np.array_equal(tc.bits(N_(lw)[s]), tc.bits(want[2]))
        assert np.array_equal(tc.bits(N_(bw)[s]), tc.bits(want[4])) and np.array_equal(N_(pg)[s], want[5])
        assert np.array_equal(tc.bits(N_(rois)[s][:, 1:]), tc.bits(want[0][:, 1:]))
        got = N_(bt)[s]
        assert not tc.bits(got[pos.size:]).any()
        check_encoded_rows(got[:pos.size], want[3][:pos.size], allb[pos], gts[gi2[pos] - 1], means, stds, allowed)
    assert np.array_equal(N_(labels)[:k], ref["r_%s_labels" % name]) and np.array_equal(tc.bits(N_(lw)[:k]), tc.bits(ref["r_%s_lw" % name]))
    # padding rows: zero box, background, zero weights
    assert not N_(rois)[k:num, 1:].any() and (N_(labels)[k:num] == tc.ROI_CLASSES).all() and not N_(lw)[k:num].any()
    # the exact-size path on SamplingResults gives the first k rows
    res = smp.sample(assign_result(gi, cand_lab), T(b), T(gts), T(lab), keys=T(keys))
    e_labels, e_lw, e_bt, e_bw = bbox_targets([res], [T(gts)], [T(lab)], coder, tc.ROI_CLASSES, pos_weight=pos_weight, concat=False)
    assert len(e_labels) == 1 and e_labels[0].shape == (k,)
    assert torch.equal(e_labels[0], labels[:k]) and torch.equal(e_lw[0], lw[:k]) and torch.equal(e_bw[0], bw[:k])
    assert torch.equal(e_bt[0].view(torch.int32), bt[:k].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ host synchronisation
def test_nothing_but_sample_synchronises_the_host(ref):
    """sample_padded, anchor_targets_single without a mask, bbox_targets on padded samplings and the coder under torch's sync
    debug mode ('error').  sample() is left out: its one read of the two counts is by design."""
    from iif_amd.mmdet_assigner import MaxIoUAssigner
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler, anchor_targets_single, bbox_targets
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    anchors, gts, glab, gi_full, _ = tc.anchor_inputs()
    b, rgts, rlab, rgi, rcl, (num, frac, ub, front) = tc.roi_inputs("rcnn")
    da, dg, dl, db, drg, drl = T(anchors), T(gts), T(glab), T(b), T(rgts), T(rlab)
    p5, g = tc.encode_inputs("n65_both")
    rois, d = tc.decode_inputs("k3")
    dp5, dgt, drois, dd = T(p5), T(g), T(rois), T(d)
    coder = DeltaXYWHBBoxCoder(tc.MEANS[1], tc.STDS[1])
    rpn_s = RandomSampler(256, 0.5, add_gt_as_proposals=False)
    rcnn_s = RandomSampler(num, frac, add_gt_as_proposals=True)
    asg = MaxIoUAssigner(0.7, 0.3, min_pos_iou=0.3)
    ars = [assign_result(rgi, rcl) for _ in range(2)] + [assign_result(gi_full)]
    anchor_targets_single(da, dg, None, None, asg, rpn_s, coder, 1)            # the library is loaded before the mode is on
    torch.cuda.synchronize()
    out = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        out.append(rpn_s.sample_padded(ars[2], da, dg).counts)
        out.extend(anchor_targets_single(da, dg, None, None, asg, rpn_s, coder, 1))
        out.extend(anchor_targets_single(da, dg, None, dl, asg, rpn_s, coder, tc.ANCHOR_CLASSES, pos_weight=2.0, reg_decoded_bbox=True))
        ps = [rcnn_s.sample_padded(ars[i], db, drg, drl) for i in range(2)]
        out.extend(bbox_targets(ps, [drg] * 2, [drl] * 2, coder, tc.ROI_CLASSES))
        out.append(coder.encode(dp5[:, :4], dgt))
        out.append(coder.decode(drois, dd, tc.MAX_SHAPE))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert len(out) == 19 and all(torch.isfinite(o.float()).all().item() for o in out)


# ------------------------------------------------------------------------------------------------------------ the draw
def test_the_draw_follows_the_torch_seed_and_is_uniform():
    """Same torch seed, same sample; two calls without reseeding differ.  64 positives, keep 16, 2000 calls: each candidate is
    kept 500 +- 97 times - five standard deviations of Binomial(2000, 1/4), a false alarm below 1e-4 over the 64 candidates.
    A key draw that is reused or not uniform fails this."""
    from iif_amd.mmdet_targets import RandomSampler
    gi = np.ones(64, dtype=np.int64)
    bboxes = torch.zeros((64, 4), device=DEV)
    gts = torch.zeros((1, 4), device=DEV)
    smp = RandomSampler(32, 0.5, add_gt_as_proposals=False)
    ar = assign_result(gi, num_gts=1)
    torch.manual_seed(1234)
    a = smp.sample_padded(ar, bboxes, gts)
    b = smp.sample_padded(ar, bboxes, gts)
    torch.manual_seed(1234)
    c = smp.sample_padded(ar, bboxes, gts)
    assert torch.equal(a.pos_inds, c.pos_inds) and torch.equal(a.flags, c.flags)
    assert not torch.equal(a.pos_inds, b.pos_inds)
    assert N_(a.counts).tolist() == [16, 0]
    kept = torch.zeros(64, dtype=torch.int64, device=DEV)
    for _ in range(2000):
        kept += smp.sample_padded(ar, bboxes, gts).flags == 1
    kept = N_(kept)
    print("kept per candidate: min %d, max %d" % (kept.min(), kept.max()))
    assert kept.sum() == 2000 * 16 and np.abs(kept - 500).max() <= 97, kept
