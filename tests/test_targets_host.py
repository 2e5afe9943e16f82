"""Box sampling, the delta coder and the target builders (mmdet RandomSampler, DeltaXYWHBBoxCoder, AnchorHead / BBoxHead
targets), the part that needs no device: the fixture tests/golden/g26_targets.npz against the input generators and the numpy
restatements of tests/targets_cases.py, the Python surface's constructors, attributes, assertions and errors, and the five C
entry points in header, library and ctypes table with their argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from . import targets_cases as tc
from iif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_bbox2delta", "iif_delta2bbox", "iif_random_sample", "iif_anchor_targets", "iif_roi_targets")
FIXTURE = "g26_targets"


def test_fixture_inputs_regenerate(golden):
    tc.check_generator(golden(FIXTURE))


@pytest.mark.parametrize("name", list(tc.SAMPLER_CASES))
def test_selection_rule_reproduces_the_reference_sampler(golden, name):
    """With the fixture's keys "the k smallest (key, index) pairs" is the reference's gallery[randperm[:k]]."""
    g = golden(FIXTURE)
    N, P, I, num, frac, ub, front = tc.SAMPLER_CASES[name]
    gi = tc.with_gts_in_front(tc.sampler_gt_inds(name), front)
    assert gi.size == N and (gi > 0).sum() == P and (gi < 0).sum() == I
    keys = tc.fixture_keys(g, "s", name, gi)
    assert keys.dtype == np.int32 and keys.min() >= 0
    pos, neg = tc.sample_np(gi, keys, num, frac, ub)
    assert np.array_equal(pos, g["s_%s_pos" % name]) and np.array_equal(neg, g["s_%s_neg" % name])
    assert np.all(np.diff(pos) > 0) and np.all(np.diff(neg) > 0)


def test_sampler_cases_are_what_they_are_there_for(golden):
    g = golden(FIXTURE)
    sizes = {k: (g["s_%s_pos" % k].size, g["s_%s_neg" % k].size) for k in tc.SAMPLER_CASES}
    assert sizes == {"one": (1, 0), "wave": (16, 16), "few_pos": (17, 239), "many_pos": (128, 128), "no_pos": (0, 256),
                     "short": (40, 60), "ub": (10, 30), "rcnn": (128, 384), "rpn": (128, 128)}
    # keys spread over the whole range (many histogram bins) for a drawn class
    gi = tc.sampler_gt_inds("rpn")
    keys = tc.fixture_keys(g, "s", "rpn", gi)
    assert np.unique(keys[gi == 0] >> 19).size == 4096


def test_selection_rule_with_colliding_keys():
    """Ties on the key go to the lower index; all keys equal selects the first k of each class."""
    gi = tc.sampler_gt_inds("many_pos")
    pos, neg = tc.sample_np(gi, np.full(gi.size, 12345, dtype=np.int32), 256, 0.5)
    assert np.array_equal(pos, np.nonzero(gi > 0)[0][:128]) and np.array_equal(neg, np.nonzero(gi == 0)[0][:128])
    keys = np.array([5, 1, 1, 1, 0], dtype=np.int32)
    pos, neg = tc.sample_np(np.array([1, 2, 1, 3, 0]), keys, 4, 0.5)
    assert pos.tolist() == [1, 2] and neg.tolist() == [4]


def test_one_bin_case_cuts_through_a_tie_at_the_threshold_key():
    """What the GPU tests on tc.one_bin_keys rely on: one bin of the top 12 key bits, both classes over budget, and for each
    budget a class whose threshold key has more members than the selection takes from them."""
    keys, gi = tc.one_bin_keys(), tc.one_bin_gt_inds()
    assert keys.size == 4100 and np.unique(keys >> 19).size == 1 and np.array_equal(keys[4::5], keys[3::5])
    ties = []
    for num, frac, ub in tc.ONE_BIN_BUDGETS:
        pos, neg = tc.sample_np(gi, keys, num, frac, ub)
        assert 0 < pos.size < (gi > 0).sum() and 0 < neg.size < (gi == 0).sum()
        ties.append(tc.threshold_ties(gi, keys, pos, neg))
    assert ties == [[0, 1], [1, 0]]


@pytest.mark.parametrize("name", list(tc.ENCODE_CASES))
def test_encode_restatement_against_the_fixture(golden, name):
    g = golden(FIXTURE)
    n, means, stds = tc.ENCODE_CASES[name]
    p5, gt = tc.encode_inputs(name)
    mine = tc.bbox2delta_np(p5[:, :4], gt, means, stds)
    ref_ulps = float(g["coder_ref_ulps"][0])
    exact, kinds, err = tc.encode_check(mine, p5[:, :4], gt, means, stds)
    assert exact and kinds and err <= 2 * ref_ulps, (err, ref_ulps)
    if n <= 65:
        ref = g["e_%s_out" % name]
        assert np.array_equal(tc.bits(mine[:, :2]), tc.bits(ref[:, :2]))
        exact, kinds, err = tc.encode_check(ref, p5[:, :4], gt, means, stds)
        assert exact and kinds and err <= ref_ulps
    else:
        ref = g["e_%s_head" % name]
        fin = np.isfinite(ref[:, :2])
        assert np.array_equal(tc.bits(mine[:16, :2][fin]), tc.bits(ref[:, :2][fin]))
        assert tc.bit_sum(mine[:, :2][np.isfinite(mine[:, :2])]) == g["e_%s_xy_bitsum" % name]
        kinds_ref = g["e_%s_kinds" % name]
        assert np.array_equal(tc._kind(mine), kinds_ref)
        assert kinds_ref[7].any() and not np.delete(kinds_ref, 7, axis=0).any()          # the degenerate row, and only it


@pytest.mark.parametrize("name", list(tc.DECODE_CASES))
def test_decode_restatement_against_the_fixture(golden, name):
    g = golden(FIXTURE)
    n, K, means, stds, max_shape, clip_border, ctr, ctr_clamp = tc.DECODE_CASES[name]
    rois, d = tc.decode_inputs(name)
    args = (means, stds, max_shape, tc.WH_RATIO_CLIP, clip_border, ctr, ctr_clamp)
    mine = tc.delta2bbox_np(rois, d, *args)
    assert mine.shape == (n, 4 * K)
    ref_ulps = float(g["coder_ref_ulps"][1])
    ok, kinds, err = tc.decode_check(mine, rois, d, *args)
    assert ok and kinds and err <= 2 * ref_ulps, (err, ref_ulps)
    ref = g["d_%s_out" % name] if n * K <= 65 * 3 else g["d_%s_head" % name]
    assert np.allclose(mine[:ref.shape[0]], ref, rtol=1e-5, atol=1e-3)
    clipped = g["d_%s_clipped" % name]
    if clip_border and max_shape is not None and n >= 63:
        assert clipped[0] > 0 and clipped[1] > 0
        assert (mine == 0).sum() == clipped[0]
    if not clip_border:
        assert mine.min() < 0 or mine.max() > 1333


def test_coder_error_figures_are_sane(golden):
    e = golden(FIXTURE)["coder_ref_ulps"]
    assert e.shape == (2,) and 0.4 < e[0] < 8 and 0.4 < e[1] < 8


@pytest.mark.parametrize("name", list(tc.ANCHOR_CASES))
def test_anchor_target_restatement_against_the_fixture(golden, name):
    g = golden(FIXTURE)
    with_labels, pos_weight, decoded, masked, means, stds = tc.ANCHOR_CASES[name]
    anchors, gts, glab, gi_full, inside = tc.anchor_inputs()
    gi = gi_full[inside] if masked else gi_full
    keys = tc.fixture_keys(g, "a", name, gi)
    labels, lw, bt, bw, pos, neg = tc.anchor_targets_np(anchors, gts, glab if with_labels else None, gi_full, keys,
                                                        inside if masked else None, tc.ANCHOR_CLASSES, pos_weight, decoded, means, stds)
    assert np.array_equal(pos, g["a_%s_pos" % name]) and np.array_equal(neg, g["a_%s_neg" % name])
    sel = (np.nonzero(inside)[0] if masked else np.arange(tc.A_TARGETS))[pos]
    assert np.array_equal(labels[sel], g["a_%s_labels_pos" % name])
    sums = g["a_%s_sums" % name]
    assert tc.bit_sum(lw) == sums[0] and tc.bit_sum(bw) == sums[1] and np.uint64(labels.sum()) == sums[2]
    ref_bt = g["a_%s_bt_pos" % name]
    assert np.array_equal(tc.bits(bt[sel][:, :2]), tc.bits(ref_bt[:, :2]))
    if decoded:
        assert np.array_equal(tc.bits(bt[sel]), tc.bits(ref_bt))
    else:
        assert np.allclose(bt[sel], ref_bt, rtol=1e-5, atol=1e-6)
    rest = np.ones(tc.A_TARGETS, dtype=bool)
    rest[sel] = False
    assert not bt[rest].any() and not bw[rest].any() and (labels[rest] == tc.ANCHOR_CLASSES).all()
    if masked:
        assert 0 < inside.sum() < tc.A_TARGETS and not lw[~inside].any()
    if pos_weight > 0:
        assert (lw[sel] == pos_weight).all()


@pytest.mark.parametrize("name", list(tc.ROI_CASES))
def test_roi_target_restatement_against_the_fixture(golden, name):
    g = golden(FIXTURE)
    case, means, stds, pos_weight = tc.ROI_CASES[name]
    b, gts, lab, gi, cand_lab, (num, frac, ub, front) = tc.roi_inputs(name)
    gi2 = tc.with_gts_in_front(gi, front)
    allb = np.concatenate([gts, b]) if front else b
    alll = np.concatenate([lab, cand_lab]) if front else cand_lab
    keys = tc.fixture_keys(g, "r", name, gi2)
    pos, neg = tc.sample_np(gi2, keys, num, frac, ub)
    assert np.array_equal(pos, g["r_%s_pos" % name]) and np.array_equal(neg, g["r_%s_neg" % name])
    rois, labels, lw, bt, bw, pg = tc.roi_targets_np(allb, gts, gi2, alll, pos, neg, num, tc.ROI_CLASSES, pos_weight, means, stds)
    k = pos.size + neg.size
    assert np.array_equal(labels[:k], g["r_%s_labels" % name]) and np.array_equal(tc.bits(lw[:k]), tc.bits(g["r_%s_lw" % name]))
    assert np.array_equal(tc.bits(bt[:pos.size, :2]), tc.bits(g["r_%s_bt_pos" % name][:, :2]))
    assert np.allclose(bt[:pos.size], g["r_%s_bt_pos" % name], rtol=1e-5, atol=1e-6)
    assert (labels[k:] == tc.ROI_CLASSES).all() and not lw[k:].any() and not rois[k:, 1:].any() and (pg[pos.size:] == -1).all()
    assert (name == "nopos") == (pos.size == 0)


# ------------------------------------------------------------------------------------------------------------ Python surface
def test_constructors_and_attributes_mirror_the_reference():
    from iif_amd import mmdet_targets as M
    c = M.DeltaXYWHBBoxCoder()
    assert (c.means, c.stds, c.clip_border, c.add_ctr_clamp, c.ctr_clamp) == ((0., 0., 0., 0.), (1., 1., 1., 1.), True, False, 32)
    c = M.DeltaXYWHBBoxCoder(target_means=(1, 2, 3, 4), target_stds=(.1, .1, .2, .2), clip_border=False, add_ctr_clamp=True, ctr_clamp=8)
    assert (c.means, c.stds, c.clip_border, c.add_ctr_clamp, c.ctr_clamp) == ((1, 2, 3, 4), (.1, .1, .2, .2), False, True, 8)
    s = M.RandomSampler(256, 0.5)
    assert (s.num, s.pos_fraction, s.neg_pos_ub, s.add_gt_as_proposals) == (256, 0.5, -1, True)
    assert s.pos_sampler is s and s.neg_sampler is s
    s = M.RandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=3, add_gt_as_proposals=False, rng=7)
    assert (s.num, s.pos_fraction, s.neg_pos_ub, s.add_gt_as_proposals) == (512, 0.25, 3, False)
    doc = M.RandomSampler.__doc__
    assert "randperm" in doc and "lower index" in doc and "268 569" in doc
    for word in ("PseudoSampler", "OHEM", "atch dimensions", "mask inside the assigner", "ONNX"):
        assert word in M.__doc__, word


def test_anchor_inside_flags_mirrors_the_reference():
    from iif_amd.mmdet_targets import anchor_inside_flags
    anchors, _, _, _, inside = tc.anchor_inputs()
    valid = torch.ones(tc.A_TARGETS, dtype=torch.bool)
    got = anchor_inside_flags(torch.from_numpy(anchors), valid, tc.IMG_SHAPE + (3,), 0)
    assert np.array_equal(got.numpy(), inside)
    assert anchor_inside_flags(torch.from_numpy(anchors), valid, tc.IMG_SHAPE, -1) is valid
    wide = anchor_inside_flags(torch.from_numpy(anchors), valid, tc.IMG_SHAPE, 64)
    assert inside.sum() < wide.sum().item() < tc.A_TARGETS


def test_sampling_result_mirrors_the_reference_fields():
    from iif_amd.mmdet_assigner import AssignResult
    from iif_amd.mmdet_targets import SamplingResult
    bboxes = torch.arange(24, dtype=torch.float32).view(6, 4)
    gts = torch.tensor([[0., 0., 1., 1.], [2., 2., 3., 3.]])
    ar = AssignResult(2, torch.tensor([1, 2, 0, 2, 0, -1]), torch.zeros(6), labels=torch.tensor([5, 7, -1, 7, -1, -1]))
    r = SamplingResult(torch.tensor([0, 3]), torch.tensor([2, 4]), bboxes, gts, ar, torch.tensor([1, 1, 0, 0, 0, 0], dtype=torch.uint8))
    assert r.pos_inds.tolist() == [0, 3] and r.neg_inds.tolist() == [2, 4] and r.num_gts == 2
    assert torch.equal(r.pos_bboxes, bboxes[[0, 3]]) and torch.equal(r.neg_bboxes, bboxes[[2, 4]])
    assert r.pos_is_gt.tolist() == [1, 0] and r.pos_assigned_gt_inds.tolist() == [0, 1]
    assert torch.equal(r.pos_gt_bboxes, gts[[0, 1]]) and r.pos_gt_labels.tolist() == [5, 7]
    assert torch.equal(r.bboxes, bboxes[[0, 3, 2, 4]])
    ar.labels = None
    empty = SamplingResult(torch.zeros(0, dtype=torch.long), torch.tensor([2]), bboxes, torch.zeros(0, 4), ar, torch.zeros(6, dtype=torch.uint8))
    assert empty.pos_gt_bboxes.shape == (0, 4) and empty.pos_gt_labels is None and empty.num_gts == 0


def test_error_conventions():
    from iif_amd import mmdet_targets as M
    from iif_amd.mmdet_assigner import AssignResult
    b4 = torch.zeros(3, 4)
    c = M.DeltaXYWHBBoxCoder()
    with pytest.raises(NotImplementedError):
        c.decode(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))                     # batch dimensions
    with pytest.raises(NotImplementedError):
        M.delta2bbox(b4, b4, max_shape=torch.tensor([800, 1333]))
    with pytest.raises(NotImplementedError):
        M.bbox2delta(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))
    with pytest.raises(NotImplementedError):
        M.bbox2delta(b4.double(), b4.double())
    with pytest.raises(NotImplementedError):
        M.delta2bbox(b4, b4.half())
    with pytest.raises(RuntimeError):
        M.delta2bbox(b4, b4.clone().requires_grad_(True))
    with pytest.raises(AssertionError):
        c.encode(b4, torch.zeros(2, 4))
    with pytest.raises(AssertionError):
        c.encode(torch.zeros(3, 5), torch.zeros(3, 5))                           # the coder's own size(-1) == 4
    with pytest.raises(AssertionError):
        c.decode(b4, torch.zeros(2, 4))
    with pytest.raises(AssertionError):
        M.delta2bbox(b4, torch.zeros(3, 6))
    with pytest.raises(AssertionError):
        M.bbox2delta(b4, b4, means=(0, 0, 0))
    s = M.RandomSampler(8, 0.5)
    ar = AssignResult(1, torch.tensor([1, 0, 0]), torch.zeros(3))
    # CPU tensors are rejected, not emulated
    for call in (lambda: c.encode(b4, b4), lambda: c.decode(b4, b4), lambda: M.bbox2delta(torch.zeros(0, 4), torch.zeros(0, 4)),
                 lambda: s.sample(ar, b4, torch.zeros(1, 4), torch.zeros(1, dtype=torch.long)),
                 lambda: M.RandomSampler(8, 0.5, add_gt_as_proposals=False).sample_padded(ar, b4, torch.zeros(1, 4))):
        with pytest.raises(_lib.IIFNativeError):
            call()


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_entry_points_in_header_library_and_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code)
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name])
    assert re.search(r"#define IIF_SAMPLE_WORKSPACE_BYTES\(N\) \(4 \* \(int64_t\)\(N\) \+ 65536\)", text)


def test_entry_points_check_arguments_before_launching():
    """Bad arguments return -1 before anything touches the device."""
    L = _lib.lib()
    one = 64            # a non-null, aligned stand-in: the checks below fail before any pointer is used
    f4 = (ctypes.c_float * 4)(1, 1, 1, 1)

    def enc(**kw):
        return L.iif_bbox2delta(kw.get("p", one), kw.get("ldp", 4), kw.get("g", one), kw.get("ldg", 5), kw.get("n", 3),
                                kw.get("means", f4), kw.get("stds", f4), kw.get("out", one), None)
    assert enc(p=None) == -1 and enc(g=None) == -1 and enc(out=None) == -1 and enc(means=None) == -1 and enc(stds=None) == -1
    assert enc(n=-1) == -1 and enc(ldp=3) == -1 and enc(ldg=3) == -1 and enc(p=66) == -1 and enc(out=68) == -1
    assert enc(n=0, p=None, out=None) == 0

    def dec(**kw):
        return L.iif_delta2bbox(kw.get("r", one), kw.get("ldr", 4), kw.get("d", one), kw.get("ldd", 12), kw.get("n", 3),
                                kw.get("K", 3), kw.get("means", f4), f4, 4.0, 0, 32.0, 1, 800.0, 1333.0, kw.get("out", one), None)
    assert dec(r=None) == -1 and dec(d=None) == -1 and dec(out=None) == -1 and dec(means=None) == -1
    assert dec(n=-1) == -1 and dec(K=0) == -1 and dec(ldd=11) == -1 and dec(ldr=3) == -1 and dec(d=66) == -1
    assert dec(n=0, r=None) == 0

    def smp(**kw):
        return L.iif_random_sample(kw.get("gi", one), kw.get("keys", one), kw.get("N", 100), kw.get("nep", 8), kw.get("num", 16),
                                   kw.get("ub", -1.0), kw.get("pos", one), kw.get("neg", one), kw.get("counts", one),
                                   kw.get("flags", one), kw.get("ws", one), kw.get("ws_bytes", 400 + 65536), None)
    assert smp(gi=None) == -1 and smp(keys=None) == -1 and smp(pos=None) == -1 and smp(neg=None) == -1
    assert smp(counts=None) == -1 and smp(flags=None) == -1 and smp(ws=None) == -1
    assert smp(N=-1) == -1 and smp(N=1 << 31) == -1 and smp(nep=17) == -1 and smp(nep=-1) == -1 and smp(num=-1) == -1
    assert smp(ub=float("nan")) == -1
    assert smp(ws_bytes=400 + 65535) == -1 and smp(ws=72) == -1 and smp(gi=68) == -1 and smp(keys=66) == -1

    def anc(**kw):
        return L.iif_anchor_targets(kw.get("a", one), kw.get("lda", 4), kw.get("A", 10), kw.get("flags", one), kw.get("gi", one),
                                    kw.get("rows", 10), kw.get("g", one), 4, kw.get("G", 2), None, kw.get("compact", None), 80, -1.0, 0,
                                    kw.get("means", f4), f4, kw.get("labels", one), one, kw.get("bt", one), one, None)
    assert anc(a=None) == -1 and anc(flags=None) == -1 and anc(gi=None) == -1 and anc(g=None) == -1 and anc(labels=None) == -1
    assert anc(A=-1) == -1 and anc(lda=3) == -1 and anc(means=None) == -1 and anc(bt=68) == -1
    assert anc(rows=9) == -1                                    # without compact_index the rows are the anchors
    assert anc(A=0, a=None, rows=0) == 0

    def roi(**kw):
        return L.iif_roi_targets(kw.get("b", one), kw.get("ldb", 4), 100, kw.get("gi", one), None, kw.get("g", one), 4, 2,
                                 kw.get("pos", one), kw.get("neg", one), kw.get("counts", one), kw.get("cap", 16), kw.get("cap_pos", 4),
                                 0, 80, -1.0, 0, kw.get("means", f4), f4, kw.get("rois", one), one, one, kw.get("bt", one), one, one, None)
    assert roi(b=None) == -1 and roi(gi=None) == -1 and roi(g=None) == -1 and roi(pos=None) == -1 and roi(neg=None) == -1
    assert roi(counts=None) == -1 and roi(rois=None) == -1 and roi(means=None) == -1
    assert roi(cap=-1) == -1 and roi(cap_pos=17) == -1 and roi(ldb=3) == -1 and roi(bt=68) == -1
    assert roi(cap=0, cap_pos=0) == 0
