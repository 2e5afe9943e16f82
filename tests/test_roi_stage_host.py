"""CPU-side checks of the RoI stage (iif_amd.mmdet_roi_stage): the fixture's inputs regenerate, the numpy chain of
tests/roi_stage_cases.py (assign_np, with_gts_in_front, sample_np with keys_from_ranks, roi_targets_np, refine_np) reproduces
every case of tests/golden/g33_roi_stage.npz - integers and the ``+ - * /`` columns bit for bit, the ``log`` / ``exp`` columns
within the ``coder_ref_ulps`` rule of targets_cases -, the wrappers refuse what they do not offer before touching the device,
and the library exports both entries.  No device work."""
import numpy as np
import pytest
import torch

from . import roi_stage_cases as rc
from . import targets_cases as tc

FIXTURE = "g33_roi_stage"


@pytest.fixture(scope="module")
def ref(golden):
    g = golden(FIXTURE)
    rc.check_generator(g)
    return g


@pytest.fixture(scope="module")
def ulps(golden):
    return golden("g26_targets")["coder_ref_ulps"]


def test_the_fixture_holds_the_cases_the_kernel_can_get_wrong(ref):
    a, o = ref["lowq_all_0_gt_inds"], ref["lowq_one_0_gt_inds"]
    # an exact tie on gt 2's maximum: both mirrored proposals with gt_max_assign_all, the lower one alone without
    assert (a[5 + 100], a[5 + 250]) == (3, 3) and (o[5 + 100], o[5 + 250]) == (3, -1) and not np.array_equal(a, o)
    assert (ref["lowq_all_0_gt_inds"] == -1).any()                                  # candidates in neither interval
    assert (ref["many_gt_0_gt_inds"] > 0).sum() > ref["many_gt_0_pos"].size == 128    # more positives than num_expected_pos
    assert ref["rcnn_1_gt_inds"].size == 37 + 9 and ref["rcnn_2_pos"].size == 0 and ref["rcnn_2_neg"].size == 512
    assert ref["ub_0_neg"].size == 3 * ref["ub_0_pos"].size                          # neg_pos_ub binds


@pytest.mark.parametrize("name", list(rc.CASES))
def test_numpy_chain_reproduces_the_reference(ref, ulps, name):
    case = rc.CASES[name]
    gts = rc.inputs(name)[2]
    for b in range(len(case["images"])):
        pre = "%s_%d_" % (name, b)
        gi = rc.assign_front_np(name, b)[0]
        assert np.array_equal(gi, ref[pre + "gt_inds"]), (name, b)
        rois, labels, lw, bt, bw, pg, pos, neg, is_gt = rc.chain_np(name, b, rc.fixture_keys(ref, name, b))
        assert np.array_equal(pos, ref[pre + "pos"]) and np.array_equal(neg, ref[pre + "neg"]), (name, b)
        kp, k = pos.size, pos.size + neg.size
        assert np.array_equal(labels[:k], ref[pre + "labels"]) and np.array_equal(tc.bits(lw[:k]), tc.bits(ref[pre + "lw"]))
        assert (labels[k:] == rc.NUM_CLASSES).all() and not lw[k:].any() and not rois[k:, 1:].any() and (pg[kp:] == -1).all()
        want = ref[pre + "bt_pos"]
        if case["decoded"]:
            assert np.array_equal(tc.bits(bt[:kp]), tc.bits(want))
        else:
            assert np.array_equal(tc.bits(bt[:kp, :2]), tc.bits(want[:, :2]))
            exact, kinds, err = tc.encode_check(bt[:kp], rois[:kp, 1:], gts[b][gi[pos] - 1], case["means"], case["stds"])
            assert exact and kinds and err <= 2 * ulps[0], (name, b, err)
            exact, kinds, err = tc.encode_check(want, rois[:kp, 1:], gts[b][gi[pos] - 1], case["means"], case["stds"])
            assert exact and kinds and err <= ulps[0], (name, b, err)
        assert not tc.bits(bt[kp:]).any() and int(is_gt.sum()) == int((pos < rc.assign_front_np(name, b)[3]).sum())


@pytest.mark.parametrize("name", rc.REFINE_CASES)
@pytest.mark.parametrize("agnostic", [False, True])
def test_numpy_refine_reproduces_the_reference(ref, ulps, name, agnostic):
    case = rc.CASES[name]
    num = case["num"]
    r_lab, r_pred = rc.refine_inputs(name, agnostic)
    for b in range(len(case["images"])):
        rois, _, _, _, _, _, pos, neg, is_gt = rc.chain_np(name, b, rc.fixture_keys(ref, name, b))
        k = pos.size + neg.size
        s = slice(b * num, (b + 1) * num)
        mine = rc.refine_np(rois, r_lab[s], r_pred[s], is_gt, k, case["means"], case["stds"], rc.IMG, agnostic)
        want = ref["refine_%s_%d_%d" % (name, int(agnostic), b)]
        assert mine.shape == want.shape == (k - int(is_gt.sum()), 4)
        keep = is_gt[:k] == 0
        d = r_pred[s][:k] if agnostic else np.stack([r_pred[s][np.arange(k), 4 * r_lab[s][:k] + j] for j in range(4)], 1)
        for out, allowed in ((mine, 2 * ulps[1]), (want, ulps[1])):
            ok, kinds, err = tc.decode_check(out, rois[:k, 1:][keep], np.ascontiguousarray(d[keep]), case["means"], case["stds"], rc.IMG,
                                             tc.WH_RATIO_CLIP, True, False, 32)
            assert ok and kinds and err <= allowed, (name, agnostic, b, err)


def _parts():
    from iif_amd.mmdet_assigner import MaxIoUAssigner
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler
    return MaxIoUAssigner(0.5, 0.5, 0.5, match_low_quality=False), RandomSampler(64, 0.25), DeltaXYWHBBoxCoder()


def test_wrappers_refuse_before_touching_the_device():
    from iif_amd import _lib
    from iif_amd import mmdet_roi_stage as rs
    asg, smp, coder = _parts()
    props, gts, labs = torch.zeros(2, 10, 5), [torch.zeros(3, 4)] * 2, [torch.zeros(3, dtype=torch.int64)] * 2
    call = lambda p=props, c=None, g=gts, l=labs, s=smp, **kw: rs.roi_stage_targets_padded(p, c, g, l, asg, s, coder, 80, **kw)   # noqa: E731
    with pytest.raises(_lib.IIFNativeError):
        call()                                                                       # CPU tensors
    with pytest.raises(_lib.IIFNativeError):
        call(p=[torch.zeros(4, 4), torch.zeros(2, 4)])
    with pytest.raises(NotImplementedError):
        call(gt_bboxes_ignore=[None, None])
    with pytest.raises(ValueError):
        call(g=gts[:1])                                                              # mismatched list lengths
    with pytest.raises(ValueError):
        call(p=[torch.zeros(4, 4)])
    with pytest.raises(ValueError):
        call(l=labs[:1])
    z = torch.zeros
    for bad in (dict(p=z(17, 10, 4), g=gts[:1] * 17, l=labs[:1] * 17),             # shapes over the limits, still on the CPU:
                dict(p=z(2, 4097, 4)),                                               # the limits are checked first
                dict(p=[z(4097, 4), z(2, 4)]),
                dict(g=[z(1025, 4)] * 2, l=[z(1025, dtype=torch.int64)] * 2),
                dict(s=type(smp)(1025, 0.25))):
        with pytest.raises(ValueError, match="per-image chain"):
            call(**bad)
    with pytest.raises(ValueError, match="keys"):
        call(keys=torch.zeros(2, 13, dtype=torch.int64))                            # wrong key dtype
    with pytest.raises(ValueError, match="keys"):
        call(keys=torch.zeros(2, 10, dtype=torch.int32))                            # wrong key shape: 3 gts in front
    with pytest.raises(ValueError):
        call(c=torch.zeros(3, dtype=torch.int64))
    # refine
    rois, lab, pred = torch.zeros(8, 5), torch.zeros(8, dtype=torch.int64), torch.zeros(8, 20)
    is_gt, counts = torch.zeros(8, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int64)
    shapes = [(100, 100)] * 2
    with pytest.raises(_lib.IIFNativeError):
        rs.refine_bboxes_padded(rois, lab, pred, is_gt, counts, shapes, coder)
    with pytest.raises(ValueError):
        rs.refine_bboxes_padded(rois, lab, pred, is_gt, counts, shapes * 9, coder)
    with pytest.raises(ValueError):
        rs.refine_bboxes_padded(rois[:7], lab, pred, is_gt, counts, shapes, coder)
    with pytest.raises(ValueError):
        rs.refine_bboxes_padded(rois, lab, pred, is_gt, counts, shapes, coder, reg_class_agnostic=True)
    with pytest.raises(ValueError):
        rs.refine_bboxes_padded(rois, lab, pred, is_gt, counts[:1], shapes, coder)
    with pytest.raises(_lib.IIFNativeError):
        rs.refine_bboxes(rois, lab, pred, [is_gt[:2]] * 2, [dict(img_shape=(100, 100, 3))] * 2, coder)


def test_library_exports_both_entries_and_checks_their_limits():
    import ctypes
    from iif_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "iif_roi_stage_targets") and hasattr(L, "iif_refine_bboxes")
    assert "iif_roi_stage_targets" in _lib.SIGNATURES and "iif_refine_bboxes" in _lib.SIGNATURES
    img = (_lib.RoiImage * 1)()
    f4 = (ctypes.c_float * 4)(1, 1, 1, 1)
    buf = (ctypes.c_int64 * 64)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    tail = [f4, f4] + [a] * 11 + [None]

    def stage(B=1, P=0, num=0, nep=0):
        return L.iif_roi_stage_targets(img, B, None, 4, 0, P, None, None, 0, 0.5, 0.0, 0.5, 0.5, 1, 0, 1, nep, num, -1.0, 80, -1.0, 0, *tail)
    # the argument checks return before anything is launched
    assert stage(B=0) == -1 and stage(B=17) == -1 and stage(P=4097) == -1 and stage(num=1025) == -1 and stage(num=4, nep=5) == -1
    assert stage(P=8) == -1                                                          # proposals without a pointer
    img[0].G = 1025
    assert stage() == -1
    assert L.iif_refine_bboxes(a, 5, a, a, 4, 1, 1, a, a, 17, 4, f4, f4, f4, 4.0, 0, 32.0, 1, a, a, None) == -1
    assert L.iif_refine_bboxes(a, 5, a, a, 4, 1, 1, a, a, 1, 1025, f4, f4, f4, 4.0, 0, 32.0, 1, a, a, None) == -1
    assert L.iif_refine_bboxes(a, 5, a, a, 16, 5, 0, a, a, 1, 4, f4, f4, f4, 4.0, 0, 32.0, 1, a, a, None) == -1   # pitch < 4 C
