"""Box assignment on the MI355X: iif_amd.mmdet_assigner against the reference's own runs (tests/golden/g25_assign.npz) and the
numpy restatement that the fixture's generator and tests/test_assign_host.py tie to the reference bit for bit.

EXACT equality everywhere, no tolerance: every arithmetic step of the overlaps is a single IEEE float32 operation, and step 4
of the assignment compares overlaps for equality.  ``max_overlaps`` and ``bbox_overlaps`` are compared as bit patterns."""
import numpy as np
import pytest
import torch

from . import assign_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = "g25_assign"


def T(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def assigner(run, **kw):
    from iif_amd.mmdet_assigner import MaxIoUAssigner
    pos, neg, min_pos, assign_all, ign_thr, ign_wrt, mlq = run
    return MaxIoUAssigner(pos, neg, min_pos_iou=min_pos, gt_max_assign_all=assign_all, ignore_iof_thr=ign_thr,
                          ignore_wrt_candidates=ign_wrt, match_low_quality=mlq, **kw)


@pytest.fixture(scope="module")
def ref(golden):
    g = golden(FIXTURE)
    ac.check_generator(g)
    return g


@pytest.fixture(scope="module")
def dev_in():
    """Device copies of a case's inputs, made on first use and never written: (bboxes, gts, ignore or None, labels)."""
    cache = {}

    def get(name):
        if name not in cache:
            b, g, ign, lab = ac.inputs(name)
            cache[name] = (T(b), T(g), T(ign), T(lab))
        return cache[name]
    return get


def stored_mo(g, name, r):
    key = "%s_%d" % (name, r)
    if key + "_mo_as" in g.files:
        key = "%s_%d" % (name, int(g[key + "_mo_as"]))
    return g[key + "_mo"]


def same(res, other):
    return (torch.equal(res.gt_inds, other.gt_inds) and torch.equal(res.max_overlaps.view(torch.int32), other.max_overlaps.view(torch.int32))
            and (res.labels is None) == (other.labels is None) and (res.labels is None or torch.equal(res.labels, other.labels)))


@pytest.mark.parametrize("name", ac.SMALL)
def test_assignment_equals_the_reference(ref, dev_in, name):
    """Every run of every small case: gt_inds, labels and the bits of max_overlaps equal the reference's; without gt_labels
    the result's labels are None and the rest does not change."""
    N, G = ac.CASES[name][:2]
    b, g, ign, lab = dev_in(name)
    if name == "rcnn":                                     # pitch-5 candidates: proposals with a score column, read in place
        b = torch.cat([b, torch.full((N, 1), 0.25, device=DEV)], dim=1)
    for r, run in enumerate(ac.CASES[name][4]):
        key = "%s_%d" % (name, r)
        res = assigner(run).assign(b, g, gt_bboxes_ignore=ign, gt_labels=lab)
        assert res.num_gts == G and res.num_preds == N
        assert res.gt_inds.dtype == torch.int64 and res.labels.dtype == torch.int64 and res.max_overlaps.dtype == torch.float32
        gi, lb, mo = res.gt_inds.cpu().numpy(), res.labels.cpu().numpy(), res.max_overlaps.cpu().numpy()
        want = stored_mo(ref, name, r)
        bad = np.nonzero(ac.bits(mo) != ac.bits(want))[0]
        assert bad.size == 0, (key, bad[:8], mo[bad[:8]], want[bad[:8]])
        bad = np.nonzero(gi != ref[key + "_gt_inds"])[0]
        assert bad.size == 0, (key, bad[:8], gi[bad[:8]], ref[key + "_gt_inds"][bad[:8]])
        assert np.array_equal(lb, ref[key + "_labels"]), key
        nolab = assigner(run).assign(b, g, gt_bboxes_ignore=ign)
        assert nolab.labels is None
        assert torch.equal(nolab.gt_inds, res.gt_inds) and torch.equal(nolab.max_overlaps, res.max_overlaps)


def test_full_case_equals_the_reference_within_its_memory_bound(ref, dev_in):
    """The crowded RPN shape, 268 569 candidates x 300 gts.  gt_inds and labels equal the reference's everywhere,
    max_overlaps at the kept candidates and in the exact sum of its bit patterns.  Memory: the call may allocate the three
    outputs (8 + 4 + 8 bytes per candidate) and the O(G) workspace, so the peak rises by less than 32 N + 64 G + 1 MiB -
    the overlap matrix alone would be 322 MB."""
    N, G = ac.CASES["full"][:2]
    b, g, ign, lab = dev_in("full")
    asg = assigner(ac.CASES["full"][4][0])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    res = asg.assign(b, g, gt_bboxes_ignore=ign, gt_labels=lab)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("full case: peak memory rose by %d bytes (bound %d)" % (rise, 32 * N + 64 * G + (1 << 20)))
    assert rise < 32 * N + 64 * G + (1 << 20), rise
    gi, lb, mo = res.gt_inds.cpu().numpy(), res.labels.cpu().numpy(), res.max_overlaps.cpu().numpy()
    keep = ac.full_keep(N)
    assert np.array_equal(ac.bits(mo[keep]), ac.bits(ref["full_0_mo_kept"]))
    assert ac.bit_sum(mo) == ref["full_0_mo_bitsum"]
    bad = np.nonzero(gi != ref["full_0_gt_inds"])[0]
    assert bad.size == 0, (bad[:8], gi[bad[:8]], ref["full_0_gt_inds"][bad[:8]])
    assert np.array_equal(lb, ref["full_0_labels"])


@pytest.mark.parametrize("name", ac.OVERLAP_CASES)
def test_bbox_overlaps_equals_the_reference_bit_for_bit(ref, dev_in, name):
    """All three modes, pairwise (gts x candidates) and aligned, pitch 4 and pitch 5, through the function and through
    BboxOverlaps2D: the whole output against the numpy restatement, the kept part and the bit sum against the fixture."""
    from iif_amd.mmdet_assigner import BboxOverlaps2D, bbox_overlaps
    b_np, g_np, _, _ = ac.inputs(name)
    p_np, q_np = ac.aligned_pair(name)
    b, g, _, _ = dev_in(name)
    p, q = T(p_np), T(q_np)

    def five(t):
        return torch.cat([t, torch.full((t.size(0), 1), 0.25, device=DEV)], dim=1)
    calc = BboxOverlaps2D()
    for mode in ac.MODES:
        key = "ov_%s_%s" % (name, mode)
        want_pw, want_al = ac.overlaps_np(g_np, b_np, mode), ac.overlaps_np(p_np, q_np, mode, True)
        for pw in (bbox_overlaps(g, b, mode), calc(g, five(b), mode), calc(five(g), five(b)[:, :4], mode)):
            assert pw.shape == want_pw.shape and pw.dtype == torch.float32
            out = pw.cpu().numpy()
            bad = np.argwhere(ac.bits(out) != ac.bits(want_pw))
            assert bad.size == 0, (key, bad[:4], [(out[i, j], want_pw[i, j]) for i, j in bad[:4]])
            assert np.array_equal(ac.bits(out.reshape(-1)[ac.overlap_keep(out.size)]), ac.bits(ref[key + "_pair"]))
            assert ac.bit_sum(out) == ref[key + "_pair_bitsum"]
        for al in (bbox_overlaps(p, q, mode, is_aligned=True), calc(five(p), q, mode, True), calc(p, five(q), mode, True)):
            assert al.shape == want_al.shape
            out = al.cpu().numpy()
            assert np.array_equal(ac.bits(out), ac.bits(want_al)) and np.array_equal(ac.bits(out), ac.bits(ref[key + "_aligned"])), key
    # another eps goes into both clamps
    out = bbox_overlaps(g, b, "giou", eps=0.5).cpu().numpy()
    assert np.array_equal(ac.bits(out), ac.bits(ac.overlaps_np(g_np, b_np, "giou", eps=0.5)))


def test_empty_inputs_follow_the_reference(dev_in):
    """G = 0: everything background (gt_inds 0, max_overlaps 0, labels -1).  N = 0: empty results.  Both: empty.  And the
    calculator's empty shapes (0, n), (m, 0), (0,)."""
    from iif_amd.mmdet_assigner import BboxOverlaps2D, bbox_overlaps
    b, g, _, lab = dev_in("one")
    e4 = torch.zeros((0, 4), device=DEV)
    el = torch.zeros((0,), dtype=torch.int64, device=DEV)
    for run in (ac.RPN, ac._with(ac.RCNN, mlq=False)):
        asg = assigner(run)
        res = asg.assign(b, e4, gt_labels=el)
        assert res.num_gts == 0 and res.gt_inds.dtype == torch.int64 and res.max_overlaps.dtype == torch.float32
        assert res.gt_inds.tolist() == [0] * 67 and res.max_overlaps.tolist() == [0.0] * 67 and res.labels.tolist() == [-1] * 67
        assert asg.assign(b, e4).labels is None
        res = asg.assign(e4, g, gt_labels=lab)
        assert res.num_gts == 1 and res.gt_inds.shape == res.max_overlaps.shape == res.labels.shape == (0,)
        assert res.gt_inds.dtype == torch.int64 and res.labels.dtype == torch.int64
        res = asg.assign(e4, e4, gt_labels=el)
        assert res.num_gts == 0 and res.gt_inds.shape == res.max_overlaps.shape == res.labels.shape == (0,)
        assert asg.assign(e4, e4).labels is None
    assert bbox_overlaps(e4, b).shape == (0, 67) and bbox_overlaps(b, e4).shape == (67, 0) and bbox_overlaps(e4, e4).shape == (0, 0)
    assert bbox_overlaps(e4, e4, is_aligned=True).shape == (0,) and BboxOverlaps2D()(e4, b, "giou").shape == (0, 67)
    # an empty ignore set and a threshold that is off are both "no ignore boxes"
    _, _, ign, _ = dev_in("ignore")
    bi, gi_, _, li = dev_in("rpn")
    base = assigner(ac.RPN).assign(bi, gi_, gt_labels=li)
    assert same(assigner(ac._with(ac.RPN, ign_thr=0.5)).assign(bi, gi_, gt_bboxes_ignore=e4, gt_labels=li), base)
    assert same(assigner(ac.RPN).assign(bi, gi_, gt_bboxes_ignore=ign, gt_labels=li), base)


def test_views_and_unaligned_bases_give_identical_results(dev_in):
    """Candidates as a [:, :4] view of an [N, 5] tensor, as a tensor one element past a 16-byte boundary (the scalar-load
    path), transposed storage (copied by the wrapper), and gts with a pitch of 5: the same tensors as the plain call."""
    from iif_amd.mmdet_assigner import bbox_overlaps
    for name, r in (("rpn", 0), ("ignore", 1), ("rcnn", 1)):
        b, g, ign, lab = dev_in(name)
        N = b.size(0)
        asg = assigner(ac.CASES[name][4][r])
        base = asg.assign(b, g, gt_bboxes_ignore=ign, gt_labels=lab)
        five = torch.cat([b, torch.rand((N, 1), device=DEV)], dim=1)
        flat = torch.zeros(4 * N + 1, device=DEV)
        flat[1:] = b.reshape(-1)
        off = flat[1:].view(N, 4)
        assert off.data_ptr() % 16 == 4 and five[:, :4].stride() == (5, 1)
        g5 = torch.cat([g, torch.rand((g.size(0), 1), device=DEV)], dim=1)
        i5 = None if ign is None else torch.cat([ign, torch.rand((ign.size(0), 1), device=DEV)], dim=1)
        for cand, gts, ig in ((five[:, :4], g, ign), (five, g5, i5), (off, g5[:, :4], ign), (b.t().contiguous().t(), g, ign)):
            assert same(asg.assign(cand, gts, gt_bboxes_ignore=ig, gt_labels=lab), base), name
        if name == "rcnn":
            want = bbox_overlaps(g, b, "giou")
            for cand in (five[:, :4], off, b.t().contiguous().t()):
                assert torch.equal(bbox_overlaps(g5[:, :4], cand, "giou").view(torch.int32), want.view(torch.int32))


def test_calls_repeat_and_leave_no_state(dev_in):
    """Two calls give identical tensors; so does a call made right after one with a different, larger G (a workspace that
    leaked between calls would show here), and after one with other options."""
    b, g, ign, lab = dev_in("rpn")
    bm, gm, _, lm = dev_in("many")
    for r in (0, 1):
        asg = assigner(ac.CASES["rpn"][4][r])
        first = asg.assign(b, g, gt_labels=lab)
        assert same(asg.assign(b, g, gt_labels=lab), first)
        assigner(ac.CASES["many"][4][r]).assign(bm, gm, gt_labels=lm)
        assert same(asg.assign(b, g, gt_labels=lab), first)
        assigner(ac._with(ac.RCNN, mlq=False)).assign(bm[:300], gm[:100])
        assert same(asg.assign(b, g, gt_labels=lab), first)


def test_assign_never_synchronises_the_host(dev_in):
    """assign under torch's sync debug mode ('error'): with and without labels, ignore boxes in both directions, low-quality
    matching on and off, the tuple threshold, no gts and no candidates."""
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    b, g, ign, lab = dev_in("ignore")
    e4 = torch.zeros((0, 4), device=DEV)
    asgs = [assigner(run) for run in ac.CASES["ignore"][4] + ac.CASES["rpn"][4] + ac.CASES["tuple"][4]]
    asgs[0].assign(b, g, gt_bboxes_ignore=ign, gt_labels=lab)                 # the library is loaded before the mode is on
    torch.cuda.synchronize()
    out = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for a in asgs:
            out.append(a.assign(b, g, gt_bboxes_ignore=ign, gt_labels=lab))
            out.append(a.assign(b, g, gt_bboxes_ignore=ign))
            out.append(a.assign(b, g, gt_labels=lab))
            out.append(a.assign(b, e4, gt_labels=lab[:0]))
            out.append(a.assign(e4, g, gt_bboxes_ignore=ign))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert len(out) == 5 * len(asgs) and all(o.gt_inds.min().item() >= -1 for o in out if o.num_preds)


def test_gpu_assign_thr_has_no_effect_and_add_gt_concatenates(dev_in):
    b, g, _, lab = dev_in("rcnn")
    base = assigner(ac.RCNN).assign(b, g, gt_labels=lab)
    res = assigner(ac.RCNN, gpu_assign_thr=1).assign(b, g, gt_labels=lab)
    assert same(res, base) and res.gt_inds.is_cuda and res.max_overlaps.is_cuda and res.labels.is_cuda
    res.add_gt_(lab)
    G = g.size(0)
    assert res.num_preds == b.size(0) + G and res.gt_inds[:G].tolist() == list(range(1, G + 1))
    assert torch.equal(res.labels[:G], lab) and res.max_overlaps[:G].tolist() == [1.0] * G
    assert torch.equal(res.gt_inds[G:], base.gt_inds)
