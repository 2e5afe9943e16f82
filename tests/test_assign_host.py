"""Box assignment (mmdet MaxIoUAssigner, bbox_overlaps), the part that needs no device: the fixture
tests/golden/g25_assign.npz against the input generators and the numpy restatements of tests/assign_cases.py, the edge
elements the cases are there for, the Python surface's constructors and errors, and the two C entry points in header, library
and ctypes table with their argument checks."""
import os
import re

import numpy as np
import pytest
import torch

from . import assign_cases as ac
from iif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_bbox_overlaps", "iif_max_iou_assign")
FIXTURE = "g25_assign"

_runs = {}


def run_np(name, r):
    """assign_np of one run, computed once per session."""
    if (name, r) not in _runs:
        b, g, ign, lab = ac.inputs(name)
        _runs[(name, r)] = ac.assign_np(b, g, ign, lab, ac.CASES[name][4][r])
    return _runs[(name, r)]


def stored_mo(g, name, r):
    key = "%s_%d" % (name, r)
    if key + "_mo_as" in g.files:
        key = "%s_%d" % (name, int(g[key + "_mo_as"]))
    return g[key + "_mo"]


def test_fixture_inputs_regenerate(golden):
    ac.check_generator(golden(FIXTURE))


@pytest.mark.parametrize("name", ac.SMALL)
def test_restatement_reproduces_the_fixture(golden, name):
    g = golden(FIXTURE)
    N, G = ac.CASES[name][:2]
    for r in range(len(ac.CASES[name][4])):
        gi, mo, lb, _, _ = run_np(name, r)
        key = "%s_%d" % (name, r)
        assert gi.shape == mo.shape == lb.shape == (N,)
        assert np.array_equal(gi, g[key + "_gt_inds"]) and np.array_equal(lb, g[key + "_labels"]), key
        assert np.array_equal(ac.bits(mo), ac.bits(stored_mo(g, name, r))), key


def test_restatement_reproduces_the_full_case(golden):
    g = golden(FIXTURE)
    N = ac.CASES["full"][0]
    gi, mo, lb, _, _ = run_np("full", 0)
    assert np.array_equal(gi, g["full_0_gt_inds"]) and np.array_equal(lb, g["full_0_labels"])
    assert np.array_equal(ac.bits(mo[ac.full_keep(N)]), ac.bits(g["full_0_mo_kept"]))
    assert ac.bit_sum(mo) == g["full_0_mo_bitsum"]
    assert (gi > 0).sum() > 1000 and (gi == 0).sum() > 1000 and (gi == -1).sum() > 1000


@pytest.mark.parametrize("name", ac.OVERLAP_CASES)
def test_overlaps_restatement_reproduces_the_fixture(golden, name):
    g = golden(FIXTURE)
    b, gts, _, _ = ac.inputs(name)
    p, q = ac.aligned_pair(name)
    for mode in ac.MODES:
        key = "ov_%s_%s" % (name, mode)
        pw = ac.overlaps_np(gts, b, mode)
        assert pw.shape == (gts.shape[0], b.shape[0])
        assert np.array_equal(ac.bits(pw.reshape(-1)[ac.overlap_keep(pw.size)]), ac.bits(g[key + "_pair"]))
        assert ac.bit_sum(pw) == g[key + "_pair_bitsum"]
        assert np.array_equal(ac.bits(ac.overlaps_np(p, q, mode, True)), ac.bits(g[key + "_aligned"]))


def test_cases_hold_the_edge_elements(golden):
    """What each case of the table is there for is really in its inputs and in the reference's stored result."""
    g = golden(FIXTURE)
    f = np.float32
    # tiny: the min_pos_iou = 0 quirk
    assert g["tiny_0_gt_inds"].tolist() == [2, 2, 2]
    # rcnn: an IoU of exactly 0.5 counts as positive at pos_iou_thr 0.5; a candidate equal to three identical gts takes the
    # highest of them with low-quality matching and the lowest without
    b, gts, _, lab = ac.inputs("rcnn")
    assert ac.overlaps_np(gts[0:1], b[5:6])[0, 0] == f(0.5)
    assert np.array_equal(gts[4], gts[5]) and np.array_equal(gts[4], gts[20]) and np.array_equal(b[11], gts[4])
    mo = g["rcnn_0_mo"]
    assert mo[10] == 1.0 and mo[11] == 1.0
    assert g["rcnn_0_gt_inds"][11] == 21 and g["rcnn_1_gt_inds"][11] == 5
    assert g["rcnn_0_gt_inds"][5] == 1 or mo[5] > f(0.5)
    assert g["rcnn_0_labels"][11] == lab[20] and g["rcnn_1_labels"][11] == lab[4]
    # rpn: best candidates at index 0 and in the last, partial block; two candidates in different blocks tie for gt 12
    b, gts, _, _ = ac.inputs("rpn")
    _, _, _, gmax, garg = run_np("rpn", 0)
    assert garg[9] == 0 and garg[7] == b.shape[0] - 1 and b.shape[0] % 256 != 0
    r12 = ac.overlaps_np(gts[12:13], b)[0]
    assert np.nonzero(r12 == gmax[12])[0].tolist() == [300, 3000] and f(0.3) <= gmax[12] < f(0.7)
    assert g["rpn_0_gt_inds"][300] == 13 and g["rpn_0_gt_inds"][3000] == 13                 # gt_max_assign_all
    assert g["rpn_1_gt_inds"][300] == 13 and g["rpn_1_gt_inds"][3000] != 13                 # only the argmax, the lower one
    # ignore: candidates are ignored in both directions; everything that overlaps gt 2 is ignored (wrt candidates)
    b, gts, ign, _ = ac.inputs("ignore")
    for r in (0, 1):
        run = ac.CASES["ignore"][4][r]
        ig = ac.ignored_np(b, ign, run[4], run[5])
        assert 0 < ig.sum() < b.shape[0]
        assert (stored_mo(g, "ignore", r)[ig] == -1).all() and (g["ignore_%d_gt_inds" % r][ig] == -1).all()
    ig = ac.ignored_np(b, ign, 0.5, True)
    r2 = ac.overlaps_np(gts[2:3], b)[0]
    assert (r2 > 0).sum() > 0 and ig[r2 > 0].all()
    assert run_np("ignore", 0)[3][2] == 0.0 and not (g["ignore_0_gt_inds"] == 3).any()
    assert ac.ignored_np(b, ign, 0.5, False)[[300, 3000]].all()
    # tuple: overlaps below neg_iou_thr[0] stay -1
    mo, gi = g["tuple_0_mo"], g["tuple_0_gt_inds"]
    assert ((mo < f(0.1)) & (gi == -1)).any() and ((mo >= f(0.1)) & (mo < f(0.4)) & (gi == 0)).any()
    # many: more gts than one LDS chunk, argmaxima beyond it
    assert ac.CASES["many"][1] > 512 and (g["many_0_gt_inds"] > 512).any()
    # degenerate: zero-area and inverted boxes on both sides, a union clamped at eps, every overlap finite
    b, gts, _, _ = ac.inputs("degenerate")
    wb, hb = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    assert (wb == 0).any() and (hb == 0).any() and (wb < 0).any() and ((wb < 0) & (hb < 0)).any()
    assert gts[1, 2] == gts[1, 0] and gts[2, 2] < gts[2, 0] and np.array_equal(b[6], gts[3])
    assert ac.overlaps_np(gts[3:4], b[6:7])[0, 0] == 0.0                                       # 0 / eps
    assert g["degenerate_0_mo"][12] == 1.0


def test_surface_imports_without_a_device_and_mirrors_the_constructors():
    from iif_amd import mmdet_assigner as M
    a = M.MaxIoUAssigner(0.7, 0.3)
    assert (a.pos_iou_thr, a.neg_iou_thr, a.min_pos_iou, a.gt_max_assign_all, a.ignore_iof_thr, a.ignore_wrt_candidates,
            a.match_low_quality, a.gpu_assign_thr) == (0.7, 0.3, 0.0, True, -1, True, True, -1)
    assert isinstance(a.iou_calculator, M.BboxOverlaps2D)
    a = M.MaxIoUAssigner(0.5, (0.1, 0.4), 0.5, False, 0.5, False, False, 100, dict(type="BboxOverlaps2D"))
    assert (a.neg_iou_thr, a.min_pos_iou, a.gt_max_assign_all, a.ignore_iof_thr, a.ignore_wrt_candidates, a.match_low_quality,
            a.gpu_assign_thr) == ((0.1, 0.4), 0.5, False, 0.5, False, False, 100)
    assert M.MaxIoUAssigner(0.5, 0.5, iou_calculator=M.BboxOverlaps2D()).iou_calculator.dtype is None
    c = M.BboxOverlaps2D()
    assert (c.scale, c.dtype) == (1.0, None) and repr(c) == "BboxOverlaps2D(scale=1.0, dtype=None)"
    assert callable(M.bbox_overlaps) and callable(M.MaxIoUAssigner.assign)
    assert M.register_into_mmdet() is False                   # no mmdet here: no error either


def test_assign_result_mirrors_the_reference():
    from iif_amd.mmdet_assigner import AssignResult
    r = AssignResult(2, torch.tensor([0, 2, -1]), torch.tensor([0.1, 0.8, -1.0]), labels=torch.tensor([-1, 7, -1]))
    assert (r.num_gts, r.num_preds) == (2, 3) and set(r.info) == {"num_gts", "num_preds", "gt_inds", "max_overlaps", "labels"}
    r.set_extra_property("x", 1)
    assert r.get_extra_property("x") == 1 and r.get_extra_property("y") is None and "x" in r.info
    r.add_gt_(torch.tensor([5, 7]))
    assert r.gt_inds.tolist() == [1, 2, 0, 2, -1] and r.labels.tolist() == [5, 7, -1, 7, -1]
    assert r.max_overlaps.tolist()[:2] == [1.0, 1.0] and r.num_preds == 5 and r.gt_inds.dtype == torch.long
    r = AssignResult(1, torch.tensor([0]), torch.tensor([0.0]))
    r.add_gt_(torch.tensor([3]))
    assert r.labels is None and r.gt_inds.tolist() == [1, 0]


def test_error_conventions():
    from iif_amd import mmdet_assigner as M
    b4, b5 = torch.zeros(3, 4), torch.zeros(3, 5)
    with pytest.raises(NotImplementedError):
        M.BboxOverlaps2D(dtype="fp16")(b4, b4)
    with pytest.raises(NotImplementedError):
        M.bbox_overlaps(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))             # batch dimensions
    with pytest.raises(NotImplementedError):
        M.bbox_overlaps(b4.half(), b4.half())
    with pytest.raises(NotImplementedError):
        M.bbox_overlaps(b4.double(), b4)
    with pytest.raises(AssertionError):
        M.bbox_overlaps(b4, b4, mode="diou")
    with pytest.raises(AssertionError):
        M.bbox_overlaps(b4, torch.zeros(2, 4), is_aligned=True)
    with pytest.raises(AssertionError):
        M.BboxOverlaps2D()(torch.zeros(3, 6), b4)
    with pytest.raises(RuntimeError):
        M.bbox_overlaps(b4.clone().requires_grad_(True), b4, mode="giou")       # no autograd
    with pytest.raises(NotImplementedError):
        M.MaxIoUAssigner(0.5, 0.5, iou_calculator=dict(type="BboxOverlaps3D"))
    with pytest.raises(NotImplementedError):
        M.MaxIoUAssigner(0.5, 0.5, iou_calculator=dict(type="BboxOverlaps2D", dtype="fp16"))
    with pytest.raises(NotImplementedError):
        M.MaxIoUAssigner(0.5, 0.5, iou_calculator=lambda a, b, mode="iou": None)
    a = M.MaxIoUAssigner(0.5, 0.5)
    with pytest.raises(NotImplementedError):
        a.assign_wrt_overlaps(torch.zeros(2, 3))
    with pytest.raises(NotImplementedError):
        a.assign(b4.double(), b4)
    with pytest.raises(NotImplementedError):
        a.assign(torch.zeros(2, 3, 4), b4)
    # CPU tensors are rejected, not emulated - the empty shapes included
    for call in (lambda: M.bbox_overlaps(b4, b5), lambda: M.BboxOverlaps2D()(b5, b4, "iof"), lambda: a.assign(b5, b4),
                 lambda: a.assign(b4, torch.zeros(0, 4)), lambda: M.bbox_overlaps(torch.zeros(0, 4), b4)):
        with pytest.raises(_lib.IIFNativeError):
            call()


def test_entry_points_in_header_library_and_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code)
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name])


def test_entry_points_check_arguments_before_launching():
    """Bad arguments return -1 before anything touches the device."""
    L = _lib.lib()
    one = 64            # a non-null, aligned stand-in: the checks below fail before any pointer is used

    def ov(**kw):
        return L.iif_bbox_overlaps(kw.get("b1", one), kw.get("ld1", 4), kw.get("m", 3), kw.get("b2", one), kw.get("ld2", 5),
                                   kw.get("n", 3), kw.get("mode", 0), kw.get("aligned", 0), 1e-6, kw.get("out", one), None)
    assert ov(out=None) == -1 and ov(b1=None) == -1 and ov(b2=None) == -1
    assert ov(m=-1) == -1 and ov(n=-1) == -1 and ov(m=1 << 31) == -1
    assert ov(ld1=3) == -1 and ov(ld2=3) == -1                  # a pitch below four elements
    assert ov(mode=3) == -1 and ov(mode=-1) == -1
    assert ov(aligned=1, m=2) == -1                             # aligned pairs need m == n
    assert ov(b1=66) == -1 and ov(out=66) == -1                 # float32 on a 2-byte boundary
    assert ov(m=0, b1=None, out=None) == 0 and ov(n=0) == 0     # nothing to do

    def asg(**kw):
        return L.iif_max_iou_assign(kw.get("b", one), kw.get("ldb", 4), kw.get("N", 8), kw.get("g", one), kw.get("ldg", 4),
                                    kw.get("G", 2), kw.get("ig", None), kw.get("ldi", 4), kw.get("I", 0), kw.get("pos", 0.7),
                                    kw.get("neg_lo", 0.0), kw.get("neg_hi", 0.3), 0.3, kw.get("ign_thr", -1.0), 1, 1,
                                    kw.get("mlq", 1), kw.get("gt_labels", None), kw.get("gt_inds", one), kw.get("mo", one),
                                    kw.get("labels", None), kw.get("ws", one), kw.get("ws_bytes", 24), None)
    assert asg(gt_inds=None) == -1 and asg(mo=None) == -1       # null outputs
    assert asg(N=-1) == -1 and asg(G=-1) == -1 and asg(I=-1) == -1 and asg(N=1 << 31) == -1
    assert asg(ldb=3) == -1 and asg(ldg=3) == -1 and asg(ig=one, I=1, ldi=3) == -1
    assert asg(neg_lo=0.4, neg_hi=0.3) == -1 and asg(neg_lo=float("nan")) == -1 and asg(pos=float("nan")) == -1
    assert asg(b=None) == -1 and asg(g=None) == -1
    assert asg(labels=one) == -1                                # labels wanted, no gt_labels to take them from
    assert asg(ws=None) == -1 and asg(ws_bytes=16) == -1        # low-quality matching needs 8 (G + 1) bytes
    assert asg(ws=68) == -1 and asg(b=66) == -1 and asg(gt_inds=68) == -1
    assert asg(N=0, b=None) == 0                                # nothing to do
