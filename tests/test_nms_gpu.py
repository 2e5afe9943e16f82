"""The native NMS / RPN proposals (csrc/nms.hip, iif_amd/mmdet_nms.py) on the MI355X against tests/golden/g28_nms.npz, which the
reference's RPNHead produced on the CPU (tests/golden/make_golden_nms.py).

  * plain and batched NMS: keep, count, padding and dets EXACTLY.  The overlap test is single float32 operations in mmcv's
    order and the rank is a total order, so there is nothing to tolerate.
  * RPN candidates: identities, levels and valid flags exactly.  The coordinates the clip replaced are exact
    (targets_cases.decode_check); the others depend on exp and stay within 2 x ref_decode_ulps of the float64 continuation, the
    scores within 2 x ref_sigmoid_ulps: the device's and the CPU's roundings are each about one rounding from the truth, but not
    the same rounding (the reason given in test_targets_gpu.py).
  * RPN result against the device's own candidates: the numpy restatement on the returned candidates gives exactly the returned
    dets and counts - no margin, ties included.
  * RPN result against the reference: kept anchors and counts equal for the cases whose inputs the generator proved robust
    against the rounding of exp.
"""
import types

import numpy as np
import pytest
import torch

from . import nms_cases as nc

pytestmark = pytest.mark.gpu
tc = nc.tc


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g28_nms")


@pytest.fixture(scope="module")
def mn():
    from iif_amd import mmdet_nms
    return mmdet_nms


def _check_padded(dets, keep, count, boxes, scores, want, cap):
    dets, keep, n = dets.cpu().numpy(), keep.cpu().numpy(), int(count.item())
    assert keep.shape == (cap,) and dets.shape == (cap, 5)
    assert n == want.size
    assert np.array_equal(keep[:n], want)
    assert (keep[n:] == -1).all() and not nc.bits(dets[n:]).any()
    assert np.array_equal(nc.bits(dets[:n]), nc.bits(nc.dets_np(boxes, scores, want)))


@pytest.mark.parametrize("name", list(nc.PLAIN_CASES))
def test_plain_nms_is_exact(dev, g, mn, name):
    c = nc.PLAIN_CASES[name]
    boxes, scores = nc.plain_inputs(name)
    want = g["p_%s_keep" % name].astype(np.int64)
    tb, ts = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)
    args = (c["thr"], c["offset"], c["score_threshold"], c["max_num"])
    cap = min(c["max_num"], c["n"]) if c["max_num"] > 0 else c["n"]
    _check_padded(*mn.nms_padded(tb, ts, *args), boxes, scores, want, cap)
    dets, inds = mn.nms(tb, ts, *args)
    assert dets.shape == (want.size, 5) and np.array_equal(inds.cpu().numpy(), want)
    assert np.array_equal(nc.bits(dets.cpu().numpy()), nc.bits(nc.dets_np(boxes, scores, want)))


def test_plain_nms_reads_five_column_rows_in_place(dev, g, mn):
    boxes, scores = nc.plain_inputs("n129")
    rows = torch.from_numpy(np.concatenate([boxes, scores[:, None]], axis=1)).to(dev)
    dets, inds = mn.nms(rows[:, :4], rows[:, 4], 0.5)
    assert np.array_equal(inds.cpu().numpy(), g["p_n129_keep"])


@pytest.mark.parametrize("name", list(nc.BATCHED_CASES))
def test_batched_nms_is_exact(dev, g, mn, name):
    c = nc.BATCHED_CASES[name]
    boxes, scores, ids = nc.batched_inputs(name)
    want = g["b_%s_keep" % name].astype(np.int64)
    t = [torch.from_numpy(x).to(dev) for x in (boxes, scores, ids)]
    _check_padded(*mn.batched_nms_padded(*t, nc.nms_cfg(name), class_agnostic=c["class_agnostic"]), boxes, scores, want, c["n"])
    dets, keep = mn.batched_nms(*t, nc.nms_cfg(name), class_agnostic=c["class_agnostic"])
    assert dets.shape == (want.size, 5) and np.array_equal(keep.cpu().numpy(), want)


def test_nms_is_deterministic_and_ignores_the_workspace_contents(dev, mn):
    boxes, scores, ids = nc.batched_inputs("ids5")
    t = [torch.from_numpy(x).to(dev) for x in (boxes, scores, ids)]
    first = mn.batched_nms_padded(*t, nc.nms_cfg("ids5"))
    ws = torch.full((mn.workspace_bytes(1, boxes.shape[0]),), 0xFF, dtype=torch.uint8, device=dev)
    for again in (mn.batched_nms_padded(*t, nc.nms_cfg("ids5")), mn.batched_nms_padded(*t, nc.nms_cfg("ids5"), workspace=ws)):
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ------------------------------------------------------------------------------------------------------------ RPN
class _Coder:
    means, stds, clip_border, add_ctr_clamp, ctr_clamp = nc.MEANS, nc.STDS, True, False, 32


def _cfg(c):
    return types.SimpleNamespace(nms_pre=c["nms_pre"], max_per_img=c["max_per_img"], min_bbox_size=c["min_size"],
                                 nms=dict(type="nms", iou_threshold=c["thr"]))


_runs = {}


def _run(mn, dev, name, workspace=None):
    """(inputs, dets [B, max_per_img, 5], counts [B], candidates as numpy): computed once per case and shared."""
    if name in _runs and workspace is None:
        return _runs[name]
    c = nc.rpn_case(name)
    cls, reg, anchors = nc.rpn_inputs(name)
    tcls = [torch.from_numpy(x).to(dev) for x in cls]
    treg = [torch.from_numpy(x).to(dev) for x in reg]
    if c["channels_last"]:
        tcls = [x.contiguous(memory_format=torch.channels_last) for x in tcls]
        treg = [x.contiguous(memory_format=torch.channels_last) for x in treg]
        assert tcls[0].stride(1) == 1
    tanc = [torch.from_numpy(x).to(dev) for x in anchors]
    dets, counts, cand = mn.rpn_proposals_padded(tcls, treg, tanc, c["shapes"], _cfg(c), _Coder(), return_candidates=True,
                                                 workspace=workspace)
    out = ((cls, reg, anchors), dets.cpu().numpy(), counts.cpu().numpy(),
           types.SimpleNamespace(index=cand.index.cpu().numpy(), boxes=cand.boxes.cpu().numpy(), scores=cand.scores.cpu().numpy(),
                                 level=cand.level.cpu().numpy(), valid=cand.valid.cpu().numpy().astype(bool)))
    if workspace is None:
        _runs[name] = out
    return out


@pytest.mark.parametrize("name", list(nc.RPN_CASES))
def test_rpn_candidates(dev, g, mn, name):
    (cls, reg, anchors), dets, counts, cand = _run(mn, dev, name)
    c = nc.RPN_CASES[name]
    dec, sig = float(g["ref_decode_ulps"]), float(g["ref_sigmoid_ulps"])
    all_anchors = np.concatenate(anchors)
    for b in range(len(c["shapes"])):
        pre = "r_%s_%d_" % (name, b)
        nv = int(g[pre + "nvalid"])
        print(name, b, "valid", int(cand.valid[b].sum()), "of", cand.valid[b].size, "expected", nv)
        # ties included: equal logits go to the lower index, at the nms_pre cut and in the rank; the generator asserts for every
        # case that no side lies near min_bbox_size, so the valid flags do not depend on the rounding of exp
        assert np.array_equal(cand.index[b], g[pre + "index"])
        assert np.array_equal(cand.level[b], g[pre + "level"])
        assert int(cand.valid[b].sum()) == nv and cand.valid[b][:nv].all()
        flat = nc.rpn_flat(cls, reg, b)
        deltas = np.concatenate([d for _, d in flat])[cand.index[b]]
        logits = np.concatenate([x for x, _ in flat])[cand.index[b]]
        ok, kinds, err = tc.decode_check(cand.boxes[b], all_anchors[cand.index[b]], deltas, *nc.decode_args(c["shapes"][b]))
        serr = nc.sigmoid_ulps(cand.scores[b], logits)
        print(name, b, "decode ulps", err, "allowed", 2 * dec, "sigmoid ulps", serr, "allowed", 2 * sig)
        assert ok and kinds
        assert err <= 2 * dec
        assert serr <= 2 * sig


def _check_result_follows(mn, dev, name):
    _, dets, counts, cand = _run(mn, dev, name)
    c = nc.rpn_case(name)
    for b in range(len(c["shapes"])):
        v = cand.valid[b]
        nv = int(v.sum())
        assert v[:nv].all()
        keep = nc.rpn_nms_np(cand.boxes[b], cand.level[b].astype(np.int64), v, c["thr"], c["max_per_img"])
        assert int(counts[b]) == keep.size
        want = np.concatenate([cand.boxes[b][keep], cand.scores[b][keep, None]], axis=1)
        assert np.array_equal(nc.bits(dets[b, :keep.size]), nc.bits(want))
        assert not nc.bits(dets[b, keep.size:]).any()
        assert dets.shape[1] == c["max_per_img"]


@pytest.mark.parametrize("name", list(nc.RPN_CASES))
def test_rpn_result_follows_from_the_returned_candidates(dev, mn, name):
    """Exact, no margin: the restatement of the NMS stage on the device's own ranked candidates."""
    _check_result_follows(mn, dev, name)


@pytest.mark.parametrize("name", list(nc.RPN_LONG_CASES))
def test_rpn_select_takes_a_second_stride_step(dev, mn, name):
    """A level of 17 280 anchors beside one of 288: identities and levels equal the restatement's (every candidate is valid, so
    the rank is by logit and index alone and no exp enters), and the result follows from the candidates, exactly."""
    (cls, reg, anchors), dets, counts, cand = _run(mn, dev, name)
    for b in range(len(nc.rpn_case(name)["shapes"])):
        idx, lvl, logits, _, _ = nc.rpn_candidates_np(name, b, cls, reg, anchors)
        order = nc.rpn_rank_np(idx, logits, np.ones(idx.size, dtype=bool))
        assert idx.size == 512 and cand.valid[b].all()
        assert np.array_equal(cand.index[b], idx[order])
        assert np.array_equal(cand.level[b], lvl[order])
    _check_result_follows(mn, dev, name)


@pytest.mark.parametrize("name", [k for k in nc.RPN_CASES if k not in nc.RPN_TIE_CASES])
def test_rpn_result_equals_the_reference(dev, g, mn, name):
    (cls, reg, anchors), dets, counts, cand = _run(mn, dev, name)
    c = nc.RPN_CASES[name]
    dec, sig = float(g["ref_decode_ulps"]), float(g["ref_sigmoid_ulps"])
    all_anchors = np.concatenate(anchors)
    for b in range(len(c["shapes"])):
        pre = "r_%s_%d_" % (name, b)
        keep = g[pre + "keep"]
        n = int(counts[b])
        assert n == keep.size
        kept = g[pre + "index"][keep]                                  # the anchors the reference kept, in its order
        # identities: the device's dets rows are its candidates at the kept positions (previous test); find them by position
        mine = nc.rpn_nms_np(cand.boxes[b], cand.level[b].astype(np.int64), cand.valid[b], c["thr"], c["max_per_img"])
        assert np.array_equal(cand.index[b][mine], kept)
        if n:
            flat = nc.rpn_flat(cls, reg, b)
            deltas = np.concatenate([d for _, d in flat])[kept]
            logits = np.concatenate([x for x, _ in flat])[kept]
            ok, kinds, err = tc.decode_check(dets[b, :n, :4], all_anchors[kept], deltas, *nc.decode_args(c["shapes"][b]))
            assert ok and kinds and err <= 2 * dec
            assert nc.sigmoid_ulps(dets[b, :n, 4], logits) <= 2 * sig


def test_rpn_reads_anchor_rows_that_are_not_16_byte_pieces(dev, mn):
    """Anchors kept as the first four columns of five-column rows (pitch 5: the scalar loads of the gather) give the same bits."""
    name = "fpn5"
    c = nc.RPN_CASES[name]
    cls, reg, anchors = nc.rpn_inputs(name)
    t = lambda xs: [torch.from_numpy(x).to(dev) for x in xs]          # noqa: E731
    wide = [torch.cat([a, a.new_zeros((a.shape[0], 1))], dim=1)[:, :4] for a in t(anchors)]
    assert wide[0].stride(0) == 5
    dets, counts = mn.rpn_proposals_padded(t(cls), t(reg), wide, c["shapes"], _cfg(c), _Coder())
    _, want, want_counts, _ = _run(mn, dev, name)
    assert np.array_equal(nc.bits(dets.cpu().numpy()), nc.bits(want)) and np.array_equal(counts.cpu().numpy(), want_counts)


def test_rpn_is_deterministic_and_ignores_the_workspace_contents(dev, mn):
    _, dets, counts, cand = _run(mn, dev, "fpn5")
    ws = torch.full((mn.workspace_bytes(2, cand.index.shape[1]),), 0xFF, dtype=torch.uint8, device=dev)
    _, dets2, counts2, cand2 = _run(mn, dev, "fpn5", workspace=ws)
    _, dets3, counts3, cand3 = _run(mn, dev, "fpn5", workspace=ws)
    for other_d, other_c, other in ((dets2, counts2, cand2), (dets3, counts3, cand3)):
        assert np.array_equal(nc.bits(dets), nc.bits(other_d)) and np.array_equal(counts, other_c)
        assert np.array_equal(cand.index, other.index) and np.array_equal(nc.bits(cand.boxes), nc.bits(other.boxes))
        assert np.array_equal(nc.bits(cand.scores), nc.bits(other.scores)) and np.array_equal(cand.valid, other.valid)


@pytest.mark.parametrize("name", ["fpn5", "none"])
def test_rpn_get_bboxes_returns_the_reference_shapes(dev, g, mn, name):
    c = nc.RPN_CASES[name]
    cls, reg, anchors = nc.rpn_inputs(name)
    t = lambda xs: [torch.from_numpy(x).to(dev) for x in xs]          # noqa: E731
    metas = [dict(img_shape=s, scale_factor=np.ones(4, dtype=np.float32)) for s in c["shapes"]]
    out = mn.rpn_get_bboxes(t(cls), t(reg), t(anchors), metas, _cfg(c), _Coder())
    assert isinstance(out, list) and len(out) == len(c["shapes"])
    for b, p in enumerate(out):
        assert p.shape == (g["r_%s_%d_keep" % (name, b)].size, 5) and p.dtype == torch.float32
    if name == "none":
        assert all(p.shape == (0, 5) for p in out)
