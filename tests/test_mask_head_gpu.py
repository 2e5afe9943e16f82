"""The two ends of the mask branch on the MI355X (csrc/mask_ops.hip through iif_amd.mmdet_mask_target and
iif_amd.mmdet_mask_loss) against tests/golden/g30_mask_head.npz - the reference's own outputs - and the float64 restatement of
tests/mask_cases.py.  Binary outputs must equal the fixture exactly (no pixel is excluded: the generator keeps every value at
least 1e-4 from its threshold, or exactly on it); soft targets may differ from float64 by 4x the float32 reference's own error
(another summation order), the factor of test_roi_extract_gpu.py."""
import numpy as np
import pytest
import torch

from . import mask_cases as mc

pytestmark = pytest.mark.gpu
FIXTURE = "g30_mask_head"
DEV = "cuda:0"


def _bits(g, key, shape):
    return np.unpackbits(g[key])[:int(np.prod(shape))].reshape(shape).astype(bool)


def _target_inputs(name):
    rows = mc.target_rows(name)
    rois = torch.from_numpy(np.ascontiguousarray(rows[:, [0, 2, 3, 4, 5]])).to(DEV)
    gt = torch.from_numpy(rows[:, 1].astype(np.int64)).to(DEV)
    masks = [torch.from_numpy(m.copy()).to(DEV) for m in mc.case_masks(name)]
    return rows, rois, gt, masks


@pytest.mark.parametrize("name", list(mc.TARGET_CASES))
def test_binary_targets_equal_the_reference(golden, name):
    from iif_amd.mmdet_mask_target import mask_targets_padded
    g = golden(FIXTURE)
    rows, rois, gt, masks = _target_inputs(name)
    size = mc.TARGET_CASES[name][1]
    out = mask_targets_padded(rois, gt, masks, size)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(rows),) + size
    got = out.cpu().numpy()
    assert set(np.unique(got).tolist()) <= {0.0, 1.0}
    want = _bits(g, "t_%s_bits" % name, got.shape)
    wrong = np.argwhere(got.astype(bool) != want)
    assert wrong.size == 0, (len(wrong), wrong[:5].tolist())
    if name == "kinds_28":                                      # averages of exactly 0.5 come out as 1
        tie = mc.target_reference64(name)[mc.TIE_ROW] == 0.5
        assert tie.sum() >= 20 and got[mc.TIE_ROW][tie].all()


@pytest.mark.parametrize("name", list(mc.TARGET_CASES))
def test_soft_targets_within_four_times_the_float32_reference(golden, name):
    from iif_amd.mmdet_mask_target import mask_targets_padded
    g = golden(FIXTURE)
    rows, rois, gt, masks = _target_inputs(name)
    got = mask_targets_padded(rois, gt, masks, mc.TARGET_CASES[name][1], binarize=False).cpu().numpy().astype(np.float64)
    want = mc.target_reference64(name)
    err, ref = float(np.abs(got - want).max()), float(g["t_%s_ref_f32_err" % name])
    print("soft targets %s: max error %.3e, float32 reference %.3e, ratio %.2f" % (name, err, ref, err / ref))
    assert err <= 4 * ref
    assert not got[[k for k in range(len(rows)) if not want[k].any()]].any()       # zero rows are exactly zero


def test_mask_target_equals_the_padded_entry_row_for_row():
    from iif_amd.mmdet_mask_target import mask_target, mask_target_single, mask_targets_padded
    rows, rois, gt, masks = _target_inputs("kinds_28")
    valid = np.array([mc.target_row_valid(r, mc.IMAGES) for r in rows])
    sel = [np.nonzero(valid & (rows[:, 0] == i))[0] for i in range(len(mc.IMAGES))]
    props = [rois[torch.from_numpy(s).to(DEV)][:, 1:].contiguous() for s in sel]
    inds = [gt[torch.from_numpy(s).to(DEV)] for s in sel]
    order = torch.from_numpy(np.concatenate(sel)).to(DEV)
    host_masks = mc.case_masks("kinds_28")

    class Bitmap:                                               # BitmapMasks by duck type: host masks, uploaded per call
        def __init__(self, m):
            self.masks, self.height, self.width = m, m.shape[1], m.shape[2]
    for size, cfg in (((28, 28), dict(mask_size=28)), ((7, 11), dict(mask_size=(7, 11), soft_mask_target=True))):
        padded = mask_targets_padded(rois, gt, masks, size, binarize=not cfg.get("soft_mask_target", False))
        for gts in (masks, [Bitmap(m) for m in host_masks], list(host_masks)):
            out = mask_target(props, inds, gts, cfg)
            assert out.dtype == torch.float32 and out.is_cuda and torch.equal(out, padded[order])
        one = mask_target_single(props[1], inds[1], masks[1], cfg)
        assert torch.equal(one, padded[torch.from_numpy(sel[1]).to(DEV)])
    empty = mask_target_single(props[0][:0], inds[0][:0], masks[0], dict(mask_size=(7, 11)))
    assert tuple(empty.shape) == (0, 7, 11) and empty.is_cuda
    assert tuple(mask_targets_padded(rois[:0], gt[:0], masks, 28).shape) == (0, 28, 28)


def test_device_bitmap_masks_crop_and_resize():
    from iif_amd.mmdet_mask_target import DeviceBitmapMasks, mask_target_single
    rows, rois, gt, masks = _target_inputs("kinds_28")
    keep = np.nonzero((rows[:, 0] == 0) & (rows[:, 1] >= 0) & (rows[:, 1] < 3))[0]
    idx = torch.from_numpy(keep).to(DEV)
    host = mc.case_masks("kinds_28")[0]
    d = DeviceBitmapMasks(host.copy(), host.shape[1], host.shape[2])
    want = mask_target_single(rois[idx][:, 1:].contiguous(), gt[idx], masks[0], dict(mask_size=28))
    got = d.crop_and_resize(rows[keep, 2:6], (28, 28), rows[keep, 1].astype(np.int64), device=DEV)
    assert got.is_cuda and torch.equal(got, want)
    assert d.device_masks(DEV) is d.device_masks(DEV)           # uploaded once
    soft = d.crop_and_resize(rois[idx][:, 1:], 28, gt[idx], binarize=False)
    assert torch.equal(soft, mask_target_single(rois[idx][:, 1:].contiguous(), gt[idx], d, dict(mask_size=28, soft_mask_target=True)))
    sub = d[[2]]                                                # indexing keeps the class; mask 2 alone is index 0
    tie = torch.from_numpy(rows[mc.TIE_ROW:mc.TIE_ROW + 1, 2:6].copy()).to(DEV)
    assert torch.equal(sub.crop_and_resize(tie, 28, torch.zeros(1, dtype=torch.int64, device=DEV)),
                       d.crop_and_resize(tie, 28, torch.full((1,), 2, dtype=torch.int64, device=DEV)))
    assert tuple(DeviceBitmapMasks([], 8, 8).crop_and_resize(tie, 28, torch.zeros(1, dtype=torch.int64, device=DEV)).shape) == (0, 28, 28)


def test_masks_read_in_place_from_a_wider_buffer_give_the_same_bits():
    """Views into wider buffers (pitch > W, rows and masks that start at any byte), bool storage and 255 for "inside"."""
    from iif_amd.mmdet_mask_target import mask_targets_padded
    rows, rois, gt, masks = _target_inputs("kinds_28")
    for binarize in (True, False):
        want = mask_targets_padded(rois, gt, masks, 28, binarize=binarize)
        views = []
        for i, m in enumerate(masks):
            G, H, W = m.shape
            buf = torch.full((G, H + 3, W + 21 + i), 1, dtype=torch.uint8, device=DEV)       # ones around the view: a read outside shows
            v = buf[:, 2:2 + H, 5 + i:5 + i + W]
            v.copy_(m)
            assert v.stride(1) == W + 21 + i and not v.is_contiguous()
            views.append(v)
        assert torch.equal(mask_targets_padded(rois, gt, views, 28, binarize=binarize), want)
        assert torch.equal(mask_targets_padded(rois, gt, [m * 255 for m in masks], 28, binarize=binarize), want)
        assert torch.equal(mask_targets_padded(rois, gt, [m.bool() for m in masks], 28, binarize=binarize), want)
        wide = torch.zeros((rois.size(0), 9), device=DEV)                                    # rois with a pitch
        wide[:, 2:7] = rois
        assert torch.equal(mask_targets_padded(wide[:, 2:7], gt, masks, 28, binarize=binarize), want)


# ------------------------------------------------------------------------------------------------------------ paste
def _paste_inputs(name, dtype=torch.float32):
    C, agnostic, activated = mc.PASTE_CASES[name]
    pred = torch.from_numpy(mc.paste_pred(name).copy()).to(DEV).to(dtype)
    boxes = torch.from_numpy(mc.paste_boxes().copy()).to(DEV)
    labels = torch.from_numpy(mc.paste_labels()).to(DEV)
    return pred, boxes, labels, agnostic, activated


@pytest.mark.parametrize("name,dtype", [("c5_logits", torch.float32), ("c5_logits", torch.bfloat16), ("c1_agnostic", torch.float32),
                                        ("c1_agnostic", torch.bfloat16), ("c5_activated", torch.float32)])
def test_pasted_masks_equal_the_reference(golden, name, dtype):
    from iif_amd.mmdet_mask_loss import paste_masks
    g = golden(FIXTURE)
    pred, boxes, labels, agnostic, activated = _paste_inputs(name, dtype)
    out = paste_masks(pred, boxes, labels, mc.IMG_H, mc.IMG_W, 0.5, class_agnostic=agnostic, activated=activated)
    assert out.dtype == torch.bool and tuple(out.shape) == (len(mc.BOXES), mc.IMG_H, mc.IMG_W)
    got = out.cpu().numpy()
    want = _bits(g, "p_%s_bits" % name, got.shape)
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, (len(wrong), wrong[:5].tolist())
    if not activated:                                           # a probability of exactly 0.5 meets the threshold 0.5
        tie = mc.paste_reference64(name)[mc.PASTE_TIE] == 0.5
        assert tie.sum() >= 400 and got[mc.PASTE_TIE][tie].all()
    # threshold 0: every pixel is true, padding included
    assert bool(paste_masks(pred, boxes, labels, mc.IMG_H, mc.IMG_W, 0, class_agnostic=agnostic, activated=activated).all())
    # boxes read in place with another pitch
    wide = torch.zeros((boxes.size(0), 8), device=DEV)
    wide[:, 1:6] = boxes
    assert torch.equal(paste_masks(pred, wide[:, 1:6], labels, mc.IMG_H, mc.IMG_W, 0.5, class_agnostic=agnostic, activated=activated), out)


def test_paste_edge_rows():
    from iif_amd.mmdet_mask_loss import paste_masks
    pred, boxes, labels, _, _ = _paste_inputs("c5_logits")
    base = paste_masks(pred, boxes, labels, mc.IMG_H, mc.IMG_W, 0.5)
    bad = labels.clone()
    bad[0], bad[6] = 5, -1                                      # a label outside [0, C): an all-false mask, even at threshold 0
    for thr in (0.5, 0.0):
        out = paste_masks(pred, boxes, bad, mc.IMG_H, mc.IMG_W, thr)
        assert not out[0].any() and not out[6].any()
    assert torch.equal(paste_masks(pred, boxes, bad, mc.IMG_H, mc.IMG_W, 0.5)[1:6], base[1:6])
    empty = paste_masks(pred[:0], boxes[:0], labels[:0], mc.IMG_H, mc.IMG_W, 0.5)
    assert empty.dtype == torch.bool and tuple(empty.shape) == (0, mc.IMG_H, mc.IMG_W)
    one = paste_masks(pred[2:3], boxes[2:3], labels[2:3], mc.IMG_H, mc.IMG_W, 0.5)
    assert torch.equal(one[0], base[2])
    # an output that does not start on a 16-byte boundary, and an image narrower than one 16-byte store
    narrow = paste_masks(pred, boxes, labels, 7, 13, 0.5)
    assert torch.equal(narrow, base[:, :7, :13])


def test_get_seg_masks_returns_the_reference_structure(golden):
    from iif_amd.mmdet_mask_loss import get_seg_masks
    g = golden(FIXTURE)
    pred, boxes, labels, _, _ = _paste_inputs("c5_logits")
    want = _bits(g, "p_c5_logits_bits", (len(mc.BOXES), mc.IMG_H, mc.IMG_W))
    cfg = dict(mask_thr_binary=0.5)

    def check(segms, want):
        assert isinstance(segms, list) and len(segms) == 5 and sum(len(s) for s in segms) == len(mc.BOXES)
        for c in range(5):
            mine = [n for n in range(len(mc.BOXES)) if mc.LABELS[n] == c]
            assert len(segms[c]) == len(mine)
            for m, n in zip(segms[c], mine):
                assert isinstance(m, np.ndarray) and m.dtype == np.bool_ and m.shape == (mc.IMG_H, mc.IMG_W) and np.array_equal(m, want[n])
    # rescale: the boxes are divided by the factor, the image is ori_shape
    scaled = boxes.clone()
    scaled[:, :4] *= 2
    check(get_seg_masks(pred, scaled, labels, cfg, (mc.IMG_H, mc.IMG_W, 3), torch.full((4,), 2.0, device=DEV), True, 5), want)
    check(get_seg_masks(pred, scaled, labels, cfg, (mc.IMG_H, mc.IMG_W, 3), np.full(4, 2.0, dtype=np.float32), True, 5), want)
    # no rescale: the image is ori_shape times the factor, rounded
    check(get_seg_masks(pred, boxes, labels, cfg, (mc.IMG_H / 2, mc.IMG_W / 2, 3), np.array([2.0, 2.0, 2.0, 2.0]), False, 5), want)
    check(get_seg_masks(pred, boxes, labels, cfg, (mc.IMG_H, mc.IMG_W, 3), np.ones(4), True, 5, pin_memory=False), want)      # a pageable block
    # the AugTest branch: an ndarray of probabilities
    act, _, _, _, _ = _paste_inputs("c5_activated")
    check(get_seg_masks(act.cpu().numpy(), boxes, labels, cfg, (mc.IMG_H, mc.IMG_W, 3), np.ones(4), True, 5),
          _bits(g, "p_c5_activated_bits", want.shape))
    # class-agnostic: one channel, the labels only sort the result
    ag, _, _, _, _ = _paste_inputs("c1_agnostic")
    check(get_seg_masks(ag, boxes, labels, cfg, (mc.IMG_H, mc.IMG_W, 3), np.ones(4), True, 5, class_agnostic=True),
          _bits(g, "p_c1_agnostic_bits", want.shape))
    assert get_seg_masks(pred[:0], boxes[:0], labels[:0], cfg, (mc.IMG_H, mc.IMG_W, 3), np.ones(4), True, 5) == [[], [], [], [], []]


def test_no_host_synchronisation():
    """mask_targets_padded followed by mask_cross_entropy under autograd, and paste_masks, with synchronising calls forbidden."""
    from iif_amd.mmdet_mask_loss import mask_cross_entropy, paste_masks
    from iif_amd.mmdet_mask_target import mask_target, mask_targets_padded
    rows, rois, gt, masks = _target_inputs("kinds_28")
    K = rois.size(0)
    logits = torch.from_numpy(mc.paste_pred("c5_logits")[np.arange(K) % len(mc.BOXES)].copy()).to(DEV).requires_grad_(True)
    cls = torch.from_numpy((np.arange(K) % 5).astype(np.int64)).to(DEV)
    pred, boxes, labels, _, _ = _paste_inputs("c5_logits")
    props = [rois[:4, 1:].contiguous(), rois[4:6, 1:].contiguous()]
    inds = [torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        targets = mask_targets_padded(rois, gt, masks, 28)
        loss = mask_cross_entropy(logits, targets, cls)
        loss.backward()
        listed = mask_target(props, inds, masks, dict(mask_size=28))
        pasted = paste_masks(pred, boxes, labels, mc.IMG_H, mc.IMG_W, 0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss).all() and logits.grad is not None and bool(logits.grad.abs().sum() > 0)
    assert tuple(listed.shape) == (6, 28, 28) and bool(pasted.any())


def test_wide_image_paths_against_the_restatement():
    """A 300 x 1100 image: runs cut into 8 parts, fewer than 16 rows per pass (the row pitch is above 1024 bytes), four slabs -
    the paths the fixture's small images do not reach.  Soft targets against the float64 restatement, allowed 4x the error of
    the restatement's own float32 evaluation; binary targets wherever float64 is at least MARGIN from 0.5 (printed: how many
    are not)."""
    from iif_amd.mmdet_mask_target import mask_targets_padded
    H, W = 300, 1100
    m = mc.masks(H, W, 1, salt=8700)
    rows = np.array([(0, 0, 0.0, 0.0, W, H), (0, 0, 17.25, 40.5, 1093.0, 171.0), (0, 0, 600.0, 10.0, 1150.0, 310.0)], dtype=np.float32)
    v64 = mc.targets_np(rows, [m], (28, 28), mc.F64)
    v32 = mc.targets_np(rows, [m], (28, 28), mc.F32)
    ref = float(np.abs(v32.astype(np.float64) - v64).max())
    rois = torch.from_numpy(np.ascontiguousarray(rows[:, [0, 2, 3, 4, 5]])).to(DEV)
    gt = torch.zeros(3, dtype=torch.int64, device=DEV)
    md = [torch.from_numpy(m.copy()).to(DEV)]
    soft = mask_targets_padded(rois, gt, md, 28, binarize=False).cpu().numpy().astype(np.float64)
    err = float(np.abs(soft - v64).max())
    print("wide image soft targets: max error %.3e, float32 restatement %.3e, ratio %.2f" % (err, ref, err / ref))
    assert 0 < ref < 1e-4 and err <= 4 * ref
    hard = mask_targets_padded(rois, gt, md, 28).cpu().numpy()
    clear = np.abs(v64 - 0.5) >= mc.MARGIN
    print("wide image binary targets: %d of %d values within %g of 0.5 left out" % (int((~clear).sum()), clear.size, mc.MARGIN))
    assert clear.mean() > 0.99 and np.array_equal(hard.astype(bool)[clear], (v64 >= 0.5)[clear])
    assert np.array_equal(hard, (soft >= 0.5).astype(np.float32))


def test_more_images_than_one_launch_takes_and_one_row_views():
    from iif_amd.mmdet_mask_loss import paste_masks
    from iif_amd.mmdet_mask_target import mask_target, mask_targets_padded
    rows, rois, gt, masks = _target_inputs("kinds_28")
    want = mask_targets_padded(rois, gt, masks, 28)
    # 17 images: mask_target splits the list into launches of 16
    pick = [k for k in range(len(rows)) if mc.target_row_valid(rows[k], mc.IMAGES)][:17]
    props = [rois[k:k + 1, 1:].contiguous() for k in pick]
    inds = [gt[k:k + 1] for k in pick]
    out = mask_target(props, inds, [masks[int(rows[k, 0])] for k in pick], dict(mask_size=28))
    assert torch.equal(out, want[torch.tensor(pick, device=DEV)])
    # one row whose COLUMN stride is not 1 (every other column of a wider row): copied, not misread
    k = pick[0]
    col = torch.zeros((1, 10), device=DEV)[:, ::2]
    col.copy_(rois[k:k + 1])
    assert col.shape == (1, 5) and col.stride(1) != 1
    assert torch.equal(mask_targets_padded(col, gt[k:k + 1], masks, 28), want[k:k + 1])
    pred, boxes, labels, _, _ = _paste_inputs("c5_logits")
    base = paste_masks(pred, boxes, labels, mc.IMG_H, mc.IMG_W, 0.5)
    bcol = torch.zeros((1, 10), device=DEV)[:, ::2]
    bcol.copy_(boxes[2:3])
    assert bcol.stride(1) != 1
    assert torch.equal(paste_masks(pred[2:3], bcol, labels[2:3], mc.IMG_H, mc.IMG_W, 0.5)[0], base[2])
