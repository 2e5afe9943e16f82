"""COCO run-length encoding on the MI355X (csrc/mask_rle.hip through iif_amd.mmdet_mask_loss: paste_masks_rle, encode_masks,
get_seg_masks_rle) against tests/rle_ref.py applied to the boolean images: those of tests/golden/g30_mask_head.npz (the
reference's own outputs) and those paste_masks / get_seg_masks give.  Everything is compared byte for byte."""
import numpy as np
import pytest
import torch

from . import mask_cases as mc
from . import rle_ref as R
from .test_mask_rle_host import big_rectangle, crossing_mask

pytestmark = pytest.mark.gpu
FIXTURE = "g30_mask_head"
DEV = "cuda:0"


def _bits(g, key, shape):
    return np.unpackbits(g[key])[:int(np.prod(shape))].reshape(shape).astype(bool)


def _paste_inputs(name, dtype=torch.float32):
    C, agnostic, activated = mc.PASTE_CASES[name]
    pred = torch.from_numpy(mc.paste_pred(name).copy()).to(DEV).to(dtype)
    boxes = torch.from_numpy(mc.paste_boxes().copy()).to(DEV)
    labels = torch.from_numpy(mc.paste_labels()).to(DEV)
    return pred, boxes, labels, agnostic, activated


def _want(masks):
    """bool [N, H, W] (tensor or ndarray) -> what pycocotools' encode gives for each."""
    if isinstance(masks, torch.Tensor):
        masks = masks.cpu().numpy()
    return [R.encode_rle(m) for m in masks]


def _check_against_paste(pred, boxes, labels, H, W, thr, **kw):
    from iif_amd.mmdet_mask_loss import paste_masks, paste_masks_rle
    got = paste_masks_rle(pred, boxes, labels, H, W, thr, **kw)
    want = _want(paste_masks(pred, boxes, labels, H, W, thr, **kw))
    assert isinstance(got, list) and len(got) == pred.size(0)
    for n, (a, b) in enumerate(zip(got, want)):
        assert a == b, (n, R.from_string(a["counts"])[:8], R.from_string(b["counts"])[:8])
        assert isinstance(a["counts"], bytes) and a["size"] == [H, W]
    return got


@pytest.mark.parametrize("name,dtype", [("c5_logits", torch.float32), ("c5_logits", torch.bfloat16), ("c1_agnostic", torch.float32),
                                        ("c1_agnostic", torch.bfloat16), ("c5_activated", torch.float32)])
def test_pasted_rle_equals_the_reference_bits(golden, name, dtype):
    """Boxes inside, across every edge, outside, of zero width, below one pixel, the whole image and larger, and the exact tie."""
    from iif_amd.mmdet_mask_loss import paste_masks_rle
    g = golden(FIXTURE)
    pred, boxes, labels, agnostic, activated = _paste_inputs(name, dtype)
    got = paste_masks_rle(pred, boxes, labels, mc.IMG_H, mc.IMG_W, 0.5, class_agnostic=agnostic, activated=activated)
    want = _want(_bits(g, "p_%s_bits" % name, (len(mc.BOXES), mc.IMG_H, mc.IMG_W)))
    assert len(got) == len(want)
    for n, (a, b) in enumerate(zip(got, want)):
        assert a == b, (n, R.from_string(a["counts"])[:8], R.from_string(b["counts"])[:8])
    assert got[3]["counts"] == R.to_string([mc.IMG_H * mc.IMG_W])                  # the box outside the image


def test_pasted_rle_equals_the_pasted_masks():
    pred, boxes, labels, _, _ = _paste_inputs("c5_logits")
    H, W = mc.IMG_H, mc.IMG_W
    # threshold 0: every pixel is set, padding included - the leading run of zeros is empty
    for a in _check_against_paste(pred, boxes, labels, H, W, 0):
        assert a["counts"] == R.to_string([0, H * W])
    # a label outside [0, C): an all-false mask, even at threshold 0
    bad = labels.clone()
    bad[0], bad[6] = 5, -1
    for thr in (0.5, 0.0):
        got = _check_against_paste(pred, boxes, bad, H, W, thr)
        assert got[0]["counts"] == got[6]["counts"] == R.to_string([H * W])
    from iif_amd.mmdet_mask_loss import paste_masks_rle
    assert paste_masks_rle(pred[:0], boxes[:0], labels[:0], H, W, 0.5) == []
    base = _check_against_paste(pred, boxes, labels, H, W, 0.5)
    assert _check_against_paste(pred[2:3], boxes[2:3], labels[2:3], H, W, 0.5) == base[2:3]
    for h, w in ((1, 1), (1, 300), (300, 1), (7, 13)):
        for thr in (0.5, 0.0):
            _check_against_paste(pred, boxes, labels, h, w, thr)
    # boxes read in place at another pitch
    wide = torch.zeros((boxes.size(0), 8), device=DEV)
    wide[:, 1:6] = boxes
    assert _check_against_paste(pred, wide[:, 1:6], labels, H, W, 0.5) == base
    # class-agnostic and activated inputs take the same path as paste_masks
    ag, _, _, _, _ = _paste_inputs("c1_agnostic", torch.bfloat16)
    _check_against_paste(ag, boxes, labels, H, W, 0.5, class_agnostic=True)
    act, _, _, _, _ = _paste_inputs("c5_activated")
    _check_against_paste(act, boxes, labels, H, W, 0.5, activated=True)


def test_pasted_rle_on_an_image_wider_than_a_wave_and_taller_than_a_block():
    """515 x 301: five column chunks of 64 lanes, five row segments of 128 in two blocks; boxes across the whole image, across
    three of its edges, and one that leaves the first column and the first row outside the rectangle at threshold 0."""
    pred, _, labels, _, _ = _paste_inputs("c5_logits")
    boxes = torch.tensor([[-3.5, 2.25, 298.75, 520.0], [100.5, -20.0, 330.0, 400.0], [40.0, 150.0, 260.0, 505.5]], device=DEV)
    for thr in (0.5, 0.0):
        got = _check_against_paste(pred[:3], boxes, labels[:3], 515, 301, thr)
    assert _check_against_paste(pred[:1], boxes[:1], labels[:1], 515, 301, 0.5) == _check_against_paste(
        pred[:3], boxes, labels[:3], 515, 301, 0.5)[:1]
    assert len(R.from_string(got[0]["counts"])) == 2


def _check_encode(masks):
    from iif_amd.mmdet_mask_loss import encode_masks
    got = encode_masks(masks)
    want = _want(masks if masks.dim() == 3 else masks[None])
    assert isinstance(got, list) and len(got) == len(want)
    for n, (a, b) in enumerate(zip(got, want)):
        assert a == b, (n, R.from_string(a["counts"])[:8], R.from_string(b["counts"])[:8])
    return got


def test_encode_masks():
    from iif_amd.mmdet_mask_loss import encode_masks
    from iif_amd.mmdet_mask_target import DeviceBitmapMasks
    rng = np.random.RandomState(4200)
    H, W = 61, 93
    simple = np.zeros((5, H, W), dtype=bool)
    simple[1] = True
    simple[2, 0, 0] = True                                      # only the first pixel
    simple[3, H - 1, W - 1] = True                              # only the last pixel
    simple[4] = crossing_mask()                                 # a run across a column boundary
    got = _check_encode(torch.from_numpy(simple).to(DEV))
    assert [R.from_string(a["counts"]) for a in got] == [[H * W], [0, H * W], [0, 1, H * W - 1], [H * W - 1, 1],
                                                          [315, 40, 11, 3, 2091, 71, 3142]]
    assert got[4]["counts"] == b"k9X1;kNPQ2T2kP1"
    yy, xx = np.mgrid[0:65, 0:257]
    checker = torch.from_numpy((yy + xx) % 2 == 1).to(DEV)       # H * W runs: the worst case
    assert len(R.from_string(_check_encode(checker[None])[0]["counts"])) == 65 * 257
    assert len(R.from_string(_check_encode(~checker[None])[0]["counts"])) == 65 * 257 + 1
    for n, h, w in ((3, 64, 64), (2, 130, 70)):
        m = torch.from_numpy(rng.rand(n, h, w) < 0.5).to(DEV)
        _check_encode(m)
        _check_encode(m.to(torch.uint8) * 255)                  # any non-zero byte is inside
        assert encode_masks(m[1]) == encode_masks(m)[1:2]       # [H, W]: a list of one
        _check_encode(m[0])
    # a view into a wider buffer of ones: pitch > W, rows and masks that start at any byte; a read outside the view shows
    m = torch.from_numpy(rng.rand(3, 130, 70) < 0.5).to(DEV)
    buf = torch.ones((3, 133, 91), dtype=torch.bool, device=DEV)
    view = buf[:, 2:132, 5:75]
    view.copy_(m)
    assert view.stride(1) == 91 and not view.is_contiguous()
    assert _check_encode(view) == encode_masks(m)
    assert _check_encode(m[:, :, ::2]) == encode_masks(m[:, :, ::2].contiguous())               # column stride 2: copied, not misread
    assert encode_masks(m[:0]) == []
    # the container of the mask targets, from host masks and from a device tensor
    host = m.cpu().numpy()
    assert encode_masks(DeviceBitmapMasks(host, 130, 70)) == encode_masks(m) == encode_masks(DeviceBitmapMasks(m, 130, 70))
    # 800 x 1333: differences of runs, five-byte counts
    got = _check_encode(torch.from_numpy(big_rectangle()).to(DEV))[0]
    assert len(got["counts"]) == 2010 and got["counts"].startswith(b"T[l4hb0X6000") and got["size"] == [800, 1333]


def test_get_seg_masks_rle_returns_the_reference_structure():
    from iif_amd.mmdet_mask_loss import get_seg_masks, get_seg_masks_rle
    pred, boxes, labels, _, _ = _paste_inputs("c5_logits")
    cfg = dict(mask_thr_binary=0.5)
    scaled = boxes.clone()
    scaled[:, :4] *= 2
    calls = [(pred, scaled, labels, cfg, (mc.IMG_H, mc.IMG_W, 3), torch.full((4,), 2.0, device=DEV), True, 5),
             (pred, scaled, labels, cfg, (mc.IMG_H, mc.IMG_W, 3), np.full(4, 2.0, dtype=np.float32), True, 5),
             (pred, boxes, labels, cfg, (mc.IMG_H / 2, mc.IMG_W / 2, 3), np.array([2.0, 2.0, 2.0, 2.0]), False, 5)]
    for args in calls:
        segms = get_seg_masks_rle(*args)
        masks = get_seg_masks(*args)
        assert isinstance(segms, list) and len(segms) == 5 and sum(len(s) for s in segms) == len(mc.BOXES)
        for c in range(5):
            mine = [n for n in range(len(mc.BOXES)) if mc.LABELS[n] == c]
            assert len(segms[c]) == len(mine) == len(masks[c])
            for rle, m in zip(segms[c], masks[c]):              # detection order within a class
                assert rle == R.encode_rle(m) and rle["size"] == [mc.IMG_H, mc.IMG_W]
    # the AugTest branch (an ndarray of probabilities) and a class-agnostic head
    act, _, _, _, _ = _paste_inputs("c5_activated")
    args = (act.cpu().numpy(), boxes, labels, cfg, (mc.IMG_H, mc.IMG_W, 3), np.ones(4), True, 5)
    assert get_seg_masks_rle(*args) == [[R.encode_rle(m) for m in ms] for ms in get_seg_masks(*args)]
    ag, _, _, _, _ = _paste_inputs("c1_agnostic")
    args = (ag, boxes, labels, cfg, (mc.IMG_H, mc.IMG_W, 3), np.ones(4), True, 5)
    assert get_seg_masks_rle(*args, class_agnostic=True) == [[R.encode_rle(m) for m in ms]
                                                             for ms in get_seg_masks(*args, class_agnostic=True)]
    assert get_seg_masks_rle(pred[:0], boxes[:0], labels[:0], cfg, (mc.IMG_H, mc.IMG_W, 3), np.ones(4), True, 5) == [[], [], [], [], []]


def test_the_bitmap_is_not_built_and_the_bytes_do_not_change():
    """N = 4 at 512 x 640: the peak of allocated device memory around paste_masks_rle rises by less than a quarter of the
    boolean block above its value before the call (runs and workspace are well under 100 KB here).  Two calls: the same bytes."""
    from iif_amd.mmdet_mask_loss import paste_masks_rle
    pred, _, labels, _, _ = _paste_inputs("c5_logits")
    N, H, W = 4, 512, 640
    boxes = torch.tensor([[30.5, 41.0, 190.0, 260.5], [300.0, 100.0, 520.25, 330.0], [-20.0, 400.0, 150.0, 530.0],
                          [410.5, 20.25, 630.0, 200.0]], device=DEV)
    pred, labels = pred[:N].contiguous(), labels[:N].contiguous()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    first = paste_masks_rle(pred, boxes, labels, H, W, 0.5)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %d bytes; the boolean block would be %d" % (rise, N * H * W))
    assert rise < N * H * W / 4
    assert all(len(a["counts"]) > 100 for a in first)           # real masks, a few hundred runs each
    assert paste_masks_rle(pred, boxes, labels, H, W, 0.5) == first
    _check_against_paste(pred, boxes, labels, H, W, 0.5)


def test_two_device_reads():
    """The totals (with the labels), then the runs: nothing else comes to the host."""
    from iif_amd.mmdet_mask_loss import encode_masks, get_seg_masks_rle, paste_masks_rle
    pred, boxes, labels, _, _ = _paste_inputs("c5_logits")
    m = torch.from_numpy(crossing_mask()).to(DEV)
    cfg = dict(mask_thr_binary=0.5)
    ori, sf = (mc.IMG_H, mc.IMG_W, 3), torch.ones(4, device=DEV)        # on the device: an upload would synchronise as well
    calls = [lambda: paste_masks_rle(pred, boxes, labels, mc.IMG_H, mc.IMG_W, 0.5), lambda: encode_masks(m),
             lambda: get_seg_masks_rle(pred, boxes, labels, cfg, ori, sf, True, 5)]
    for call in calls:
        call()
        torch.cuda.synchronize()
        reads = []
        orig = torch.Tensor.cpu

        def counting(self, *a, **k):
            if self.is_cuda:
                reads.append(tuple(self.shape))
            return orig(self, *a, **k)
        torch.Tensor.cpu = counting
        torch.cuda.set_sync_debug_mode("warn")
        try:
            import warnings
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                call()
        finally:
            torch.Tensor.cpu = orig
            torch.cuda.set_sync_debug_mode("default")
        syncs = [w for w in seen if "synchroniz" in str(w.message)]
        assert len(reads) == 2 and len(syncs) <= 2, (reads, [str(w.message) for w in syncs])
