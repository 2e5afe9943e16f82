"""``valid_rows=True`` of the class-selected mask predictor and of the fused mask head tail, and ``mask_head_loss``, on the MI355X.

The padded batches of tests/mask_valid_rows_cases.py are existing cases with invalid rows (labels ``C, -1, C + 5, 2**40``, NaN
contents) in front, in the middle and at the end; the float64 reference is the case's own ``reference64`` - ``restate64`` on the
compacted rows, divisor ``K * H * W``.

Tolerances: the ones the existing GPU tests hold the same quantities to (none of them measured on the kernels):
  loss                 |L - L64| <= 1e-5 * max(1, |L64|)
  predictor gradients  max|d - d64| <= 1e-5 * max|d64|; bf16 dx: plus 2^-8 * |d64| per element (one rounding)
  tail gradients       mask_tail_cases.grad_tol = max(1e-5, 4 * e32), e32 the float32 reference path's own error; bf16 df as above
  normed predictor     normed_mask_predictor_cases.GPU_TOLERANCE (4x the float32 reference's error)
  upstream factor      UP = 2.5
"""
import pytest
import torch
import torch.nn as nn

from tests import mask_predictor_cases as mpc
from tests import mask_tail_cases as mtc
from tests import mask_valid_rows_cases as vc
from tests import normed_mask_predictor_cases as nk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UP = mpc.UP
assert mtc.UP == UP


def _leaf(t, bf16=False):
    if t is None:
        return None
    return (t.bfloat16() if bf16 else t).to(DEV).requires_grad_(True)


def _pred_run(batch, bf16=False, up=1.0, valid_rows=True):
    """(loss, dx, dweight [C, Cin], dbias or None) on the CPU of one forward + backward through (loss * up).sum()."""
    from iif_amd.mmdet_mask_predictor import class_mask_loss
    x, w, b, lb, t = batch[:5]
    xd, wd, bd = _leaf(x, bf16), _leaf(w), _leaf(b)
    loss = class_mask_loss(xd, wd, bd, lb.to(DEV), t.to(DEV), valid_rows=valid_rows)
    assert loss.shape == (1,) and loss.dtype == torch.float32
    (loss * up).sum().backward()
    assert xd.grad.dtype == xd.dtype and xd.grad.shape == xd.shape
    return loss.detach().cpu(), xd.grad.cpu(), wd.grad.cpu().reshape(w.shape[0], w.shape[1]), None if bd is None else bd.grad.cpu()


def _tail_run(batch, bf16=False, up=1.0, valid_rows=True):
    """(loss, dict of the five gradients) on the CPU."""
    from iif_amd.mmdet_mask_tail import upsampled_class_mask_loss
    f, uw, ub, w, b, lb, t = batch[:7]
    leaves = [_leaf(f, bf16), _leaf(uw), _leaf(ub), _leaf(w), _leaf(b)]
    loss = upsampled_class_mask_loss(*leaves, lb.to(DEV), t.to(DEV), valid_rows=valid_rows)
    assert loss.shape == (1,) and loss.dtype == torch.float32
    (loss * up).sum().backward()
    g = [None if v is None else v.grad.cpu() for v in leaves]
    assert g[0].dtype == leaves[0].dtype and g[0].shape == f.shape
    return loss.detach().cpu(), dict(df=g[0], dup_weight=g[1], dup_bias=g[2], dweight=g[3].reshape(w.shape[0], w.shape[1]), dbias=g[4])


def _same_bits(a, b):
    if isinstance(a, dict):
        return all(_same_bits(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return all(_same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(
        torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def _finite(*ts):
    return all(t is None or bool(torch.isfinite(t.float()).all()) for t in ts)


def _check_loss(loss, ref, what):
    e, lim = abs(float(loss) - float(ref["loss"])), 1e-5 * max(1.0, abs(float(ref["loss"])))
    print(what, "loss err / limit %.3f" % (e / lim))
    assert e <= lim, what


def _check_one(d, r, tol, scale, bf16_rounding, what):
    lim = tol * float(r.abs().max()) * scale
    err = (d.double() - r * scale).abs()
    if bf16_rounding:
        err = err - 2.0 ** -8 * (r * scale).abs()
    print(what, "err / limit %.3f" % (float(err.max()) / lim))
    assert float(err.max()) <= lim, what


def _check_pred(got, ref, valid, scale, bf16, what, tol=None):
    """got of a padded batch against the reference of its compacted rows; the invalid rows' dx slices are exact zeros."""
    tol = tol or dict(dx=1e-5, dweight=1e-5, dbias=1e-5)
    _, dx, dw, db = got
    assert _finite(got[0], dx, dw, db), what
    assert not dx[~valid].any(), what
    _check_one(dx[valid], ref["dx"], tol["dx"], scale, bf16, what + " dx")
    _check_one(dw, ref["dweight"], tol["dweight"], scale, False, what + " dweight")
    if db is not None:
        _check_one(db, ref["dbias"], tol["dbias"], scale, False, what + " dbias")


def _check_tail(got, ref, valid, tol, scale, bf16, what):
    g = got[1]
    assert _finite(got[0], *g.values()), what
    assert not g["df"][~valid].any(), what
    for k in mtc.GRADS:
        if g[k] is None:
            continue
        d = g[k][valid] if k == "df" else g[k]
        _check_one(d, ref[k], tol(k), scale, bf16 and k == "df", what + " " + k)


# ---------------------------------------------------------------------------------- 1. every padded case against float64
@pytest.mark.parametrize("name,bf16", [(n, False) for n in vc.PREDICTOR_CASES] + [("a", True), ("e", True)])
def test_predictor_padded_case_against_float64_on_the_compacted_rows(name, bf16):
    batch = vc.predictor_batch(name)
    valid = batch[5]
    ref = mpc.reference64(name, 1.0, bf16)
    one = _pred_run(batch, bf16)
    _check_loss(one[0], ref, name)
    _check_pred(one, ref, valid, 1.0, bf16, name)
    up = _pred_run(batch, bf16, UP)
    assert torch.equal(up[0], one[0])
    _check_pred(up, ref, valid, UP, bf16, name + " x2.5")
    unsel = ~mpc.selected_rows(batch[3], batch[1].shape[0])
    assert not one[2][unsel].any() and (one[3] is None or not one[3][unsel].any())


@pytest.mark.parametrize("name,bf16", [(n, False) for n in vc.TAIL_CASES] + [("a", True), ("c", True)])
def test_tail_padded_case_against_float64_on_the_compacted_rows(name, bf16):
    batch = vc.tail_batch(name)
    valid = batch[7]
    ref = mtc.reference64(name)
    tol = lambda k: mtc.grad_tol(name, k)                                        # noqa: E731
    one = _tail_run(batch, bf16)
    _check_loss(one[0], ref, name)
    _check_tail(one, ref, valid, tol, 1.0, bf16, name)
    up = _tail_run(batch, bf16, UP)
    assert torch.equal(up[0], one[0])
    _check_tail(up, ref, valid, tol, UP, bf16, name + " x2.5")
    unsel = ~mtc.selected_rows(batch[5], batch[3].shape[0])
    assert not one[1]["dweight"][unsel].any() and (one[1]["dbias"] is None or not one[1]["dbias"][unsel].any())


# ---------------------------------------------------------------------------------- 2. exact invariance
@pytest.mark.parametrize("name,bf16", [("a", False), ("e", False), ("e", True)])
def test_predictor_invalid_rows_contents_change_no_bit(name, bf16):
    nan, other = _pred_run(vc.predictor_batch(name), bf16, UP), _pred_run(vc.predictor_batch(name, -3.25), bf16, UP)
    assert _same_bits(nan, other)
    assert _same_bits(nan, _pred_run(vc.predictor_batch(name), bf16, UP))       # and the same bits from call to call


@pytest.mark.parametrize("name,bf16", [("a", False), ("c", False), ("c", True)])
def test_tail_invalid_rows_contents_change_no_bit(name, bf16):
    nan, other = _tail_run(vc.tail_batch(name), bf16, UP), _tail_run(vc.tail_batch(name, -3.25), bf16, UP)
    assert _same_bits(nan, other)
    assert _same_bits(nan, _tail_run(vc.tail_batch(name), bf16, UP))


# ---------------------------------------------------------------------------------- 3. the device count
@pytest.mark.parametrize("count", sorted(vc.COUNT_CASES))
def test_predictor_device_count(count):
    batch = vc.predictor_count_batch(count)
    valid, ref = batch[5], batch[6]
    got = _pred_run(batch, False, UP)
    if ref is None:                                                             # no valid row: exactly zero, nothing NaN
        assert got[0].view(torch.int32).item() == 0
        assert all(not g.any() and _finite(g) for g in got[1:])
        return
    _check_loss(got[0], ref, count)
    _check_pred(got, ref, valid, UP, False, count)


@pytest.mark.parametrize("count", sorted(vc.COUNT_CASES))
def test_tail_device_count(count):
    batch = vc.tail_count_batch(count)
    valid, ref, tol = batch[7], batch[8], batch[9]
    got = _tail_run(batch, False, UP)
    if ref is None:
        assert got[0].view(torch.int32).item() == 0
        assert all(not g.any() and _finite(g) for g in got[1].values())
        return
    _check_loss(got[0], ref, count)
    _check_tail(got, ref, valid, lambda k: tol[k], UP, False, count)


# ---------------------------------------------------------------------------------- 4. no padding
def test_predictor_without_padding_both_modes_agree():
    name = vc.NOPAD_PREDICTOR
    batch = mpc.inputs(name)
    ref = mpc.reference64(name)
    everyone = torch.ones(batch[0].shape[0], dtype=torch.bool)
    on, off = _pred_run(batch, False, UP, True), _pred_run(batch, False, UP, False)
    _check_loss(on[0], ref, name)
    _check_pred(on, ref, everyone, UP, False, name)
    assert abs(float(on[0]) - float(off[0])) <= 1e-5 * max(1.0, abs(float(ref["loss"])))
    for a, b, k in zip(on[1:], off[1:], ("dx", "dweight", "dbias")):
        assert float((a.double() - b.double()).abs().max()) <= 1e-5 * float(ref[k].abs().max()) * UP, k


def test_tail_without_padding_both_modes_agree():
    name = vc.NOPAD_TAIL
    batch = mtc.inputs(name)
    ref = mtc.reference64(name)
    everyone = torch.ones(batch[0].shape[0], dtype=torch.bool)
    tol = lambda k: mtc.grad_tol(name, k)                                        # noqa: E731
    on, off = _tail_run(batch, False, UP, True), _tail_run(batch, False, UP, False)
    _check_loss(on[0], ref, name)
    _check_tail(on, ref, everyone, tol, UP, False, name)
    assert abs(float(on[0]) - float(off[0])) <= 1e-5 * max(1.0, abs(float(ref["loss"])))
    for k in mtc.GRADS:
        assert float((on[1][k].double() - off[1][k].double()).abs().max()) <= tol(k) * float(ref[k].abs().max()) * UP, k


# ---------------------------------------------------------------------------------- 5. the class_agnostic modules
AGNOSTIC_CLASSES = 5


def _agnostic_labels(valid):
    """A label in [0, num_classes) on every valid row (all of them select row 0), num_classes on the padded rows."""
    lb = torch.full((valid.numel(),), AGNOSTIC_CLASSES, dtype=torch.int64)
    lb[valid] = torch.arange(int(valid.sum())) % AGNOSTIC_CLASSES
    return lb


@pytest.mark.parametrize("normed", [False, True])
def test_class_agnostic_predictor_modules(normed):
    """Cases g (C = 1, no bias: the modules' zero-initialised bias) of the plain and of the normed predictor."""
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor, class_mask_loss
    from iif_amd.mmdet_normed_mask_predictor import ClassSelectedNormedMaskPredictor, normed_class_mask_loss
    cases = nk if normed else mpc
    x, w, b, _, t = cases.inputs("g")
    assert b is None and w.shape[0] == 1
    ref = cases.reference64("g")
    valid = vc.layout(x.shape[0])
    lb = _agnostic_labels(valid).to(DEV)
    if normed:
        temp, q, eps = nk.cfg("g")
        m = ClassSelectedNormedMaskPredictor(w.shape[1], AGNOSTIC_CLASSES, class_agnostic=True, tempearture=temp, power=q, eps=eps)
    else:
        m = ClassSelectedMaskPredictor(w.shape[1], AGNOSTIC_CLASSES, class_agnostic=True)
    m = m.to(DEV)
    with torch.no_grad():
        m.weight.copy_(w.to(DEV))
    xp, tp = vc._spread(x, valid, float("nan")), vc._spread(t, valid, float("nan"))
    xd = xp.to(DEV).requires_grad_(True)
    loss = m.loss(xd, lb, tp.to(DEV), valid_rows=True)["loss_mask"]
    (loss * UP).sum().backward()
    got = (loss.detach().cpu(), xd.grad.cpu(), m.weight.grad.cpu().reshape(1, -1), m.bias.grad.cpu())
    tol = nk.GPU_TOLERANCE if normed else None
    e, lim = abs(float(got[0]) - float(ref["loss"])), (tol["loss"] if normed else 1e-5) * max(1.0, abs(float(ref["loss"])))
    assert e <= lim
    _check_pred(got, ref, valid, UP, False, "agnostic normed" if normed else "agnostic", tol)
    # without valid_rows: as today - every label selects row 0, the padded rows included, and the divisor is N * H * W
    x0, t0 = vc._spread(x, valid, 0.0).to(DEV), vc._spread(t, valid, 0.0).to(DEV)
    with torch.no_grad():
        today = m.loss(x0, lb, t0)["loss_mask"]
        if normed:
            want = normed_class_mask_loss(x0, m.weight, m.bias, torch.zeros_like(lb), t0, temp, q, eps)
        else:
            want = class_mask_loss(x0, m.weight, m.bias, torch.zeros_like(lb), t0)
    assert torch.equal(today, want)


def test_class_agnostic_fused_tail_module():
    from iif_amd.mmdet_mask_tail import FusedMaskHeadTail, upsampled_class_mask_loss
    name = "f"
    f, uw, ub, w, b, _, t = mtc.inputs(name)
    assert b is None and w.shape[0] == 1
    ref = mtc.reference64(name)
    valid = vc.layout(f.shape[0])
    lb = _agnostic_labels(valid).to(DEV)
    m = FusedMaskHeadTail(f.shape[1], uw.shape[1], AGNOSTIC_CLASSES, class_agnostic=True).to(DEV)
    m.load_state_dict({"upsample.weight": uw, "upsample.bias": ub, "conv_logits.weight": w, "conv_logits.bias": torch.zeros(1)})
    fd = vc._spread(f, valid, float("nan")).to(DEV).requires_grad_(True)
    loss = m.loss(fd, lb, vc._spread(t, valid, float("nan")).to(DEV), valid_rows=True)["loss_mask"]
    (loss * UP).sum().backward()
    grads = dict(df=fd.grad.cpu(), dup_weight=m.upsample.weight.grad.cpu(), dup_bias=m.upsample.bias.grad.cpu(),
                 dweight=m.conv_logits.weight.grad.cpu().reshape(1, -1), dbias=m.conv_logits.bias.grad.cpu())
    _check_loss(loss.detach().cpu(), ref, "agnostic tail")
    _check_tail((loss.detach().cpu(), grads), ref, valid, lambda k: mtc.grad_tol(name, k), UP, False, "agnostic tail")
    f0, t0 = vc._spread(f, valid, 0.0).to(DEV), vc._spread(t, valid, 0.0).to(DEV)
    with torch.no_grad():
        today = m.loss(f0, lb, t0)["loss_mask"]
        want = upsampled_class_mask_loss(f0, *m._args(), torch.zeros_like(lb), t0)
    assert torch.equal(today, want)


# ---------------------------------------------------------------------------------- 6. mask_head_loss is the two calls
def _rows_and_masks(k, num_classes, seed):
    """k padded rows over two images (the second row block padded): pos_rois [k, 5], pos_gt_inds, pos_labels, the gt masks."""
    g = torch.Generator().manual_seed(seed)
    masks = [(torch.rand(m, 48, 64, generator=g) < 0.5).to(torch.uint8).to(DEV) for m in (3, 2)]
    img = torch.tensor([0, 0, -1, 1, 1, -1, 0, -1][:k], dtype=torch.float32)
    xy = torch.rand(k, 2, generator=g) * 20
    rois = torch.cat([img[:, None], xy, xy + 8 + torch.rand(k, 2, generator=g) * 20], 1)
    pad = img < 0
    rois[pad, 1:] = 0
    gt = torch.where(pad, torch.full((k,), -1), torch.randint(0, 2, (k,), generator=g))
    lb = torch.where(pad, torch.full((k,), num_classes), torch.randint(0, num_classes, (k,), generator=g))
    return rois.to(DEV), gt.to(DEV), lb.to(DEV), masks


@pytest.mark.parametrize("kind", ["tail", "plain", "normed"])
def test_mask_head_loss_is_targets_then_loss_bit_for_bit(kind):
    from iif_amd.mmdet_mask_head_loss import mask_head_loss
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor
    from iif_amd.mmdet_mask_tail import FusedMaskHeadTail
    from iif_amd.mmdet_mask_target import mask_targets_padded
    from iif_amd.mmdet_normed_mask_predictor import ClassSelectedNormedMaskPredictor
    c, k = 4, 8
    torch.manual_seed(11)
    m = {"tail": lambda: FusedMaskHeadTail(8, 8, c), "plain": lambda: ClassSelectedMaskPredictor(8, c),
         "normed": lambda: ClassSelectedNormedMaskPredictor(8, c)}[kind]().to(DEV)
    side = 7 if kind == "tail" else 14
    rois, gt, lb, masks = _rows_and_masks(k, c, 5)
    feats = torch.randn(k, 8, side, side, generator=torch.Generator().manual_seed(6)).to(DEV)
    feats[lb == c] = float("nan")

    def run(call):
        m.zero_grad()
        fd = feats.clone().requires_grad_(True)
        out = call(fd)
        assert set(out) == {"loss_mask"}
        out["loss_mask"].sum().backward()
        return (out["loss_mask"].detach().cpu(), fd.grad.cpu()) + tuple(p.grad.cpu().clone() for p in m.parameters())
    one = run(lambda fd: mask_head_loss(m, fd, rois, gt, lb, masks, 14))
    two = run(lambda fd: m.loss(fd, lb, mask_targets_padded(rois, gt, masks, 14), valid_rows=True))
    assert _same_bits(one, two)
    assert _finite(*one) and float(one[0]) > 0 and not one[1][(lb == c).cpu()].any() and one[1].any()


# ---------------------------------------------------------------------------------- 7. the chain without a host read
def test_the_padded_chain_makes_no_host_read():
    """roi_stage_targets_padded (two images, one without ground truth) -> SingleRoIExtractor on pos_rois -> one nn.Conv2d ->
    mask_head_loss -> backward, under torch's sync debug mode ('error'), with FusedMaskHeadTail and once more with
    ClassSelectedMaskPredictor.  The loss is then compared with the module's loss on the compacted rows."""
    import numpy as np
    from iif_amd.mmdet_mask_head_loss import mask_head_loss
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor
    from iif_amd.mmdet_mask_tail import FusedMaskHeadTail
    from iif_amd.mmdet_mask_target import mask_targets_padded
    from iif_amd.mmdet_roi_extractor import SingleRoIExtractor
    from iif_amd.mmdet_roi_stage import roi_stage_targets_padded
    from iif_amd.mmdet_assigner import MaxIoUAssigner
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler
    from tests import roi_stage_cases as rc
    from tests import targets_cases as tc
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    dev = torch.device(DEV)
    H, W = rc.IMG
    p0, g0 = rc.image_boxes(40, 5, 7700)
    p1, _ = rc.image_boxes(40, 0, 7710)
    props = torch.from_numpy(np.stack([p0, p1])).to(dev)
    gts = [torch.from_numpy(np.array(g0)).to(dev), torch.zeros(0, 4, device=dev)]
    labs = [torch.from_numpy(rc._u(5, 7720, rc.NUM_CLASSES)).to(dev), torch.zeros(0, dtype=torch.int64, device=dev)]
    gen = torch.Generator().manual_seed(8)
    masks = [(torch.rand(5, H, W, generator=gen) < 0.5).to(torch.uint8).to(dev), torch.zeros(0, H, W, dtype=torch.uint8, device=dev)]
    pos, neg, min_pos, assign_all, _, _, mlq = rc.RCNN
    asg = MaxIoUAssigner(pos, neg, min_pos_iou=min_pos, gt_max_assign_all=assign_all, match_low_quality=mlq)
    smp, coder = RandomSampler(32, 0.25, neg_pos_ub=-1, add_gt_as_proposals=True), DeltaXYWHBBoxCoder(tc.MEANS[0], tc.STDS[1])
    strides = [4, 8, 16, 32]
    levels = [torch.randn(2, 8, -(-H // s), -(-W // s), generator=gen).to(dev).requires_grad_(True) for s in strides]
    ext = SingleRoIExtractor(dict(type='RoIAlign', output_size=14, sampling_ratio=0), 8, strides)
    torch.manual_seed(12)
    conv = nn.Conv2d(8, 8, 3, padding=1).to(dev)
    heads = [(FusedMaskHeadTail(8, 8, rc.NUM_CLASSES).to(dev), 28), (ClassSelectedMaskPredictor(8, rc.NUM_CLASSES).to(dev), 14)]

    def chain(head, size):
        t = roi_stage_targets_padded(props, None, gts, labs, asg, smp, coder, rc.NUM_CLASSES)
        feats = torch.relu(conv(ext(levels, t.pos_rois)))
        loss = mask_head_loss(head, feats, t.pos_rois, t.pos_gt_inds, t.pos_labels, masks, size)["loss_mask"]
        loss.sum().backward()
        return t, feats.detach(), loss.detach()
    for head, size in heads:                             # the library and the convolution's plans are loaded before the mode is on
        chain(head, size)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    results = []
    for head, size in heads:
        for p in list(head.parameters()) + list(conv.parameters()) + levels:
            p.grad = None
        torch.cuda.set_sync_debug_mode("error")
        try:
            t, feats, loss = chain(head, size)
        finally:
            torch.cuda.set_sync_debug_mode(before)
        torch.cuda.synchronize()
        results.append((head, size, t, feats, loss))
    assert torch.cuda.get_sync_debug_mode() == before
    for head, size, t, feats, loss in results:
        real = t.pos_labels < rc.NUM_CLASSES
        k = int(real.sum())
        assert t.pos_rois.shape[0] == 16 and 0 < k < 16 and bool((t.pos_rois[~real, 0] == -1).all())
        assert not bool(real[8:].any())                                         # the image without ground truth has no positive
        assert _finite(loss, conv.weight.grad, *[lv.grad for lv in levels], *[p.grad for p in head.parameters()])
        assert float(loss) > 0 and bool(conv.weight.grad.any()) and bool(levels[0].grad.any() or levels[1].grad.any())
        with torch.no_grad():
            targets = mask_targets_padded(t.pos_rois, t.pos_gt_inds, masks, size)
            want = head.loss(feats[real], t.pos_labels[real], targets[real])["loss_mask"]
        assert abs(float(loss) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
