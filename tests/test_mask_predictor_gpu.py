"""The class-selected mask predictor (iif_amd/mmdet_mask_predictor.py on csrc/mask_predictor.hip) against the float64
restatement of tests/mask_predictor_cases.py, which tests/test_mask_predictor_host.py ties to the reference's own FCNMaskHead.

Tolerances (none of them measured on the kernels):
  logits   per element |z - z64| <= (Cin + 2) * 2^-24 * (sum_c |w x| + |b|): the first-order bound of an fp32 sum of Cin products
           plus a bias in any order, with or without FMA.  A bf16 accumulator or a skipped channel breaks it.
  loss     |L - L64| <= 1e-5 * max(1, |L64|), as tests/test_mmdet_mask_gpu.py has it for this loss
  dx, dweight, dbias   max|d - d64| <= 1e-5 * max|d64|, that file's gradient tolerance; the float32 reference itself stays
           within 2.5e-6 (host test), so the margin is at least 4x.  bf16 dx: plus 2^-8 * |d64| per element (one rounding).
"""

import pytest
import torch
import torch.nn.functional as F

from tests import mask_predictor_cases as mpc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24


def _dev(name, bf16=False, grad=True):
    x, w, b, lb, t = mpc.inputs(name)
    x = x.bfloat16() if bf16 else x
    xd = x.to(DEV).requires_grad_(grad)
    wd = w.to(DEV).requires_grad_(grad)
    bd = None if b is None else b.to(DEV).requires_grad_(grad)
    return xd, wd, bd, lb.to(DEV), t.to(DEV)


def _loss_run(name, bf16=False, up=1.0):
    """(loss, dx, dweight [C, Cin], dbias or None) of one forward + backward through (loss * up).sum(), on the CPU."""
    from iif_amd.mmdet_mask_predictor import class_mask_loss
    xd, wd, bd, lb, t = _dev(name, bf16)
    loss = class_mask_loss(xd, wd, bd, lb, t)
    assert loss.shape == (1,) and loss.dtype == torch.float32
    (loss * up).sum().backward()
    assert xd.grad.dtype == xd.dtype and xd.grad.shape == xd.shape and wd.grad.shape == wd.shape
    return (loss.detach().cpu(), xd.grad.cpu(), wd.grad.cpu().reshape(wd.shape[0], wd.shape[1]), None if bd is None else bd.grad.cpu())


def _check_grads(got, ref, scale, bf16, what):
    _, dx, dw, db = got
    lim = 1e-5 * float(ref["dx"].abs().max()) * scale
    err = (dx.double() - ref["dx"] * scale).abs()
    if bf16:
        err = err - 2.0 ** -8 * (ref["dx"] * scale).abs()
    print(what, "dx err / limit %.3f" % (float(err.max()) / lim))
    assert float(err.max()) <= lim, what
    for k, d in (("dweight", dw), ("dbias", db)):
        if d is None:
            continue
        lim = 1e-5 * float(ref[k].abs().max()) * scale
        e = float((d.double() - ref[k] * scale).abs().max())
        print(what, k, "err / limit %.3f" % (e / lim))
        assert e <= lim, (what, k)


CASE_PARAMS = [(n, False) for n in sorted(mpc.CASES)] + [("a", True), ("e", True)]        # the last two: case h


@pytest.mark.parametrize("name,bf16", CASE_PARAMS)
def test_case_against_float64(name, bf16):
    from iif_amd.mmdet_mask_predictor import class_mask_logits
    n, c, cin, h, w = mpc.CASES[name][:5]
    ref = mpc.reference64(name, 1.0, bf16)
    labels = mpc.inputs(name)[3]
    # logits, per element
    xd, wd, bd, lb, _ = _dev(name, bf16, grad=False)
    z = class_mask_logits(xd, wd, bd, lb)
    assert z.shape == (n, 1, h, w) and z.dtype == torch.float32
    zerr = (z.cpu().double()[:, 0] - ref["z"]).abs()
    bound = (cin + 2) * U24 * ref["zabs"]
    print(name, "logit err / bound %.3f" % float((zerr / bound).max()))
    assert bool((zerr <= bound).all())
    # loss and gradients, upstream 1 and 2.5
    one = _loss_run(name, bf16)
    assert abs(float(one[0]) - float(ref["loss"])) <= 1e-5 * max(1.0, abs(float(ref["loss"])))
    _check_grads(one, ref, 1.0, bf16, name)
    up = _loss_run(name, bf16, mpc.UP)
    assert torch.equal(up[0], one[0])
    _check_grads(up, ref, mpc.UP, bf16, name + " x2.5")
    # rows of classes no RoI has: exactly zero
    unsel = ~mpc.selected_rows(labels, c)
    assert not one[2][unsel].any() and (one[3] is None or not one[3][unsel].any())
    assert one[2][~unsel].any(1).all()
    # the same bits from call to call
    again = _loss_run(name, bf16)
    for a, b in zip(one, again):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("name", ["a", "e"])
def test_logits_backward_with_a_random_upstream_gradient(name):
    from iif_amd.mmdet_mask_predictor import class_mask_logits
    n, c, cin, h, w = mpc.CASES[name][:5]
    x, wt, b, labels, _ = mpc.inputs(name)
    gz = torch.randn(n, 1, h, w, generator=torch.Generator().manual_seed(7))
    xd, wd, bd, lb, _ = _dev(name)
    z = class_mask_logits(xd, wd, bd, lb)
    z.backward(gz.to(DEV))
    x64 = x.double().requires_grad_(True)
    w64 = wt.double().reshape(c, cin).requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    z64 = torch.einsum("nc,nchw->nhw", w64[labels], x64) + b64[labels][:, None, None]
    (z64 * gz[:, 0].double()).sum().backward()
    for got, ref in ((xd.grad, x64.grad), (wd.grad.reshape(c, cin), w64.grad), (bd.grad, b64.grad)):
        assert float((got.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    unsel = ~mpc.selected_rows(labels, c)
    assert not wd.grad.cpu()[unsel].any() and not bd.grad.cpu()[unsel].any()
    # gradient for x alone: nothing else is computed
    xd2 = xd.detach().clone().requires_grad_(True)
    class_mask_logits(xd2, wd.detach(), bd.detach(), lb).backward(gz.to(DEV))
    assert torch.equal(xd2.grad, xd.grad)


def test_no_rois():
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor
    m = ClassSelectedMaskPredictor(16, 5).to(DEV)
    x = torch.zeros(0, 16, 6, 6, device=DEV, requires_grad=True)
    lb = torch.zeros(0, dtype=torch.int64, device=DEV)
    loss = m.loss(x, lb, torch.zeros(0, 6, 6, device=DEV))["loss_mask"]
    assert loss.shape == (1,) and float(loss.detach()) == 0
    loss.sum().backward()
    assert x.grad.shape == x.shape
    assert m.weight.grad is not None and not m.weight.grad.any() and m.bias.grad is not None and not m.bias.grad.any()
    z = m(x, lb)
    assert z.shape == (0, 1, 6, 6) and z.requires_grad


def test_labels_outside_the_classes():
    """Labels -1 and C among valid ones: zero loss and a zero dx slice for those RoIs, nothing in dweight / dbias, the divisor
    still N * HW, and the other RoIs exactly as without them."""
    from iif_amd.mmdet_mask_predictor import class_mask_logits, class_mask_loss
    n, c, cin, h, w = mpc.CASES["a"][:5]
    x, wt, b, labels, t = mpc.inputs("a")
    bad = labels.clone()
    bad[1], bad[3] = -1, c
    valid = (bad >= 0) & (bad < c)
    ref = mpc.restate64(x, wt, b, bad, t, 1.0, valid)

    def run(lbs):
        xd, wd, bd, _, td = _dev("a")
        loss = class_mask_loss(xd, wd, bd, lbs.to(DEV), td)
        loss.sum().backward()
        return loss.detach().cpu(), xd.grad.cpu(), wd.grad.cpu().reshape(c, cin), bd.grad.cpu()
    got, good = run(bad), run(labels)
    assert abs(float(got[0]) - float(ref["loss"])) <= 1e-5 * max(1.0, abs(float(ref["loss"])))
    assert not got[1][~valid].any()
    assert torch.equal(got[1][valid], good[1][valid])
    _check_grads(got, ref, 1.0, False, "bad labels")
    unsel = ~mpc.selected_rows(bad, c)
    assert not got[2][unsel].any() and not got[3][unsel].any()
    z = class_mask_logits(x.to(DEV), wt.to(DEV), b.to(DEV), bad.to(DEV)).cpu()
    assert not z[~valid].any() and torch.equal(z[valid], class_mask_logits(x.to(DEV), wt.to(DEV), b.to(DEV), labels.to(DEV)).cpu()[valid])


def test_strided_weight_rows_and_non_contiguous_x():
    from iif_amd.mmdet_mask_predictor import class_mask_loss
    n, c, cin, h, w = mpc.CASES["e"][:5]
    base = _loss_run("e")
    x, wt, b, labels, t = mpc.inputs("e")
    wide = torch.full((c, cin + 7, 1, 1), float("nan"))
    wide[:, :cin] = wt
    wview = wide.to(DEV)[:, :cin].requires_grad_(True)                          # ld_w = Cin + 7
    assert wview.stride(0) == cin + 7
    xnc = x.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2).requires_grad_(True)     # channels_last strides
    assert not xnc.is_contiguous()
    bd = b.to(DEV).requires_grad_(True)
    loss = class_mask_loss(xnc, wview, bd, labels.to(DEV), t.to(DEV))
    loss.sum().backward()
    assert torch.equal(loss.detach().cpu(), base[0]) and torch.equal(xnc.grad.cpu(), base[1])
    assert torch.equal(wview.grad.cpu().reshape(c, cin), base[2]) and torch.equal(bd.grad.cpu(), base[3])
    w2 = wt.reshape(c, cin).to(DEV).requires_grad_(True)                         # [C, Cin] weights
    class_mask_loss(x.to(DEV), w2, b.to(DEV), labels.to(DEV), t.to(DEV)).sum().backward()
    assert w2.grad.shape == (c, cin) and torch.equal(w2.grad.cpu(), base[2])


def test_agrees_with_the_full_convolution_path_on_the_device():
    """mask_cross_entropy(F.conv2d(x, w, b), t, labels): what the package offered before this predictor."""
    from iif_amd.mmdet_mask_loss import mask_cross_entropy
    c, cin = mpc.CASES["c"][1:3]
    new = _loss_run("c")
    xd, wd, bd, lb, t = _dev("c")
    loss = mask_cross_entropy(F.conv2d(xd, wd, bd), t, lb)
    loss.sum().backward()
    assert abs(float(loss) - float(new[0])) <= 2e-5
    for got, old in ((new[1], xd.grad), (new[2], wd.grad.reshape(c, cin)), (new[3], bd.grad)):
        old = old.cpu()
        assert float((got - old).abs().max()) <= 2e-5 * float(old.abs().max())


def test_peak_memory_at_the_lvis_class_count():
    """The point of the feature: one forward + backward at case f stays below HALF the bytes of the full logits alone
    (N * C * HW * 4 = 241 MB); dx, the compact gradient, the scratch and dweight come to about 55 MB."""
    from iif_amd.mmdet_mask_predictor import class_mask_loss
    n, c, cin, h, w = mpc.CASES["f"][:5]
    xd, wd, bd, lb, t = _dev("f")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    class_mask_loss(xd, wd, bd, lb, t).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.1f MB, full logits %.1f MB" % (rise / 1e6, n * c * h * w * 4 / 1e6))
    assert rise < n * c * h * w * 4 / 2


def test_selected_logits_paste_like_the_full_tensor():
    """The test end: [N, 1, h, w] logits through paste_masks(class_agnostic=True) give exactly the masks of the full
    [N, C, h, w] tensor read at det_labels."""
    from iif_amd.mmdet_mask_loss import paste_masks
    from iif_amd.mmdet_mask_predictor import class_mask_logits
    n, c, cin, h, w = mpc.CASES["a"][:5]
    xd, wd, bd, lb, _ = _dev("a", grad=False)
    sel = class_mask_logits(xd, wd, bd, lb)
    full = torch.zeros(n, c, h, w, device=DEV)
    full[torch.arange(n, device=DEV), lb] = sel[:, 0]
    g = torch.Generator().manual_seed(3)
    xy = torch.rand(n, 2, generator=g) * 40
    boxes = torch.cat([xy, xy + 8 + torch.rand(n, 2, generator=g) * 50], 1).to(DEV)
    a = paste_masks(sel, boxes, lb, 96, 112, 0.5, class_agnostic=True)
    b = paste_masks(full, boxes, lb, 96, 112, 0.5)
    assert a.shape == (n, 96, 112) and a.any() and not a.all()
    assert torch.equal(a, b)
