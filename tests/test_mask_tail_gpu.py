"""The fused mask head tail (iif_amd/mmdet_mask_tail.py on csrc/mask_tail.hip) against the float64 restatement of
tests/mask_tail_cases.py, which tests/test_mask_tail_host.py ties to the reference's own FCNMaskHead.

Tolerances (none of them measured on the kernels):
  logits   per element |z - z64| <= (Ci + Co + 4) * 2^-24 * zabs_bound, zabs_bound = sum_co |weight[l, co]| (sum_ci |f up_weight|
           + |up_bias[co]|) + |bias[l]|: the first-order bound of the two nested fp32 sums in any order, with or without FMA; the
           ReLU is 1-Lipschitz and adds nothing.
  loss     |L - L64| <= 1e-5 * max(1, |L64|), the project's tolerance for this loss
  gradients (grid cases, on which no sign of the ReLU's input depends on rounding)   per tensor max|d - d64| <= tol * max|d64|,
           tol = max(1e-5, 4 * e32(case, tensor)): 1e-5 is the project's tolerance for this loss; the second term only keeps the
           4x margin over the float32 reference on case e (mask_tail_cases.e32; the host test prints and bounds it).
           bf16 df: plus 2^-8 * |d64| per element (one rounding).
"""
import pytest
import torch
import torch.nn.functional as F

from tests import mask_tail_cases as mtc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24


def _dev(name, bf16=False, grad=True):
    """(f, up_weight, up_bias, weight, bias, labels, targets) on the device; the five tensors are leaves."""
    f, uw, ub, w, b, lb, t = mtc.inputs(name)
    f = f.bfloat16() if bf16 else f
    leaves = [None if x is None else x.to(DEV).requires_grad_(grad) for x in (f, uw, ub, w, b)]
    return leaves + [lb.to(DEV), t.to(DEV)]


def _grads(leaves):
    f, uw, ub, w, b = leaves
    return dict(df=f.grad.cpu(), dup_weight=uw.grad.cpu(), dup_bias=ub.grad.cpu(), dweight=w.grad.cpu().reshape(w.shape[0], w.shape[1]),
                dbias=None if b is None else b.grad.cpu())


@pytest.fixture(scope="module")
def loss_run():
    """name, bf16, up -> (loss, gradients dict) of one forward + backward through (loss * up).sum(), on the CPU.  Computed once
    per key; a second run for the repeatability check is asked for with again=True."""
    from iif_amd.mmdet_mask_tail import upsampled_class_mask_loss
    cache = {}

    def run(name, bf16=False, up=1.0, again=False):
        key = (name, bf16, up)
        if again or key not in cache:
            a = _dev(name, bf16)
            loss = upsampled_class_mask_loss(*a)
            assert loss.shape == (1,) and loss.dtype == torch.float32
            (loss * up).sum().backward()
            assert a[0].grad.dtype == a[0].dtype and all(x is None or x.grad.shape == x.shape for x in a[:5])
            out = (loss.detach().cpu(), _grads(a[:5]))
            if again:
                return out
            cache[key] = out
        return cache[key]
    return run


def _check_grads(got, ref, name, scale, bf16, what):
    for k in mtc.GRADS:
        d = got[k]
        if d is None:
            continue
        tol = mtc.grad_tol(name, k)
        lim = tol * float(ref[k].abs().max()) * scale
        err = (d.double() - ref[k] * scale).abs()
        if bf16 and k == "df":
            err = err - 2.0 ** -8 * (ref[k] * scale).abs()
        print(what, k, "e32 %.2e tol %.2e err / limit %.3f" % (mtc.e32(name).get(k, 0.0), tol, float(err.max()) / lim))
        assert float(err.max()) <= lim, (what, k)


@pytest.mark.parametrize("name", sorted(mtc.CASES))
def test_logits_and_loss_against_float64(name, loss_run):
    from iif_amd.mmdet_mask_tail import upsampled_class_mask_logits
    n, c, ci, co, h, w = mtc.CASES[name][:6]
    ref = mtc.reference64(name)
    a = _dev(name, grad=False)
    z = upsampled_class_mask_logits(*a[:6])
    assert z.shape == (n, 1, 2 * h, 2 * w) and z.dtype == torch.float32
    zerr = (z.cpu().double()[:, 0] - ref["z"]).abs()
    bound = (ci + co + 4) * U24 * ref["zabs_bound"]
    print(name, "logit err / bound %.3f" % float((zerr / bound).max()))
    assert bool((zerr <= bound).all())
    loss = loss_run(name)[0]
    print(name, "loss err %.2e" % abs(float(loss) - float(ref["loss"])))
    assert abs(float(loss) - float(ref["loss"])) <= 1e-5 * max(1.0, abs(float(ref["loss"])))


@pytest.mark.parametrize("name,bf16", [(n, False) for n in mtc.GRID_CASES] + [("a", True), ("c", True)])
def test_gradients_against_float64(name, bf16, loss_run):
    c = mtc.CASES[name][1]
    ref = mtc.reference64(name)
    labels = mtc.inputs(name)[5]
    one = loss_run(name, bf16)
    assert abs(float(one[0]) - float(ref["loss"])) <= 1e-5 * max(1.0, abs(float(ref["loss"])))
    _check_grads(one[1], ref, name, 1.0, bf16, name)
    up = loss_run(name, bf16, mtc.UP)
    assert torch.equal(up[0], one[0])
    _check_grads(up[1], ref, name, mtc.UP, bf16, name + " x2.5")
    # rows of classes no RoI has: exactly zero
    unsel = ~mtc.selected_rows(labels, c)
    assert not one[1]["dweight"][unsel].any() and (one[1]["dbias"] is None or not one[1]["dbias"][unsel].any())
    assert one[1]["dweight"][~unsel].any(1).all()
    # the same bits from call to call
    again = loss_run(name, bf16, again=True)
    assert torch.equal(one[0], again[0])
    for k in mtc.GRADS:
        assert (one[1][k] is None and again[1][k] is None) or torch.equal(one[1][k], again[1][k]), k


@pytest.mark.parametrize("name", ["a", "g"])
def test_df_alone_equals_the_df_of_the_full_backward(name, loss_run):
    from iif_amd.mmdet_mask_tail import upsampled_class_mask_loss
    a = _dev(name, grad=False)
    a[0].requires_grad_(True)
    upsampled_class_mask_loss(*a).sum().backward()
    assert all(x is None or x.grad is None for x in a[1:5])
    assert torch.equal(a[0].grad.cpu(), loss_run(name)[1]["df"])
    # and the parameters alone
    b = _dev(name)
    f = b[0].detach()
    upsampled_class_mask_loss(f, *b[1:]).sum().backward()
    got = loss_run(name)[1]
    assert torch.equal(b[1].grad.cpu(), got["dup_weight"]) and torch.equal(b[3].grad.cpu().reshape(got["dweight"].shape), got["dweight"])


@pytest.mark.parametrize("name", ["a", "c"])
def test_logits_backward_with_a_random_upstream_gradient(name):
    from iif_amd.mmdet_mask_tail import upsampled_class_mask_logits
    n, c, ci, co, h, w = mtc.CASES[name][:6]
    f, uw, ub, wt, b, labels, _ = mtc.inputs(name)
    gz = torch.randn(n, 1, 2 * h, 2 * w, generator=torch.Generator().manual_seed(7))
    a = _dev(name)
    z = upsampled_class_mask_logits(*a[:6])
    z.backward(gz.to(DEV))
    leaves = [x.double().requires_grad_(True) for x in (f, uw, ub, wt.reshape(c, co), b)]
    y = torch.relu(F.conv_transpose2d(leaves[0], leaves[1], leaves[2], stride=2))
    z64 = torch.einsum("nc,nchw->nhw", leaves[3][labels], y) + leaves[4][labels][:, None, None]
    (z64 * gz[:, 0].double()).sum().backward()
    got = _grads(a[:5])
    for k, ref in zip(mtc.GRADS, leaves):
        e = float((got[k].double() - ref.grad).abs().max())
        print(name, k, "err / limit %.3f" % (e / (1e-5 * float(ref.grad.abs().max()))))
        assert e <= 1e-5 * float(ref.grad.abs().max()), k
    unsel = ~mtc.selected_rows(labels, c)
    assert not got["dweight"][unsel].any() and not got["dbias"][unsel].any()
    # gradient for f alone: nothing else is computed, the same bits
    f2 = a[0].detach().clone().requires_grad_(True)
    upsampled_class_mask_logits(f2, *[x.detach() for x in a[1:5]], a[5]).backward(gz.to(DEV))
    assert torch.equal(f2.grad, a[0].grad)


def test_no_rois():
    from iif_amd.mmdet_mask_tail import FusedMaskHeadTail
    m = FusedMaskHeadTail(16, 8, 5).to(DEV)
    f = torch.zeros(0, 16, 6, 6, device=DEV, requires_grad=True)
    lb = torch.zeros(0, dtype=torch.int64, device=DEV)
    loss = m.loss(f, lb, torch.zeros(0, 12, 12, device=DEV))["loss_mask"]
    assert loss.shape == (1,) and float(loss.detach()) == 0
    loss.sum().backward()
    assert f.grad.shape == f.shape
    for p in m.parameters():
        assert p.grad is not None and not p.grad.any()
    z = m(f, lb)
    assert z.shape == (0, 1, 12, 12) and z.requires_grad


def test_labels_outside_the_classes(loss_run):
    """Labels -1 and C among valid ones: zero loss and a zero df slice for those RoIs, nothing in any parameter gradient, the
    divisor still N * 4hw, and the other RoIs exactly as without them."""
    from iif_amd.mmdet_mask_tail import upsampled_class_mask_logits, upsampled_class_mask_loss
    name = "g"
    n, c = mtc.CASES[name][:2]
    inp = mtc.inputs(name)
    labels = inp[5]
    bad = labels.clone()
    bad[1], bad[3] = -1, c
    valid = (bad >= 0) & (bad < c)
    ref = mtc.restate64(*inp[:5], bad, inp[6], 1.0, valid)
    a = _dev(name)
    loss = upsampled_class_mask_loss(*a[:5], bad.to(DEV), a[6])
    loss.sum().backward()
    got, good = _grads(a[:5]), loss_run(name)[1]
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-5 * max(1.0, abs(float(ref["loss"])))
    assert not got["df"][~valid].any()
    assert torch.equal(got["df"][valid], good["df"][valid])
    _check_grads(got, ref, name, 1.0, False, "bad labels")
    unsel = ~mtc.selected_rows(bad, c)
    assert not got["dweight"][unsel].any() and not got["dbias"][unsel].any()
    b = _dev(name, grad=False)
    z = upsampled_class_mask_logits(*b[:5], bad.to(DEV)).cpu()
    assert not z[~valid].any() and torch.equal(z[valid], upsampled_class_mask_logits(*b[:6]).cpu()[valid])


def test_non_contiguous_f_and_strided_weight_rows(loss_run):
    from iif_amd.mmdet_mask_tail import upsampled_class_mask_loss
    name = "c"
    n, c, ci, co = mtc.CASES[name][:4]
    base = loss_run(name)
    f, uw, ub, wt, b, labels, t = mtc.inputs(name)
    wide = torch.full((c, co + 7, 1, 1), float("nan"))
    wide[:, :co] = wt
    wview = wide.to(DEV)[:, :co].requires_grad_(True)                           # ld_w = Co + 7
    assert wview.stride(0) == co + 7
    fnc = f.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2).requires_grad_(True)      # channels_last strides
    assert not fnc.is_contiguous()
    rest = [x.to(DEV).requires_grad_(True) for x in (uw, ub, b)]
    loss = upsampled_class_mask_loss(fnc, rest[0], rest[1], wview, rest[2], labels.to(DEV), t.to(DEV))
    loss.sum().backward()
    assert torch.equal(loss.detach().cpu(), base[0]) and torch.equal(fnc.grad.cpu(), base[1]["df"])
    assert torch.equal(rest[0].grad.cpu(), base[1]["dup_weight"]) and torch.equal(rest[1].grad.cpu(), base[1]["dup_bias"])
    assert torch.equal(wview.grad.cpu().reshape(c, co), base[1]["dweight"]) and torch.equal(rest[2].grad.cpu(), base[1]["dbias"])


def test_agrees_with_the_composed_path_on_the_device(loss_run):
    """class_mask_loss(relu(conv_transpose2d(f, ...)), ...): what the package offered before this feature."""
    from iif_amd.mmdet_mask_predictor import class_mask_loss
    new = loss_run("g")
    a = _dev("g")
    loss = class_mask_loss(torch.relu(F.conv_transpose2d(a[0], a[1], a[2], stride=2)), a[3], a[4], a[5], a[6])
    loss.sum().backward()
    assert abs(float(loss.detach()) - float(new[0])) <= 2e-5
    old = _grads(a[:5])
    for k in mtc.GRADS:
        e = float((new[1][k] - old[k]).abs().max())
        print(k, "fused - composed / limit %.3f" % (e / (2e-5 * float(old[k].abs().max()))))
        assert e <= 2e-5 * float(old[k].abs().max()), k


def test_peak_memory_stays_below_one_upsampled_tensor():
    """The point of the feature: at case e one forward + backward - df, the sign bits, the dup_weight partials and every other
    scratch included - rises by less than the bytes of ONE [N, Co, 2h, 2w] float32 tensor (56.2 MB); the composed path holds at
    least two (the activation and its gradient)."""
    from iif_amd.mmdet_mask_tail import upsampled_class_mask_loss
    n, c, ci, co, h, w = mtc.CASES["e"][:6]
    a = _dev("e")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    upsampled_class_mask_loss(*a).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    one = n * co * 4 * h * w * 4
    print("peak rise %.1f MB, one upsampled tensor %.1f MB" % (rise / 1e6, one / 1e6))
    assert rise < one


def test_fused_logits_paste_like_the_composed_logits():
    """The test end: the fused [N, 1, 2h, 2w] logits through paste_masks(class_agnostic=True) give exactly the masks of the
    composed path's logits pasted the same way."""
    from iif_amd.mmdet_mask_loss import paste_masks
    from iif_amd.mmdet_mask_predictor import class_mask_logits
    from iif_amd.mmdet_mask_tail import FusedMaskHeadTail
    n = mtc.CASES["a"][0]
    f, uw, ub, w, b, lb, _ = _dev("a", grad=False)
    m = FusedMaskHeadTail(f.shape[1], uw.shape[1], w.shape[0]).to(DEV)
    m.load_state_dict({"upsample.weight": uw, "upsample.bias": ub, "conv_logits.weight": w, "conv_logits.bias": b})
    with torch.no_grad():
        fused = m(f, lb)
        composed = class_mask_logits(torch.relu(F.conv_transpose2d(f, uw, ub, stride=2)), w, b, lb)
    g = torch.Generator().manual_seed(3)
    xy = torch.rand(n, 2, generator=g) * 40
    boxes = torch.cat([xy, xy + 8 + torch.rand(n, 2, generator=g) * 50], 1).to(DEV)
    pa = paste_masks(fused, boxes, lb, 96, 112, 0.5, class_agnostic=True)
    pb = paste_masks(composed, boxes, lb, 96, 112, 0.5, class_agnostic=True)
    assert pa.shape == (n, 96, 112) and pa.any() and not pa.all()
    assert torch.equal(pa, pb)
