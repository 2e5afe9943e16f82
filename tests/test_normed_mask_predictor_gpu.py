"""The class-selected NormedConv2d mask predictor (iif_amd/mmdet_normed_mask_predictor.py on csrc/normed_mask_predictor.hip)
against the float64 restatement of tests/normed_mask_predictor_cases.py, which tests/test_normed_mask_predictor_host.py ties to
the reference's own FCNMaskHead(predictor_cfg=dict(type='NormedConv2d', tempearture=20)).

Tolerances (none of them measured on the kernels):
  logits   per element |z - z64| <= ((1 + q)(Cin + 2) + 16) * 2^-24 * s_x s_w sum_c |w x| + 2 * 2^-24 * (|bias| + |z64|): the
           first-order bound of the fp32 dot product plus the two norms.  The float32 torch-CPU reference sits at 0.023 of it at
           most (host test), far within the half that the bound's constant needs: the constant is not widened.
  loss, dx, dweight, dbias   4x the float32 reference's own worst error over these cases, relative to the largest element of
           the quantity (the loss: to max(1, |loss|)).  The host test measures that error: loss 8.55e-8, dx 5.07e-7,
           dweight 5.47e-7, dbias 1.10e-6, recorded (rounded up) as normed_mask_predictor_cases.F32_REFERENCE_ERROR; the
           tolerances are therefore loss 3.44e-7, dx 2.04e-6, dweight 2.2e-6, dbias 4.44e-6.
           bf16 x: plus 2^-8 * |d64| per element of dx (one rounding).
  Case i (pixels that are zero in every channel, where dx = g * (T / eps) * what is 1e6 times the rest): dx is checked on those
  pixels and on the others separately, each against its own largest element - relative to the whole it would say nothing about
  the others.
"""

import pytest
import torch

from tests import normed_mask_predictor_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = K.GPU_TOLERANCE


def _dev(name, bf16=False, grad=True):
    x, w, b, lb, t = K.inputs(name)
    x = x.bfloat16() if bf16 else x
    xd = x.to(DEV).requires_grad_(grad)
    wd = w.to(DEV).requires_grad_(grad)
    bd = None if b is None else b.to(DEV).requires_grad_(grad)
    return xd, wd, bd, lb.to(DEV), t.to(DEV)


def _kw(name):
    t, q, eps = K.cfg(name)
    return dict(tempearture=t, power=q, eps=eps)


def _run(xd, wd, bd, lb, t, up=1.0, **kw):
    """(loss, dx, dweight [C, Cin], dbias or None) of one forward + backward through (loss * up).sum(), on the CPU."""
    from iif_amd.mmdet_normed_mask_predictor import normed_class_mask_loss
    loss = normed_class_mask_loss(xd, wd, bd, lb, t, **kw)
    assert loss.shape == (1,) and loss.dtype == torch.float32
    (loss * up).sum().backward()
    assert xd.grad.dtype == xd.dtype and xd.grad.shape == xd.shape and wd.grad.shape == wd.shape
    return (loss.detach().cpu(), xd.grad.cpu(), wd.grad.cpu().reshape(wd.shape[0], wd.shape[1]), None if bd is None else bd.grad.cpu())


def _loss_run(name, bf16=False, up=1.0):
    return _run(*_dev(name, bf16), up=up, **_kw(name))


def _check_dx(dx, ref, scale, bf16, what, mask=None):
    want = ref * scale
    err = (dx.double() - want).abs()
    if bf16:
        err = err - 2.0 ** -8 * want.abs()
    if mask is not None:
        err, want = err[mask], want[mask]
    lim = TOL["dx"] * float(want.abs().max())
    print(what, "dx err / limit %.3f" % (float(err.max()) / lim))
    assert float(err.max()) <= lim, what


def _check_grads(got, ref, scale, bf16, what, zero_pixels=None):
    _, dx, dw, db = got
    assert all(bool(torch.isfinite(d).all()) for d in (dx.float(), dw) + (() if db is None else (db,)))
    if zero_pixels is None:
        _check_dx(dx, ref["dx"], scale, bf16, what)
    else:
        m = zero_pixels[:, None].expand_as(dx)
        _check_dx(dx, ref["dx"], scale, bf16, what + " zero pixels", m)
        _check_dx(dx, ref["dx"], scale, bf16, what + " other pixels", ~m)
    for k, d in (("dweight", dw), ("dbias", db)):
        if d is None:
            continue
        lim = TOL[k] * float(ref[k].abs().max()) * scale
        e = float((d.double() - ref[k] * scale).abs().max())
        print(what, k, "err / limit %.3f" % (e / lim))
        assert e <= lim, (what, k)


def _check_loss(loss, ref, what):
    e = abs(float(loss) - float(ref["loss"]))
    lim = TOL["loss"] * max(1.0, abs(float(ref["loss"])))
    print(what, "loss err / limit %.3f" % (e / lim))
    assert e <= lim, what


CASE_PARAMS = [(n, False) for n in sorted(K.CASES)] + [("a", True), ("e", True)]


@pytest.mark.parametrize("name,bf16", CASE_PARAMS)
def test_case_against_float64(name, bf16):
    from iif_amd.mmdet_normed_mask_predictor import normed_class_mask_logits
    n, c, cin, h, w = K.CASES[name][:5]
    ref = K.reference64(name, 1.0, bf16)
    x, _, _, labels, _ = K.inputs(name)
    zero_pixels = (x.abs().sum(1) == 0) if K.CASES[name][10] else None
    assert zero_pixels is None or int(zero_pixels.sum()) == len(K.ZERO_PIXELS)
    # logits, per element
    xd, wd, bd, lb, _ = _dev(name, bf16, grad=False)
    z = normed_class_mask_logits(xd, wd, bd, lb, **_kw(name))
    assert z.shape == (n, 1, h, w) and z.dtype == torch.float32 and bool(torch.isfinite(z).all())
    zerr = (z.cpu().double()[:, 0] - ref["z"]).abs()
    bound = K.logit_bound(ref, cin, K.cfg(name)[1])
    print(name, "logit err / bound %.3f" % float((zerr / bound).max()))
    assert bool((zerr <= bound).all())
    # loss and gradients, upstream 1 and 2.5
    one = _loss_run(name, bf16)
    _check_loss(one[0], ref, name)
    _check_grads(one, ref, 1.0, bf16, name, zero_pixels)
    up = _loss_run(name, bf16, K.UP)
    assert torch.equal(up[0], one[0])
    _check_grads(up, ref, K.UP, bf16, name + " x2.5", zero_pixels)
    # rows of classes no RoI has: exactly zero
    unsel = ~K.selected_rows(labels, c)
    assert not one[2][unsel].any() and (one[3] is None or not one[3][unsel].any())
    assert one[2][~unsel].any(1).all()
    # the same bits from call to call
    again = _loss_run(name, bf16)
    for a, b in zip(one, again):
        assert (a is None and b is None) or torch.equal(a, b)


def test_zero_pixels_take_the_subgradient_form():
    """Case i: at a pixel that is zero in every channel dx = g * s_x * what with s_x = T / eps, the B term exactly 0."""
    x, wt, b, labels, t = K.inputs("i")
    temp, q, eps = K.cfg("i")
    n, c, cin, h, w = K.CASES["i"][:5]
    _, dx, _, _ = _loss_run("i")
    for r, y, xx in K.ZERO_PIXELS:
        wl = wt[labels[r], :, 0, 0].double()
        what = wl / (wl.norm() + eps)
        g = (torch.sigmoid(b[labels[r]].double()) - t[r, y, xx].double()) / (n * h * w)       # z = bias there
        want = g * (temp / eps) * what
        assert float((dx[r, :, y, xx].double() - want).abs().max()) <= TOL["dx"] * float(want.abs().max())


@pytest.mark.parametrize("name", ["a", "e", "h"])
def test_logits_backward_with_a_random_upstream_gradient(name):
    """The logits function alone, differentiated through a random gz against float64 autograd of the restated logits; the same
    kernels and therefore the same gradient tolerances as the loss."""
    from iif_amd.mmdet_normed_mask_predictor import normed_class_mask_logits
    n, c, cin, h, w = K.CASES[name][:5]
    temp, q, eps = K.cfg(name)
    x, wt, b, labels, _ = K.inputs(name)
    gz = torch.randn(n, 1, h, w, generator=torch.Generator().manual_seed(7))
    xd, wd, bd, lb, _ = _dev(name)
    z = normed_class_mask_logits(xd, wd, bd, lb, **_kw(name))
    z.backward(gz.to(DEV))
    x64 = x.double().requires_grad_(True)
    w64 = wt.double().reshape(c, cin).requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    what = w64[labels] / (w64[labels].norm(dim=1, keepdim=True).pow(q) + eps)
    xn = x64 / (x64.norm(dim=1, keepdim=True).pow(q) + eps) * temp
    z64 = torch.einsum("nc,nchw->nhw", what, xn) + b64[labels][:, None, None]
    (z64 * gz[:, 0].double()).sum().backward()
    for k, got, ref in (("dx", xd.grad, x64.grad), ("dweight", wd.grad.reshape(c, cin), w64.grad), ("dbias", bd.grad, b64.grad)):
        e = float((got.cpu().double() - ref).abs().max()) / float(ref.abs().max())
        print(name, k, "err / limit %.3f" % (e / TOL[k]))
        assert e <= TOL[k], (name, k)
    unsel = ~K.selected_rows(labels, c)
    assert not wd.grad.cpu()[unsel].any() and not bd.grad.cpu()[unsel].any()
    # gradient for x alone: nothing else is computed, the same bits
    xd2 = xd.detach().clone().requires_grad_(True)
    normed_class_mask_logits(xd2, wd.detach(), bd.detach(), lb, **_kw(name)).backward(gz.to(DEV))
    assert torch.equal(xd2.grad, xd.grad)


def test_agrees_with_the_dense_path_on_the_device():
    """NormedConv2d + mask_cross_entropy on the device - what the package offered for the cos-norm head before - at case a."""
    from iif_amd.mmdet_mask_loss import mask_cross_entropy
    from iif_amd.mmdet_normed_mask_predictor import ClassSelectedNormedMaskPredictor
    n, c, cin, h, w = K.CASES["a"][:5]
    new = _loss_run("a")
    xd, wd, bd, lb, t = _dev("a")
    m = ClassSelectedNormedMaskPredictor(cin, c, **_kw("a")).to(DEV)
    with torch.no_grad():
        m.weight.copy_(wd)
        m.bias.copy_(bd)
    conv = m.to_conv()
    loss = mask_cross_entropy(conv(xd), t, lb)
    loss.sum().backward()
    assert abs(float(loss.detach()) - float(new[0])) <= TOL["loss"] * max(1.0, abs(float(new[0])))
    for k, got, old in (("dx", new[1], xd.grad), ("dweight", new[2], conv.weight.grad.reshape(c, cin)), ("dbias", new[3], conv.bias.grad)):
        old = old.cpu()
        e = float((got - old).abs().max()) / float(old.abs().max())
        print(k, "against dense: err / limit %.3f" % (e / TOL[k]))
        assert e <= TOL[k], k
    # and the module's own loss is the function's
    m.zero_grad()
    xm = xd.detach().clone().requires_grad_(True)
    lm = m.loss(xm, lb, t)["loss_mask"]
    lm.sum().backward()
    assert torch.equal(lm.detach().cpu(), new[0]) and torch.equal(xm.grad.cpu(), new[1])
    assert torch.equal(m.weight.grad.cpu().reshape(c, cin), new[2]) and torch.equal(m.bias.grad.cpu(), new[3])


def _bad_labels():
    n, c = K.CASES["a"][:2]
    labels = K.inputs("a")[3]
    bad = labels.clone()
    bad[1], bad[3] = c, -1
    return bad, (bad >= 0) & (bad < c)


@pytest.mark.parametrize("valid_rows", [False, True])
def test_labels_outside_the_classes(valid_rows):
    """A label equal to C and a label of -1 among valid ones: zero loss contribution, a zero dx slice, nothing in dweight / dbias;
    NaN in the x of those RoIs changes no bit of any output; with valid_rows the result equals the call on the valid RoIs
    alone."""
    from iif_amd.mmdet_normed_mask_predictor import normed_class_mask_logits
    n, c, cin, h, w = K.CASES["a"][:5]
    x, wt, b, _, t = K.inputs("a")
    bad, valid = _bad_labels()
    ref = K.restate64(x, wt, b, bad, t, *K.cfg("a"), valid=valid, valid_rows=valid_rows)

    def run(xs, lbs, ts, vr):
        return _run(xs.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True), lbs.to(DEV),
                    ts.to(DEV), valid_rows=vr, **_kw("a"))
    got = run(x, bad, t, valid_rows)
    _check_loss(got[0], ref, "bad labels")
    _check_grads(got, ref, 1.0, False, "bad labels")
    assert not got[1][~valid].any()
    unsel = ~K.selected_rows(bad, c)
    assert not got[2][unsel].any() and not got[3][unsel].any()
    xnan = x.clone()
    xnan[~valid] = float("nan")
    for a, bb in zip(got, run(xnan, bad, t, valid_rows)):
        assert torch.equal(a, bb)
    z = normed_class_mask_logits(xnan.to(DEV), wt.to(DEV), b.to(DEV), bad.to(DEV), **_kw("a")).cpu()
    assert not z[~valid].any() and bool(torch.isfinite(z).all())
    if valid_rows:
        alone = run(x[valid], bad[valid], t[valid], False)               # the valid RoIs alone: divisor n_valid * HW
        ref_alone = K.restate64(x[valid], wt, b, bad[valid], t[valid], *K.cfg("a"))
        assert abs(float(got[0]) - float(alone[0])) <= TOL["loss"] * max(1.0, abs(float(ref_alone["loss"])))
        for k, i, a, bb in (("dx", "dx", got[1][valid], alone[1]), ("dweight", "dweight", got[2], alone[2]), ("dbias", "dbias", got[3], alone[3])):
            assert float((a - bb).abs().max()) <= TOL[k] * float(ref_alone[i].abs().max()), k
    else:
        good = run(x, K.inputs("a")[3], t, False)                         # the other RoIs exactly as without the bad labels
        assert torch.equal(got[1][valid], good[1][valid])


@pytest.mark.parametrize("valid_rows", [False, True])
def test_all_labels_invalid(valid_rows):
    x, wt, b, _, t = K.inputs("a")
    lbs = torch.tensor(K.VALID_ROWS_LABELS["all"], dtype=torch.int64)
    got = _run(x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True), lbs.to(DEV), t.to(DEV),
               valid_rows=valid_rows, **_kw("a"))
    for v in got:
        assert bool(torch.isfinite(v).all()) and not v.any()


def test_valid_rows_without_invalid_labels_changes_nothing():
    a, b = _loss_run("a"), _run(*_dev("a"), valid_rows=True, **_kw("a"))
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_no_host_synchronisation():
    """Forward + backward of both functions, with and without valid_rows, under set_sync_debug_mode('error')."""
    from iif_amd.mmdet_normed_mask_predictor import normed_class_mask_logits, normed_class_mask_loss
    xd, wd, bd, lb, t = _dev("e")
    bad = torch.tensor([10, K.CASES["e"][1], -1], dtype=torch.int64, device=DEV)      # one valid, a padded row, a negative label
    gz = torch.ones(K.CASES["e"][0], 1, *K.CASES["e"][3:5], device=DEV)
    up = torch.full((1,), 2.0, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for labels in (lb, bad):
            for vr in (False, True):
                normed_class_mask_loss(xd, wd, bd, labels, t, valid_rows=vr, **_kw("e")).backward(up)
            normed_class_mask_logits(xd, wd, bd, labels, **_kw("e")).backward(gz)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(xd.grad).all()) and bool(torch.isfinite(wd.grad).all())


def test_only_requested_gradients(monkeypatch):
    """weight / bias without requires_grad: no [N, Cin + 1] scratch is allocated, dweight stays None, dx has the same bits; x
    without requires_grad: no dx-sized tensor is allocated, dweight / dbias have the same bits."""
    from iif_amd import mmdet_normed_mask_predictor as mod
    n, c, cin, h, w = K.CASES["e"][:5]
    full = _loss_run("e")
    shapes = []
    real_empty, real_like = torch.empty, torch.empty_like

    def empty(*a, **k):
        out = real_empty(*a, **k)
        shapes.append(tuple(out.shape))
        return out

    def empty_like(*a, **k):
        out = real_like(*a, **k)
        shapes.append(tuple(out.shape))
        return out
    monkeypatch.setattr(mod.torch, "empty", empty)
    monkeypatch.setattr(mod.torch, "empty_like", empty_like)
    xd, wd, bd, lb, t = _dev("e")
    wd.requires_grad_(False), bd.requires_grad_(False)
    mod.normed_class_mask_loss(xd, wd, bd, lb, t, **_kw("e")).sum().backward()
    assert wd.grad is None and bd.grad is None and torch.equal(xd.grad.cpu(), full[1])
    assert (n, cin + 1) not in shapes and (c, cin) not in shapes and (n, cin, h, w) in shapes and (3, n, h * w) in shapes
    del shapes[:]
    xd, wd, bd, lb, t = _dev("e")
    xd.requires_grad_(False)
    mod.normed_class_mask_loss(xd, wd, bd, lb, t, **_kw("e")).sum().backward()
    assert xd.grad is None and torch.equal(wd.grad.cpu().reshape(c, cin), full[2]) and torch.equal(bd.grad.cpu(), full[3])
    assert (n, cin, h, w) not in shapes and (n, cin + 1) in shapes and (2, n, h * w) in shapes
    del shapes[:]
    xd, wd, bd, lb, t = _dev("e", grad=False)                       # nothing asked for: no compact arrays at all
    loss = mod.normed_class_mask_loss(xd, wd, bd, lb, t, **_kw("e"))
    assert not loss.requires_grad and torch.equal(loss.cpu(), full[0]) and (0, n, h * w) in shapes


def test_no_rois():
    from iif_amd.mmdet_normed_mask_predictor import ClassSelectedNormedMaskPredictor
    m = ClassSelectedNormedMaskPredictor(16, 5).to(DEV)
    x = torch.zeros(0, 16, 6, 6, device=DEV, requires_grad=True)
    lb = torch.zeros(0, dtype=torch.int64, device=DEV)
    for vr in (False, True):
        loss = m.loss(x, lb, torch.zeros(0, 6, 6, device=DEV), valid_rows=vr)["loss_mask"]
        assert loss.shape == (1,) and float(loss.detach()) == 0 and loss.requires_grad
        m.zero_grad()
        loss.sum().backward()
        assert x.grad.shape == x.shape
        assert m.weight.grad is not None and not m.weight.grad.any() and m.bias.grad is not None and not m.bias.grad.any()
    z = m(x, lb)
    assert z.shape == (0, 1, 6, 6) and z.requires_grad


def test_non_contiguous_and_channels_last_x():
    n, c, cin, h, w = K.CASES["e"][:5]
    base = _loss_run("e")
    x, wt, b, labels, t = K.inputs("e")
    cl = x.to(DEV).contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and cl.is_contiguous(memory_format=torch.channels_last)
    wide = torch.full((n, cin, h, w + 3), float("nan"))
    wide[..., :w] = x
    nc = wide.to(DEV)[..., :w]                                          # a strided view of a wider buffer
    assert not nc.is_contiguous()
    for xs in (cl, nc):
        got = _run(xs.requires_grad_(True), wt.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True), labels.to(DEV), t.to(DEV),
                   **_kw("e"))
        for u, v in zip(got, base):
            assert torch.equal(u, v)


def test_peak_memory_at_the_lvis_class_count():
    """One forward + backward at case f stays below HALF the bytes of the full logits alone (N * C * HW * 4 = 241 MB): dx, three
    compact arrays, the scratch and dweight come to about 58 MB."""
    from iif_amd.mmdet_normed_mask_predictor import normed_class_mask_loss
    n, c, cin, h, w = K.CASES["f"][:5]
    xd, wd, bd, lb, t = _dev("f")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    normed_class_mask_loss(xd, wd, bd, lb, t).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.1f MB, full logits %.1f MB" % (rise / 1e6, n * c * h * w * 4 / 1e6))
    assert rise < n * c * h * w * 4 / 2
