"""The float64 per-unit reference of tests/unit_reference.py against torch autograd in float64 (no device needed): the GPU
checks in tests/test_step_units_gpu.py are only as good as this reference, so its convolutions, BN backward with a ReLU mask
and a residual, x-hat conventions, max-pool scatter, option-A shortcut and squeeze-and-excitation stages are pinned here to float64
rounding."""
import pytest
import torch
import torch.nn.functional as F

from tests import unit_reference as U

F64 = torch.float64


def _close(a, b, tol=1e-11):
    assert U.rel_l2(a, b) <= tol, U.rel_l2(a, b)


@pytest.mark.parametrize("n,c,co,h,k,stride,pad,groups", [
    (2, 8, 16, 9, 1, 1, 0, 1), (2, 8, 16, 9, 1, 2, 0, 1), (2, 8, 12, 10, 3, 1, 1, 1), (2, 8, 12, 9, 3, 2, 1, 1),
    (2, 3, 8, 14, 7, 2, 3, 1), (2, 16, 16, 8, 3, 1, 1, 4), (2, 16, 16, 9, 3, 2, 1, 8)])
def test_convolutions_against_autograd(n, c, co, h, k, stride, pad, groups):
    g = torch.Generator().manual_seed(n * 1000 + c * 10 + k)
    x = torch.randn(n, h, h, c, generator=g, dtype=F64, requires_grad=True)
    w = torch.randn(co, c // groups, k, k, generator=g, dtype=F64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=pad, groups=groups).permute(0, 2, 3, 1)
    _close(U.conv_fwd(x.detach(), w.detach(), stride, pad, groups), y)
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    gx, gw = torch.autograd.grad(y, (x, w), dy)
    _close(U.conv_wgrad(x.detach(), dy, tuple(w.shape), stride, pad, groups), gw)
    _close(U.conv_dgrad(dy, w.detach(), tuple(x.shape), stride, pad, groups), gx)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_backward_with_mask_and_residual_against_autograd(residual, relu):
    """y = act(BN(x) + r) with batch statistics: the reference's dx / dgamma / dbeta from (gy, mask y > 0, x-hat, gamma,
    invstd) and the residual's gradient (the gated gy) against autograd."""
    g = torch.Generator().manual_seed(7 + residual + 2 * relu)
    m, c = 300, 12
    x = (torch.randn(m, c, generator=g, dtype=F64) * 3 + 1).requires_grad_()
    gamma = (torch.rand(c, generator=g, dtype=F64) + 0.5).requires_grad_()
    beta = torch.randn(c, generator=g, dtype=F64).requires_grad_()
    r = torch.randn(m, c, generator=g, dtype=F64, requires_grad=True)
    pre = F.batch_norm(x, None, None, gamma, beta, training=True, eps=1e-5) + (r if residual else 0)
    y = pre.clamp_min(0) if relu else pre
    gy = torch.randn(m, c, generator=g, dtype=F64)
    gx, ggam, gbet, gr = torch.autograd.grad(y, (x, gamma, beta, r), gy, allow_unused=True)
    mean, invstd = U.bn_stats(x.detach())
    a = gamma.detach() * invstd
    _close(U.bn_act(x.detach(), a, beta.detach() - mean * a, r.detach() if residual else None, relu), y)
    mask = (y > 0).to(F64) if relu else None
    dx, dgam, dbet, gt = U.bn_backward(gy, mask, (x.detach() - mean) * invstd, gamma.detach(), invstd)
    _close(dx, gx)
    _close(dgam, ggam)
    _close(dbet, gbet)
    if residual:
        _close(gt, gr)


@pytest.mark.parametrize("convention", ["stored_rounded", "unrounded"])
def test_unit_x_hat_conventions_against_autograd(convention):
    """A whole conv + BN + residual + ReLU unit.  "stored_rounded": the product is rounded to bf16 before BN (statistics and
    x-hat of the stored output; the rounding passes the gradient straight through, as the engine's backward does);
    "unrounded": statistics and x-hat of the unrounded product (the never-stored forward, "sums from P").  The reference
    pipeline (conv_fwd -> bn_stats -> bn_backward -> conv_wgrad / conv_dgrad + gated residual) equals autograd in both."""
    g = torch.Generator().manual_seed(11)
    n, h, c, co = 3, 6, 8, 16
    src = torch.randn(n, h, h, c, generator=g, dtype=F64, requires_grad=True)
    w = (torch.randn(co, c, 3, 3, generator=g, dtype=F64) * 0.2).requires_grad_()
    gamma = (torch.rand(co, generator=g, dtype=F64) + 0.5).requires_grad_()
    beta = torch.randn(co, generator=g, dtype=F64).requires_grad_()
    r = torch.randn(n, h, h, co, generator=g, dtype=F64)
    x = F.conv2d(src.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    if convention == "stored_rounded":
        x = x + (x.to(torch.bfloat16).to(F64) - x).detach()
    pre = F.batch_norm(x.reshape(-1, co), None, None, gamma, beta, training=True, eps=1e-5).view(x.shape) + r
    y = pre.clamp_min(0)
    gy = torch.randn(y.shape, generator=g, dtype=F64)
    gsrc, gw, ggam, gbet = torch.autograd.grad(y, (src, w, gamma, beta), gy)

    xr = U.conv_fwd(src.detach(), w.detach(), 1, 1)
    xs = xr.to(torch.bfloat16).to(F64) if convention == "stored_rounded" else xr
    mean, invstd = U.bn_stats(xs)
    dx, dgam, dbet, gt = U.bn_backward(gy, (y > 0).to(F64), (xs - mean) * invstd, gamma.detach(), invstd)
    _close(dgam, ggam)
    _close(dbet, gbet)
    _close(U.conv_wgrad(src.detach(), dx, tuple(w.shape), 1, 1), gw)
    _close(U.conv_dgrad(dx, w.detach(), tuple(src.shape), 1, 1), gsrc)
    # the other convention's x-hat is measurably wrong at this size: the checker can tell the routes apart
    other = xr if convention == "stored_rounded" else xr.to(torch.bfloat16).to(F64)
    mean2, invstd2 = U.bn_stats(other)
    _, dgam2, _, _ = U.bn_backward(gy, (y > 0).to(F64), (other - mean2) * invstd2, gamma.detach(), invstd2)
    assert U.rel_l2(dgam2, ggam) > 1e-6


def test_maxpool_windows_and_scatter_against_autograd():
    g = torch.Generator().manual_seed(3)
    y = torch.randn(2, 9, 10, 5, generator=g, dtype=F64).clamp_min(0).requires_grad_()
    out, ind = F.max_pool2d(y.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    win = U.maxpool_windows(y.detach())
    _close(win.max(-1).values, out.permute(0, 2, 3, 1))
    # arg max codes kh * 3 + kw from the flat indices of torch's pool
    ho, wo = out.shape[2], out.shape[3]
    hh, ww = ind // 10, ind % 10
    kh = hh - (torch.arange(ho).view(1, 1, ho, 1) * 2 - 1)
    kw = ww - (torch.arange(wo).view(1, 1, 1, wo) * 2 - 1)
    code = (kh * 3 + kw).permute(0, 2, 3, 1).to(torch.uint8)
    assert torch.equal(win.gather(-1, code.long().unsqueeze(-1)).squeeze(-1), out.permute(0, 2, 3, 1).detach())
    gp = torch.randn(out.shape, generator=g, dtype=F64)
    (gy,) = torch.autograd.grad(out, y, gp)
    _close(U.maxpool_scatter(gp.permute(0, 2, 3, 1), code, (9, 10)), gy)


def test_option_a_shortcut_against_autograd():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 7, 8, 6, generator=g, dtype=F64, requires_grad=True)
    ref = F.pad(x.permute(0, 3, 1, 2)[:, :, ::2, ::2], (0, 0, 0, 0, 3, 3)).permute(0, 2, 3, 1)
    _close(U.shortcut_a_fwd(x.detach(), 12), ref)
    gs = torch.randn(ref.shape, generator=g, dtype=F64)
    (gx,) = torch.autograd.grad(ref, x, gs)
    _close(U.shortcut_a_bwd(gs, tuple(x.shape)), gx)


@pytest.mark.parametrize("residual", ["identity", "normalised_shortcut", "none"])
@pytest.mark.parametrize("c,hid,side", [(16, 4, 8), (64, 16, 3), (256, 16, 14)])
def test_se_block_stages_against_autograd(c, hid, side, residual):
    """o = bn(x), e = sigmoid(W2 relu(W1 mean_hw(o))), y = relu(o e + identity): every SE reference function (squeeze sums, q,
    h, e, the apply, S1 / S2, dz2, dz1, the offset o, both weight gradients, the form G) against autograd, then G through the
    reference's BN backward without a mask, and the masked gradient through the identity / the normalised shortcut."""
    g = torch.Generator().manual_seed(c + 3 * side + len(residual))
    n, hw = 3, side * side
    R = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    x = (R(n, side, side, c) * 2 + 0.5).requires_grad_()
    gamma = (torch.rand(c, generator=g, dtype=F64) + 0.5).requires_grad_()
    beta = (R(c) * 0.3).requires_grad_()
    w1 = (R(hid, c) * 2 / c ** 0.5).requires_grad_()
    w2 = (R(c, hid) * 2 / hid ** 0.5).requires_grad_()
    xd = (R(n, side, side, c) + 1).requires_grad_()
    gam_d = (torch.rand(c, generator=g, dtype=F64) + 0.5).requires_grad_()
    bet_d = R(c).requires_grad_()

    def bn(t, ga, be):
        return F.batch_norm(t.reshape(-1, c), None, None, ga, be, training=True, eps=1e-5).view(t.shape)

    o = bn(x, gamma, beta)
    oa, ob = o + 0, o + 0                      # the two ways o reaches y: scaled by the gate, and through the squeeze
    q = ob.mean((1, 2))
    z1 = q @ w1.t()
    h = z1.clamp_min(0)
    z2 = h @ w2.t()
    e = torch.sigmoid(z2)
    res = {"identity": xd, "normalised_shortcut": bn(xd, gam_d, bet_d), "none": None}[residual]
    pre = oa * e[:, None, None, :]
    y = (pre if res is None else pre + res).clamp_min(0)
    for t in (oa, ob, z1, z2) + (() if res is None else (res,)):
        t.retain_grad()
    gy = R(*y.shape)
    y.backward(gy)

    D = lambda t: t.detach()                   # noqa: E731
    mean, invstd = U.bn_stats(D(x))
    a = D(gamma) * invstd
    b = D(beta) - mean * a
    sums = U.se_squeeze(D(x))
    _close(sums, D(x).sum((1, 2)))
    qr = U.se_q(sums, a, b, hw)
    _close(qr, q)
    hr = U.se_h(qr, D(w1))
    _close(hr, h)
    er = U.se_e(hr, D(w2))
    _close(er, e)
    rres = None
    if residual == "identity":
        rres = D(xd)
    elif residual == "normalised_shortcut":
        mean_d, inv_d = U.bn_stats(D(xd))
        a_d = D(gam_d) * inv_d
        rres = D(xd) * a_d + (D(bet_d) - mean_d * a_d)
    yr = U.se_apply(D(x), a, b, er, rres)
    _close(yr, y)
    gt = gy * (yr > 0).to(F64)
    s1, s2 = U.se_backward_sums(gt, D(x))
    dz2 = U.se_dz2(s1, s2, a, b, er)
    _close(dz2, z2.grad)
    dz1 = U.se_dz1(dz2, D(w2), hr)
    _close(dz1, z1.grad)
    off = U.se_offset(dz1, D(w1), hw)
    _close(off[:, None, None, :].expand(ob.grad.shape), ob.grad)
    _close(U.se_dw(dz1, qr), w1.grad)
    _close(U.se_dw(dz2, hr), w2.grad)
    G = U.se_form(gt, er, off)
    _close(G, oa.grad + ob.grad)
    dx, dgam, dbet, _ = U.bn_backward(G, None, (D(x) - mean) * invstd, D(gamma), invstd)
    _close(dx, x.grad)
    _close(dgam, gamma.grad)
    _close(dbet, beta.grad)
    if residual == "identity":
        _close(gt, xd.grad)
    elif residual == "normalised_shortcut":
        _close(gt, res.grad)
        dxd, dgd, dbd, _ = U.bn_backward(gt, None, (D(xd) - mean_d) * inv_d, D(gam_d), inv_d)
        _close(dxd, xd.grad)
        _close(dgd, gam_d.grad)
        _close(dbd, bet_d.grad)


@pytest.mark.parametrize("dt,vec", [(torch.bfloat16, 8), (torch.float32, 4)])
def test_relu_bit_layout(dt, vec):
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(4, 3, 5, 16, generator=g) > 0.5
    flat = mask.reshape(-1, vec).int()
    packed = (flat << torch.arange(vec).view(1, vec)).sum(1).to(torch.uint8)
    assert torch.equal(U.unpack_bits(packed, dt, mask.shape), mask)


def test_failures_and_worst():
    met = {"a": {"dw": 1e-3, "dgamma": 5e-4}, "b": {"dw": 2e-2, "dgamma": float("nan")}}
    f = U.failures(met, {"dw": 1e-2, "dgamma": 1e-3})
    assert sorted((u, k) for u, k, _, _ in f) == [("b", "dgamma"), ("b", "dw")]      # NaN never passes
    assert U.worst(met)["dw"] == (2e-2, "b")
