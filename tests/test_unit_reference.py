"""The float64 per-unit reference of tests/unit_reference.py against torch autograd in float64 (no device needed): the GPU
checks in tests/test_step_units_gpu.py are only as good as this reference, so its convolutions, BN backward with a ReLU mask
and a residual, x-hat conventions, max-pool scatter and option-A shortcut are pinned here to float64 rounding."""
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
