"""The float64 closed forms of tests/head_cases.py against float64 autograd of the formulas the kernels restate
(``F.normalize``, ``x * scale / (1 + norm)``, the ``normed_predictor`` form ``v * scale / (norm ** power + eps)``): the
yardstick of tests/test_norm_head_gpu.py does not depend on the code under test.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

from tests import head_cases as H

F64 = torch.float64
TOL = 1e-12                                    # float64 closed form against float64 autograd, relative to the row's largest


def _close(a, b, tol=TOL, mag=None):
    """|a - b| <= tol * the row's largest |b| (or ``mag``, the size of the terms where the result is a cancelling difference)."""
    scale = b.abs().amax(-1, keepdim=True).clamp_min(1e-300) if b.dim() > 1 else b.abs().clamp_min(1e-300)
    if mag is not None:
        scale = torch.maximum(scale, mag)
    return bool(((a - b).abs() <= tol * scale).all())


def _xg(rows, cols, seed):
    x = H.rows_matrix(rows, cols, seed, special=False)
    g = H.rows_matrix(rows, cols, seed + 1, special=False)
    return x, g


@pytest.mark.parametrize("cols", [1, 63, 640])
@pytest.mark.parametrize("scale", [1.0, 16.0])
def test_rowmap_mode0_is_the_cosine_feature_map(cols, scale):
    x, g = _xg(5, cols, 3)
    xa = x.clone().requires_grad_(True)
    out = xa * scale / (1 + torch.norm(xa, 2, 1, keepdim=True))              # resnet_cifar.py:74-75
    out.backward(g)
    ref, n = H.rowmap_forward(x, 0, scale, 1e-12)
    assert _close(ref, out.detach()) and _close(n, x.norm(dim=1))
    assert _close(H.rowmap_backward(x, n, g, 0, scale, 1e-12), xa.grad, mag=scale * g.abs().amax(-1, keepdim=True))


@pytest.mark.parametrize("cols", [1, 63, 640])
@pytest.mark.parametrize("eps", [1e-12, 0.0])
def test_rowmap_mode1_is_f_normalize(cols, eps):
    x, g = _xg(5, cols, 5)
    if eps > 0:
        x[3] = x[3] / x[3].norm() * 1e-13                                    # below eps: F.normalize is x / eps there
    xa = x.clone().requires_grad_(True)
    out = F.normalize(xa, dim=1, eps=eps)
    out.backward(g)
    ref, n = H.rowmap_forward(x, 1, 1.0, eps)
    assert _close(ref, out.detach())
    dx = H.rowmap_backward(x, n, g, 1, 1.0, eps)
    assert _close(dx, xa.grad, mag=g.abs().amax(-1, keepdim=True) / n.clamp_min(eps)[:, None])
    if eps > 0:
        assert _close(dx[3], g[3] / eps) and _close(ref[3], x[3] / eps)


def test_rowmap_rows_of_zeros():
    """The conventions for a row of zeros: forward 0 in both modes; mode 0 backward scale * g (the limit, and autograd's
    value); mode 1 backward 0 - the kernels leave the row alone where the forward did (with eps = 0, which the cosine
    head's weight rows use, F.normalize has no gradient there at all)."""
    x, g = _xg(3, 65, 7)
    x[1] = 0
    for mode in (0, 1):
        out, n = H.rowmap_forward(x, mode, 4.0, 1e-12)
        assert n[1] == 0 and (out[1] == 0).all()
    xa = x.clone().requires_grad_(True)
    (xa * 4.0 / (1 + torch.norm(xa, 2, 1, keepdim=True))).backward(g)
    d0 = H.rowmap_backward(x, n, g, 0, 4.0, 1e-12)
    assert _close(d0, xa.grad) and torch.equal(d0[1], 4.0 * g[1])
    for eps in (1e-12, 0.0):
        d1 = H.rowmap_backward(x, n, g, 1, 1.0, eps)
        assert (d1[1] == 0).all() and torch.isfinite(d1).all()


@pytest.mark.parametrize("cols", [1, 65, 2304])
@pytest.mark.parametrize("power", [1.0, 2.0, 0.5])
@pytest.mark.parametrize("with_r", [False, True])
def test_rownorm_is_the_normed_predictor(cols, power, with_r):
    x, g = _xg(6, cols, 11)
    r = None
    if with_r:
        r = torch.tensor([1.5, 0.0, -2.0, 0.25, 1.0, 3.0], dtype=F64)
    x[4] = 0
    scale, eps = 20.0, 1e-6
    xa = x.clone().requires_grad_(True)
    v = xa if r is None else xa * r[:, None]
    # normed_predictor.py:34-40 (the norm of a row of zeros has sub-gradient 0 under autograd, as in the closed form)
    out = v * scale / (v.norm(dim=1, keepdim=True).pow(power) + eps)
    out.backward(g)
    ref, n = H.rownorm_forward(x, r, power, scale, eps)
    assert _close(ref, out.detach())
    dx = H.rownorm_backward(x, r, n, g, power, scale, eps)
    # power < 1: autograd's pow has no finite derivative at norm 0 (0.5 * 0 ** -0.5 times the zero sub-gradient is NaN); the
    # row of zeros is then checked by its stated value alone, below
    keep = [i for i in range(6) if power >= 1 or (i != 4 and not (with_r and i == 1))]    # row 1: row scale 0
    assert torch.isfinite(dx).all()
    assert _close(dx[keep], xa.grad[keep], 1e-11, mag=(g.abs().amax(-1) * scale / (n ** power + eps))[keep, None])
    rr = 1.0 if r is None else r[4]
    assert (ref[4] == 0).all() and _close(dx[4], rr * g[4] * scale / eps)
    if with_r:
        assert (ref[1] == 0).all() and (dx[1] == 0).all()


def test_bounds_are_positive_and_cover_a_float32_evaluation():
    """The derived bound is no smaller than the error of the same expressions evaluated in float32 by torch (a sanity check
    of the derivation: a bound that plain fp32 arithmetic misses would be a wrong bound, not a finding)."""
    for cols in (1, 65, 2048):
        x = H.rows_matrix(5, cols, 21)
        g = H.rows_matrix(5, cols, 22, special=False)
        for mode, eps in ((0, 1e-12), (1, 1e-12), (1, 0.0)):
            out, b_out, n, b_n = H.rowmap_forward_bounds(x, mode, 2.5, eps)
            x32 = x.float()
            n32 = (x32 * x32).sum(-1).sqrt()
            if mode == 0:
                o32 = x32 * (2.5 / (1 + n32))[:, None]
            else:
                o32 = torch.where(n32[:, None] > 0, x32 / n32.clamp_min(eps)[:, None], torch.zeros_like(x32))
            assert H.worst_ratio(o32, out, b_out)[0] <= 1.0
            assert H.worst_ratio(n32, n, b_n)[0] <= 1.0
            dx, b_dx = H.rowmap_backward_bounds(x, n.float().to(F64), g, mode, 2.5, eps)
            assert (b_dx >= 0).all() and torch.isfinite(b_dx).all() and torch.isfinite(dx).all()
    a, b = H.rows_matrix(10, 1000, 1, special=False), H.rows_matrix(10, 1000, 2, special=False)
    ref, bound = H.dot_window(a, b, 2.0, 5.0)
    assert abs(float((a * b).sum() * 2.0 / 5.0) - ref.item()) <= 1e-15 * abs(ref.item()) and bound > 0
