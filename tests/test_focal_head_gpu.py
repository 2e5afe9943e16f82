"""The fused sigmoid BCE / focal head (iif_sigmoid_focal_fwd_bwd, iif_amd.custom.FocalLoss) on the MI355X: the reference's
own results (tests/golden/g19_focal.npz, |x| <= 12), an fp64 evaluation of the exact function at large shapes and |x| up
to 80 (where the reference's fp32 nn.BCELoss saturates), the surface contracts, and the fused training step."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from iif_amd import _lib

from .focal_cases import golden_cases, golden_mixup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_closed_form(x, ta, gamma, alpha=None, weights=None, reduction="mean", tb=None, lam=1.0):
    """fp64 (loss, d loss / d x) of the reference formula with stable softplus forms, on x's device."""
    x = x.double()
    B, C = x.shape
    sp, spn = torch.nn.functional.softplus(x), torch.nn.functional.softplus(-x)
    s, q = torch.exp(-spn), torch.exp(-sp)
    k = 1.0 / B if reduction == "sum" else 1.0 / (B * C)
    w = None if weights is None else weights.double().reshape(1, C).to(x.device)

    def one(t):
        y = torch.zeros_like(x)
        y[torch.arange(B, device=x.device), t.to(x.device)] = 1.0
        if gamma == 0:
            l, d = sp - x * y, s - y
        else:
            l = torch.where(y > 0, q ** gamma * spn, s ** gamma * sp)
            d = torch.where(y > 0, -(q ** gamma) * (gamma * s * spn + q), s ** gamma * (s + gamma * q * sp))
            if alpha:
                at = alpha * y + (1 - alpha) * (1 - y)
                l, d = l * at, d * at
        if w is not None:
            l, d = l * w, d * w
        return l.sum() * k, d * k

    la, da = one(ta)
    if tb is None:
        return la, da
    lb, db = one(tb)
    return lam * la + (1 - lam) * lb, lam * da + (1 - lam) * db


def run(crit, x, t, tb=None, lam=1.0):
    p = x.detach().clone().requires_grad_(True)
    loss = crit(p, t) if tb is None else crit.mixup_loss(p, t, tb, lam)
    loss.backward()
    return loss.detach(), p.grad


def lt_weights(C):
    c = torch.tensor([int(500 * 0.01 ** (i / max(C - 1.0, 1.0))) for i in range(C)])
    return (c.sum() / c).float().to(DEV)


def test_golden_cases_against_the_reference(golden):
    from iif_amd.custom import FocalLoss
    g = golden("g19_focal")
    for name, x, t, kw, loss, grad, rows in golden_cases(g):
        w = None if kw["weights"] is None else torch.from_numpy(kw["weights"]).to(DEV)
        crit = FocalLoss(kw["gamma"], alpha=kw["alpha"], reduction=kw["reduction"], weights=w)
        l, d = run(crit, torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV))
        assert abs(l.item() - loss) <= 1e-4 * abs(loss), name
        ref = torch.from_numpy(grad)
        assert (d[rows].cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item(), name
    x, ya, yb, lam, kw, loss, grad, rows = golden_mixup(g)
    crit = FocalLoss(kw["gamma"], alpha=kw["alpha"], reduction="mean", weights=torch.from_numpy(kw["weights"]).to(DEV))
    l, d = run(crit, torch.from_numpy(x).to(DEV), torch.from_numpy(ya).to(DEV), torch.from_numpy(yb).to(DEV), lam)
    assert abs(l.item() - loss) <= 1e-4 * abs(loss)
    ref = torch.from_numpy(grad)
    assert (d[rows].cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def big_logits(B, C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, C, device=DEV, generator=g) * 4
    pick = torch.rand(B, C, device=DEV, generator=g)
    x = torch.where(pick < 0.01, torch.full_like(x, 80.0), x)
    x = torch.where(pick > 0.99, torch.full_like(x, -80.0), x)
    x = torch.where((pick > 0.5) & (pick < 0.505), x.sign() * 30.0, x)
    t = torch.randint(0, C, (B,), device=DEV, generator=g)
    x[torch.arange(0, B, 7, device=DEV), t[::7]] = -80.0            # confident and wrong: the reference's saturated case
    x[torch.arange(3, B, 7, device=DEV), t[3::7]] = 80.0
    return x, t


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("gamma,alpha,weighted,reduction", [(0.0, None, True, "mean"), (2.0, 0.25, True, "sum"),
                                                             (2.5, None, False, "mean"), (1.0, 0.75, False, "none")])
def test_large_batch_against_fp64(dtype, gamma, alpha, weighted, reduction):
    from iif_amd.custom import FocalLoss
    B, C = 65536, 1000
    x, t = big_logits(B, C, 11)
    x = x.to(dtype)
    w = lt_weights(C) if weighted else None
    l, d = run(FocalLoss(gamma, alpha=alpha, reduction=reduction, weights=w), x, t)
    assert d.dtype == dtype
    rl, rd = torch_closed_form(x, t, gamma, alpha, w, reduction)
    assert math.isfinite(l.item()) and bool(torch.isfinite(d).all())
    assert abs(l.item() - rl.item()) <= 1e-5 * abs(rl.item())
    gmax = rd.abs().max().item()
    err = (d.double() - rd).abs()
    if dtype == torch.float32:
        assert err.max().item() <= 2e-6 * gmax
    else:            # one bf16 rounding of the exact value (2^-9 relative) plus the fp32 arithmetic
        assert bool((err <= rd.abs() * 2.0 ** -8 + 2e-6 * gmax).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [13, 100, 1000])
def test_every_column_as_the_target(C, dtype):
    from iif_amd.custom import FocalLoss
    g = torch.Generator(device=DEV).manual_seed(C)
    x = (torch.randn(C, C, device=DEV, generator=g) * 3).to(dtype)
    t = torch.arange(C, device=DEV)
    for gamma, alpha in ((0.0, None), (2.0, 0.25), (0.5, None)):
        l, d = run(FocalLoss(gamma, alpha=alpha, weights=lt_weights(C)), x, t)
        rl, rd = torch_closed_form(x, t, gamma, alpha, lt_weights(C))
        assert abs(l.item() - rl.item()) <= 1e-5 * abs(rl.item())
        err = (d.double() - rd).abs()
        tol = 2e-6 * rd.abs().max().item() + (rd.abs() * 2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
        assert bool((err <= tol).all()), (C, gamma)


def test_fused_mixup_equals_two_launches():
    from iif_amd.custom import FocalLoss, Mixup
    B, C = 512, 100
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(B, C, device=DEV, generator=g) * 3
    ya = torch.randint(0, C, (B,), device=DEV, generator=g)
    yb = ya[torch.randperm(B, device=DEV, generator=g)]
    lam = 0.3
    crit = FocalLoss(2.0, alpha=0.25, weights=lt_weights(C))
    l1, d1 = run(crit, x, ya, yb, lam)
    p = x.clone().requires_grad_(True)
    l2 = lam * crit(p, ya) + (1 - lam) * crit(p, yb)
    l2.backward()
    assert abs(l1.item() - l2.item()) <= 1e-6 * abs(l2.item())
    assert (d1 - p.grad).abs().max().item() <= 1e-6 * p.grad.abs().max().item()
    p3 = x.clone().requires_grad_(True)
    Mixup(crit).mixup_criterion(p3, ya, yb, lam).backward()          # dispatches to the single launch
    assert torch.equal(p3.grad, d1)


@pytest.mark.parametrize("bad", [100, -1])
def test_out_of_range_label_raises_at_check_label_status(bad):
    from iif_amd.custom import FocalLoss, check_label_status
    try:
        check_label_status()                                          # start from a clear status word
    except IndexError:
        pass
    x = torch.randn(8, 100, device=DEV)
    t = torch.randint(0, 100, (8,), device=DEV)
    t[5] = bad
    crit = FocalLoss(2.0)
    l, d = run(crit, x, t)
    assert bool((d[5] == 0).all())                                    # the row contributes zero
    t_ok = t.clone(); t_ok[5] = 0
    keep = torch.ones(8, dtype=torch.bool, device=DEV); keep[5] = False
    _, d_ok = run(crit, x, t_ok)
    assert torch.equal(d[keep], d_ok[keep])
    with pytest.raises(IndexError):
        check_label_status()
    check_label_status()                                              # cleared


def test_backward_twice_and_scaled_upstream():
    from iif_amd.custom import FocalLoss
    x = torch.randn(64, 100, device=DEV) * 3
    t = torch.randint(0, 100, (64,), device=DEV)
    crit = FocalLoss(2.0, alpha=0.25)
    _, d = run(crit, x, t)
    p = x.clone().requires_grad_(True)
    loss = crit(p, t)
    (3.0 * loss).backward(retain_graph=True)
    assert torch.allclose(p.grad, 3.0 * d, rtol=1e-6, atol=0)
    loss.backward()
    assert torch.allclose(p.grad, 4.0 * d, rtol=1e-6, atol=0)


def _entry(x, t, dx, loss, C, B, ws, rows, status):
    return _lib.lib().iif_sigmoid_focal_fwd_bwd(
        _lib.ptr(x), _lib.dtype_code(x), x.stride(0) if B else C, _lib.ptr(t), 0, 1.0, 0, 2.0, 1, 0.25, 1.0 / (max(B, 1) * C),
        B, C, _lib.ptr(rows), _lib.ptr(loss), _lib.ptr(dx), dx.stride(0) if dx is not None and B else C, _lib.ptr(status),
        _lib.ptr(ws), _lib.stream_ptr())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_strided_rows_unaligned_pointers_and_empty_batch(dtype):
    from iif_amd.custom import FocalLoss
    B, C = 37, 1003
    big = (torch.randn(B, C + 9, device=DEV) * 3).to(dtype)
    t = torch.randint(0, C, (B,), device=DEV)
    tol = lambda rd: 2e-6 * rd.abs().max().item() + (rd.abs() * 2.0 ** -8 if dtype == torch.bfloat16 else 0.0)  # noqa: E731
    for off in (0, 1, 3):
        x = big[:, off:off + C]                                       # row pitch C + 9, pointer off elements in
        rl, rd = torch_closed_form(x, t, 2.0, 0.25)
        leaf = big.clone().requires_grad_(True)
        l = FocalLoss(2.0, alpha=0.25)(leaf[:, off:off + C], t)       # the strided view itself goes to the kernel
        l.backward()
        d = leaf.grad[:, off:off + C]
        assert abs(l.item() - rl.item()) <= 1e-5 * abs(rl.item())
        assert bool(((d.double() - rd).abs() <= tol(rd)).all()), off
        # through the entry, dlogits in the logits' 16-byte phase: head / 16-byte body / tail on every row
        dbig = torch.zeros(B, C + 9, dtype=dtype, device=DEV)
        ws = torch.zeros(1 + 2048, dtype=torch.int32, device=DEV)
        rows = torch.empty(B, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        loss = torch.empty((), device=DEV)
        assert _entry(x, t, dbig[:, off:off + C], loss, C, B, ws, rows, status) == 0
        assert abs(loss.item() - rl.item()) <= 1e-5 * abs(rl.item())
        assert bool(((dbig[:, off:off + C].double() - rd).abs() <= tol(rd)).all()), off
        assert bool((dbig[:, :off] == 0).all()) and bool((dbig[:, off + C:] == 0).all())     # nothing outside the rows
        assert int(ws[0]) == 0 and int(status[0]) == 0
    # B == 0: the entry writes a zero loss; the module returns the reference's NaN (mean of nothing)
    loss = torch.full((), 7.0, device=DEV)
    e = torch.empty(0, C, dtype=dtype, device=DEV)
    assert _entry(e, torch.empty(0, dtype=torch.int64, device=DEV), None, loss, C, 0, None, None, None) == 0
    assert loss.item() == 0.0
    assert math.isnan(FocalLoss(2.0)(e, torch.empty(0, dtype=torch.int64, device=DEV)).item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_launches_are_bit_identical(dtype):
    from iif_amd.custom import FocalLoss
    x, t = big_logits(8192, 1000, 3)
    x = x.to(dtype)
    crit = FocalLoss(2.0, alpha=0.25, weights=lt_weights(1000))
    l1, d1 = run(crit, x, t)
    l2, d2 = run(crit, x, t)
    assert torch.equal(l1, l2) and torch.equal(d1, d2)


# ------------------------------------------------------------------------------------------------ through the network
class DS:
    def __init__(self, c):
        self.c = list(c)

    def get_cls_num_list(self):
        return self.c


def _net_and_batch(C=100, B=128):
    from iif_amd import resnet_cifar
    from oracle import resnet_oracle as R
    net = resnet_cifar.resnet32(num_classes=C, use_norm="None", compute_dtype=torch.float32)
    net.load_state_dict(R.init_cifar("resnet32", C, seed=3))
    net.train()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, 32, 32, generator=g).to(DEV)
    t = torch.randint(0, C, (B,), generator=g).to(DEV)
    return net, x, t


def test_fused_step_gradient_arena_matches_drop_in_path():
    from iif_amd.custom import FocalLoss
    net, x, t = _net_and_batch()
    w = lt_weights(100)
    crit = FocalLoss(2.0, 0.25, weights=w)
    loss, _ = net.loss_and_backward(x, t, crit)
    fused = [v.clone() for v in net._grad_views]
    fused_loss = loss.item()
    logits = net(x)                                                   # drop-in: autograd through the native network
    xl = logits.double()
    sp, spn = torch.nn.functional.softplus(xl), torch.nn.functional.softplus(-xl)
    s, q = torch.exp(-spn), torch.exp(-sp)
    y = torch.nn.functional.one_hot(t, 100).double()
    p_t = s * y + q * (1 - y)
    bce = y * spn + (1 - y) * sp
    ref = (bce * (1 - p_t) ** 2 * w.double().unsqueeze(0) * (0.25 * y + 0.75 * (1 - y))).mean()
    ref.backward()
    assert abs(fused_loss - ref.item()) <= 1e-5 * abs(ref.item())
    for a, b in zip(fused, net._grad_views):
        assert (a - b).abs().max().item() <= 1e-5 * max(b.abs().max().item(), 1e-30)


def test_iif_step_unchanged_by_a_focal_step():
    from iif_amd.custom import FocalLoss, IIFLoss
    net, x, t = _net_and_batch()
    counts = [int(500 * 0.01 ** (i / 99.0)) for i in range(100)]
    iif = IIFLoss(DS(counts), variant="raw")
    l1, _ = net.loss_and_backward(x, t, iif)
    l1, a1 = l1.item(), net.grad_arena.clone()
    net.loss_and_backward(x, t, FocalLoss(2.0, 0.25, weights=lt_weights(100)))
    l2, _ = net.loss_and_backward(x, t, iif)
    assert l2.item() == l1 and torch.equal(net.grad_arena, a1)
    net.check_labels()


@pytest.mark.parametrize("classif", ["focal_loss", "bce"])
def test_train_cli_runs_with_sigmoid_criteria(classif):
    cmd = [sys.executable, "-m", "iif_amd.train", "--model", "resnet32", "--classif", classif, "--gamma", "2", "--alpha",
           "0.25", "--deffered", "--mixup", "1.0", "--epochs", "1", "--max-iters", "3", "-j", "0", "--print-freq", "1"]
    r = subprocess.run(["timeout", "-k", "10", "600"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(v) for v in re.findall(r"loss: (\S+)", r.stdout)]
    assert losses and all(math.isfinite(v) for v in losses), r.stdout[-2000:]
