"""Mask-side class-channel selection against the CPU restatement in oracle.mmdet_iif:
gather bit-exact, BCE loss / gradient within 1e-5 relative (fp32); then fp32 and bf16 logits at the edge shapes against a
float64 evaluation with derived bounds, saturated logits, and the out-of-range label report."""
import pytest
import torch

from oracle import mmdet_iif as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n,c,hw", [(7, 11, 2), (64, 1203, 28), (1, 3, 28), (33, 80, 14)])
def test_gather_is_bit_exact(n, c, hw):
    from iif_amd.mmdet_mask_loss import gather_class_masks
    g = torch.Generator().manual_seed(n)
    pred = torch.rand(n, c, hw, hw, generator=g)
    labels = torch.randint(0, c, (n,), generator=g)
    out = gather_class_masks(pred.to(DEV), labels.to(DEV))
    assert torch.equal(out.cpu(), M.gather_class_masks(pred, labels))


@pytest.mark.parametrize("n,c,hw,scale", [(3, 11, 2, 1000.0), (64, 1203, 28, 3.0), (33, 80, 14, 1.0)])
def test_mask_cross_entropy_loss_and_grad(n, c, hw, scale):
    from iif_amd.mmdet_mask_loss import mask_cross_entropy
    g = torch.Generator().manual_seed(c)
    pred = torch.randn(n, c, hw, hw, generator=g) * scale          # the reference's doctest uses *1000
    target = torch.rand(n, hw, hw, generator=g)
    labels = torch.randint(0, c, (n,), generator=g)
    pd = pred.to(DEV).requires_grad_(True)
    loss = mask_cross_entropy(pd, target.to(DEV), labels.to(DEV))
    assert loss.shape == (1,)
    (loss * 2.5).sum().backward()
    pr = pred.clone().requires_grad_(True)
    ref = M.mask_cross_entropy(pr, target, labels)
    (ref * 2.5).sum().backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    assert (pd.grad.cpu() - pr.grad).abs().max().item() <= 1e-5 * pr.grad.abs().max().item()
    # only the selected channels carry gradient
    sel = torch.zeros(n, c, dtype=torch.bool)
    sel[torch.arange(n), labels] = True
    assert pd.grad.cpu()[~sel].abs().max().item() == 0


def test_mask_loss_argument_contract():
    from iif_amd.mmdet_mask_loss import mask_cross_entropy
    p = torch.zeros(2, 3, 4, 4, device=DEV)
    t = torch.zeros(2, 4, 4, device=DEV)
    lb = torch.zeros(2, dtype=torch.long, device=DEV)
    with pytest.raises(AssertionError):
        mask_cross_entropy(p, t, lb, reduction="sum")
    with pytest.raises(AssertionError):
        mask_cross_entropy(p, t, lb, ignore_index=255)
    assert abs(mask_cross_entropy(p, t, lb).item() - 0.6931472) < 1e-6


# ------------------------------------------------------------------ float64 yardstick, bf16 logits, edge shapes
# (n, C, hw): hw below / at / above one pass of the 256 threads and the 28 x 28 mask of the head; one RoI; one class
EDGE_SHAPES = [(3, 5, 1), (1, 1, 255), (4, 3, 256), (5, 7, 257), (2, 1, 257), (3, 4, 784), (1, 6, 784)]
U24 = 2.0 ** -24
F64 = torch.float64


def _edge_case(n, c, hw, dtype, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    pred = (torch.randn(n, c, hw, generator=g) * scale).to(dtype)
    target = torch.rand(n, hw, generator=g)
    labels = torch.randint(0, c, (n,), generator=g)
    labels[0] = c - 1                                  # the last class, and class 0 where there is a second RoI
    if n > 1:
        labels[1] = 0
    return pred, target, labels


def _bce_reference(pred, target, labels, upstream):
    """float64 BCE-with-logits on the class channel, from the logits as stored (bf16 logits widened): (loss, loss bound,
    gradient [n, C, hw], gradient bound).  Bounds.  A RoI's loss is an fp32 sum of hw terms max(x, 0) - x t + log1p(exp(-|x|)):
    one thread's chain ceil(hw / 256), six shuffle steps, four wave totals -> L = ceil(hw / 256) + 10, S the sum of the
    magnitudes of the three parts; or 4 x the error of the same sum in float32 on the CPU.  The RoI sums are added in double
    and rounded once: 2^-24 |loss|.  A gradient element (sigmoid(x) - t) * upstream / (n hw) is no sum: 16 * 2^-24 times
    the magnitudes of its two terms."""
    n, c, hw = pred.shape
    x = pred.to(F64)[torch.arange(n), labels]
    t = target.to(F64)
    parts = (x.clamp_min(0), x * t, torch.log1p(torch.exp(-x.abs())))
    rows = (parts[0] - parts[1] + parts[2]).sum(-1)
    s_mag = (parts[0].abs() + parts[1].abs() + parts[2]).sum(-1)
    x32, t32 = x.float(), t.float()
    cpu32 = (x32.clamp_min(0) - x32 * t32 + torch.log1p(torch.exp(-x32.abs()))).sum(-1).to(F64)
    chain = (hw + 255) // 256 + 10
    b_rows = torch.maximum((chain + 16) * U24 * s_mag, 4 * (cpu32 - rows).abs())
    loss = rows.sum() / (n * hw)
    b_loss = b_rows.sum() / (n * hw) + U24 * loss.abs()
    sig = torch.sigmoid(x)
    k = upstream / (n * hw)
    grad = torch.zeros(n, c, hw, dtype=F64)
    b_grad = torch.zeros(n, c, hw, dtype=F64)
    grad[torch.arange(n), labels] = (sig - t) * k
    b_grad[torch.arange(n), labels] = 16 * U24 * (sig + t) * k
    return loss, b_loss, grad, b_grad


def _run_loss(pred, target, labels, upstream):
    from iif_amd.mmdet_mask_loss import mask_cross_entropy
    pd = pred.to(DEV).requires_grad_(True)
    loss = mask_cross_entropy(pd, target.to(DEV), labels.to(DEV))
    (loss * upstream).sum().backward()
    return loss.detach().cpu().to(F64)[0], pd.grad.cpu()


@pytest.mark.parametrize("n,c,hw", EDGE_SHAPES)
def test_gather_bf16_is_the_widened_value(n, c, hw):
    from iif_amd.mmdet_mask_loss import gather_class_masks
    pred, _, labels = _edge_case(n, c, hw, torch.bfloat16, 10 + hw)
    out = gather_class_masks(pred.to(DEV), labels.to(DEV))
    assert out.dtype == torch.float32 and out.shape == (n, hw)
    assert torch.equal(out.cpu(), pred.float()[torch.arange(n), labels])
    p32 = pred.float() + 0.001                                             # not bf16-representable: the fp32 path, same shapes
    assert torch.equal(gather_class_masks(p32.to(DEV), labels.to(DEV)).cpu(), p32[torch.arange(n), labels])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,c,hw", EDGE_SHAPES)
def test_mask_loss_against_float64(n, c, hw, dtype):
    """Measured on the MI355X, worst over the shapes: loss |error| / bound 0.04 (7.7e-8 absolute); gradient 0.31 for fp32 logits,
    0.99 for bf16 ones (the gradient comes back in bf16: one rounding, up to 2^-8 just above a power of two)."""
    pred, target, labels = _edge_case(n, c, hw, dtype, 20 + hw)
    loss, grad = _run_loss(pred, target, labels, 2.5)
    ref, b_loss, gref, b_grad = _bce_reference(pred, target, labels, 2.5)
    if dtype == torch.bfloat16:
        assert grad.dtype == torch.bfloat16
        b_grad = b_grad + 2.0 ** -8 * gref.abs()
    e_loss = (loss - ref).abs().item()
    e_grad = (grad.to(F64) - gref).abs()
    print("\n  loss err %.3e bound %.3e | grad worst err/bound %.3f" %
          (e_loss, b_loss.item(), (e_grad / b_grad.clamp_min(1e-300)).max().item()))
    assert e_loss <= b_loss.item()
    assert (e_grad <= b_grad).all()                     # bound 0 off the selected channels: exactly no gradient there


@pytest.mark.parametrize("mag", [100.0, 1e4])
def test_mask_loss_saturated_logits(mag):
    """fp32 logits of +-100 and +-1e4: the loss is finite and equals the float64 value, the gradient saturates to -t and
    1 - t (times upstream / (n hw))."""
    n, c, hw = 3, 4, 257
    pred, target, labels = _edge_case(n, c, hw, torch.float32, 77)
    sign = torch.where(torch.rand(n, c, hw, generator=torch.Generator().manual_seed(5)) < 0.5, -1.0, 1.0)
    pred = sign * mag
    loss, grad = _run_loss(pred, target, labels, 1.0)
    ref, b_loss, gref, b_grad = _bce_reference(pred, target, labels, 1.0)
    assert torch.isfinite(loss) and (loss - ref).abs().item() <= b_loss.item()
    assert ((grad.to(F64) - gref).abs() <= b_grad).all()
    x = pred[torch.arange(n), labels]
    sat = torch.where(x > 0, 1 - target.to(F64), -target.to(F64)) / (n * hw)
    assert (gref[torch.arange(n), labels] - sat).abs().max().item() <= 1e-15 * sat.abs().max().item()   # float64 rounding
    assert ((grad.to(F64)[torch.arange(n), labels] - sat).abs() <= b_grad[torch.arange(n), labels]).all()


def test_mask_loss_without_grad_allocates_no_gradient():
    from iif_amd.mmdet_mask_loss import mask_cross_entropy
    n, c, hw = 8, 16, 784
    pred, target, labels = _edge_case(n, c, hw, torch.float32, 31)
    pd, td, ld = pred.to(DEV), target.to(DEV), labels.to(DEV)
    with_grad = mask_cross_entropy(pd.clone().requires_grad_(True), td, ld)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = mask_cross_entropy(pd, td, ld)
    torch.cuda.synchronize()
    assert not loss.requires_grad and loss.grad_fn is None
    assert torch.equal(loss, with_grad.detach())
    # the [n, C, hw] fp32 gradient would be 401 408 bytes; the target copy, the row losses and the loss are a tenth of it
    assert torch.cuda.max_memory_allocated() - before < pred.numel() * 4 // 2


def test_out_of_range_label_is_reported():
    """A label outside [0, C) (the reference raises): gather returns a row of zeros, the loss counts the RoI as zero and
    gives it no gradient, and both set the flag that custom.check_label_status() raises on and clears."""
    from iif_amd import custom
    from iif_amd.mmdet_mask_loss import gather_class_masks, mask_cross_entropy
    n, c, hw = 5, 7, 257
    for dtype in (torch.float32, torch.bfloat16):
        pred, target, labels = _edge_case(n, c, hw, dtype, 41)
        gather_class_masks(pred.to(DEV), labels.to(DEV))
        mask_cross_entropy(pred.to(DEV), target.to(DEV), labels.to(DEV))
        custom.check_label_status()                       # clean
        for bad_value in (c, -1):
            bad = labels.clone()
            bad[2] = bad_value
            out = gather_class_masks(pred.to(DEV), bad.to(DEV)).cpu()
            with pytest.raises(IndexError):
                custom.check_label_status()
            custom.check_label_status()                   # flag was cleared
            keep = [0, 1, 3, 4]
            assert (out[2] == 0).all()
            assert torch.equal(out[keep], pred.float()[torch.arange(n), labels][keep])
            pd = pred.to(DEV).requires_grad_(True)
            loss = mask_cross_entropy(pd, target.to(DEV), bad.to(DEV))
            loss.sum().backward()
            with pytest.raises(IndexError):
                custom.check_label_status()
            custom.check_label_status()
            ref, b_loss, gref, b_grad = _bce_reference(pred[keep], target[keep], labels[keep], 1.0)
            # the mean stays over all n RoIs
            assert abs(loss.item() - ref.item() * len(keep) / n) <= b_loss.item() * len(keep) / n
            assert (pd.grad[2] == 0).all()


def test_in_range_labels_add_no_synchronisation():
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    from iif_amd.mmdet_mask_loss import gather_class_masks, mask_cross_entropy
    pred, target, labels = _edge_case(4, 5, 257, torch.float32, 51)
    pd, td, ld = pred.to(DEV).requires_grad_(True), target.to(DEV), labels.to(DEV)
    mask_cross_entropy(pd.detach(), td, ld)               # the shared workspace exists before the mode is switched on
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = gather_class_masks(pd.detach(), ld)
        loss = mask_cross_entropy(pd, td, ld)
        loss.sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(pd.grad).all()
