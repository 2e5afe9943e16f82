"""The classifier head of the REAL training step - average pool, feature map, weight normalisation, head GEMM, fused loss and
everything the head part of the backward forms - stage by stage against float64 (tests/unit_reference.check_head).

tests/test_step_units_gpu.py stops at the last block; the whole-network comparisons see the head only through bf16-route
bounds of 3e-2 .. 0.75, and in bf16 the cosine and normed heads were checked for finiteness alone.  Here every stage is
evaluated from the operands the step stored, with per-element bounds derived from the arithmetic (tests/head_cases.py), in
bf16 and fp32, for the linear, cosine, lr_cosine and normed heads, on two networks that run in a few seconds (NETS)."""
import pytest
import torch

from oracle import resnet_oracle as R
from tests import unit_reference as U
from tests.test_resnet_gpu import DS, _data, damp_residual_branches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, FP32 = torch.bfloat16, torch.float32
# arch: (classes, batch, image size).  resnet32: D = 64 (one lane chunk per row), C = 100 -> out_padded 104: four zero pad
# rows of the weights, four pad columns of logits / dlogits.  resnet50: D = 2048 (32 chunks), C = 1000, the transposed
# weights padded to 1008 columns.
NETS = {"resnet32": (100, 16, 32), "resnet50": (1000, 8, 64)}
HEADS = ("linear", "cosine", "lr_cosine", "norm")
FORWARD = ("pooled", "ex", "xnorm", "wn", "wnorm", "w_pad", "w_cast", "wt", "w_t", "logits", "loss", "dlogits", "dl_pad", "dl_cast")


def _counts(C):
    return [max(int(1000 * (5 / 1000) ** (i / (C - 1.0))), 1) for i in range(C)]


def build(arch, head, dt):
    from iif_amd import resnet_cifar, resnet_pytorch
    from iif_amd.custom import IIFLoss
    C, B, hw = NETS[arch]
    counts = _counts(C)
    cifar = arch in R.CIFAR_ARCHS
    sd = (R.init_cifar if cifar else R.init_imagenet)(arch, C, seed=3)
    if head != "linear":
        sd = R.set_head(sd, arch, C, head, seed=1)
    if not cifar:
        damp_residual_branches(sd, arch)
    mod = resnet_cifar if cifar else resnet_pytorch
    kw = {} if cifar else {"pretrained": "None"}
    net = getattr(mod, arch)(num_classes=C, use_norm=head if head != "linear" else "None", compute_dtype=dt, **kw)
    net.load_state_dict(sd)
    x, y = _data(B, hw, counts, seed=41)
    crit = IIFLoss(DS(counts), variant="raw")
    net.train()
    return net, x.to(DEV), y.to(DEV), crit


def step(net, xd, yd, crit):
    cap = U.StepCapture()
    loss, _ = U.run_step(net, xd, yd, crit, capture=cap)
    return cap, loss


def report(tag, met):
    print("\n[%s] %s" % (tag, "  ".join("%s=%.3g(%.1e)" % (k, v, U.HEAD_ERRORS.get(k, 0.0)) for k, v in sorted(met.items()))))


@pytest.mark.parametrize("dt", [BF16, FP32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("arch", list(NETS))
def test_head_against_float64(arch, head, dt):
    """Measured on the MI355X, worst |error| / bound over the eight (network, head) pairs:
        bf16   pooled 1.00  ex 0.99  dex 0.98  dpooled 0.99  dgrad 0.50 (each one or two bf16 roundings: 2^-8 just above a power
               of two is the whole bf16 term)  xnorm 0.02  wn 0.10  wnorm 0.05  logits 0.006  loss 0.02  dlogits 0.19  dwn 0.16
               dw 0.16  db 0.13  ds 0.62  dw_full 2.0e-3 (relative L2)
        fp32   pooled 0.07  ex 0.10  xnorm 0.03  logits 0.03  loss 0.02  dlogits 0.18  dwn 0.25  dw 0.20  db 0.13  ds 0.45
               dex 0.05  dpooled 0.13  dgrad 0.07  dw_full 8.1e-8
        exact in every case: w_cast, wt, w_t, w_pad, dl_pad, dl_cast.
    The softmax of resnet32 / lr_cosine has exponentials below fp32's normal range that the kernel returns as 0 (|error| up to
    2^-126): the bound carries that floor."""
    net, xd, yd, crit = build(arch, head, dt)
    cap, loss = step(net, xd, yd, crit)
    plan = net._saved
    assert plan.dt == dt and plan.head_kind == ("cosine" if head == "lr_cosine" else head)
    met = U.check_head(net, cap, yd, crit)
    report("%s %s %s" % (arch, head, str(dt)[6:]), met)
    want = {"pooled", "w_cast", "logits", "loss", "dlogits", "dl_pad", "dl_cast", "dw", "dw_full", "dpooled", "dgrad"}
    want |= {"db"} if head == "linear" else {"ex", "xnorm", "wn", "wnorm", "w_pad", "wt", "dwn", "dex"}
    want |= {"ds"} if head == "lr_cosine" else set()
    want |= {"w_t"} if head == "norm" else set()
    assert want <= set(met), sorted(want - set(met))
    bad = U.head_failures(met, dt)
    assert not bad, bad
    if (arch, head, dt) == ("resnet50", "cosine", BF16):
        # what test_bf16_cosine_head_runs asserted: two steps with an update in between stay finite, |logits| <= scale
        assert torch.isfinite(torch.tensor(loss)).item()
        net.sgd_step(0.01, 0.9, 1e-4)
        l1, lg = net.loss_and_backward(xd, yd, crit)
        assert torch.isfinite(l1).item() and lg.abs().max().item() <= 16.0 + 1e-2


def _flagged(met, dt):
    return {k for k, _, _ in U.head_failures(met, dt)}


def test_negative_control_weight_gradient_scaled():
    """(a) the head's weight gradient scaled by 0.8 after the step: ``dw`` (and the report-only ``dw_full``, the same tensor
    against the unrounded route) and nothing else."""
    net, xd, yd, crit = build("resnet32", "cosine", BF16)
    cap, _ = step(net, xd, yd, crit)
    assert not U.head_failures(U.check_head(net, cap, yd, crit), BF16)
    net._head._g2d.mul_(0.8)
    met = U.check_head(net, cap, yd, crit)
    assert _flagged(met, BF16) - {"dw_full"} == {"dw"}, U.head_failures(met, BF16)


@pytest.mark.parametrize("which", ["data", "weight"])
def test_negative_control_wrong_norm_in_rowmap_backward(which, monkeypatch):
    """(b) the row-map backward handed norms 5 % too large, at the data call (flags dpooled and, downstream, dgrad) or at the
    weight call (flags dw; dw_full follows); no forward metric either way."""
    from iif_amd import ops
    net, xd, yd, crit = build("resnet32", "cosine", BF16)
    head = net._head
    orig = ops.rowmap_backward

    def patched(x, norms, g, mode, scale, dx, eps=1e-12):
        is_weight = x.data_ptr() == head._w2d.data_ptr()
        if is_weight == (which == "weight"):
            norms = norms * 1.05
        return orig(x, norms, g, mode, scale, dx, eps=eps)

    monkeypatch.setattr(ops, "rowmap_backward", patched)
    cap, _ = step(net, xd, yd, crit)
    met = U.check_head(net, cap, yd, crit)
    got = _flagged(met, BF16)
    assert not got & set(FORWARD), U.head_failures(met, BF16)
    expect = {"dpooled", "dgrad"} if which == "data" else {"dw"}
    assert got - {"dw_full"} == expect, U.head_failures(met, BF16)


def test_negative_control_scale_gradient_halved():
    """(c) lr_cosine with the gradient of the learnable scale halved: ``ds`` only."""
    net, xd, yd, crit = build("resnet32", "lr_cosine", BF16)
    cap, _ = step(net, xd, yd, crit)
    assert not U.head_failures(U.check_head(net, cap, yd, crit), BF16)
    net._head._gs1d.mul_(0.5)
    met = U.check_head(net, cap, yd, crit)
    assert _flagged(met, BF16) == {"ds"}, U.head_failures(met, BF16)
