"""Cases of the class-selected mask predictor (iif_amd/mmdet_mask_predictor.py): the seeded input recipe and a float64 restatement.

The restatement is torch on the CPU: an einsum with the SELECTED weight rows only, BCE-with-logits, autograd.
tests/test_mask_predictor_host.py shows that it reproduces the reference's own FCNMaskHead.forward + .loss
(tests/golden/g31_mask_predictor.npz) to 1e-12; the GPU tests compare the kernels against it.

Recipe (torch CPU generator, seeded per case): x = relu(randn); weight ~ N(0, 8 / Cin), which gives logits of standard deviation
about 2 on such an x; bias ~ N(0, 0.01); targets Bernoulli(0.5) as floats, uniform soft targets where the case says so.
"""
import functools

import torch

# name -> (N, C, Cin, H, W, labels or None (seeded random), bias, soft targets)
CASES = {
    "a": (5, 7, 256, 28, 28, [0, 6, 3, 3, 0], True, False),     # the head's real tile; repeated and edge labels
    "b": (9, 4, 256, 28, 28, [3] * 9, True, False),             # one class owns every RoI: the ordered segment sum, dbias
    "c": (33, 80, 80, 14, 14, None, True, True),                # Cin not a multiple of 64; HW = 196; soft targets
    "d": (1, 3, 3, 2, 2, [1], True, False),                     # everything smaller than a wave
    "e": (3, 11, 65, 7, 9, [10, 0, 4], True, False),            # HW = 63: rows not 16-byte aligned, vector tails, odd Cin
    "f": (64, 1203, 256, 28, 28, None, True, False),            # the LVIS class count: >= 1139 zero rows of dweight
    "g": (6, 1, 256, 28, 28, [0] * 6, False, False),            # the class_agnostic head, bias=None
    # s: the smallest N that sends the per-class list builder through a second 2048-RoI piece (eight full rounds of 256, then 3 RoIs);
    # every class owns RoIs on both sides of the boundary; the eight-wide row sum runs with its remainder loop
    "s": (2051, 3, 3, 2, 2, [i % 3 for i in range(2051)], True, False),
}
UP = 2.5                                                        # the upstream factor of the scaled-backward checks


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x [N, Cin, H, W], weight [C, Cin, 1, 1], bias [C] or None, labels int64 [N], targets [N, H, W]) float32, CPU.  Shared:
    do not modify."""
    n, c, cin, h, w, labels, has_bias, soft = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    x = torch.relu(torch.randn(n, cin, h, w, generator=g))
    weight = torch.randn(c, cin, 1, 1, generator=g) * (8.0 / cin) ** 0.5
    bias = torch.randn(c, generator=g) * 0.1 if has_bias else None
    u = torch.rand(n, h, w, generator=g)
    targets = u if soft else (u < 0.5).float()
    lb = torch.randint(0, c, (n,), generator=g) if labels is None else torch.tensor(labels, dtype=torch.int64)
    return x, weight, bias, lb, targets


def restate64(x, weight, bias, labels, targets, up=1.0, valid=None):
    """Float64 restatement on the given values (widened exactly).  Returns a dict of float64 CPU tensors: z [N, H, W], zabs (the
    sum of |w x| + |b| behind every logit: the scale of its rounding bound), loss (1,), and the gradients of (loss * up).sum():
    dx, dweight [C, Cin], dbias [C] (zeros for bias None).  valid: bool [N], RoIs that take part (others: zero loss, zero
    gradients, the divisor stays N * HW) - the contract for labels outside [0, C)."""
    x = x.detach().double().clone().requires_grad_(True)
    c, cin = weight.shape[0], weight.shape[1]
    w2 = weight.detach().double().reshape(c, cin).clone().requires_grad_(True)
    b = (torch.zeros(c, dtype=torch.float64) if bias is None else bias.detach().double().clone()).requires_grad_(True)
    n = x.shape[0]
    valid = torch.ones(n, dtype=torch.bool) if valid is None else valid
    lb = torch.where(valid, labels, torch.zeros_like(labels))
    wsel = w2[lb]                                                        # [N, Cin]: the selected rows only
    z = torch.einsum("nc,nchw->nhw", wsel, x) + b[lb][:, None, None]
    zabs = torch.einsum("nc,nchw->nhw", wsel.detach().abs(), x.detach().abs()) + b.detach()[lb].abs()[:, None, None]
    t = targets.detach().double()
    rows = z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
    rows = rows * valid[:, None, None].double()
    loss = (rows.sum() / rows.numel())[None]
    (loss * up).sum().backward()
    zz = z.detach() * valid[:, None, None].double()
    return dict(z=zz, zabs=zabs, loss=loss.detach(), dx=x.grad, dweight=w2.grad, dbias=b.grad)


@functools.lru_cache(maxsize=None)
def reference64(name, up=1.0, bf16=False):
    """restate64 of a case (bf16: on x rounded to bfloat16 and widened exactly).  Shared: do not modify."""
    x, weight, bias, labels, targets = inputs(name)
    if bf16:
        x = x.bfloat16().float()
    return restate64(x, weight, bias, labels, targets, up)


def selected_rows(labels, c):
    sel = torch.zeros(c, dtype=torch.bool)
    sel[labels[(labels >= 0) & (labels < c)]] = True
    return sel
