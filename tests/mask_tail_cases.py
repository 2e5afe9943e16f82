"""Cases of the fused mask head tail (iif_amd/mmdet_mask_tail.py): the seeded input recipe, a float64 restatement and the error of
the float32 reference path that the GPU tolerances rest on.

The restatement is torch on the CPU: conv_transpose2d, relu, an einsum with the SELECTED weight rows only, BCE-with-logits,
autograd.  tests/test_mask_tail_host.py shows that it reproduces the reference's own FCNMaskHead.forward + .loss
(tests/golden/g32_mask_tail.npz) to 1e-12; the GPU tests compare the kernels against it.

Grid inputs.  The ReLU makes the gradients discontinuous in pre = up_bias + sum f * up_weight, so the cases put f, up_weight and
up_bias on a dyadic grid on which pre is exact in float32 in ANY summation order:
    f         = clamp(round(relu(randn) * 8), 0, 32) / 8                                 multiples of 2^-3, at most 4
    up_weight = clamp(round(randn * max(sqrt(2 / Ci), 1 / 16) * 64), -64, 64) / 64       multiples of 2^-6, at most 1
    up_bias   = round(randn * 6.4) / 64                                                  multiples of 2^-6
Every product is a multiple of 2^-9 and every partial sum is below 2^13 for Ci <= 1024: 22 bits.  f is exact in bfloat16 too.
weight ~ N(0, 8 / Co), bias ~ N(0, 0.01) and the targets are ordinary floats.  Case r has plain randn inputs (logits and loss only).
"""
import functools

import torch
import torch.nn.functional as F

# name -> (N, C, Ci, Co, h, w, labels or None (seeded random), bias, soft targets)
CASES = {
    "a": (3, 5, 256, 256, 14, 14, [4, 0, 0], True, False),      # the real tile; hw = 196 is no tile multiple; a repeated label
    "b": (4, 5, 8, 8, 5, 5, [4, 0, 2, 2], True, True),          # the fixture's shape
    "c": (3, 4, 65, 33, 3, 5, [3, 3, 1], True, False),          # odd Ci / Co, 60 output pixels per RoI
    "d": (1, 2, 3, 3, 2, 2, [1], True, False),                  # smaller than a wave
    "e": (70, 1203, 256, 256, 14, 14, None, True, False),       # more RoIs than any split: dup_weight sums 13 720 rows; LVIS
    "f": (6, 1, 256, 256, 14, 14, [0] * 6, False, False),       # the class_agnostic head, bias=None
    "g": (5, 7, 300, 130, 7, 7, None, True, True),              # Co > 128 and no tile multiple
    "r": (3, 5, 256, 256, 14, 14, [4, 0, 0], True, False),      # a's shape, plain randn inputs
    # s: the smallest N that sends the per-class list builder through a second 2048-RoI piece (eight full rounds of 256, then 3 RoIs);
    # every class owns RoIs on both sides of the boundary; the eight-wide row sum runs with its remainder loop
    "s": (2051, 3, 3, 3, 2, 2, [i % 3 for i in range(2051)], True, False),
}
GRID_CASES = ("a", "b", "c", "d", "e", "f", "g", "s")
UP = 2.5                                                        # the upstream factor of the scaled-backward checks
GRADS = ("df", "dup_weight", "dup_bias", "dweight", "dbias")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(f [N, Ci, h, w], up_weight [Ci, Co, 2, 2], up_bias [Co], weight [C, Co, 1, 1], bias [C] or None, labels int64 [N],
    targets [N, 2h, 2w]) float32, CPU.  Shared: do not modify."""
    n, c, ci, co, h, w, labels, has_bias, soft = CASES[name]
    g = torch.Generator().manual_seed(2000 + sorted(CASES).index(name))
    if name == "r":
        f = torch.randn(n, ci, h, w, generator=g)
        up_weight = torch.randn(ci, co, 2, 2, generator=g) * (2.0 / ci) ** 0.5
        up_bias = torch.randn(co, generator=g) * 0.1
    else:
        f = torch.clamp(torch.round(torch.relu(torch.randn(n, ci, h, w, generator=g)) * 8), 0, 32) / 8
        up_weight = torch.clamp(torch.round(torch.randn(ci, co, 2, 2, generator=g) * max((2.0 / ci) ** 0.5, 1 / 16) * 64), -64, 64) / 64
        up_bias = torch.round(torch.randn(co, generator=g) * 6.4) / 64
    weight = torch.randn(c, co, 1, 1, generator=g) * (8.0 / co) ** 0.5
    bias = torch.randn(c, generator=g) * 0.1 if has_bias else None
    u = torch.rand(n, 2 * h, 2 * w, generator=g)
    targets = u if soft else (u < 0.5).float()
    lb = torch.randint(0, c, (n,), generator=g) if labels is None else torch.tensor(labels, dtype=torch.int64)
    return f, up_weight, up_bias, weight, bias, lb, targets


def restate64(f, up_weight, up_bias, weight, bias, labels, targets, up=1.0, valid=None):
    """Float64 restatement on the given values (widened exactly).  Returns a dict of float64 CPU tensors: pre [N, Co, 2h, 2w],
    z [N, 2h, 2w], zabs_bound (sum_co |weight[l, co]| (sum_ci |f up_weight| + |up_bias[co]|) + |bias[l]|: the scale of the
    first-order rounding bound of the two nested sums), loss (1,), and the gradients of (loss * up).sum(): df, dup_weight,
    dup_bias, dweight [C, Co], dbias [C] (zeros for bias None).  valid: bool [N], RoIs that take part (others: zero loss, zero
    gradients, the divisor stays N * 4hw) - the contract for labels outside [0, C)."""
    f = f.detach().double().clone().requires_grad_(True)
    uw = up_weight.detach().double().clone().requires_grad_(True)
    ub = up_bias.detach().double().clone().requires_grad_(True)
    c, co = weight.shape[0], weight.shape[1]
    w2 = weight.detach().double().reshape(c, co).clone().requires_grad_(True)
    b = (torch.zeros(c, dtype=torch.float64) if bias is None else bias.detach().double().clone()).requires_grad_(True)
    n = f.shape[0]
    valid = torch.ones(n, dtype=torch.bool) if valid is None else valid
    lb = torch.where(valid, labels, torch.zeros_like(labels))
    pre = F.conv_transpose2d(f, uw, ub, stride=2)
    y = torch.relu(pre)
    wsel = w2[lb]                                                        # [N, Co]: the selected rows only
    z = torch.einsum("nc,nchw->nhw", wsel, y) + b[lb][:, None, None]
    with torch.no_grad():
        inner = F.conv_transpose2d(f.abs(), uw.abs(), ub.abs(), stride=2)
        zabs = torch.einsum("nc,nchw->nhw", wsel.abs(), inner) + b[lb].abs()[:, None, None]
    t = targets.detach().double()
    rows = z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
    rows = rows * valid[:, None, None].double()
    loss = (rows.sum() / rows.numel())[None]
    (loss * up).sum().backward()
    zz = z.detach() * valid[:, None, None].double()
    return dict(pre=pre.detach(), z=zz, zabs_bound=zabs, loss=loss.detach(), df=f.grad, dup_weight=uw.grad, dup_bias=ub.grad,
                dweight=w2.grad, dbias=b.grad)


@functools.lru_cache(maxsize=None)
def reference64(name, up=1.0):
    """restate64 of a case.  Shared: do not modify.  (The grid f is exact in bfloat16: the bfloat16 runs share it.)"""
    return restate64(*inputs(name), up)


@functools.lru_cache(maxsize=None)
def e32(name):
    """The error of the float32 REFERENCE path on a case, per tensor, relative to max|d64|: torch CPU float32 conv_transpose2d,
    relu, F.conv2d to all C channels and oracle.mmdet_iif.mask_cross_entropy against the restatement.  'loss' is absolute.  The
    GPU gradient tolerance of a tensor is max(1e-5, 4 * e32): it never comes from the code under test."""
    from oracle import mmdet_iif as M
    f, up_weight, up_bias, weight, bias, labels, targets = inputs(name)
    r = reference64(name)
    leaves = [t.clone().requires_grad_(True) for t in (f, up_weight, up_bias, weight)]
    bs = None if bias is None else bias.clone().requires_grad_(True)
    y = torch.relu(F.conv_transpose2d(leaves[0], leaves[1], leaves[2], stride=2))
    loss = M.mask_cross_entropy(F.conv2d(y, leaves[3], bs), targets, labels)
    loss.sum().backward()
    c, co = weight.shape[:2]
    got = dict(df=leaves[0].grad, dup_weight=leaves[1].grad, dup_bias=leaves[2].grad, dweight=leaves[3].grad.reshape(c, co))
    if bs is not None:
        got["dbias"] = bs.grad
    out = {k: float((v.double() - r[k]).abs().max()) / max(float(r[k].abs().max()), 1e-300) for k, v in got.items()}
    out["loss"] = abs(float(loss.detach()) - float(r["loss"]))
    return out


def grad_tol(name, key):
    return max(1e-5, 4.0 * e32(name).get(key, 0.0))


def selected_rows(labels, c):
    sel = torch.zeros(c, dtype=torch.bool)
    sel[labels[(labels >= 0) & (labels < c)]] = True
    return sel
