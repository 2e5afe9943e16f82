"""Padded batches for ``valid_rows=True`` of the class-selected mask predictor and of the fused mask head tail.

A padded batch is an existing case of tests/mask_predictor_cases.py / tests/mask_tail_cases.py with four INVALID rows inserted -
one in front, two in the middle, one at the end - whose labels are ``C, -1, C + 5, 2**40`` and whose ``x`` / ``f`` and targets are
NaN.  The rows that remain after compaction are the case itself, so the float64 reference of a padded batch is the case's own
cached ``reference64``: its divisor is ``K * H * W``, ``K`` the number of valid rows, which is what ``valid_rows=True`` promises.
Both restatements are tied to the reference's own ``FCNMaskHead`` by existing host tests (g31_mask_predictor.npz,
g32_mask_tail.npz); tests/test_mask_valid_rows_host.py ties the compacted call to ``restate64(..., valid=mask)``.

The count cases (tiny: 3 channels, 2 x 2 pixels, 3 classes) take their valid rows from the front of case ``s`` of either file.
"""
import functools

import torch

from tests import mask_predictor_cases as mpc
from tests import mask_tail_cases as mtc

PREDICTOR_CASES = ("a", "c", "d", "e", "g")       # the real tile, odd Cin + soft targets, sub-wave, HW = 63, class_agnostic
TAIL_CASES = ("a", "c", "d", "f")                 # the real 14 x 14 tile, odd sizes, sub-wave, class_agnostic
NOPAD_PREDICTOR, NOPAD_TAIL = "e", "c"

# name -> (N, valid rows): every second row invalid around the 256-thread round of the counting kernel, one valid row among 64,
# no valid row at all
COUNT_CASES = {
    "n1": (1, (0,)),
    "n255": (255, tuple(range(0, 255, 2))),
    "n256": (256, tuple(range(0, 256, 2))),
    "n257": (257, tuple(range(0, 257, 2))),
    "one_of_64": (64, (37,)),
    "none": (64, ()),
}


def invalid_labels(c):
    return [c, -1, c + 5, 2 ** 40]


def layout(n):
    """(bool [n + 4]: which rows of the padded batch are valid) for a case of n rows: one invalid row in front, two after the
    first half, one at the end."""
    h = (n + 1) // 2
    return torch.tensor([False] + [True] * h + [False, False] + [True] * (n - h) + [False])


def _spread(t, valid, fill):
    out = torch.full((valid.numel(),) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    out[valid] = t
    return out


def _pad_labels(labels, valid, c):
    out = _spread(labels, valid, 0)
    out[~valid] = torch.tensor(invalid_labels(c), dtype=torch.int64)[:int((~valid).sum())]
    return out


@functools.lru_cache(maxsize=None)
def predictor_batch(name, fill=float("nan")):
    """(x, weight, bias, labels, targets, valid) of the padded batch of predictor case `name`; `fill`: the contents of the
    invalid rows' x and targets.  Shared: do not modify."""
    x, w, b, lb, t = mpc.inputs(name)
    valid = layout(x.shape[0])
    return _spread(x, valid, fill), w, b, _pad_labels(lb, valid, w.shape[0]), _spread(t, valid, fill), valid


@functools.lru_cache(maxsize=None)
def tail_batch(name, fill=float("nan")):
    """(f, up_weight, up_bias, weight, bias, labels, targets, valid) of the padded batch of tail case `name`.  Shared: do not
    modify."""
    f, uw, ub, w, b, lb, t = mtc.inputs(name)
    valid = layout(f.shape[0])
    return _spread(f, valid, fill), uw, ub, w, b, _pad_labels(lb, valid, w.shape[0]), _spread(t, valid, fill), valid


def _count_batch(rows, labels_at, count):
    n, where = COUNT_CASES[count]
    valid = torch.zeros(n, dtype=torch.bool)
    valid[list(where)] = True
    k = len(where)
    out = [_spread(r[:k], valid, float("nan")) for r in rows]
    lb = _spread(labels_at[:k], valid, 0)
    bad = torch.tensor(invalid_labels(3), dtype=torch.int64)
    lb[~valid] = bad[torch.arange(int((~valid).sum())) % 4]
    return out, lb, valid


@functools.lru_cache(maxsize=None)
def predictor_count_batch(count):
    """(x, weight, bias, labels, targets, valid, reference) - the valid rows are the first K rows of predictor case s; the
    reference is restate64 on them at upstream 1 (None for K = 0)."""
    x, w, b, lb, t = mpc.inputs("s")
    (xp, tp), lbp, valid = _count_batch((x, t), lb, count)
    k = int(valid.sum())
    ref = mpc.restate64(x[:k], w, b, lb[:k], t[:k]) if k else None
    return xp, w, b, lbp, tp, valid, ref


def _e32_tail(f, uw, ub, w, b, lb, t, ref):
    """mask_tail_cases.e32 on given rows: the error of the float32 reference path per gradient, relative to max|d64|."""
    import torch.nn.functional as F
    from oracle import mmdet_iif as M
    leaves = [v.clone().requires_grad_(True) for v in (f, uw, ub, w, b)]
    y = torch.relu(F.conv_transpose2d(leaves[0], leaves[1], leaves[2], stride=2))
    M.mask_cross_entropy(F.conv2d(y, leaves[3], leaves[4]), t, lb).sum().backward()
    got = dict(zip(mtc.GRADS, (v.grad for v in leaves)))
    got["dweight"] = got["dweight"].reshape(w.shape[0], w.shape[1])
    return {k: float((v.double() - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-300) for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def tail_count_batch(count):
    """(f, up_weight, up_bias, weight, bias, labels, targets, valid, reference, tolerances) - the valid rows are the first K rows
    of tail case s; the reference is restate64 on them at upstream 1 (None for K = 0), the tolerance of a gradient
    max(1e-5, 4 * e32) with e32 the float32 reference path's own error on those rows (the rule of mask_tail_cases.grad_tol)."""
    f, uw, ub, w, b, lb, t = mtc.inputs("s")
    (fp, tp), lbp, valid = _count_batch((f, t), lb, count)
    k = int(valid.sum())
    ref = tol = None
    if k:
        ref = mtc.restate64(f[:k], uw, ub, w, b, lb[:k], t[:k])
        e32 = _e32_tail(f[:k], uw, ub, w, b, lb[:k], t[:k], ref)
        tol = {key: max(1e-5, 4.0 * e32[key]) for key in mtc.GRADS}
    return fp, uw, ub, w, b, lbp, tp, valid, ref, tol
