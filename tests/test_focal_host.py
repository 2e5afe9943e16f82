"""Sigmoid BCE / focal loss without a device: the reference's fixture (tests/golden/g19_focal.npz) against an fp64
closed form, the 'bce' / 'focal_loss' criterion factory, and the argument checks of iif_sigmoid_focal_fwd_bwd
(which return before any HIP call)."""
import types

import numpy as np
import pytest

from iif_amd import _lib

from .focal_cases import closed_form, golden_cases, golden_mixup

EINVAL = -1


def test_fixture_matches_fp64_closed_form(golden):
    g = golden("g19_focal")
    n = 0
    for name, x, t, kw, loss, grad, rows in golden_cases(g):
        cl, cg = closed_form(x, t, **kw)
        assert abs(loss - cl) <= 1e-4 * abs(cl), name
        assert np.abs(grad - cg[rows]).max() <= 1e-4 * np.abs(cg).max(), name
        n += 1
    assert n == 130
    x, ya, yb, lam, kw, loss, grad, rows = golden_mixup(g)
    cl, cg = closed_form(x, ya, targets_b=yb, lam=lam, **kw)
    assert abs(loss - cl) <= 1e-4 * abs(cl)
    assert np.abs(grad - cg[rows]).max() <= 1e-4 * np.abs(cg).max()


class DS:
    def get_cls_num_list(self):
        return [500, 200, 80, 30, 10]


def _args(classif, deffered, **kw):
    a = dict(classif=classif, deffered=deffered, reduction="sum", gamma=2.0, alpha=0.25, iif="raw", iif_norm=0,
             device="cpu")
    a.update(kw)
    return types.SimpleNamespace(**a)


@pytest.mark.parametrize("deffered", [False, True])
def test_get_criterion_bce_and_focal_loss(deffered):
    import torch
    from iif_amd import custom, initialisers
    w = torch.tensor([500, 200, 80, 30, 10])
    w = w.sum() / w
    bce = initialisers.get_criterion(_args("bce", deffered), DS(), None, 5)
    assert isinstance(bce, custom.FocalLoss)
    assert bce.gamma == 0 and bce.alpha is None and bce.reduction == "sum"
    fl = initialisers.get_criterion(_args("focal_loss", deffered, reduction="mean"), DS(), None, 5)
    assert isinstance(fl, custom.FocalLoss)
    assert fl.gamma == 2.0 and fl.alpha == 0.25 and fl.reduction == "mean"
    for crit in (bce, fl):
        if deffered:
            assert tuple(crit.weights.shape) == (1, 5) and torch.equal(crit.weights[0], w)
        else:
            assert crit.weights == 1
        assert not hasattr(crit, "iif")               # train.evaluate scores raw logits
    fl.set_weights(w)
    assert torch.equal(fl.weights, w.unsqueeze(0))
    assert fl.scale(8, 5) == 1.0 / 40 and bce.scale(8, 5) == 1.0 / 8


def test_get_criterion_unknown_name_still_raises():
    from iif_amd import initialisers
    with pytest.raises(NotImplementedError):
        initialisers.get_criterion(_args("asl", False), DS(), None, 5)


def _call(logits=0x1000, dtype=_lib.IIF_F32, ld=16, ta=0x2000, gamma=2.0, B=4, C=10, rows=0x3000, dx=0, lddx=16):
    return _lib.lib().iif_sigmoid_focal_fwd_bwd(logits, dtype, ld, ta, 0, 1.0, 0, gamma, 1, 0.25, 0.1, B, C, rows, 0,
                                                dx, lddx, 0, 0, 0)


@pytest.mark.parametrize("kw", [
    dict(B=-1), dict(C=0), dict(C=-3), dict(dtype=7), dict(logits=0), dict(ta=0), dict(rows=0),
    dict(gamma=-0.5), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(ld=9),
    dict(dx=0x4000, lddx=9), dict(logits=0x1002), dict(dx=0x4001)])
def test_sigmoid_focal_entry_rejects_bad_arguments(kw):
    assert _call(**kw) == EINVAL
