"""Host-side checks of the class-selected mask predictor (iif_amd/mmdet_mask_predictor.py, csrc/mask_predictor.hip): no device.

  * the float64 restatement of tests/mask_predictor_cases.py reproduces the REFERENCE's own FCNMaskHead.forward + .loss
    (tests/golden/g31_mask_predictor.npz, written by tests/golden/make_golden_mask_predictor.py) to 1e-12, and the reference's
    own gradient rows of unselected classes are exactly zero: the equivalence the feature rests on;
  * torch-CPU float32 F.conv2d + oracle.mmdet_iif.mask_cross_entropy - what a float32 run of the reference computes - stays
    within 2.5e-6 of the restatement on every case the GPU tests use, which is what gives their 1e-5 a margin of 4x;
  * the module contract and the argument checks of the three C entries (they return before any launch).
"""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from iif_amd import _lib
from oracle import mmdet_iif as M
from tests import mask_predictor_cases as mpc

GOLDEN_CASES = ("multi", "soft", "agnostic")


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_restatement_reproduces_the_reference_head(golden, name):
    g = golden("g31_mask_predictor")
    get = lambda k, p: torch.from_numpy(g["%s_%s_%s" % (name, k, p)])          # noqa: E731
    labels = get("labels", "f64")
    c = get("weight", "f64").shape[0]
    if c == 1:                                                                  # the class_agnostic head: FCNMaskHead.loss passes zeros
        labels = torch.zeros_like(labels)
    r = mpc.restate64(get("x", "f64"), get("weight", "f64"), get("bias", "f64"), labels, get("targets", "f64"))
    assert abs(float(r["loss"]) - float(get("loss", "f64"))) <= 1e-12 * abs(float(get("loss", "f64")))
    assert _rel(r["dx"], get("dx", "f64")) <= 1e-12
    assert _rel(r["dweight"], get("dweight", "f64").reshape(c, -1)) <= 1e-12
    assert _rel(r["dbias"], get("dbias", "f64")) <= 1e-12
    # in the reference's OWN gradients (both precisions) the rows of classes no RoI has are exactly zero
    unsel = ~mpc.selected_rows(labels, c)
    for p in ("f64", "f32"):
        assert not get("dweight", p)[unsel].any() and not get("dbias", p)[unsel].any()
        assert get("dweight", p)[~unsel].reshape(int((~unsel).sum()), -1).any(1).all()
    assert (unsel.sum() > 0) == (c > 1)


@pytest.mark.parametrize("name", sorted(mpc.CASES))
def test_float32_reference_error_leaves_the_gpu_tolerance_a_margin(name):
    """The float32 reference path against the float64 restatement: within 2.5e-6 x max|.| for dx, dweight, dbias and 2.5e-6 for
    the loss (measured worst case with this recipe: 1.1e-6, dweight of case f), a quarter of the GPU tests' 1e-5."""
    x, weight, bias, labels, targets = mpc.inputs(name)
    r = mpc.reference64(name)
    xs = x.clone().requires_grad_(True)
    ws = weight.clone().requires_grad_(True)
    bs = None if bias is None else bias.clone().requires_grad_(True)
    loss = M.mask_cross_entropy(F.conv2d(xs, ws, bs), targets, labels)
    loss.sum().backward()
    c, cin = weight.shape[:2]
    sel = mpc.selected_rows(labels, c)
    assert not ws.grad[~sel].any()
    errs = dict(loss=abs(float(loss.detach()) - float(r["loss"])), dx=_rel(xs.grad.double(), r["dx"]),
                dweight=_rel(ws.grad.double().reshape(c, cin), r["dweight"]))
    if bs is not None:
        errs["dbias"] = _rel(bs.grad.double(), r["dbias"])
    print(name, {k: "%.2e" % v for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= 2.5e-6, (name, k, v)


def test_module_matches_conv2d_state_dict_and_round_trips():
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor
    for cin, c, agnostic in ((256, 1203, False), (16, 5, False), (256, 80, True)):
        m = ClassSelectedMaskPredictor(cin, c, class_agnostic=agnostic)
        conv = nn.Conv2d(cin, 1 if agnostic else c, 1)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in conv.state_dict().items()}
        assert list(m.state_dict()) == list(conv.state_dict())
        m.load_state_dict(conv.state_dict())                        # a reference checkpoint's conv_logits.* loads unchanged
        back = m.to_conv()
        assert torch.equal(back.weight, conv.weight) and torch.equal(back.bias, conv.bias)
        again = ClassSelectedMaskPredictor.from_conv(conv)
        assert again.class_agnostic == (conv.out_channels == 1)
        assert torch.equal(again.weight, conv.weight) and torch.equal(again.bias, conv.bias)
    with pytest.raises(NotImplementedError):
        ClassSelectedMaskPredictor.from_conv(nn.Conv2d(4, 4, 3))


def test_module_initialisation_is_the_references():
    """kaiming_normal_(mode='fan_out', nonlinearity='relu'): N(0, 2 / C) for a 1x1 kernel; zero bias (fcn_mask_head.py:123-125)."""
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor
    torch.manual_seed(5)
    m = ClassSelectedMaskPredictor(256, 1203)
    assert not m.bias.any()
    std = (2.0 / 1203) ** 0.5
    w = m.weight.detach().double()
    n = w.numel()
    assert abs(float(w.mean())) <= 5 * std / n ** 0.5
    assert abs(float(w.std()) / std - 1) <= 5 / (2 * n) ** 0.5       # five standard errors of a normal sample's deviation
    assert float(w.abs().max()) <= 7 * std
    torch.manual_seed(5)                                             # and it IS that initialiser: the same draws
    ref = torch.empty(1203, 256, 1, 1)
    nn.init.kaiming_normal_(ref, mode="fan_out", nonlinearity="relu")
    assert torch.equal(m.weight.detach(), ref)


def test_cpu_tensors_shapes_and_dtypes_raise(monkeypatch):
    from iif_amd.mmdet_mask_predictor import ClassSelectedMaskPredictor, class_mask_logits, class_mask_loss
    x = torch.zeros(2, 4, 3, 3)
    w = torch.zeros(5, 4, 1, 1)
    b = torch.zeros(5)
    lb = torch.zeros(2, dtype=torch.int64)
    t = torch.zeros(2, 3, 3)
    with pytest.raises(_lib.IIFNativeError):
        class_mask_logits(x, w, b, lb)
    with pytest.raises(_lib.IIFNativeError):
        class_mask_loss(x, w, b, lb, t)
    with pytest.raises(_lib.IIFNativeError):
        class_mask_loss(x[:0], w, b, lb[:0], t[:0])
    m = ClassSelectedMaskPredictor(4, 5)
    with pytest.raises(_lib.IIFNativeError):
        m(x, lb)
    with pytest.raises(_lib.IIFNativeError):
        m.loss(x, lb, t)
    # shapes and dtypes, with the device check out of the way
    from iif_amd import mmdet_mask_predictor as mp
    monkeypatch.setattr(_lib, "require_gpu", lambda *a: None)
    for bad in ((x[0], w, b, lb), (x, w[:, :3], b, lb), (x, torch.zeros(5, 4, 3, 3), b, lb), (x, w, b[:4], lb), (x, w, b, lb[:1]),
                (x, torch.zeros(5, 4, 1), b, lb), (torch.zeros(2, 4, 65, 64), w, b, lb), (torch.zeros(2, 2049, 1, 1), torch.zeros(5, 2049), b, lb)):
        with pytest.raises(ValueError):
            mp._prep(*bad)
    for bad in ((x.half(), w, b, lb), (x.double(), w, b, lb), (x, w.double(), b, lb), (x, w, b.bfloat16(), lb), (x.bfloat16(), w.bfloat16(), b, lb),
                (x, w, b, lb.float())):
        with pytest.raises(NotImplementedError):
            mp._prep(*bad)
    out = mp._prep(x.bfloat16().to(memory_format=torch.channels_last), w.reshape(5, 4), None, lb.int())
    assert out[0].is_contiguous() and out[3].dtype == torch.int64 and out[4:] == (2, 5, 4, 9)
    wide = torch.zeros(5, 7, 1, 1)[:, :4]                          # a row-strided view is read in place
    assert mp._ld(mp._prep(x, wide, b, lb)[1]) == 7


def test_c_entries_reject_bad_arguments_before_any_launch():
    """As the iif_slab_sum checks of tests/test_cabi.py: host buffers stand in for device memory, nothing may be launched."""
    L = _lib.lib()
    raw = (ctypes.c_float * 64)()
    p = ctypes.addressof(raw)
    F32 = _lib.IIF_F32
    fwd = lambda **k: L.iif_mask_predict_fwd(*[k.get(a, d) for a, d in (                       # noqa: E731
        ("x", p), ("dtype", F32), ("weight", p), ("ld_w", 4), ("bias", p), ("labels", p), ("target", p), ("n", 2), ("c", 3), ("cin", 4),
        ("hw", 4), ("z", p), ("g0", p), ("rows", p), ("loss", p), ("status", p), ("stream", None))])
    dxe = lambda **k: L.iif_mask_predict_bwd_input(*[k.get(a, d) for a, d in (                # noqa: E731
        ("g", p), ("up", None), ("weight", p), ("ld_w", 4), ("labels", p), ("n", 2), ("c", 3), ("cin", 4), ("hw", 4), ("dx", p),
        ("dtype", F32), ("stream", None))])
    dwe = lambda **k: L.iif_mask_predict_bwd_weight(*[k.get(a, d) for a, d in (               # noqa: E731
        ("x", p), ("dtype", F32), ("g", p), ("up", None), ("labels", p), ("n", 2), ("c", 3), ("cin", 4), ("hw", 4), ("scratch", p),
        ("dweight", p), ("dbias", p), ("stream", None))])
    for entry, ptrs in ((fwd, ("x", "weight", "labels", "status", "rows", "loss")), (dxe, ("g", "weight", "labels", "dx")),
                        (dwe, ("x", "g", "labels", "scratch"))):
        for name in ptrs:
            assert entry(**{name: None}) == -1, name
        assert entry(cin=0) == -1 and entry(cin=2049) == -1
        assert entry(hw=0) == -1 and entry(hw=4097) == -1
        assert entry(n=-1) == -1 and entry(n=65536) == -1
        assert entry(c=0) == -1 and entry(c=-3) == -1
        assert entry(dtype=7) == -1
        assert entry(n=0) == 0                                        # nothing to do: IIF_OK, nothing enqueued
    assert fwd(ld_w=3) == -1 and dxe(ld_w=3) == -1                    # rows that overlap
    assert fwd(z=None, target=None) == -1                             # nothing asked for
    assert fwd(target=None) == -1                                     # g0 without a target
    assert dwe(dweight=None, dbias=None) == -1
