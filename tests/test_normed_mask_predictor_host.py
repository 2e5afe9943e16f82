"""Host-side checks of the class-selected NormedConv2d mask predictor (iif_amd/mmdet_normed_mask_predictor.py,
csrc/normed_mask_predictor.hip): no device.

  * the float64 restatement of tests/normed_mask_predictor_cases.py reproduces the REFERENCE's own
    FCNMaskHead(predictor_cfg=dict(type='NormedConv2d', tempearture=20)) forward + .loss
    (tests/golden/g35_normed_mask_predictor.npz, written by tests/golden/make_golden_normed_mask_predictor.py) to 1e-12 -
    power 2 and pixels that are zero in every channel included - and the reference's own gradient rows of unselected classes are
    exactly zero: the equivalence the feature rests on;
  * the float32 torch-CPU reference path (oracle.mmdet_iif.normed_conv2d_1x1 + mask_cross_entropy + autograd) against the
    restatement on every case the GPU tests use: its logits sit within HALF the GPU test's per-element bound, and its worst
    relative errors are what normed_mask_predictor_cases.F32_REFERENCE_ERROR records (the GPU tolerance is 4x that record);
  * valid_rows in the restatement: everything is the plain mean's times N / max(1, n_valid);
  * the module contract and the argument checks of the three C entries (they return before any launch).
"""
import ctypes

import pytest
import torch
import torch.nn as nn

from iif_amd import _lib
from tests import normed_mask_predictor_cases as K

GOLDEN_CASES = ("multi", "soft", "agnostic", "power2", "zeropix")


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_restatement_reproduces_the_reference_head(golden, name):
    g = golden("g35_normed_mask_predictor")
    get = lambda k, p: torch.from_numpy(g["%s_%s_%s" % (name, k, p)])          # noqa: E731
    labels = get("labels", "f64")
    c = get("weight", "f64").shape[0]
    if c == 1:                                                                  # the class_agnostic head: FCNMaskHead.loss passes zeros
        labels = torch.zeros_like(labels)
    temp, power, eps = (float(v) for v in get("cfg", "f64"))
    assert temp == 20 and power == (2 if name == "power2" else 1) and eps == 1e-6
    x = get("x", "f64")
    if name == "zeropix":                                                       # (with 8 post-ReLU channels a few more occur by chance)
        assert int((x.abs().sum(1) == 0).sum()) >= 3
    r = K.restate64(x, get("weight", "f64"), get("bias", "f64"), labels, get("targets", "f64"), temp, power, eps)
    assert abs(float(r["loss"]) - float(get("loss", "f64"))) <= 1e-12 * abs(float(get("loss", "f64")))
    assert _rel(r["dx"], get("dx", "f64")) <= 1e-12
    assert _rel(r["dweight"], get("dweight", "f64").reshape(c, -1)) <= 1e-12
    assert _rel(r["dbias"], get("dbias", "f64")) <= 1e-12
    # in the reference's OWN gradients (both precisions) the rows of classes no RoI has are exactly zero
    unsel = ~K.selected_rows(labels, c)
    for p in ("f64", "f32"):
        assert not get("dweight", p)[unsel].any() and not get("dbias", p)[unsel].any()
        assert get("dweight", p)[~unsel].reshape(int((~unsel).sum()), -1).any(1).all()
    assert (unsel.sum() > 0) == (c > 1)


def test_zero_pixel_gradient_is_the_subgradient_form(golden):
    """Where a pixel is zero in every channel the reference's dx is g * s_x * what with s_x = T / eps: the B term is exactly 0."""
    g = golden("g35_normed_mask_predictor")
    get = lambda k: torch.from_numpy(g["zeropix_%s_f64" % k])                   # noqa: E731
    x, w, b, labels, t, dx = get("x"), get("weight")[:, :, 0, 0], get("bias"), get("labels"), get("targets"), get("dx")
    n, cin, h, wd = x.shape
    hits = 0
    for i, y, xx in (x.abs().sum(1) == 0).nonzero().tolist():
        what = w[labels[i]] / (w[labels[i]].norm() + 1e-6)
        gg = (torch.sigmoid(b[labels[i]]) - t[i, y, xx]) / (n * h * wd)          # z = bias there
        want = gg * (20 / 1e-6) * what
        assert float((dx[i, :, y, xx] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        hits += 1
    assert hits >= 3


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_float32_reference_error_sets_the_gpu_tolerance(name):
    """The float32 reference path against the float64 restatement, per case: the logits within half the GPU test's bound (so
    the bound's constant needs no widening), and loss / dx / dweight / dbias errors relative to the largest element.  Measured
    here per quantity, worst over the cases: loss 8.55e-8 (h), dx 5.07e-7 (h), dweight 5.47e-7 (f), dbias 1.10e-6 (f); logits at
    most 0.023 of the bound (c).  F32_REFERENCE_ERROR records those figures; a float32 run whose summation order differs (other
    thread counts) may land elsewhere, but within twice the record the GPU tolerance of 4x keeps a margin of at least 2."""
    n, c, cin = K.CASES[name][:3]
    r = K.reference64(name)
    z, loss, dx, dw, db = K.float32_reference(name)
    labels = K.inputs(name)[3]
    assert not dw[~K.selected_rows(labels, c)].any()
    zfrac = float(((z.double() - r["z"]).abs() / K.logit_bound(r, cin, K.cfg(name)[1])).max())
    errs = dict(loss=abs(float(loss) - float(r["loss"])) / max(1.0, abs(float(r["loss"]))), dx=_rel(dx.double(), r["dx"]),
                dweight=_rel(dw.double(), r["dweight"]))
    if db is not None:
        errs["dbias"] = _rel(db.double(), r["dbias"])
    print(name, "logits / bound %.3f" % zfrac, {k: "%.2e" % v for k, v in errs.items()})
    assert zfrac <= 0.5
    for k, v in errs.items():
        assert v <= 2 * K.F32_REFERENCE_ERROR[k], (name, k, v)
    assert K.GPU_TOLERANCE == {k: 4 * v for k, v in K.F32_REFERENCE_ERROR.items()}


@pytest.mark.parametrize("which", sorted(K.VALID_ROWS_LABELS))
def test_valid_rows_is_the_plain_mean_rescaled(which):
    """In the restatement the valid-row divisor multiplies the loss and every gradient by N / max(1, n_valid)."""
    x, weight, bias, _, targets = K.inputs("a")
    n, c = K.CASES["a"][:2]
    labels = torch.tensor(K.VALID_ROWS_LABELS[which], dtype=torch.int64)
    valid = (labels >= 0) & (labels < c)
    nv = int(valid.sum())
    assert nv == dict(none=5, mixed=3, all=0)[which]
    plain = K.restate64(x, weight, bias, labels, targets, valid=valid)
    vr = K.restate64(x, weight, bias, labels, targets, valid=valid, valid_rows=True)
    f = n / max(1, nv)
    for k in ("loss", "dx", "dweight", "dbias"):
        assert float((vr[k] - plain[k] * f).abs().max()) <= 1e-12 * float((plain[k] * f).abs().max()), k
        assert bool(torch.isfinite(vr[k]).all())
        assert bool(vr[k].any()) == (nv > 0)
    assert not vr["dx"][~valid].any()


def test_module_matches_normed_conv2d_state_dict_and_round_trips():
    from iif_amd.mmdet_normed_mask_predictor import ClassSelectedNormedMaskPredictor
    from iif_amd.mmdet_normed_predictor import NormedConv2d
    for cin, c, agnostic, kw in ((256, 1203, False, {}), (16, 5, False, dict(tempearture=8, power=2.0, eps=1e-5)),
                                 (256, 80, True, dict(norm_over_kernel=True))):
        m = ClassSelectedNormedMaskPredictor(cin, c, class_agnostic=agnostic, **kw)
        conv = NormedConv2d(cin, 1 if agnostic else c, 1, **kw)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in conv.state_dict().items()}
        assert list(m.state_dict()) == list(conv.state_dict())
        m.load_state_dict(conv.state_dict())                        # a reference checkpoint's conv_logits.* loads unchanged
        back = m.to_conv()
        assert type(back) is NormedConv2d
        assert torch.equal(back.weight, conv.weight) and torch.equal(back.bias, conv.bias)
        again = ClassSelectedNormedMaskPredictor.from_conv(conv)
        assert again.class_agnostic == (conv.out_channels == 1)
        assert torch.equal(again.weight, conv.weight) and torch.equal(again.bias, conv.bias)
        for k in ("tempearture", "power", "eps", "norm_over_kernel"):
            assert getattr(again, k) == getattr(conv, k) == getattr(back, k) == getattr(m, k)
    with pytest.raises(NotImplementedError):
        ClassSelectedNormedMaskPredictor.from_conv(nn.Conv2d(4, 4, 1))             # a plain convolution is the other module's
    with pytest.raises(NotImplementedError):
        ClassSelectedNormedMaskPredictor.from_conv(NormedConv2d(4, 4, 3, padding=1))
    with pytest.raises(ValueError):
        ClassSelectedNormedMaskPredictor(4, 4, power=0)


def test_module_initialisation_is_the_references():
    """kaiming_normal_(mode='fan_out', nonlinearity='relu'), zero bias: what FCNMaskHead.init_weights gives conv_logits
    (fcn_mask_head.py:117-125) - the same draws under the same seed."""
    from iif_amd.mmdet_normed_mask_predictor import ClassSelectedNormedMaskPredictor
    torch.manual_seed(5)
    m = ClassSelectedNormedMaskPredictor(256, 1203)
    assert not m.bias.any() and (m.tempearture, m.power, m.eps) == (20, 1.0, 1e-6)
    torch.manual_seed(5)
    ref = torch.empty(1203, 256, 1, 1)
    nn.init.kaiming_normal_(ref, mode="fan_out", nonlinearity="relu")
    assert torch.equal(m.weight.detach(), ref)


def test_cpu_tensors_shapes_and_dtypes_raise(monkeypatch):
    from iif_amd.mmdet_normed_mask_predictor import (ClassSelectedNormedMaskPredictor, normed_class_mask_logits,
                                                     normed_class_mask_loss)
    x = torch.zeros(2, 4, 3, 3)
    w = torch.zeros(5, 4, 1, 1)
    b = torch.zeros(5)
    lb = torch.zeros(2, dtype=torch.int64)
    t = torch.zeros(2, 3, 3)
    with pytest.raises(_lib.IIFNativeError):
        normed_class_mask_logits(x, w, b, lb)
    with pytest.raises(_lib.IIFNativeError):
        normed_class_mask_loss(x, w, b, lb, t)
    with pytest.raises(_lib.IIFNativeError):
        normed_class_mask_loss(x, w, b, lb, t, valid_rows=True)
    with pytest.raises(_lib.IIFNativeError):
        normed_class_mask_loss(x[:0], w, b, lb[:0], t[:0])
    m = ClassSelectedNormedMaskPredictor(4, 5)
    with pytest.raises(_lib.IIFNativeError):
        m(x, lb)
    with pytest.raises(_lib.IIFNativeError):
        m.loss(x, lb, t, valid_rows=True)
    with pytest.raises(ValueError):
        normed_class_mask_logits(x, w, b, lb, power=0.0)
    with pytest.raises(ValueError):
        normed_class_mask_loss(x, w, b, lb, t, power=-1)
    # shapes and dtypes, with the device check out of the way: the functions reach the shared argument checks
    monkeypatch.setattr(_lib, "require_gpu", lambda *a: None)
    for bad in ((x[0], w, b, lb), (x, w[:, :3], b, lb), (x, torch.zeros(5, 4, 3, 3), b, lb), (x, w, b[:4], lb), (x, w, b, lb[:1]),
                (torch.zeros(2, 4, 65, 64), w, b, lb), (torch.zeros(2, 2049, 1, 1), torch.zeros(5, 2049), b, lb)):
        with pytest.raises(ValueError):
            normed_class_mask_logits(*bad)
        with pytest.raises(ValueError):
            normed_class_mask_loss(*bad, t)
    for bad in ((x.half(), w, b, lb), (x.double(), w, b, lb), (x, w.double(), b, lb), (x, w, b.bfloat16(), lb), (x, w, b, lb.float())):
        with pytest.raises(NotImplementedError):
            normed_class_mask_logits(*bad)
        with pytest.raises(NotImplementedError):
            normed_class_mask_loss(*bad, t)
    # the class_agnostic module reads channel 0, and with valid_rows keeps a padded row (label num_classes) invalid
    m = ClassSelectedNormedMaskPredictor(4, 5, class_agnostic=True)
    lbs = torch.tensor([3, 5, -1, 0])
    assert m._labels(lbs).tolist() == [0, 0, 0, 0] and m._labels(lbs, True).tolist() == [0, -1, -1, 0]


def test_c_entries_reject_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory, nothing may be launched."""
    L = _lib.lib()
    raw = (ctypes.c_float * 64)()
    p = ctypes.addressof(raw)
    F32 = _lib.IIF_F32
    fwd = lambda **k: L.iif_normed_mask_predict_fwd(*[k.get(a, d) for a, d in (              # noqa: E731
        ("x", p), ("dtype", F32), ("weight", p), ("ld_w", 4), ("bias", p), ("labels", p), ("target", p), ("n", 2), ("c", 3), ("cin", 4),
        ("hw", 4), ("temp", 20.0), ("power", 1.0), ("eps", 1e-6), ("valid_rows", 0), ("z", p), ("g", p), ("a", p), ("b", p), ("rows", p),
        ("loss", p), ("inv", p), ("stream", None))])
    dxe = lambda **k: L.iif_normed_mask_predict_bwd_input(*[k.get(a, d) for a, d in (        # noqa: E731
        ("x", p), ("dtype", F32), ("g", p), ("a", p), ("b", p), ("up", None), ("inv", None), ("weight", p), ("ld_w", 4), ("labels", p),
        ("n", 2), ("c", 3), ("cin", 4), ("hw", 4), ("power", 1.0), ("eps", 1e-6), ("dx", p), ("stream", None))])
    dwe = lambda **k: L.iif_normed_mask_predict_bwd_weight(*[k.get(a, d) for a, d in (       # noqa: E731
        ("x", p), ("dtype", F32), ("g", p), ("a", p), ("up", None), ("inv", None), ("weight", p), ("ld_w", 4), ("labels", p), ("n", 2),
        ("c", 3), ("cin", 4), ("hw", 4), ("power", 1.0), ("eps", 1e-6), ("scratch", p), ("dweight", p), ("dbias", p), ("stream", None))])
    for entry, ptrs in ((fwd, ("x", "weight", "labels", "rows", "loss", "inv")), (dxe, ("x", "g", "a", "b", "weight", "labels", "dx")),
                        (dwe, ("x", "g", "a", "weight", "labels", "scratch"))):
        for name in ptrs:
            assert entry(**{name: None}) == -1, name
        assert entry(cin=0) == -1 and entry(cin=2049) == -1
        assert entry(hw=0) == -1 and entry(hw=4097) == -1
        assert entry(n=-1) == -1 and entry(n=65536) == -1
        assert entry(c=0) == -1 and entry(c=-3) == -1
        assert entry(dtype=7) == -1
        assert entry(power=0.0) == -1 and entry(power=-1.0) == -1 and entry(power=float("nan")) == -1
        assert entry(ld_w=3) == -1                                    # rows that overlap
        assert entry(n=0) == 0                                        # nothing to do: IIF_OK, nothing enqueued
        assert entry(n=0, power=2.0) == 0
    assert fwd(z=None, target=None) == -1                             # nothing asked for
    assert fwd(target=None) == -1                                     # g without a target
    assert dwe(dweight=None, dbias=None) == -1
