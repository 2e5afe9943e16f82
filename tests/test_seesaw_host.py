"""Seesaw head, the part that needs no device: the float64 closed form of tests/seesaw_cases.py against the reference's
own float64 run (tests/golden/g22_seesaw.npz), the module's constructor / protocol errors and state_dict, the CPU-tensor
rejection, and the new C entry points in header and ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

from . import seesaw_cases as sc
from iif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_seesaw_fwd_bwd", "iif_seesaw_activation", "iif_seesaw_accuracy", "iif_seesaw_scale_grad")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_fixture_inputs_regenerate(golden):
    sc.check_generator(golden("g22_seesaw"))


def test_closed_form_matches_the_reference_float64_run(golden):
    """The log-domain restatement is the reference's function: <= 1e-12 of its float64 run on every case (measured
    4.0e-15), and the float32 run the GPU tests compare with sits <= 2e-6 from it (measured 9.3e-7)."""
    g = golden("g22_seesaw")
    lc64, lo64, lc32, lo32 = (sc.unpack(g, k) for k in ("loss_cls64", "loss_obj64", "loss_cls", "loss_obj"))
    g64, g32 = sc.unpack(g, "grad64"), sc.unpack(g, "grad")
    worst = worst32 = 0.0
    cases = sc.grid_cases()
    assert len(cases) == len(g["case_meta"])
    for i, (si, scale, p, q, wf, af, red) in enumerate(cases):
        assert tuple(g["case_meta"][i]) == (si, scale, p, q, wf, af, sc.REDUCTIONS.index(red))
        name, N, C, keep = sc.SHAPES[si]
        x, labels, weights = sc.shape_inputs(name, scale)
        c, o, d = sc.closed_form(x, labels, g[name + "_cum1"], C, p, q, sc.EPS, weights if wf else None, red,
                                 sc.AVG_FACTOR if af else None)
        worst = max(worst, _rel(c, lc64[i]), _rel(o, lo64[i]))
        if len(g64[i]):
            worst = max(worst, _rel(d, g64[i]))
        worst32 = max(worst32, _rel(lc32[i], c), _rel(lo32[i], o), _rel(g32[i], d[list(keep)]))
    assert worst <= 1e-12, worst
    assert worst32 <= 2e-6, worst32


def test_closed_form_known_answers(golden):
    """The reference's own test vectors (tests/test_metrics/test_losses.py:134-183)."""
    g = golden("g22_seesaw")
    xa, xb = g["known_xa"], g["known_xb"]
    zero = np.zeros(3, dtype=np.float32)
    c, o, _ = sc.closed_form(xa, [1], sc.updated_cum(zero, [1], 2), 2, 0.0, 0.0)
    assert c == 0.0 and o == 200.0
    c, o, _ = sc.closed_form(xa, [0], sc.updated_cum(g["known_cum_e"], [0], 2), 2, 1.0, 0.0)
    assert abs(c - 180.0) < 1e-5 and o == 200.0
    c, o, _ = sc.closed_form(xa, [0], sc.updated_cum(zero, [0], 2), 2, 0.0, 1.0)
    assert abs(c - (200.0 + np.log(100.0))) < 1e-12
    assert np.allclose(g["known_loss"], [[0.0, 200.0], [180.0, 200.0], [200.0 + np.log(100.0), 200.0]], rtol=1e-6)
    assert np.allclose(sc.activation(xb, 2), [[1.0, 0.0, 0.0]]) and sc.accuracy(xb, np.array([0]), 2) == (100.0, 100.0)


def test_count_is_one_float_addition_per_class(golden):
    g = golden("g22_seesaw")
    cum = sc.updated_cum(sc.special_cum("big"), sc.special_labels("big"), 5)
    assert cum[2] == np.float32(16777220.0)            # three +1.0f would have stayed at 16777216
    assert np.array_equal(cum, g["big_cum1"])
    for name, _, C, _ in sc.SHAPES:
        assert np.array_equal(sc.updated_cum(g[name + "_cum0"], g[name + "_labels"], C), g[name + "_cum1"])


def test_module_protocol_and_errors():
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    with pytest.raises(AssertionError):
        SeesawLoss(use_sigmoid=True, device="cpu")
    m = SeesawLoss(p=0.0, q=0.0, num_classes=2, device="cpu")
    assert m.custom_cls_channels and m.custom_activation and m.custom_accuracy
    assert m.get_cls_channels(2) == 4
    with pytest.raises(AssertionError):
        m.get_cls_channels(3)
    lab = torch.tensor([1])
    for bad in ([[-100.0, 100.0]], [[-100.0, 100.0, -100.0]]):
        with pytest.raises(AssertionError):
            m(torch.tensor(bad), lab)
    x = torch.tensor([[-100.0, 100.0, -100.0, 100.0]])
    with pytest.raises(AssertionError):
        m(x, lab, reduction_override="max")
    with pytest.raises(ValueError):
        m(x, lab, avg_factor=2.0, reduction_override="sum")
    # defaults of the reference's constructor
    d = SeesawLoss(device="cpu")
    assert (d.p, d.q, d.num_classes, d.eps, d.reduction, d.loss_weight, d.return_dict) == (0.8, 2.0, 1203, 1e-2, "mean", 1.0, True)


def test_state_dict_is_the_reference_layout():
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    m = SeesawLoss(num_classes=80, device="cpu")
    sd = m.state_dict()
    assert list(sd) == ["cum_samples"]
    assert sd["cum_samples"].shape == (81,) and sd["cum_samples"].dtype == torch.float32
    assert not sd["cum_samples"].any()
    m.load_state_dict({"cum_samples": torch.arange(81, dtype=torch.float32)})        # a reference checkpoint's entry
    assert m.cum_samples[80] == 80.0


def test_cpu_tensor_is_rejected_not_emulated():
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    m = SeesawLoss(num_classes=2, device="cpu")
    x = torch.tensor([[-100.0, 100.0, -100.0, 100.0]])
    lab = torch.tensor([1])
    with pytest.raises(_lib.IIFNativeError):
        m(x, lab)
    with pytest.raises(_lib.IIFNativeError):
        m.get_activation(x)
    with pytest.raises(_lib.IIFNativeError):
        m.get_accuracy(x, lab)
    assert not m.cum_samples.any()


def test_entry_points_in_header_library_and_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.lib()
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "IIF_SEESAW_WORKSPACE_BYTES" in code


def test_entry_points_check_arguments_before_launching():
    """Bad arguments return before anything touches the device."""
    lib = _lib.lib()
    f = lib.iif_seesaw_fwd_bwd
    one = 16            # a non-null stand-in: the checks below fail before any pointer is used
    args = lambda **kw: [kw.get("x", one), kw.get("dtype", 0), kw.get("ld", 1205), one, None, one, 1, kw.get("p", 0.8), 2.0, 1e-2,    # noqa: E731
                         1.0, 1, 1.0, kw.get("N", 4), kw.get("C", 1203), one, one, kw.get("out", one), None, 0, None,
                         kw.get("ws", one), None]
    assert f(*args(dtype=1)) == -1                       # bf16: fp32 only
    assert f(*args(C=2047)) == -2                        # C + 2 > 2048: IIF_EUNSUPPORTED, no slow path
    assert f(*args(ld=1204)) == -1
    assert f(*args(N=-1)) == -1 and f(*args(C=0)) == -1 and f(*args(p=-1.0)) == -1
    assert f(*args(x=None)) == -1 and f(*args(ws=None)) == -1 and f(*args(out=None)) == -1
    assert lib.iif_seesaw_activation(one, 1, 1205, 4, 1203, one, 1204, None) == -1
    assert lib.iif_seesaw_activation(one, 0, 1205, 4, 2047, one, 2048, None) == -2
    assert lib.iif_seesaw_activation(one, 0, 1205, 4, 1203, one, 1203, None) == -1
    assert lib.iif_seesaw_activation(one, 0, 1205, 0, 1203, one, 1204, None) == 0          # N == 0: nothing to do
    assert lib.iif_seesaw_accuracy(one, 0, 1204, one, 4, 1203, one, one, None) == -1
    assert lib.iif_seesaw_accuracy(one, 0, 1205, one, 4, 1203, one, None, None) == -1
    assert lib.iif_seesaw_scale_grad(one, 1204, 4, 1203, one, one, 0, one, 1205, None) == -1
    assert lib.iif_seesaw_scale_grad(one, 1205, 0, 1203, one, one, 0, one, 1205, None) == 0
