"""Box-regression head (mmdet L1Loss / SmoothL1Loss, BBoxHead.loss's regression term), the part that needs no device: the
fixture tests/golden/g24_bbox_reg.npz against the input generator and the float64 closed forms of tests/bbox_reg_cases.py, the
modules' constructors, attributes and error conventions, the CPU-tensor rejection, and the two new C entry points in header,
library and ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

from . import bbox_reg_cases as bc
from iif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_bbox_reg_fwd", "iif_bbox_reg_scatter_grad")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a).max())


def test_fixture_inputs_regenerate(golden):
    bc.check_generator(golden("g24_bbox_reg"))


def test_inputs_hold_the_edge_elements():
    """Every input set of more than a handful of elements has d = 0 and |d| = 1 exactly, zero weights and, in gather mode,
    positive, background and negative labels and all-zero weight rows."""
    for si, (name, shape, _) in enumerate(bc.PLAIN_SHAPES):
        p, t, w = bc.plain_inputs(si)
        assert p.shape == t.shape == w.shape == shape and p.dtype == t.dtype == w.dtype == np.float32
        if p.size >= 1027:
            d = p - t
            assert (d == 0).any() and (d == 1).any() and (d == -1).any() and (w == 0).any() and (np.abs(d) < 1.0 / 9.0).any()
    for si, (name, N, C, K, agnostic, mode) in enumerate(bc.GATHER_SHAPES):
        for bf in (0, 1):
            p, lab, t, w = bc.gather_inputs(si, bf)
            assert p.shape == (N, 4 * C) and lab.shape == (N,) and t.shape == w.shape == (N, 4)
            pos, sel = bc.select(p, lab, K, agnostic)
            if mode == "nopos":
                assert pos.size == 0 and (lab == K).any() and (lab == -1).any()
                continue
            d = sel - t[pos]
            assert (d == 0).any() and (d == 1).any() and (d == -1).any()
            assert (lab == K).any() and (lab == -1).any() and 0 < pos.size < N
            assert (w[pos] == 0).all(axis=1).any() and ((w[pos] == 0).any(axis=1) & (w[pos] != 0).any(axis=1)).any()
            if bf:
                assert np.array_equal(bc.bf16_round(p), p)


def test_float32_float64_and_closed_form_agree(golden):
    """The float64 closed form is the reference's float64 run to 1e-12 (measured 3.0e-16), and the reference's float32 run (what
    the GPU tests compare with) sits <= 1e-6 from both (measured 1.6e-7 over all cases, 9.3e-8 on the [1024, 4812] ones)."""
    g = golden("g24_bbox_reg")
    l32, l64, g32 = (bc.unpack(g, "plain_" + k) for k in ("loss", "loss64", "grad"))
    cases = bc.plain_cases()
    assert len(cases) == len(l32) == len(l64) == len(g32) == 120
    worst32 = worst_cf = 0.0
    for i, (si, ki, wf, af, red) in enumerate(cases):
        _, shape, keep = bc.PLAIN_SHAPES[si]
        p, t, w = bc.plain_inputs(si)
        c_l, c_g = bc.closed_form_plain(p, t, w if wf else None, bc.KINDS[ki][1], red, bc.AVG_FACTOR if af else None)
        if red == "none":
            c_l = c_l.reshape(-1)[list(keep)]
        worst_cf = max(worst_cf, _rel(c_l, l64[i]))
        worst32 = max(worst32, _rel(l32[i], l64[i]), _rel(g32[i], c_g.reshape(-1)[list(keep)]))
    l32, l64, rows = (bc.unpack(g, "gather_" + k) for k in ("loss", "loss64", "rows"))
    cases = bc.gather_cases()
    assert len(cases) == len(l32) == len(l64) == len(rows) == len(g["gather_nnz"]) == 24
    for i, (si, ki, bf) in enumerate(cases):
        _, N, C, K, agnostic, mode = bc.GATHER_SHAPES[si]
        p, lab, t, w = bc.gather_inputs(si, bf)
        c_l, c_rows = bc.closed_form_gather(p, lab, t, w, K, agnostic, bc.KINDS[ki][1])
        worst_cf = max(worst_cf, _rel(c_l, l64[i]))
        worst32 = max(worst32, _rel(l32[i], l64[i]), _rel(rows[i].reshape(N, 4), c_rows))
        assert int(g["gather_nnz"][i]) == np.count_nonzero(c_rows) == np.count_nonzero(rows[i])
        if mode == "nopos":
            assert float(l32[i][0]) == 0.0 and int(g["gather_nnz"][i]) == 0
        else:
            assert 0 < int(g["gather_nnz"][i]) < 4 * N
    assert worst_cf <= 1e-12, worst_cf
    assert worst32 <= 1e-6, worst32
    assert g["worst"][0] <= 1e-6 and g["worst"][1] <= 1e-12


def test_fixture_empty_input_table(golden):
    """What the reference does with a [0, 4] prediction, as recorded: no weight -> a 0-d zero for every reduction; an empty
    weight -> NaN for 'mean' without avg_factor, 0 with one, 0 for 'sum', an empty tensor for 'none'; 'sum' with an avg_factor
    raises either way."""
    g = golden("g24_bbox_reg")
    want = {("none", "mean", 0): (0, 0.0), ("none", "mean", 1): (0, 0.0), ("none", "sum", 0): (0, 0.0), ("none", "sum", 1): (1, 0.0),
            ("none", "none", 0): (0, 0.0), ("none", "none", 1): (0, 0.0), ("empty", "mean", 0): (0, float("nan")),
            ("empty", "mean", 1): (0, 0.0), ("empty", "sum", 0): (0, 0.0), ("empty", "sum", 1): (1, 0.0),
            ("empty", "none", 0): (2, 0.0), ("empty", "none", 1): (2, 0.0)}
    for i, case in enumerate(bc.empty_cases()):
        s, v = want[case]
        assert int(g["empty_status"][i]) == s, case
        assert (np.isnan(g["empty_value"][i]) and np.isnan(v)) or float(g["empty_value"][i]) == v, case


def test_modules_import_without_a_device_and_mirror_the_constructors():
    from iif_amd import mmdet_bbox_loss as M
    m = M.L1Loss()
    assert (m.reduction, m.loss_weight) == ("mean", 1.0) and not hasattr(m, "beta")
    m = M.L1Loss("sum", 0.5)                                  # the reference's positional order
    assert (m.reduction, m.loss_weight) == ("sum", 0.5)
    m = M.SmoothL1Loss()
    assert (m.beta, m.reduction, m.loss_weight) == (1.0, "mean", 1.0)
    m = M.SmoothL1Loss(1.0 / 9.0, "none", 2.0)
    assert (m.beta, m.reduction, m.loss_weight) == (1.0 / 9.0, "none", 2.0)
    assert isinstance(m, torch.nn.Module) and not list(m.parameters())
    assert callable(M.l1_loss) and callable(M.smooth_l1_loss) and callable(M.bbox_head_reg_loss)
    assert M.register_into_mmdet() is False                   # no mmdet here: no error either


def test_error_conventions():
    from iif_amd import mmdet_bbox_loss as M
    p, t = torch.zeros(3, 4), torch.zeros(3, 4)
    for m in (M.L1Loss(), M.SmoothL1Loss()):
        with pytest.raises(AssertionError):
            m(p, t, reduction_override="max")
        with pytest.raises(ValueError):
            m(p, t, avg_factor=2.0, reduction_override="sum")
    with pytest.raises(ValueError):
        M.L1Loss(reduction="sum")(p, t, avg_factor=2.0)
    for beta in (0.0, -1.0):
        with pytest.raises(AssertionError):
            M.SmoothL1Loss(beta=beta)(p, t)
        with pytest.raises(AssertionError):
            M.smooth_l1_loss(p, t, beta=beta)
    with pytest.raises(ValueError):
        M.l1_loss(p, t, reduction="sum", avg_factor=1.0)
    with pytest.raises(TypeError):
        M.L1Loss()(p, t, beta=1.0)                            # L1Loss.forward takes no further keywords
    # BBoxHead.loss always passes an avg_factor: 'sum' raises, as the reference does
    lab = torch.tensor([0, 1, 2])
    with pytest.raises(ValueError):
        M.bbox_head_reg_loss(M.L1Loss(reduction="sum"), torch.zeros(3, 12), lab, t, t, 3)
    with pytest.raises(ValueError):
        M.bbox_head_reg_loss(M.SmoothL1Loss(), torch.zeros(3, 12), lab, t, t, 3, reduction_override="sum")
    with pytest.raises(AssertionError):
        M.bbox_head_reg_loss(M.L1Loss(), torch.zeros(3, 12), lab, t, t, 3, reduction_override="max")


def test_cpu_tensor_is_rejected_not_emulated():
    from iif_amd import mmdet_bbox_loss as M
    p, t = torch.ones(3, 4), torch.zeros(3, 4)
    for call in (lambda: M.L1Loss()(p, t), lambda: M.SmoothL1Loss()(p, t, t), lambda: M.l1_loss(p, t, reduction="none"),
                 lambda: M.smooth_l1_loss(p, t, beta=0.5), lambda: M.L1Loss()(p[:0], t[:0]),
                 lambda: M.bbox_head_reg_loss(M.L1Loss(), torch.zeros(3, 12), torch.tensor([0, 1, 3]), t, t, 3),
                 lambda: M.bbox_head_reg_loss(M.SmoothL1Loss(), p, torch.tensor([0, 1, 3]), t, t, 3, reg_class_agnostic=True)):
        with pytest.raises(_lib.IIFNativeError):
            call()


def test_other_loss_objects_take_the_reference_formulation():
    """A loss_bbox that is not one of the native classes is called as bbox_head.py:284-311 calls it (on the CPU here: the
    fall-through is torch indexing around the caller's own module)."""
    from iif_amd.mmdet_bbox_loss import bbox_head_reg_loss
    si = bc.shape_index("g67x5", bc.GATHER_SHAPES)
    _, N, C, K, _, _ = bc.GATHER_SHAPES[si]
    p, lab, t, w = bc.gather_inputs(si)
    seen = {}

    def other(pred, target, weight, avg_factor=None, reduction_override=None):
        seen["shapes"] = (tuple(pred.shape), tuple(target.shape), tuple(weight.shape), avg_factor, reduction_override)
        return ((pred - target).abs() * weight).sum() / avg_factor
    pt = torch.from_numpy(p).requires_grad_(True)
    out = bbox_head_reg_loss(other, pt, torch.from_numpy(lab), torch.from_numpy(t), torch.from_numpy(w), K)
    out.backward()
    pos, _ = bc.select(p, lab, K, False)
    assert seen["shapes"] == ((pos.size, 4), (pos.size, 4), (pos.size, 4), N, None)
    c_l, c_rows = bc.closed_form_gather(p, lab, t, w, K, False, 0.0, 1.0)
    assert _rel(out.item(), c_l) <= 1e-6 and _rel(pt.grad.numpy(), bc.scatter(c_rows, lab, K, C, False)) <= 1e-6
    # no positives: the reference's bbox_pred[pos_inds].sum(), and the module is not called
    seen.clear()
    nolab = torch.from_numpy(bc.gather_labels(bc.shape_index("n67x5", bc.GATHER_SHAPES)))
    assert bbox_head_reg_loss(other, pt, nolab, torch.from_numpy(t), torch.from_numpy(w), K).item() == 0.0 and not seen


def test_entry_points_in_header_library_and_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code)
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name])


def test_entry_points_check_arguments_before_launching():
    """Bad arguments return before anything touches the device."""
    L = _lib.lib()
    one = 16            # a non-null stand-in: the checks below fail before any pointer is used

    def fwd(**kw):
        return L.iif_bbox_reg_fwd(kw.get("x", one), kw.get("dtype", 0), kw.get("ld", 12), kw.get("labels", one), kw.get("K", 3),
                                  kw.get("C", 3), kw.get("tgt", one), None, kw.get("beta", 1.0), 1.0, kw.get("n", 16), kw.get("N", 4),
                                  None, kw.get("out", one), None, kw.get("ws", one), None)
    assert fwd(dtype=2) == -1 and fwd(n=-1) == -1 and fwd(N=-1) == -1 and fwd(C=0) == -1
    assert fwd(beta=-0.5) == -1 and fwd(beta=float("nan")) == -1
    assert fwd(n=15) == -1                                    # gather mode: four elements per row
    assert fwd(ld=11) == -1                                   # a pitch below 4C
    assert fwd(K=4) == -1                                     # a positive label would index past pred's classes
    assert fwd(K=0) == -1
    assert fwd(labels=None) == -1                             # plain mode is C == 1
    assert fwd(x=None) == -1 and fwd(tgt=None) == -1
    assert fwd(ws=None) == -1                                 # a scalar loss needs the workspace
    assert fwd(x=18) == -1                                    # fp32 predictions on a 2-byte boundary
    assert fwd(tgt=18) == -1
    assert fwd(n=0, N=0, out=None, ws=None) == 0              # nothing to do

    def sc(**kw):
        return L.iif_bbox_reg_scatter_grad(kw.get("dsel", one), kw.get("labels", one), kw.get("K", 3), kw.get("N", 4),
                                           kw.get("C", 3), None, kw.get("d", one), kw.get("dtype", 0), kw.get("ld", 12), None)
    assert sc(dtype=2) == -1 and sc(N=-1) == -1 and sc(C=0) == -1 and sc(K=0) == -1 and sc(K=4) == -1
    assert sc(dsel=None) == -1 and sc(labels=None) == -1 and sc(d=None) == -1
    assert sc(ld=11) == -1 and sc(d=18) == -1 and sc(dsel=18) == -1
    assert sc(N=0) == 0
