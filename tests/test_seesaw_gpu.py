"""Fused Seesaw head on the MI355X against the reference's own float32 run (tests/golden/g22_seesaw.npz, written by
tests/golden/make_golden_seesaw.py) and the float64 closed form of tests/seesaw_cases.py.

Bound: loss, gradient and activation within REL = 1e-4 of the reference's float32 numbers, max-abs difference over max-abs
reference - the project's bound for the mmdet head (tests/test_mmdet_golden.py).  The reference's float32 run sits 9.3e-7 from
its float64 run and the closed form 4e-15, so the bound leaves two decades for the hardware exp2 / log2.  cum_samples and
the accuracies are compared bit for bit."""
import numpy as np
import pytest
import torch

from . import seesaw_cases as sc

pytestmark = pytest.mark.gpu
REL = 1e-4
DEV = "cuda"


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a).max())


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def inputs():
    """Device copies of every shape's inputs, made once and never written."""
    out = {}
    for name, _, _, _ in sc.SHAPES:
        for scale in sc.SCALES:
            x, labels, weights = sc.shape_inputs(name, scale)
            out[name, scale] = (x, labels, weights, _t(x), _t(labels), _t(weights))
    return out


def _module(C, p=0.8, q=2.0, red="mean", cum0=None, **kw):
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    m = SeesawLoss(p=p, q=q, num_classes=C, eps=sc.EPS, reduction=red, loss_weight=sc.LOSS_WEIGHT, device=DEV, **kw)
    if cum0 is not None:
        m.cum_samples.copy_(_t(cum0))
    return m


def _run(C, xt, lt, wt, cum0, p=0.8, q=2.0, red="mean", avg=None):
    """Forward + backward of (classes + objectness) on a fresh module -> numpy (classes, objectness, grad, cum after)."""
    m = _module(C, p, q, red, cum0)
    xl = xt.clone().requires_grad_(True)
    out = m(xl, lt, wt, avg_factor=avg)
    lc, lo = out["loss_cls_classes"], out["loss_cls_objectness"]
    (lc.sum() + lo.sum()).backward()
    return lc.detach().cpu().numpy(), lo.detach().cpu().numpy(), xl.grad.cpu().numpy(), m.cum_samples.cpu().numpy()


def test_every_case_against_the_reference(golden, inputs):
    """All 169 cases of the fixture: (p, q) x weights x avg_factor x reduction x logit scale on [9, 7] and [64, 82], every
    (p, q) x scale on the LVIS row [70, 1205], and [16400, 7] (two histogram blocks).  Largest measured error (MI355X):
    loss 2.5e-7, gradient 5.6e-7 (activation, test_activation_and_accuracy: 1.9e-7) against the bound of 1e-4."""
    g = golden("g22_seesaw")
    sc.check_generator(g)
    lc32, lo32, g32 = sc.unpack(g, "loss_cls"), sc.unpack(g, "loss_obj"), sc.unpack(g, "grad")
    worst = {"loss": 0.0, "grad": 0.0}
    for i, (si, scale, p, q, wf, af, red) in enumerate(sc.grid_cases()):
        name, N, C, keep = sc.SHAPES[si]
        x, labels, weights, xt, lt, wt = inputs[name, scale]
        lc, lo, d, cum = _run(C, xt, lt, wt if wf else None, g[name + "_cum0"], p, q, red, sc.AVG_FACTOR if af else None)
        assert np.array_equal(cum, g[name + "_cum1"]), (name, i)
        e_l = max(_rel(lc, lc32[i]), _rel(lo, lo32[i]))
        e_g = _rel(d[list(keep)], g32[i])
        worst["loss"], worst["grad"] = max(worst["loss"], e_l), max(worst["grad"], e_g)
        assert e_l <= REL and e_g <= REL, (name, i, scale, p, q, wf, af, red, e_l, e_g)
        # the rows the fixture does not keep: the float64 closed form (the reference's function to 4e-15)
        _, _, dc = sc.closed_form(x, labels, cum, C, p, q, sc.EPS, weights if wf else None, red, sc.AVG_FACTOR if af else None)
        e_c = _rel(d, dc)
        worst["grad"] = max(worst["grad"], e_c)
        assert e_c <= REL, (name, i, e_c)
    print("seesaw worst relative error: loss %.2e, gradient %.2e" % (worst["loss"], worst["grad"]))


@pytest.mark.parametrize("C", [150, 600, 2046])
def test_class_counts_between_the_instantiated_chunk_counts(C):
    """C = 150 / 600 run on the 4- / 12-chunk instances (every chunk tested against C, not only the last one), 2046 is the
    largest supported row; against the float64 closed form (the reference's function to 4e-15)."""
    N = 6
    x, labels, weights = sc.make_inputs(N, C, 40 + C, 6)
    cum0 = sc.make_cum(C, 9)
    xt, lt, wt = _t(x), _t(labels), _t(weights)
    lc, lo, d, cum = _run(C, xt, lt, wt, cum0)
    assert np.array_equal(cum, sc.updated_cum(cum0, labels, C))
    c, o, dc = sc.closed_form(x, labels, cum, C, weights=weights)
    assert _rel(lc, c) <= REL and _rel(lo, o) <= REL and _rel(d, dc) <= REL
    m = _module(C)
    assert _rel(m.get_activation(xt).cpu().numpy(), sc.activation(x, C)) <= REL
    acc = m.get_accuracy(xt, lt)
    got = (np.float32(acc["acc_objectness"].item()), np.float32(acc["acc_classes"].item()))
    assert got == sc.accuracy(x, labels, C)


def test_known_answers(golden):
    """The reference's test vectors (test_losses.py:134-183): 0 / 200, 180 with p = 1 and cum[0] = e^20, 200 + ln 100 with
    q = 1 (the eps clamp), and return_dict=False with activation [1, 0, 0] and both accuracies 100."""
    g = golden("g22_seesaw")
    xa, xb = _t(g["known_xa"]), _t(g["known_xb"])
    l0, l1 = torch.tensor([0], device=DEV), torch.tensor([1], device=DEV)
    want = g["known_loss"]
    for k, (lab, p, q, cum0) in enumerate(((l1, 0.0, 0.0, None), (l0, 1.0, 0.0, g["known_cum_e"]), (l0, 0.0, 1.0, None))):
        out = _module(2, p, q, cum0=cum0)(xa, lab)
        got = [float(out["loss_cls_classes"]), float(out["loss_cls_objectness"])]
        assert _rel(got, want[k]) <= REL, (k, got, want[k])
    assert abs(want[1][0] - 180.0) < 1e-3 and abs(want[2][0] - (200.0 + np.log(100.0))) < 1e-3
    m = _module(2, 0.0, 1.0, return_dict=False)
    loss = m(xb, l0)
    assert loss.dim() == 0 and abs(float(loss)) <= 1e-4
    assert _rel(m.get_activation(xb).cpu().numpy(), g["known_act"]) <= REL
    acc = m.get_accuracy(xb, l0)
    assert float(acc["acc_objectness"]) == 100.0 and float(acc["acc_classes"]) == 100.0


def test_all_background_all_positive_and_the_2p24_count(golden, inputs):
    g = golden("g22_seesaw")
    name, N, C, _ = sc.SHAPES[0]
    x, _, weights, xt, _, wt = inputs[name, 1]
    for sp in sc.SPECIALS:
        labels = sc.special_labels(sp)
        lt = _t(labels)
        lc, lo, d, cum = _run(C, xt, lt, wt, sc.special_cum(sp))
        assert np.array_equal(cum, g[sp + "_cum1"]), sp
        assert _rel(lc, g[sp + "_loss_cls"]) <= REL and _rel(lo, g[sp + "_loss_obj"]) <= REL, sp
        assert _rel(d, g[sp + "_grad"]) <= REL, sp
        acc = _module(C).get_accuracy(xt, lt)
        got = np.array([acc["acc_objectness"].item(), acc["acc_classes"].item()], dtype=np.float32)
        assert np.array_equal(got, g[sp + "_acc"]), (sp, got)
        if sp == "allbg":
            assert float(lc) == 0.0 and not d[:, :C].any() and got[1] == 0.0
        if sp == "big":
            assert cum[2] == np.float32(16777220.0)           # one +3, not three +1.0f


def test_state_carries_over_three_calls(golden):
    g = golden("g22_seesaw")
    m = _module(80)
    for k in range(sc.STATE_CALLS):
        x, labels, weights = sc.state_inputs(k)
        xl = _t(x).requires_grad_(True)
        out = m(xl, _t(labels), _t(weights))
        (out["loss_cls_classes"] + out["loss_cls_objectness"]).backward()
        assert np.array_equal(m.cum_samples.cpu().numpy(), g["state%d_cum" % k]), k
        got = [float(out["loss_cls_classes"].detach()), float(out["loss_cls_objectness"].detach())]
        assert _rel(got, g["state%d_loss" % k]) <= REL, k
        assert _rel(xl.grad.cpu().numpy()[[1, 6, 63]], g["state%d_grad" % k]) <= REL, k


def test_repeat_calls_are_bit_identical(golden, inputs):
    g = golden("g22_seesaw")
    for name, scale in (("l70x1203", 6), ("c16400x5", 1), ("s9x5", 1)):
        C = sc.SHAPES[sc.shape_index(name)][2]
        _, _, _, xt, lt, wt = inputs[name, scale]
        a = _run(C, xt, lt, wt, g[name + "_cum0"])
        b = _run(C, xt, lt, wt, g[name + "_cum0"])
        for u, v in zip(a, b):
            assert np.array_equal(u, v), name


def test_row_pitch_wider_than_the_row(golden, inputs):
    """cls_score as a column slice of a wider tensor: ld = C + 7, rows start one element into the pitch."""
    g = golden("g22_seesaw")
    for name in ("s9x5", "l70x1203"):
        _, N, C, _ = sc.SHAPES[sc.shape_index(name)]
        _, _, _, xt, lt, wt = inputs[name, 1]
        ref = _run(C, xt, lt, wt, g[name + "_cum0"])
        wide = torch.full((N, C + 7), 1.0e4, device=DEV)
        wide[:, 1:C + 3] = xt
        wide.requires_grad_(True)
        m = _module(C, cum0=g[name + "_cum0"])
        view = wide[:, 1:C + 3]
        assert view.stride(0) == C + 7
        out = m(view, lt, wt)
        (out["loss_cls_classes"] + out["loss_cls_objectness"]).backward()
        assert float(out["loss_cls_classes"]) == float(ref[0]) and float(out["loss_cls_objectness"]) == float(ref[1])
        gw = wide.grad.cpu().numpy()
        assert np.array_equal(gw[:, 1:C + 3], ref[2]) and not gw[:, 0].any() and not gw[:, C + 3:].any()
        assert torch.equal(m.get_activation(view), m.get_activation(xt))
        a, b = m.get_accuracy(view, lt), m.get_accuracy(xt, lt)
        assert torch.equal(a["acc_classes"], b["acc_classes"]) and torch.equal(a["acc_objectness"], b["acc_objectness"])


def test_upstream_gradients_scale_their_own_columns(golden, inputs):
    """Backward with non-unit, unequal upstream values: class columns take the class loss's, objectness columns the
    objectness loss's; reduction='none' scales rows."""
    g = golden("g22_seesaw")
    name, N, C, _ = sc.SHAPES[1]
    x, labels, weights, xt, lt, wt = inputs[name, 1]
    cum1 = g[name + "_cum1"]
    m = _module(C, cum0=g[name + "_cum0"])
    xl = xt.clone().requires_grad_(True)
    out = m(xl, lt, wt)
    (1.75 * out["loss_cls_classes"] - 0.375 * out["loss_cls_objectness"]).backward()
    _, _, d = sc.closed_form(x, labels, cum1, C, weights=weights)
    d[:, :C] *= 1.75
    d[:, C:] *= -0.375
    assert _rel(xl.grad.cpu().numpy(), d) <= REL
    # only one of the two losses used
    m = _module(C, cum0=g[name + "_cum0"])
    xl = xt.clone().requires_grad_(True)
    m(xl, lt, wt)["loss_cls_objectness"].backward()
    got = xl.grad.cpu().numpy()
    _, _, d = sc.closed_form(x, labels, cum1, C, weights=weights)
    assert not got[:, :C].any() and _rel(got[:, C:], d[:, C:]) <= REL
    # 'none': one upstream value per row
    m = _module(C, red="none", cum0=g[name + "_cum0"])
    xl = xt.clone().requires_grad_(True)
    out = m(xl, lt, wt)
    pos = labels < C
    assert out["loss_cls_classes"].shape == (int(pos.sum()),) and out["loss_cls_objectness"].shape == (N,)
    uc = np.linspace(-1.0, 2.0, int(pos.sum())).astype(np.float32)
    uo = np.linspace(0.5, -1.5, N).astype(np.float32)
    ((out["loss_cls_classes"] * _t(uc)).sum() + (out["loss_cls_objectness"] * _t(uo)).sum()).backward()
    _, _, d = sc.closed_form(x, labels, cum1, C, weights=weights, reduction="none")
    full = np.zeros(N)
    full[pos] = uc
    d[:, :C] *= full[:, None]
    d[:, C:] *= uo[:, None].astype(np.float64)
    assert _rel(xl.grad.cpu().numpy(), d) <= REL


def test_out_of_range_label_zeroes_its_row_and_sets_the_status(golden, inputs):
    from iif_amd import custom
    g = golden("g22_seesaw")
    name, N, C, _ = sc.SHAPES[0]
    x, labels, weights, xt, _, wt = inputs[name, 1]
    custom.check_label_status()                         # clean slate
    for bad in (C + 1, -1):
        labels = labels.copy()
        labels[4] = bad
        lc, lo, d, cum = _run(C, xt, _t(labels), wt, g[name + "_cum0"])
        assert np.array_equal(cum, sc.updated_cum(g[name + "_cum0"], labels, C))        # counted nowhere
        c, o, dc = sc.closed_form(x, labels, cum, C, weights=weights)
        assert not d[4].any()
        assert _rel(lc, c) <= REL and _rel(lo, o) <= REL and _rel(d, dc) <= REL
        with pytest.raises(IndexError):
            custom.check_label_status()
        custom.check_label_status()                     # the flag is cleared by the check


def test_empty_batch():
    m = _module(5, cum0=sc.make_cum(5, 1))
    x = torch.zeros((0, 7), device=DEV, requires_grad=True)
    lab = torch.zeros(0, dtype=torch.int64, device=DEV)
    out = m(x, lab)
    assert float(out["loss_cls_classes"]) == 0.0 and np.isnan(float(out["loss_cls_objectness"]))     # torch: mean of nothing
    out = m(x, lab, avg_factor=3.0)
    assert float(out["loss_cls_classes"]) == 0.0 and float(out["loss_cls_objectness"]) == 0.0
    (out["loss_cls_classes"] + out["loss_cls_objectness"]).backward()
    assert x.grad.shape == (0, 7)
    assert np.array_equal(m.cum_samples.cpu().numpy(), sc.make_cum(5, 1))
    assert m.get_activation(x).shape == (0, 6)
    acc = m.get_accuracy(x, lab)
    assert float(acc["acc_objectness"]) == 0.0 and float(acc["acc_classes"]) == 0.0


def test_activation_and_accuracy(golden, inputs):
    g = golden("g22_seesaw")
    worst = 0.0
    for name, N, C, keep in sc.SHAPES:
        for scale in sc.SCALES:
            x, labels, _, xt, lt, _ = inputs[name, scale]
            m = _module(C)
            act = m.get_activation(xt).cpu().numpy()
            assert act.shape == (N, C + 1)
            e = max(_rel(act[list(keep)], g["%s_x%d_act" % (name, scale)]), _rel(act, sc.activation(x, C)))
            worst = max(worst, e)
            assert e <= REL, (name, scale, e)
            acc = m.get_accuracy(xt, lt)
            assert acc["acc_objectness"].shape == (1,) and acc["acc_classes"].shape == (1,)
            got = np.array([acc["acc_objectness"].item(), acc["acc_classes"].item()], dtype=np.float32)
            assert np.array_equal(got, g["%s_x%d_acc" % (name, scale)]), (name, scale, got)
    print("seesaw activation worst relative error %.2e" % worst)


def test_accuracy_tie_rule():
    """iif_topk_hits' rule: an equal score at a lower index beats the target."""
    m = _module(3)
    x = torch.tensor([[1.0, 1.0, 0.0, 2.0, 2.0], [1.0, 1.0, 0.0, 2.0, 2.0], [0.0, 0.0, 0.0, 0.0, 1.0]], device=DEV)
    acc = m.get_accuracy(x, torch.tensor([0, 1, 3], device=DEV))
    # row 0: hit (lowest index of the tie), objectness label 0 hit; row 1: miss; row 2: background, objectness hit
    assert float(acc["acc_classes"]) == 50.0
    assert float(acc["acc_objectness"]) == np.float32(3.0) * np.float32(100.0 / 3)
    acc = m.get_accuracy(x[:2], torch.tensor([3, 3], device=DEV))          # objectness tie: label 1 loses to index 0
    assert float(acc["acc_objectness"]) == 0.0 and float(acc["acc_classes"]) == 0.0


def test_forward_and_backward_do_not_synchronise(golden, inputs):
    """forward + backward under torch's sync debug mode ('error'): 'mean' with return_dict both ways."""
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    g = golden("g22_seesaw")
    name, N, C, _ = sc.SHAPES[2]
    _, _, _, xt, lt, wt = inputs[name, 1]
    mods = [_module(C, cum0=g[name + "_cum0"], return_dict=rd) for rd in (True, False)]
    xs = [xt.clone().requires_grad_(True) for _ in mods]
    mods[0](xs[0].detach(), lt, wt)                     # workspaces exist before the mode is switched on
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for m, xl in zip(mods, xs):
            for avg in (None, 12.5):
                out = m(xl, lt, wt, avg_factor=avg)
                loss = out if not m.return_dict else out["loss_cls_classes"] + out["loss_cls_objectness"]
                loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.isfinite(xl.grad).all() for xl in xs)


def test_unsupported_shapes_and_dtypes_raise():
    from iif_amd._lib import IIFNativeError
    m = _module(2047)
    with pytest.raises(IIFNativeError):
        m(torch.zeros((2, 2049), device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV))
    m = _module(5)
    with pytest.raises(IIFNativeError):
        m(torch.zeros((2, 7), device=DEV, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int64, device=DEV))
    assert not m.cum_samples.any()
