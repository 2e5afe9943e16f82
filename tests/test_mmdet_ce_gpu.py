"""mmdet CrossEntropyLoss family on the MI355X against the reference's own float32 run (tests/golden/g23_mmdet_ce.npz,
written by tests/golden/make_golden_mmdet_ce.py) and the float64 closed forms of tests/ce_cases.py.

Bound: loss, element losses and gradient within REL = 1e-4 of the reference's float32 numbers, max-abs difference over
max-abs reference - the bound of the sibling head tests (tests/test_seesaw_gpu.py, tests/test_mmdet_golden.py).  The
reference's float32 run sits at most 4.0e-6 from its float64 run and from the closed form (tests/test_mmdet_ce_host.py),
so the bound leaves more than a decade for the hardware exp2 / log2 / rcp.

Largest measured errors (MI355X): sigmoid loss 2.3e-7, gradient 2.9e-7 on every shape but [1, 1], whose single element the
reference's float32 run forms as sigmoid(x) - 1 and has 3.95e-6 from the closed form (the kernel: 3.8e-8 from the closed form, so
3.95e-6 from the fixture), dense targets 2.1e-7, softmax 2.0e-7,
counters 1.6e-7; bf16 logits: loss 1.6e-7, gradient one bf16 step from the rounded fp32-path gradient."""
import numpy as np
import pytest
import torch

from . import ce_cases as cc

pytestmark = pytest.mark.gpu
REL = 1e-4
DEV = "cuda"
LW = cc.LOSS_WEIGHT


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a).max())


def _t(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def ref(golden):
    """The fixture, unpacked once and never written."""
    g = golden("g23_mmdet_ce")
    cc.check_generator(g)
    out = {"g": g}
    for prefix in ("sig_", "dense_", "soft_"):
        out[prefix] = tuple(cc.unpack(g, prefix + k) for k in ("loss", "grad"))
    return out


@pytest.fixture(scope="module")
def sig_in():
    """Host and device copies of the sigmoid inputs of every shape, made on first use and never written."""
    cache = {}

    def get(si, bf=0):
        if (si, bf) not in cache:
            x, labels, weights, cw = cc.sig_inputs(si, bf)
            cache[si, bf] = (x, labels, weights, cw, _t(x), _t(labels), _t(weights))
        return cache[si, bf]
    return get


def _loss_module(cls_name="CrossEntropyLoss", **kw):
    from iif_amd import mmdet_ce_loss as M
    return getattr(M, cls_name)(loss_weight=LW, **kw)


def _fwd_bwd(m, xt, label, weight, avg=None, upstream=None, **kw):
    """Forward + backward (of the sum, or of sum(out * upstream)) -> numpy (loss, gradient as float32)."""
    xl = xt.clone().requires_grad_(True)
    out = m(xl, label, weight, avg_factor=avg, **kw)
    (out.sum() if upstream is None else (out * upstream).sum()).backward()
    return out.detach().float().cpu().numpy(), xl.grad.float().cpu().numpy()


def _sig(xt, lt, wt, cw, red, avg, ign=None, **kw):
    m = _loss_module(use_sigmoid=True, reduction=red, class_weight=None if cw is None else cw.tolist(), ignore_index=ign)
    return _fwd_bwd(m, xt, lt, wt, avg, **kw)


def test_sigmoid_cases_against_the_reference(ref, sig_in):
    """Every fp32 case of the fixture: shapes (1, 1), (37, 1), (100003, 1), (5, 3), (64, 81), (33, 1203 / 1204 / 1205) and
    (1024, 1204); row weights x class weight x avg_factor x reduction in full on (5, 3) and (64, 81); labels < 0, equal to the
    ignore index (-100 and a class index), == C and > C in every batch.  The rows the fixture does not keep are compared with
    the float64 closed form."""
    l32, g32 = ref["sig_"]
    worst = {"loss": 0.0, "grad": 0.0}
    for i, (si, wf, cwf, af, red, ign, bf) in enumerate(cc.sig_cases()):
        if bf:
            continue
        name, N, C, keep = cc.SIG_SHAPES[si]
        x, labels, weights, cw, xt, lt, wt = sig_in(si)
        avg = cc.AVG_FACTOR if af else None
        loss, d = _sig(xt, lt, wt if wf else None, cw if cwf else None, red, avg, ign)
        c_l, c_g = cc.closed_form_labels(x, labels, weights if wf else None, cw if cwf else None, ign, red, avg)
        assert loss.shape == ((N, C) if red == "none" else ()), (name, red, loss.shape)
        print("%s case %d: loss %.2e / %.2e, grad %.2e / %.2e (fixture / closed form)" % (
            name, i, _rel(loss[list(keep)] if red == "none" else loss, l32[i]), _rel(loss, c_l), _rel(d[list(keep)], g32[i]),
            _rel(d, c_g)))
        e_l = max(_rel(loss[list(keep)] if red == "none" else loss, l32[i]), _rel(loss, c_l))
        e_g = max(_rel(d[list(keep)], g32[i]), _rel(d, c_g))
        worst["loss"], worst["grad"] = max(worst["loss"], e_l), max(worst["grad"], e_g)
        assert e_l <= REL and e_g <= REL, (name, i, wf, cwf, af, red, ign, e_l, e_g)
    print("mmdet sigmoid BCE worst relative error: loss %.2e, gradient %.2e" % (worst["loss"], worst["grad"]))


def test_dense_target_cases_against_the_reference(ref):
    """Float targets per element (the reference's pred.dim() == label.dim() branch), with and without an elementwise weight
    and a class weight, every reduction; plus a [37] / [37] pair of vectors through the functional form."""
    from iif_amd.mmdet_ce_loss import binary_cross_entropy
    l32, g32 = ref["dense_"]
    worst = 0.0
    for i, (si, ewf, cwf, af, red) in enumerate(cc.dense_cases()):
        name, N, C, keep = cc.SIG_SHAPES[si]
        x, t, w, cw = cc.dense_inputs(si)
        avg = cc.AVG_FACTOR if af else None
        loss, d = _sig(_t(x), _t(t), _t(w) if ewf else None, cw if cwf else None, red, avg)
        c_l, c_g = cc.closed_form_dense(x, t, w if ewf else None, cw if cwf else None, red, avg)
        e = max(_rel(loss[list(keep)] if red == "none" else loss, l32[i]), _rel(loss, c_l), _rel(d[list(keep)], g32[i]),
                _rel(d, c_g))
        print("dense %s case %d: %.2e" % (name, i, e))
        worst = max(worst, e)
        assert e <= REL, (name, i, ewf, cwf, af, red, e)
    x, t, w, _ = cc.dense_inputs(cc.shape_index("s37x1"))
    xl = _t(x[:, 0]).requires_grad_(True)
    out = binary_cross_entropy(xl, _t(t[:, 0]), _t(w[:, 0]), reduction="sum")
    out.backward()
    c_l, c_g = cc.closed_form_dense(x, t, w, None, "sum", None, 1.0)
    assert _rel(out.item(), c_l) <= REL and _rel(xl.grad.cpu().numpy(), c_g[:, 0]) <= REL
    print("mmdet dense BCE worst relative error %.2e" % worst)


def _bf16_ulps(a, b):
    """Distance in bf16 steps between two bfloat16 tensors (sign-magnitude bits mapped to a monotonic integer)."""
    def key(t):
        v = t.view(torch.int16).to(torch.int32)
        return torch.where(v < 0, -(v & 0x7FFF), v)
    return int((key(a) - key(b)).abs().max().item()) if a.numel() else 0


def test_bf16_logits(ref, sig_in):
    """bf16 logits: the loss (and the fp32 element losses) meet REL against the reference run on the bf16-rounded inputs; the
    bf16 gradient is the fp32-path gradient of the same inputs rounded to bf16, to within one bf16 step."""
    l32, _ = ref["sig_"]
    for i, (si, wf, cwf, af, red, ign, bf) in enumerate(cc.sig_cases()):
        if not bf:
            continue
        name, N, C, keep = cc.SIG_SHAPES[si]
        x, labels, weights, cw, xt, lt, wt = sig_in(si, 1)
        xb = xt.to(torch.bfloat16)
        assert torch.equal(xb.float(), xt)                       # the inputs are bf16 numbers already
        m = _loss_module(use_sigmoid=True, reduction=red, class_weight=cw.tolist() if cwf else None)
        xl = xb.clone().requires_grad_(True)
        out = m(xl, lt, wt)
        out.sum().backward()
        assert xl.grad.dtype == torch.bfloat16 and out.dtype == torch.float32
        loss = out.detach().cpu().numpy()
        e = _rel(loss[list(keep)] if red == "none" else loss, l32[i])
        x32 = xt.clone().requires_grad_(True)
        m(x32, lt, wt).sum().backward()
        steps = _bf16_ulps(xl.grad, x32.grad.to(torch.bfloat16))
        print("bf16 %s %s: loss %.2e, gradient %d bf16 step(s) from the rounded fp32 gradient" % (name, red, e, steps))
        assert e <= REL, (name, red, e)
        assert steps <= 1, (name, red, steps)


@pytest.mark.parametrize("name", ["s37x1", "s5x3", "m64x81", "l33x1205"])
def test_row_pitch_wider_than_the_row(name, sig_in):
    """pred as a column slice of a wider tensor: the pitch is C + 3, rows start one element into it."""
    si = cc.shape_index(name)
    _, N, C, _ = cc.SIG_SHAPES[si]
    x, labels, weights, cw, xt, lt, wt = sig_in(si)
    for red in ("mean", "none"):
        wide = torch.full((N, C + 3), 1.0e4, device=DEV)
        wide[:, 1:C + 1] = xt
        wide.requires_grad_(True)
        view = wide[:, 1:C + 1]
        assert view.stride(0) == C + 3
        m = _loss_module(use_sigmoid=True, reduction=red, class_weight=cw.tolist())
        out = m(view, lt, wt)
        out.sum().backward()
        c_l, c_g = cc.closed_form_labels(x, labels, weights, cw, None, red)
        gw = wide.grad.cpu().numpy()
        assert _rel(out.detach().cpu().numpy(), c_l) <= REL and _rel(gw[:, 1:C + 1], c_g) <= REL
        assert not gw[:, 0].any() and not gw[:, C + 1:].any()


@pytest.mark.parametrize("name", ["s1x1", "s37x1", "s5x3", "m64x81", "c100003x1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unaligned_base(name, dtype, sig_in):
    """pred one element past a 16-byte boundary (4 bytes for fp32, 2 for bf16): the elements in front of the first and
    behind the last whole 16-byte piece take their own path."""
    si = cc.shape_index(name)
    _, N, C, _ = cc.SIG_SHAPES[si]
    x, labels, weights, cw, xt, lt, wt = sig_in(si, 1)
    buf = torch.zeros(N * C + 9, device=DEV, dtype=dtype)
    buf[1:1 + N * C] = xt.reshape(-1).to(dtype)
    buf.requires_grad_(True)
    view = buf[1:1 + N * C].view(N, C)
    assert view.data_ptr() % 16 == buf.element_size() and view.is_contiguous()
    for red in ("sum", "none"):
        buf.grad = None
        m = _loss_module(use_sigmoid=True, reduction=red, class_weight=cw.tolist())
        out = m(view, lt, wt)
        out.sum().backward()
        c_l, c_g = cc.closed_form_labels(x, labels, weights, cw, None, red)
        gb = buf.grad.float().cpu().numpy()
        # a bf16 gradient is rounded twice, by the kernel's store and by the backward's scaling with loss_weight, each by at
        # most u = 2^-8 of the value (8 significant bits): (1 + u)^2 - 1
        tol = REL if dtype == torch.float32 else 2.0 ** -7 + 2.0 ** -16
        assert _rel(out.detach().cpu().numpy(), c_l) <= REL, (name, red)
        assert _rel(gb[1:1 + N * C].reshape(N, C), c_g) <= tol, (name, red)
        assert gb[0] == 0.0 and not gb[1 + N * C:].any()


def test_all_ignored_all_background_and_empty_batches(ref, sig_in):
    g = ref["g"]
    si = cc.shape_index("m64x81")
    x, _, weights, cw, xt, _, wt = sig_in(si)
    for sp in cc.SPECIALS:
        lt = _t(cc.special_labels(sp))
        for red in ("mean", "none"):
            loss, d = _sig(xt, lt, wt, cw, red, None)
            assert _rel(loss, g["%s_%s_loss" % (sp, red)]) <= REL, (sp, red)
            assert _rel(d, g["%s_%s_grad" % (sp, red)]) <= REL, (sp, red)
            if sp == "allignored":
                assert not loss.any() and not d.any()
    lab0 = torch.zeros(0, dtype=torch.int64, device=DEV)
    for mode, kw in (("sig", dict(use_sigmoid=True)), ("soft", {})):
        for k, red in enumerate(cc.REDUCTIONS):
            x0 = torch.zeros((0, 3), device=DEV, requires_grad=True)
            out = _loss_module(reduction=red, **kw)(x0, lab0)
            if red == "none":
                assert out.shape == ((0, 3) if mode == "sig" else (0,))
            elif red == "mean":
                assert np.isnan(float(out)) and np.isnan(g["empty_" + mode][0])
            else:
                assert float(out) == 0.0 == float(g["empty_" + mode][1])
            out.sum().backward()
            assert x0.grad.shape == (0, 3)
        out = _loss_module(reduction="mean", **kw)(torch.zeros((0, 3), device=DEV), lab0, avg_factor=3.0)
        assert float(out) == 0.0 == float(g["empty_%s_avg" % mode])


def test_upstream_gradient_of_the_element_losses(sig_in):
    """reduction='none' with one upstream value per element, and a scalar loss with a non-unit upstream value."""
    si = cc.shape_index("m64x81")
    _, N, C, _ = cc.SIG_SHAPES[si]
    x, labels, weights, cw, xt, lt, wt = sig_in(si)
    u = np.linspace(-1.0, 2.0, N * C).astype(np.float32).reshape(N, C)
    _, d = _sig(xt, lt, wt, cw, "none", None, upstream=_t(u))
    _, c_g = cc.closed_form_labels(x, labels, weights, cw, None, "none")
    assert _rel(d, c_g * u) <= REL
    _, d = _sig(xt, lt, wt, cw, "mean", None, upstream=-2.5)
    _, c_g = cc.closed_form_labels(x, labels, weights, cw, None, "mean")
    assert _rel(d, -2.5 * c_g) <= REL


def test_softmax_cases_against_the_reference(ref):
    """use_sigmoid=False on (9, 7) and (33, 1204): ignore index (-100 and a class index), class weight, row weights,
    avg_factor, every reduction."""
    l32, g32 = ref["soft_"]
    worst = 0.0
    for i, (si, wf, cwf, af, red, ign) in enumerate(cc.soft_cases()):
        name, N, C, keep = cc.SOFT_SHAPES[si]
        x, labels, weights, cw = cc.soft_inputs(si, ign)
        m = _loss_module(reduction=red, class_weight=cw.tolist() if cwf else None, ignore_index=ign)
        loss, d = _fwd_bwd(m, _t(x), _t(labels), _t(weights) if wf else None, cc.AVG_FACTOR if af else None)
        assert loss.shape == ((N,) if red == "none" else ())
        e = max(_rel(loss[list(keep)] if red == "none" else loss, l32[i]), _rel(d[list(keep)], g32[i]))
        worst = max(worst, e)
        assert e <= REL, (name, i, wf, cwf, af, red, ign, e)
    print("mmdet softmax CE worst relative error %.2e" % worst)


def test_mask_mode_is_the_native_mask_loss_bit_for_bit():
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    from iif_amd.mmdet_mask_loss import mask_cross_entropy
    N, C, H = 6, 5, 7
    x = cc.make_logits(N, C * H * H, 77).reshape(N, C, H, H)
    target = (cc.make_dense(N, H * H, 77)[0] >= 0.5).astype(np.float32).reshape(N, H, H)
    label = _t(np.arange(N, dtype=np.int64) % C)
    got, want = [], []
    for fn, sink in ((CrossEntropyLoss(use_mask=True), got), (mask_cross_entropy, want)):
        xl = _t(x).requires_grad_(True)
        out = fn(xl, _t(target), label)
        out.sum().backward()
        sink.extend([out.detach(), xl.grad])
    assert got[0].shape == (1,) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _check_counters(g, m, mode, grads=True):
    for k in range(cc.COUNTER_CALLS):
        x, labels, weights = cc.counter_inputs(mode, k)
        xl = _t(x).requires_grad_(True)
        loss = m(xl, _t(labels), _t(weights))
        loss.backward()
        assert loss.dim() == 0
        assert np.array_equal(m.cum_labels.cpu().numpy(), g["cnt_%s%d_cum_labels" % (mode, k)]), (mode, k)
        e = max(_rel(m.cum_losses.cpu().numpy(), g["cnt_%s%d_cum_losses" % (mode, k)]),
                _rel(loss.item(), g["cnt_%s%d_loss" % (mode, k)]),
                _rel(xl.grad.cpu().numpy()[list(cc.COUNTER_KEEP)], g["cnt_%s%d_grad" % (mode, k)]))
        print("counters %s call %d: %.2e" % (mode, k, e))
        assert e <= REL, (mode, k, e)
    m.close_cums()
    assert not m.use_cums and m.reduction == "mean"
    assert not m.cum_losses.any() and not m.cum_labels.any()


@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
def test_counter_loss_three_calls(ref, mode):
    m = _loss_module("CrossEntropyCounterLoss", use_sigmoid=(mode == "sigmoid"), reduction="mean", use_cums=True,
                     num_classes=cc.COUNTER_CLASSES, device=DEV)
    assert m.reduction == "none" and m.reduction_old == "mean"
    _check_counters(ref["g"], m, mode)
    # closed: the plain reduction again
    x, labels, weights = cc.counter_inputs(mode, 0)
    plain = _loss_module(use_sigmoid=(mode == "sigmoid"), reduction="mean")
    assert torch.equal(m(_t(x), _t(labels), _t(weights)), plain(_t(x), _t(labels), _t(weights)))


def test_fasa_iif_loss_with_the_sigmoid_criterion(ref, tmp_path):
    """FasaIIFLoss(use_sigmoid=True) is the sigmoid counter loss (fasa_iif_loss.py:35-36): same fixture, same checks."""
    from iif_amd.mmdet_fasa import FasaIIFLoss
    path = tmp_path / "idf.csv"
    path.write_text("raw\n" + "\n".join("1.0" for _ in range(cc.COUNTER_CLASSES + 1)) + "\n")
    m = FasaIIFLoss(use_sigmoid=True, reduction="mean", loss_weight=LW, use_cums=True, num_classes=cc.COUNTER_CLASSES,
                    path=str(path), device=DEV)
    _check_counters(ref["g"], m, "sigmoid")


def test_repeat_calls_are_bit_identical_and_leave_the_ticket_at_zero(sig_in):
    from iif_amd import custom
    for name in ("l1024x1204", "c100003x1", "s5x3"):
        si = cc.shape_index(name)
        _, _, _, cw, xt, lt, wt = sig_in(si)
        a = _sig(xt, lt, wt, cw, "mean", None)
        b = _sig(xt, lt, wt, cw, "mean", None)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
        assert int(custom._workspace(xt.device, 0, False)[1][0].item()) == 0, name


def test_raw_entry_with_a_workspace_of_its_own(sig_in):
    """The C entry on a caller's workspace (IIF_CE_WORKSPACE_BYTES, zeroed once): the ticket is back at zero after every call,
    so the next call needs no reset; loss only (no dpred), and the element losses add up to the scalar."""
    from iif_amd import _lib
    si = cc.shape_index("c100003x1")
    _, N, C, _ = cc.SIG_SHAPES[si]
    x, labels, weights, _, xt, lt, wt = sig_in(si)
    ws = torch.zeros(1 + 2048, dtype=torch.int32, device=DEV)
    elems = torch.empty((N, C), device=DEV)
    got = []
    for _ in range(3):
        loss = torch.full((), -1.0, device=DEV)
        rc = _lib.lib().iif_bce_det_fwd_bwd(_lib.ptr(xt), 0, C, _lib.ptr(lt), _lib.ptr(wt), -100, None, None, None, 0.5, N, C,
                                            _lib.ptr(elems), _lib.ptr(loss), None, 0, _lib.ptr(ws), _lib.stream_ptr())
        assert rc == 0
        assert int(ws[0].item()) == 0
        got.append(float(loss))
    assert got[0] == got[1] == got[2]
    c_l, _ = cc.closed_form_labels(x, labels, weights, None, None, "sum", None, 0.5)
    assert _rel(got[0], c_l) <= REL
    assert _rel(0.5 * float(elems.double().sum()), c_l) <= REL


def test_forward_and_backward_do_not_synchronise(sig_in):
    """forward + backward under torch's sync debug mode ('error'): sigmoid (labels and dense targets) and softmax, 'mean'
    with and without avg_factor, and 'sum'."""
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    si = cc.shape_index("l33x1204")
    _, _, _, cw, xt, lt, wt = sig_in(si)
    lsoft = lt.clamp(0, 1203)
    dense = (xt > 0).float()
    mods = [(_loss_module(use_sigmoid=True, class_weight=cw.tolist()), lt, wt),
            (_loss_module(use_sigmoid=True), dense, None),
            (_loss_module(class_weight=cw.tolist()), lsoft, wt)]
    xs = [xt.clone().requires_grad_(True) for _ in mods]
    for (m, lab, w), xl in zip(mods, xs):                   # workspaces, tables and class weights exist before the mode is on
        m(xl.detach(), lab, w)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for (m, lab, w), xl in zip(mods, xs):
            for red, avg in (("mean", None), ("mean", 12.5), ("sum", None)):
                m(xl, lab, w, avg_factor=avg, reduction_override=red).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.isfinite(xl.grad).all() for xl in xs)


def test_registration_without_mmdet():
    from iif_amd import mmdet_ce_loss
    assert mmdet_ce_loss.register_into_mmdet() is False
