"""Box-regression head on the MI355X against the reference's own float32 run (tests/golden/g24_bbox_reg.npz, written by
tests/golden/make_golden_bbox_reg.py) and the float64 closed forms of tests/bbox_reg_cases.py.

Bound: loss, element losses and gradient within REL = 1e-4 of the reference's float32 numbers, max-abs difference over
max-abs reference - the bound of the sibling head tests (tests/test_mmdet_ce_gpu.py, tests/test_seesaw_gpu.py).  The
reference's float32 run sits at most 1.6e-7 from its float64 run and from the closed form (tests/test_bbox_reg_host.py).
Positions the reference leaves at zero must be exactly zero here, and the non-zero counts equal.

Largest measured errors (MI355X): plain mode loss 2.0e-7, gradient 1.0e-7; gather mode loss 1.75e-7, gradient 4.7e-8 (bit-equal
at [1024, 4812]); bf16 predictions: loss 1.8e-7, gradient 0 bf16 steps from the rounded fp32-path gradient."""
import numpy as np
import pytest
import torch

from . import bbox_reg_cases as bc

pytestmark = pytest.mark.gpu
REL = 1e-4
DEV = "cuda"
LW = bc.LOSS_WEIGHT


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


def _module(ki, red="mean", lw=LW):
    from iif_amd import mmdet_bbox_loss as M
    beta = bc.KINDS[ki][1]
    return M.L1Loss(reduction=red, loss_weight=lw) if beta == 0.0 else M.SmoothL1Loss(beta=beta, reduction=red, loss_weight=lw)


def _ticket(t):
    from iif_amd import custom
    return int(custom._workspace(t.device, 0, False)[1][0].item())


@pytest.fixture(scope="module")
def ref(golden):
    """The fixture, unpacked once and never written."""
    g = golden("g24_bbox_reg")
    bc.check_generator(g)
    return {"g": g, "plain": tuple(bc.unpack(g, "plain_" + k) for k in ("loss", "grad")),
            "gather": tuple(bc.unpack(g, "gather_" + k) for k in ("loss", "rows"))}


@pytest.fixture(scope="module")
def gather_in():
    """Host and device copies of the gather inputs, made on first use and never written."""
    cache = {}

    def get(si, bf=0):
        if (si, bf) not in cache:
            host = bc.gather_inputs(si, bf)
            cache[si, bf] = host + tuple(_t(v) for v in host)
        return cache[si, bf]
    return get


def _gather(ki, pt, lt, tt, wt, K, agnostic, upstream=None, **kw):
    """forward + backward of bbox_head_reg_loss on a fresh leaf -> (loss tensor, gradient tensor)."""
    from iif_amd.mmdet_bbox_loss import bbox_head_reg_loss
    pl = pt.clone().requires_grad_(True)
    out = bbox_head_reg_loss(_module(ki), pl, lt, tt, wt, K, reg_class_agnostic=agnostic, **kw)
    (out if upstream is None else out * upstream).backward()
    return out.detach(), pl.grad


def test_plain_cases_against_the_reference(ref):
    """Every plain case of the fixture: n = 1, 7, 1027 and [4099, 4]; L1, beta 1 and beta 1/9; with and without weight and
    avg_factor; all three reductions.  The inputs hold elements with pred == target (L1 gradient exactly 0) and with |d| == 1
    == beta.  All elements are compared with the float64 closed form, the kept ones with the fixture; where the closed-form
    gradient is zero (d = 0, weight 0) the gradient is exactly zero."""
    l32, g32 = ref["plain"]
    worst = {"loss": 0.0, "grad": 0.0}
    dev_in = {}
    for i, (si, ki, wf, af, red) in enumerate(bc.plain_cases()):
        name, shape, keep = bc.PLAIN_SHAPES[si]
        if si not in dev_in:
            host = bc.plain_inputs(si)
            dev_in[si] = host + tuple(_t(v) for v in host)
        p, t, w, pt, tt, wt = dev_in[si]
        avg = bc.AVG_FACTOR if af else None
        pl = pt.clone().requires_grad_(True)
        out = _module(ki, red)(pl, tt, wt if wf else None, avg_factor=avg)
        out.sum().backward()
        assert out.dtype == torch.float32 and tuple(out.shape) == (shape if red == "none" else ()), (name, red)
        loss, d = out.detach().cpu().numpy(), pl.grad.cpu().numpy()
        c_l, c_g = bc.closed_form_plain(p, t, w if wf else None, bc.KINDS[ki][1], red, avg)
        kp = list(keep)
        e_l = max(_rel(loss.reshape(-1)[kp] if red == "none" else loss, l32[i]), _rel(loss, c_l))
        e_g = max(_rel(d.reshape(-1)[kp], g32[i]), _rel(d, c_g))
        worst["loss"], worst["grad"] = max(worst["loss"], e_l), max(worst["grad"], e_g)
        print("%s case %d (%s, %s): loss %.2e, grad %.2e" % (name, i, bc.KINDS[ki][0], red, e_l, e_g))
        assert e_l <= REL and e_g <= REL, (name, i, ki, wf, af, red, e_l, e_g)
        assert np.array_equal(d != 0, c_g != 0), (name, i, "zero positions of the gradient")
        if red == "none":
            assert np.array_equal(loss != 0, c_l != 0), (name, i, "zero positions of the element losses")
        assert _ticket(pt) == 0
    print("box regression, plain mode, worst relative error: loss %.2e, gradient %.2e" % (worst["loss"], worst["grad"]))


def test_exact_ties():
    """pred == target: L1's gradient is 0 (torch's abs backward), and smooth L1's too; |d| == beta == 1 sits on the linear
    branch (strict comparison), where both branches give 0.5 and +-1."""
    from iif_amd.mmdet_bbox_loss import L1Loss, SmoothL1Loss
    p = torch.tensor([0.5, 0.5, 0.5, -2.0, 0.25], device=DEV)
    t = torch.tensor([0.5, -0.5, 1.5, -2.0, 0.0], device=DEV)
    for m, want_l, want_g in ((L1Loss(reduction="none"), [0.0, 1.0, 1.0, 0.0, 0.25], [0.0, 1.0, -1.0, 0.0, 1.0]),
                              (SmoothL1Loss(reduction="none"), [0.0, 0.5, 0.5, 0.0, 0.03125], [0.0, 1.0, -1.0, 0.0, 0.25])):
        pl = p.clone().requires_grad_(True)
        out = m(pl, t)
        out.sum().backward()
        assert out.tolist() == want_l and pl.grad.tolist() == want_g


def test_gather_cases_against_the_reference(ref, gather_in):
    """Every fp32 gather case of the fixture through bbox_head_reg_loss: [67, 20], [300, 148], [1024, 4812], the class-agnostic
    [67, 4] and a batch without positives, each with L1, beta 1 and beta 1/9.  The dense gradient is compared with the scatter
    of the fixture's rows; every position the reference leaves at zero is exactly zero and the non-zero counts agree."""
    l32, rows = ref["gather"]
    nnz = ref["g"]["gather_nnz"]
    worst = {"loss": 0.0, "grad": 0.0}
    for i, (si, ki, bf) in enumerate(bc.gather_cases()):
        if bf:
            continue
        name, N, C, K, agnostic, mode = bc.GATHER_SHAPES[si]
        p, lab, t, w, pt, lt, tt, wt = gather_in(si)
        out, grad = _gather(ki, pt, lt, tt, wt, K, agnostic)
        assert out.dim() == 0 and out.dtype == torch.float32 and grad.shape == pt.shape and grad.dtype == torch.float32
        want = bc.scatter(rows[i].reshape(N, 4), lab, K, C, agnostic)
        d = grad.cpu().numpy()
        e_l, e_g = _rel(out.item(), l32[i]), _rel(d, want)
        worst["loss"], worst["grad"] = max(worst["loss"], e_l), max(worst["grad"], e_g)
        print("%s %s: loss %.2e, grad %.2e, %d non-zeros" % (name, bc.KINDS[ki][0], e_l, e_g, int(nnz[i])))
        assert e_l <= REL and e_g <= REL, (name, ki, e_l, e_g)
        assert np.array_equal(d != 0, want != 0), (name, ki, "zero positions")
        assert int(np.count_nonzero(d)) == int(nnz[i]), (name, ki)
        if mode == "nopos":
            assert out.item() == 0.0 and not d.any()
        assert _ticket(pt) == 0
    print("box regression, gather mode, worst relative error: loss %.2e, gradient %.2e" % (worst["loss"], worst["grad"]))


def _bf16_ulps(a, b):
    """Distance in bf16 steps between two bfloat16 tensors (sign-magnitude bits mapped to a monotonic integer)."""
    def key(t):
        v = t.view(torch.int16).to(torch.int32)
        return torch.where(v < 0, -(v & 0x7FFF), v)
    return int((key(a) - key(b)).abs().max().item()) if a.numel() else 0


def test_bf16_predictions(ref, gather_in):
    """bf16 bbox_pred ([67, 20] and [300, 148]: odd C, rows on alternating 8-byte phases; [67, 4] class agnostic): the loss
    meets REL against the reference run on the bf16-rounded inputs; the bf16 gradient is the fp32-path gradient of the same
    inputs rounded to bf16, to within one bf16 step, with the reference's zero positions and non-zero count."""
    l32, rows = ref["gather"]
    nnz = ref["g"]["gather_nnz"]
    seen = 0
    for i, (si, ki, bf) in enumerate(bc.gather_cases()):
        if not bf:
            continue
        seen += 1
        name, N, C, K, agnostic, _ = bc.GATHER_SHAPES[si]
        p, lab, t, w, pt, lt, tt, wt = gather_in(si, 1)
        pb = pt.to(torch.bfloat16)
        assert torch.equal(pb.float(), pt)                       # the inputs are bf16 numbers already
        out, grad = _gather(ki, pb, lt, tt, wt, K, agnostic)
        assert grad.dtype == torch.bfloat16 and out.dtype == torch.float32
        _, g32 = _gather(ki, pt, lt, tt, wt, K, agnostic)
        e = _rel(out.item(), l32[i])
        steps = _bf16_ulps(grad, g32.to(torch.bfloat16))
        print("bf16 %s %s: loss %.2e, gradient %d bf16 step(s) from the rounded fp32 gradient" % (name, bc.KINDS[ki][0], e, steps))
        assert e <= REL and steps <= 1, (name, ki, e, steps)
        d = grad.float().cpu().numpy()
        assert np.array_equal(d != 0, bc.scatter(rows[i].reshape(N, 4), lab, K, C, agnostic) != 0), (name, ki)
        assert int(np.count_nonzero(d)) == int(nnz[i])
    assert seen == 9


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_offset_and_pitched_views_give_the_same_numbers(dtype, gather_in):
    """bbox_pred one element past a 16-byte boundary, and bbox_pred as a column slice of a wider tensor (pitch 4C + 3): the
    gradient is that of the contiguous tensor bit for bit, and nothing outside the view receives one.  The loss is the same
    sum taken one element per lane instead of one box per lane: two orders of the same 4N non-negative fp32 terms differ by at
    most 2 (4N - 1) 2^-24 of the sum (each order is within (4N - 1) u of the exact sum, u = 2^-24)."""
    from iif_amd.mmdet_bbox_loss import bbox_head_reg_loss
    si = bc.shape_index("g67x5", bc.GATHER_SHAPES)
    _, N, C, K, agnostic, _ = bc.GATHER_SHAPES[si]
    _, _, _, _, pt, lt, tt, wt = gather_in(si, 1)
    pt = pt.to(dtype)
    W = 4 * C
    reorder = 2.0 * (4 * N - 1) * 2.0 ** -24
    for ki in range(len(bc.KINDS)):
        base_l, base_g = _gather(ki, pt, lt, tt, wt, K, agnostic)
        buf = torch.zeros(N * W + 9, device=DEV, dtype=dtype)
        buf[1:1 + N * W] = pt.reshape(-1)
        buf.requires_grad_(True)
        view = buf[1:1 + N * W].view(N, W)
        assert view.data_ptr() % 16 == buf.element_size() and view.is_contiguous()
        out = bbox_head_reg_loss(_module(ki), view, lt, tt, wt, K)
        out.backward()
        assert abs(out.item() - base_l.item()) <= reorder * base_l.item() and base_l.item() > 0
        assert torch.equal(buf.grad[1:1 + N * W].view(N, W), base_g)
        assert buf.grad[0] == 0 and not buf.grad[1 + N * W:].any()
        wide = torch.full((N, W + 3), 1.0e4, device=DEV, dtype=dtype)
        wide[:, 1:W + 1] = pt
        wide.requires_grad_(True)
        view = wide[:, 1:W + 1]
        assert view.stride(0) == W + 3
        out = bbox_head_reg_loss(_module(ki), view, lt, tt, wt, K)
        out.backward()
        assert abs(out.item() - base_l.item()) <= reorder * base_l.item()
        assert torch.equal(wide.grad[:, 1:W + 1], base_g)
        assert not wide.grad[:, 0].any() and not wide.grad[:, W + 1:].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["g67x5", "a67", "g300x37"])
def test_scatter_entry_on_an_offset_base_and_a_wider_pitch(name, dtype, gather_in):
    """The C entry of backward on the layouts autograd never hands it: dpred one element past a 16-byte boundary and dpred
    with pitch 4C + 3 (the element-per-lane path) equal the 16-byte path bit for bit, and the columns beyond 4C stay as they
    were.  Upstream scalar 0.75."""
    from iif_amd import _lib
    si = bc.shape_index(name, bc.GATHER_SHAPES)
    _, N, C, K, agnostic, _ = bc.GATHER_SHAPES[si]
    _, lab, _, _, _, lt, _, _ = gather_in(si)
    W = 4 * C
    dsel = _t(bc._codes(N * 4, 77, 512).astype(np.float32).reshape(N, 4) / np.float32(64.0))
    g = torch.tensor(0.75, device=DEV)
    code = 0 if dtype == torch.float32 else 1

    def run(d, ld):
        rc = _lib.lib().iif_bbox_reg_scatter_grad(_lib.ptr(dsel), _lib.ptr(lt), K, N, C, _lib.ptr(g), _lib.ptr(d), code, ld,
                                                  _lib.stream_ptr())
        assert rc == 0
    fast = torch.full((N, W), 7.0, device=DEV, dtype=dtype)
    run(fast, W)
    rows = np.where(((lab >= 0) & (lab < K))[:, None], 0.75 * dsel.cpu().numpy(), 0.0).astype(np.float32)
    want = _t(bc.scatter(rows, lab, K, C, agnostic)).to(dtype)
    assert torch.equal(fast, want)
    buf = torch.full((N * W + 9,), 7.0, device=DEV, dtype=dtype)
    off = buf[1:1 + N * W].view(N, W)
    run(off, W)
    assert torch.equal(off, want) and buf[0] == 7.0 and (buf[1 + N * W:] == 7.0).all()
    wide = torch.full((N, W + 3), 7.0, device=DEV, dtype=dtype)
    run(wide, W + 3)
    assert torch.equal(wide[:, :W], want) and (wide[:, W:] == 7.0).all()


def test_none_reduction_through_the_head(gather_in):
    """'none' has a data-dependent [P, 4] result: the indices come from torch, the element losses from the kernel."""
    from iif_amd.mmdet_bbox_loss import bbox_head_reg_loss
    si = bc.shape_index("g67x5", bc.GATHER_SHAPES)
    _, N, C, K, agnostic, _ = bc.GATHER_SHAPES[si]
    p, lab, t, w, pt, lt, tt, wt = gather_in(si)
    pos, sel = bc.select(p, lab, K, agnostic)
    for ki in range(len(bc.KINDS)):
        pl = pt.clone().requires_grad_(True)
        out = bbox_head_reg_loss(_module(ki), pl, lt, tt, wt, K, reduction_override="none")
        out.sum().backward()
        c_l, c_g = bc.closed_form_plain(sel, t[pos], w[pos], bc.KINDS[ki][1], "none", None)
        rows = np.zeros((N, 4))
        rows[pos] = c_g
        assert tuple(out.shape) == (pos.size, 4)
        assert _rel(out.detach().cpu().numpy(), c_l) <= REL
        assert _rel(pl.grad.cpu().numpy(), bc.scatter(rows, lab, K, C, agnostic)) <= REL
    nolab = _t(bc.gather_labels(bc.shape_index("n67x5", bc.GATHER_SHAPES)))
    out = bbox_head_reg_loss(_module(0), pt.clone().requires_grad_(True), nolab, tt, wt, K, reduction_override="none")
    assert out.dim() == 0 and out.item() == 0.0


def test_empty_inputs_follow_the_reference(ref):
    """The empty-input table of the fixture, value for value: a 0-d zero without a weight, NaN / 0 / 0 / an empty [0, 4] with
    an empty weight, ValueError for 'sum' with an avg_factor; and the gradient of an empty prediction is empty."""
    g = ref["g"]
    for i, (wm, red, af) in enumerate(bc.empty_cases()):
        for ki in (0, 1):
            pl = torch.zeros((0, 4), device=DEV, requires_grad=True)
            wt = None if wm == "none" else torch.zeros((0, 4), device=DEV)
            call = lambda: _module(ki, red)(pl, torch.zeros((0, 4), device=DEV), wt, avg_factor=bc.AVG_FACTOR if af else None)  # noqa: E731
            status, value = int(g["empty_status"][i]), float(g["empty_value"][i])
            if status == bc.EMPTY_RAISES:
                with pytest.raises(ValueError):
                    call()
                continue
            out = call()
            if status == bc.EMPTY_TENSOR:
                assert tuple(out.shape) == (0, 4) and out.dtype == torch.float32
            else:
                assert out.dim() == 0
                assert (np.isnan(value) and np.isnan(out.item())) or out.item() == value, (wm, red, af, out.item(), value)
            out.sum().backward()
            assert pl.grad.shape == (0, 4)
    # an empty batch through the head
    from iif_amd.mmdet_bbox_loss import bbox_head_reg_loss
    pl = torch.zeros((0, 20), device=DEV, requires_grad=True)
    out = bbox_head_reg_loss(_module(0), pl, torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros((0, 4), device=DEV),
                             torch.zeros((0, 4), device=DEV), 5)
    out.backward()
    assert out.item() == 0.0 and pl.grad.shape == (0, 20)


def test_repeat_calls_are_bit_identical_and_leave_the_ticket_at_zero(gather_in):
    for name in ("g1024x1203", "g300x37", "g67x5"):
        si = bc.shape_index(name, bc.GATHER_SHAPES)
        _, N, C, K, agnostic, _ = bc.GATHER_SHAPES[si]
        _, _, _, _, pt, lt, tt, wt = gather_in(si)
        for ki in range(len(bc.KINDS)):
            a = _gather(ki, pt, lt, tt, wt, K, agnostic)
            b = _gather(ki, pt, lt, tt, wt, K, agnostic)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
            assert _ticket(pt) == 0, name
    host = bc.plain_inputs(bc.shape_index("p4099x4", bc.PLAIN_SHAPES))
    pt, tt, wt = (_t(v) for v in host)
    outs = []
    for _ in range(2):
        pl = pt.clone().requires_grad_(True)
        out = _module(2, "sum")(pl, tt, wt)
        out.backward()
        outs.append((out.detach(), pl.grad))
        assert _ticket(pt) == 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_backward_twice_and_the_upstream_scalar(gather_in):
    """retain_graph: the saved compact gradient is not overwritten by backward; an upstream scalar of 0.5 (Cascade's
    stage_loss_weights) halves the gradient exactly."""
    from iif_amd.mmdet_bbox_loss import bbox_head_reg_loss
    si = bc.shape_index("g300x37", bc.GATHER_SHAPES)
    _, N, C, K, agnostic, _ = bc.GATHER_SHAPES[si]
    _, _, _, _, pt, lt, tt, wt = gather_in(si)
    host = bc.plain_inputs(bc.shape_index("p1027", bc.PLAIN_SHAPES))
    qt, ut, vt = (_t(v) for v in host)
    for ki in range(len(bc.KINDS)):
        calls = (lambda x: bbox_head_reg_loss(_module(ki), x, lt, tt, wt, K), pt), (lambda x: _module(ki)(x, ut, vt), qt)
        for fn, x in calls:
            pl = x.clone().requires_grad_(True)
            out = fn(pl)
            out.backward(retain_graph=True)
            first = pl.grad.clone()
            pl.grad = None
            out.backward()
            assert torch.equal(pl.grad, first)
            ph = x.clone().requires_grad_(True)
            (fn(ph) * 0.5).backward()
            assert torch.equal(ph.grad, first * 0.5) and first.any()


def test_raw_entry_with_a_workspace_of_its_own():
    """The C entry on a caller's workspace (IIF_CE_WORKSPACE_BYTES, zeroed once): the ticket is back at zero after every call;
    loss only (no dsel); the element losses add up to the scalar; a flat range on a 4-byte phase (one element per lane) gives
    the numbers of the 16-byte path."""
    from iif_amd import _lib
    si = bc.shape_index("p4099x4", bc.PLAIN_SHAPES)
    p, t, w = bc.plain_inputs(si)
    n = p.size
    ws = torch.zeros(1 + 2048, dtype=torch.int32, device=DEV)
    pt, tt, wt = _t(p), _t(t), _t(w)
    elems = torch.empty(n, device=DEV)
    got = []
    for _ in range(3):
        loss = torch.full((), -1.0, device=DEV)
        rc = _lib.lib().iif_bbox_reg_fwd(_lib.ptr(pt), 0, 4, None, 1, 1, _lib.ptr(tt), _lib.ptr(wt), 1.0 / 9.0, 0.5, n, 0,
                                         _lib.ptr(elems), _lib.ptr(loss), None, _lib.ptr(ws), _lib.stream_ptr())
        assert rc == 0 and int(ws[0].item()) == 0
        got.append(float(loss))
    assert got[0] == got[1] == got[2]
    c_l, _ = bc.closed_form_plain(p, t, w, 1.0 / 9.0, "sum", None, 0.5)
    assert _rel(got[0], c_l) <= REL and _rel(0.5 * float(elems.double().sum()), c_l) <= REL
    # the same range one element off the 16-byte boundary: every array shifted alike
    shifted = [torch.zeros(n + 5, device=DEV) for _ in range(5)]
    for dst, src in zip(shifted, (pt, tt, wt)):
        dst[1:1 + n] = src.reshape(-1)
    ps, ts_, wsh, es, ds = (v[1:1 + n] for v in shifted)
    dref = torch.empty(n, device=DEV)
    loss2 = torch.empty((), device=DEV)
    for (a, b, c, e, d) in ((pt, tt, wt, elems, dref), (ps, ts_, wsh, es, ds)):
        rc = _lib.lib().iif_bbox_reg_fwd(_lib.ptr(a), 0, 4, None, 1, 1, _lib.ptr(b), _lib.ptr(c), 1.0 / 9.0, 0.5, n, 0, _lib.ptr(e),
                                         _lib.ptr(loss2), _lib.ptr(d), _lib.ptr(ws), _lib.stream_ptr())
        assert rc == 0 and int(ws[0].item()) == 0
    assert torch.equal(es, elems) and torch.equal(ds, dref) and _rel(float(loss2), c_l) <= REL
    assert shifted[3][0] == 0 and not shifted[3][1 + n:].any() and shifted[4][0] == 0 and not shifted[4][1 + n:].any()


def test_forward_and_backward_do_not_synchronise(gather_in):
    """forward + backward under torch's sync debug mode ('error'): bbox_head_reg_loss ('mean') with both modules, a batch
    without positives included, and both modules on flat inputs, 'mean' with and without avg_factor, and 'sum'."""
    from iif_amd.mmdet_bbox_loss import bbox_head_reg_loss
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    si = bc.shape_index("g300x37", bc.GATHER_SHAPES)
    _, N, C, K, agnostic, _ = bc.GATHER_SHAPES[si]
    _, _, _, _, pt, lt, tt, wt = gather_in(si)
    nolab = _t(bc.gather_labels(bc.shape_index("n67x5", bc.GATHER_SHAPES)))
    _, _, _, _, p67, _, t67, w67 = gather_in(bc.shape_index("n67x5", bc.GATHER_SHAPES))
    qt, ut, vt = (_t(v) for v in bc.plain_inputs(bc.shape_index("p4099x4", bc.PLAIN_SHAPES)))
    mods = [_module(0), _module(1), _module(2)]
    xs = [pt.clone().requires_grad_(True) for _ in mods]
    ys = [qt.clone().requires_grad_(True) for _ in mods]
    x67 = p67.clone().requires_grad_(True)
    for m in mods:                                          # the workspace exists before the mode is on
        m(qt, ut, vt)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for m, xl, yl in zip(mods, xs, ys):
            (bbox_head_reg_loss(m, xl, lt, tt, wt, K) * 0.5).backward()
            bbox_head_reg_loss(m, x67, nolab, t67, w67, 5).backward()
            for red, avg in (("mean", None), ("mean", 12.5), ("sum", None)):
                m(yl, ut, vt, avg_factor=avg, reduction_override=red).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.isfinite(v.grad).all() for v in xs + ys) and not x67.grad.any()


def test_registration_without_mmdet():
    from iif_amd import mmdet_bbox_loss
    assert mmdet_bbox_loss.register_into_mmdet() is False
