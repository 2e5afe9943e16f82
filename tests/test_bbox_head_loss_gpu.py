"""BBoxHead.loss without a host read (csrc/head_loss.hip, iif_amd/mmdet_bbox_head_loss.py) on the MI355X, against the
reference's own runs (tests/golden/g36_bbox_head_loss.npz) and the float64 restatement that the host tests pin to them.

Tolerances (none comes from what the kernel gives):
  * loss: max(4 x |float32 reference - float64 reference|, (C + 16) 2^-24 sum|term|), the project's convention for a summed loss;
  * gradient: 4 x the float32 reference's own largest error, relative to the largest element of the float64 gradient - taken
    case by case, which is never more than the largest over the fixture (2.6e-6, case o64x81).  On the small cases the
    float32 reference happens to land within a fraction of a float32 rounding unit of the float64 one (c5x81: 1.0e-8 of the
    largest element, against the 2^-24 = 6.0e-8 that a CORRECTLY ROUNDED float32 gradient may be off), so a case's reference
    error is taken no smaller than 2^-24 of the largest element: no float32 result can promise less.  bf16 scores get their
    gradient back in bf16 after two roundings to that format (the stored gradient, then the scaled one), each at most the
    format's unit roundoff 2^-8 of the element (8 significand bits): 2^-7 of the largest element is added for those cases;
  * avg_factor, the accuracy and every statement about zeros or repeated calls: exact.
Each case prints the fractions of its two bounds that it used (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

from . import bbox_head_loss_cases as hc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_CASES = [n for n, c in hc.CASES.items() if not c[3]]
BF16_CASES = [n for n, c in hc.CASES.items() if c[3]]


def T(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV, dtype=dtype)


@pytest.fixture(scope="module")
def ref(golden):
    g = golden("g36_bbox_head_loss")
    hc.check_generator(g)
    return g


@functools.lru_cache(maxsize=None)
def restated(name):
    return hc.restate_case(name)


def loss_module(name, **over):
    """Our module for the case: IIFLoss with the case's table, or the softmax CrossEntropyLoss."""
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    from iif_amd.mmdet_iif_loss import IIFLoss
    N, C, kind, bf, pad, cwf, lw, ignore, neg = hc.CASES[name]
    cw = hc.class_weight(name)
    kw = dict(loss_weight=lw, ignore_index=ignore, class_weight=None if cw is None else cw.tolist())
    kw.update(over)
    if kind == "ce":
        return CrossEntropyLoss(**kw)
    m = IIFLoss(path=hc.LVIS_CSV, num_classes=C - 1, device=DEV, **kw)
    m.iif_weights = T(hc.table(name)).unsqueeze(0)
    return m


def run(name, scores=None, labels=None, weights=None, upstream=None, crit=None):
    """head_cls_loss + backward on the case (or on replacements of its inputs): dict of host arrays and the device tensors."""
    from iif_amd.mmdet_bbox_head_loss import head_cls_loss
    x, lab, w = hc.inputs(name)
    bf = hc.CASES[name][3]
    xs = (T(x, torch.bfloat16 if bf else None) if scores is None else scores).detach().requires_grad_(True)
    out = head_cls_loss(crit or loss_module(name), xs, T(lab) if labels is None else labels, T(w) if weights is None else weights)
    key = "acc_classes" if hc.CASES[name][2] == "iif" else "acc"
    assert set(out) == {"loss_cls", key, "avg_factor"}
    loss = out["loss_cls"] if upstream is None else upstream * out["loss_cls"]
    loss.backward()
    assert xs.grad.dtype == xs.dtype and tuple(out[key].shape) == (1,) and out["avg_factor"].dim() == 0 and out["loss_cls"].dim() == 0
    return dict(loss=out["loss_cls"].detach(), acc=out[key].detach(), avg=out["avg_factor"].detach(), grad=xs.grad, x=xs, out=out)


@functools.lru_cache(maxsize=None)
def base(name):
    """The case run once, shared by the tests that only read it."""
    return run(name)


def bounds(ref, name):
    N, C, bf = hc.CASES[name][0], hc.CASES[name][1], hc.CASES[name][3]
    l32, l64 = float(ref[name + "_loss32"]), float(ref[name + "_loss64"])
    loss_tol = max(4.0 * abs(l32 - l64), (C + 16) * 2.0 ** -24 * restated(name)["sum_abs"])
    gmax = float(ref[name + "_gmax64"])
    grad_tol = 4.0 * max(float(ref[name + "_e32_grad"]), 2.0 ** -24 * gmax) + (2.0 ** -7 * gmax if bf else 0.0)
    assert grad_tol <= (4.0 * float(ref["worst"][1]) + (2.0 ** -7 if bf else 0.0)) * gmax          # never wider than the fixture-wide reading
    return loss_tol, grad_tol, gmax


def check_against_reference(ref, name, r, what=""):
    rs = restated(name)
    loss_tol, grad_tol, gmax = bounds(ref, name)
    e_l = abs(float(r["loss"]) - float(ref[name + "_loss64"]))
    e_g = float(np.abs(r["grad"].double().cpu().numpy() - rs["grad"]).max())
    print("%s%s: loss error %.3g = %.3f of its bound, gradient error %.3g (%.3g of the largest element) = %.3f of its bound"
          % (name, what, e_l, e_l / loss_tol if loss_tol else 0.0, e_g, e_g / gmax if gmax else 0.0, e_g / grad_tol if grad_tol else 0.0))
    assert e_l <= loss_tol, (name, e_l, loss_tol)
    assert e_g <= grad_tol, (name, e_g, grad_tol)
    return e_l / loss_tol if loss_tol else 0.0, e_g / grad_tol if grad_tol else 0.0


def check_integers(ref, name, r):
    assert float(r["avg"]) == float(ref[name + "_avg"]) == restated(name)["avg"]
    assert np.array_equal(r["acc"].cpu().numpy(), ref[name + "_acc_valid"]), (name, r["acc"], ref[name + "_acc_valid"])


# ---------------------------------------------------------------------------------------- 1, 2: the reference's values
@pytest.mark.parametrize("name", F32_CASES + BF16_CASES)
def test_loss_gradient_avg_factor_and_accuracy(ref, name):
    r = base(name)
    check_against_reference(ref, name, r)
    check_integers(ref, name, r)
    x, lab, w = hc.inputs(name)
    dead = (w == 0) | (lab < 0)
    assert not r["grad"][T(dead)].any()                                  # rows of weight zero and ignored rows: exact zeros


def test_a_wider_pitch_is_read_in_place(ref):
    """ld > C: a view into a wider buffer whose other columns hold NaN; the same bits as the dense case."""
    for name, pitch in (("i63x1205", 1208), ("c257x81", 83), ("c257x81b", 96)):
        x = base(name)["x"].detach()
        wide = torch.full((x.shape[0], pitch), float("nan"), dtype=x.dtype, device=DEV)
        wide[:, :x.shape[1]] = x
        r = run(name, scores=wide[:, :x.shape[1]])
        assert r["x"].stride(0) == pitch
        for k in ("loss", "acc", "avg", "grad"):
            assert torch.equal(r[k], base(name)[k]), (name, k)


@pytest.mark.parametrize("name", [n for n, c in hc.CASES.items() if c[4] == hc.PAD_NONE])
def test_unpadded_accuracy_is_get_accuracy(ref, name):
    """Without rows of weight zero the accuracy is the reference's over all rows, and our module's get_accuracy bit for bit."""
    r = base(name)
    crit = loss_module(name)
    x, lab, w = hc.inputs(name)
    assert np.array_equal(r["acc"].cpu().numpy(), ref[name + "_acc_all"])
    if hasattr(crit, "get_accuracy"):
        assert torch.equal(crit.get_accuracy(r["x"].detach(), T(lab))["acc_classes"], r["acc"])
    else:
        from iif_amd.utils import topk_hit_counts
        assert torch.equal(topk_hit_counts(r["x"].detach(), T(lab), (1,)).float() * (100.0 / x.shape[0]), r["acc"])


def test_ties_follow_the_lowest_index_rule(ref):
    from iif_amd.mmdet_bbox_head_loss import head_cls_loss
    x, lab, w = hc.inputs("c257x81")
    rows = [hc.TIE_LOWER, hc.TIE_HIGHER, hc.FLAT_FIRST, hc.FLAT_OTHER]
    want = [0.0, 100.0, 100.0, 0.0]
    for r, a in zip(rows, want):
        out = head_cls_loss(loss_module("c257x81"), T(x[r:r + 1]), T(lab[r:r + 1]), T(w[r:r + 1]))
        assert float(out["acc"]) == a and float(out["avg_factor"]) == 1.0, r


# ---------------------------------------------------------------------------------------- 3: padding
def test_every_weight_zero(ref):
    r = base("z5x5")
    assert float(r["loss"]) == 0.0 and float(r["acc"]) == 0.0 and float(r["avg"]) == 1.0 and not r["grad"].any()
    assert float(ref["z5x5_loss32"]) == 0.0 and float(ref["z5x5_avg"]) == 1.0


def test_exactly_one_valid_row(ref):
    r = base("o64x81")
    assert float(r["avg"]) == 1.0 and float(r["acc"]) == 100.0
    keep = torch.zeros(64, dtype=torch.bool, device=DEV)
    keep[hc.VALID_ROW] = True
    assert not r["grad"][~keep].any() and r["grad"][keep].any()


@pytest.mark.parametrize("name", ["c257x81", "i65x1204", "i63x1205b"])
def test_nan_in_zero_weight_rows_changes_no_bit(ref, name):
    x, lab, w = hc.inputs(name)
    xs = base(name)["x"].detach().clone()
    xs[T(w == 0)] = float("nan")
    r = run(name, scores=xs)
    for k in ("loss", "acc", "avg", "grad"):
        assert torch.equal(r[k], base(name)[k]), (name, k)
    assert not r["grad"][T(w == 0)].any() and torch.isfinite(r["grad"].float()).all()


# ---------------------------------------------------------------------------------------- 4: labels
def test_ignored_background_and_weighted_rows_are_in_the_cases():
    x, lab, w = hc.inputs("i63x1205")
    assert (lab == -1).any() and (lab == 1204).any() and w[11] == 1.0 and lab[11] == -1
    assert hc.CASES["i63x1205"][7] == -1 and hc.CASES["c5x81"][5] and hc.CASES["c5x81"][6] == 1.5 and hc.CASES["i65x1204"][6] == 0.75


def test_a_label_outside_the_classes_contributes_nothing_and_is_reported(ref):
    from iif_amd import custom
    name = "c257x81"
    x, lab, w = hc.inputs(name)
    try:
        custom.check_label_status()                                  # start clean, whatever ran before
    except IndexError:
        pass
    bad = lab.copy()
    rows = [0, 1]
    bad[rows] = [81, -7]
    w2 = w.copy()
    w2[rows] = 1.0
    r = run(name, labels=T(bad), weights=T(w2))
    with pytest.raises(IndexError):
        custom.check_label_status()
    custom.check_label_status()                                      # reported once, then clean
    # the same as the float64 restatement, which drops such rows (they still count in avg_factor: their weight is > 0)
    rs = hc.restate64(x, None, bad, w2, None, None, 1.0)
    assert float(r["avg"]) == rs["avg"] and float(r["acc"]) == float(rs["acc"])
    loss_tol, grad_tol, gmax = bounds(ref, name)
    assert abs(float(r["loss"]) - rs["loss"]) <= loss_tol
    assert float(np.abs(r["grad"].double().cpu().numpy() - rs["grad"]).max()) <= grad_tol
    assert not r["grad"][rows].any()
    # in a row of weight zero the label is not read either
    w3 = w2.copy()
    w3[rows] = 0.0
    run(name, labels=T(bad), weights=T(w3))
    custom.check_label_status()


# ---------------------------------------------------------------------------------------- 5: today's path
@pytest.mark.parametrize("name", ["i65x1204", "c257x81", "i63x1205", "c5x81", "i65x1204b"])
def test_agrees_with_the_host_avg_factor_path(ref, name):
    """The chain that exists today - torch count, .item(), the module's forward (iif_ce_fwd_bwd), autograd backward - on the
    same inputs, against the float64 reference within the bounds of check 1: parity with the parent's kernel."""
    x, lab, w = hc.inputs(name)
    crit = loss_module(name)
    xs = base(name)["x"].detach().clone().requires_grad_(True)
    wt = T(w)
    avg = max(torch.sum(wt > 0).float().item(), 1.)
    loss = crit(xs, T(lab), wt, avg_factor=avg)
    loss.backward()
    old = dict(loss=loss.detach(), grad=xs.grad)
    assert avg == float(base(name)["avg"])
    check_against_reference(ref, name, old, " (host avg_factor path)")
    loss_tol, grad_tol, gmax = bounds(ref, name)
    assert abs(float(old["loss"]) - float(base(name)["loss"])) <= 2 * loss_tol
    assert float((old["grad"].double() - base(name)["grad"].double()).abs().max()) <= 2 * grad_tol


# ---------------------------------------------------------------------------------------- 6: determinism and reuse
@pytest.mark.parametrize("name", ["i257x1204", "c257x81b", "i3x5"])
def test_two_calls_give_identical_bits(ref, name):
    a, b = run(name), run(name)
    for k in ("loss", "acc", "avg", "grad"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], base(name)[k]), (name, k)


@pytest.mark.parametrize("name", ["i65x1204", "c257x81b"])
def test_backward_twice_and_an_upstream_factor(ref, name):
    from iif_amd.mmdet_bbox_head_loss import head_cls_loss
    x, lab, w = hc.inputs(name)
    xs = base(name)["x"].detach().clone().requires_grad_(True)
    out = head_cls_loss(loss_module(name), xs, T(lab), T(w))
    out["loss_cls"].backward(retain_graph=True)
    g1 = xs.grad.clone()
    xs.grad = None
    out["loss_cls"].backward()
    assert torch.equal(xs.grad, g1) and torch.equal(g1, base(name)["grad"])
    r3 = run(name, upstream=3.0)
    assert torch.equal(r3["loss"], base(name)["loss"])
    if xs.dtype == torch.float32:
        # one rounding of (3 lw / avg) u against two of 3 ((lw / avg) u): 2 ulp of the element
        assert float((r3["grad"] - 3.0 * g1).abs().max()) <= 4 * 2.0 ** -23 * float(g1.abs().max())
    else:
        assert float((r3["grad"].float() - 3.0 * g1.float()).abs().max()) <= 2.0 ** -7 * 3.0 * float(g1.float().abs().max())
    check_against_reference(ref, name, dict(loss=r3["loss"], grad=r3["grad"].double() / 3.0), " (upstream 3)")


def test_an_empty_batch():
    from iif_amd.mmdet_bbox_head_loss import bbox_head_loss, head_cls_loss
    from iif_amd.mmdet_bbox_loss import L1Loss
    for name in ("c5x81", "i65x1204"):
        C = hc.CASES[name][1]
        xs = torch.zeros((0, C), device=DEV, requires_grad=True)
        lab, w = torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, device=DEV)
        out = head_cls_loss(loss_module(name), xs, lab, w)
        key = "acc_classes" if hc.CASES[name][2] == "iif" else "acc"
        assert float(out["loss_cls"].detach()) == 0.0 and float(out[key]) == 0.0 and float(out["avg_factor"]) == 1.0
        out["loss_cls"].backward()
        assert tuple(xs.grad.shape) == (0, C)
        # the reference adds no classification key for an empty cls_score (bbox_head.py:268)
        assert bbox_head_loss(loss_module(name), L1Loss(), xs, None, None, lab, w, None, None, C - 1) == {}


# ---------------------------------------------------------------------------------------- 7: both halves
def test_bbox_head_loss_gives_the_references_three_values_and_both_gradients(ref):
    from iif_amd.mmdet_bbox_head_loss import bbox_head_loss
    from iif_amd.mmdet_bbox_loss import L1Loss
    name, K = hc.BOTH, hc.BBOX_CLASSES
    x, lab, w = hc.inputs(name)
    p, t, bw = hc.bbox_inputs()
    crit, reg = loss_module(name), L1Loss(loss_weight=hc.BBOX_LOSS_WEIGHT)
    xs, bp = T(x).requires_grad_(True), T(p).requires_grad_(True)
    args = (None, T(lab), T(w), T(t), T(bw), K)
    losses = bbox_head_loss(crit, reg, xs, bp, *args)
    assert set(losses) == {"loss_cls", "acc", "loss_bbox"}                 # the reference's keys
    (losses["loss_cls"] + losses["loss_bbox"]).backward()
    r = dict(loss=losses["loss_cls"].detach(), grad=xs.grad, acc=losses["acc"].detach(), avg=base(name)["avg"])
    check_against_reference(ref, name, r, " (bbox_head_loss)")
    check_integers(ref, name, r)
    assert torch.equal(xs.grad, base(name)["grad"])
    # the regression half: test_bbox_reg_gpu's convention, 4 x the float32 reference's error or (n + 16) 2^-24 of the terms
    l32, l64 = float(ref["bbox_loss32"]), float(ref["bbox_loss64"])
    pos = (lab >= 0) & (lab < K)
    sel = p.reshape(len(lab), K, 4)[pos, lab[pos]]
    terms = hc.BBOX_LOSS_WEIGHT * np.abs(sel.astype(np.float64) - t[pos]) * bw[pos] / len(lab)
    assert abs(terms.sum() - l64) <= 1e-12 * abs(l64)
    assert abs(float(losses["loss_bbox"]) - l64) <= max(4 * abs(l32 - l64), (terms.size + 16) * 2.0 ** -24 * np.abs(terms).sum())
    dense = np.zeros(p.shape)
    dense[ref["bbox_grad_rows"], ref["bbox_grad_cols"]] = ref["bbox_grad64"]
    assert float(np.abs(bp.grad.double().cpu().numpy() - dense).max()) <= 4 * 2.0 ** -24 * np.abs(dense).max()
    assert np.count_nonzero(bp.grad.cpu().numpy()) == ref["bbox_grad64"].size
    # either half alone
    only_cls = bbox_head_loss(crit, reg, xs.detach(), None, *args)
    assert set(only_cls) == {"loss_cls", "acc"} and torch.equal(only_cls["loss_cls"], r["loss"]) and torch.equal(only_cls["acc"], r["acc"])
    only_reg = bbox_head_loss(crit, reg, None, bp.detach(), *args)
    assert set(only_reg) == {"loss_bbox"} and torch.equal(only_reg["loss_bbox"], losses["loss_bbox"].detach())


# ---------------------------------------------------------------------------------------- 8: no synchronisation
def test_nothing_synchronises_the_host():
    """roi_stage_targets_padded -> a linear stand-in for the head -> bbox_head_loss -> backward(), two cascade rounds with
    refine_bboxes_padded in between, under torch's sync debug mode ('error'); mirrors
    test_roi_stage_gpu.test_nothing_synchronises_the_host."""
    from iif_amd import custom
    from iif_amd.mmdet_bbox_head_loss import bbox_head_loss
    from iif_amd.mmdet_bbox_loss import SmoothL1Loss
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    from iif_amd.mmdet_roi_stage import refine_bboxes_padded, roi_stage_targets_padded
    from . import assign_cases as ac
    from . import roi_stage_cases as rc
    from .test_roi_stage_gpu import parts
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    B, num, P, K = 2, 64, 40, rc.REFINE_CLASSES                 # fewer candidates than num: every image has padding rows
    shapes = [rc.IMG] * B
    props = torch.stack([T(ac.proposals(P, 9100 + b, rc.IMG[1], rc.IMG[0], 8, 120)) for b in range(B)])
    counts = torch.tensor([P, P - 15], dtype=torch.int64, device=DEV)
    gts = [T(ac.proposals(5, 9110 + b, rc.IMG[1], rc.IMG[0], 16, 160)) for b in range(B)]
    labs = [T(rc._u(5, 9120 + b, K)) for b in range(B)]
    stages = [parts(ac._with(rc.RCNN, pos=t, neg=t, min_pos=t), num, 0.25) for t in (0.5, 0.6)]
    coder = stages[0][2]
    gen = torch.Generator(device="cpu").manual_seed(7)
    heads = [(torch.randn(K + 1, 5, generator=gen).mul_(0.01).to(DEV).requires_grad_(True),
              torch.randn(4 * K, 5, generator=gen).mul_(0.001).to(DEV).requires_grad_(True)) for _ in range(2)]
    loss_cls, loss_bbox = CrossEntropyLoss(), SmoothL1Loss(beta=1.0)

    def rounds():
        out = []
        t = roi_stage_targets_padded(props, counts, gts, labs, *stages[0], K)
        for i in range(2):
            feat = t.rois / 100.0                                                # stands for the extractor and the shared layers
            cls_score, bbox_pred = feat @ heads[i][0].t(), feat @ heads[i][1].t()
            losses = bbox_head_loss(loss_cls, loss_bbox, cls_score, bbox_pred, t.rois, t.labels, t.label_weights, t.bbox_targets,
                                    t.bbox_weights, K)
            (losses["loss_cls"] + losses["loss_bbox"]).backward()
            out.append((t, losses))
            if i == 0:
                labels = torch.where(t.labels < K, t.labels, torch.zeros_like(t.labels))          # stands for the argmax
                boxes, kept = refine_bboxes_padded(t.rois, labels, bbox_pred.detach(), t.pos_is_gt, t.counts, shapes, coder)
                t = roi_stage_targets_padded(boxes, kept, gts, labs, *stages[1], K)
        return out

    rounds()                                                                     # the library and the workspaces exist before the mode is on
    for h in heads:
        h[0].grad = h[1].grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = rounds()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    custom.check_label_status()
    for (t, losses), h in zip(out, heads):
        valid = int((t.label_weights > 0).sum())
        assert 0 < valid < B * num                                               # there are padding rows, and they did not count
        assert set(losses) == {"loss_cls", "acc", "loss_bbox"}
        assert all(torch.isfinite(v).all().item() for v in losses.values())
        assert float(losses["loss_cls"]) > 0 and 0.0 <= float(losses["acc"]) <= 100.0
        assert torch.isfinite(h[0].grad).all() and h[0].grad.abs().max() > 0 and torch.isfinite(h[1].grad).all()
        # the loss of the rows that count, by torch, on the same scores
        feat = t.rois / 100.0
        keep = t.label_weights > 0
        want = torch.nn.functional.cross_entropy((feat @ h[0].detach().t())[keep].double(), t.labels[keep])
        assert abs(float(losses["loss_cls"]) - float(want)) <= 1e-5 * float(want)
