"""The sigmoid and Seesaw kinds of BBoxHead.loss without a host read (csrc/head_loss.hip: iif_head_bce_loss_fwd;
csrc/seesaw_head.hip: iif_seesaw_head_fwd / _bwd; iif_amd/mmdet_bbox_head_loss.py) on the MI355X, against the reference's own
runs (tests/golden/g38_head_loss_kinds.npz) and the float64 restatement that the host tests pin to them.

Tolerances are test_bbox_head_loss_gpu.py's (none comes from what the kernels give):
  * a loss: max(4 x |float32 reference - float64 reference|, (K + 16) 2^-24 sum|term|), K the columns of a row;
  * the gradient: 4 x the float32 reference's own largest error on the case, relative to the largest element of the float64
    gradient and never below 2^-24 of it (no float32 result can promise less); bf16 scores get their gradient back in bf16
    after two roundings to that format: 2^-7 of the largest element is added;
  * avg_factor, the accuracies, the cum_samples bits and every statement about zeros or repeated calls: exact.
Each case prints the fractions of its bounds that it used (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

from . import head_loss_kinds_cases as kc
from . import seesaw_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV, dtype=dtype)


@pytest.fixture(scope="module")
def ref(golden):
    g = golden("g38_head_loss_kinds")
    kc.check_generator(g)
    return g


@functools.lru_cache(maxsize=None)
def restated(name):
    return kc.restate_case(name)


def loss_module(name, cum=None, **over):
    """Our module for the case: CrossEntropyLoss(use_sigmoid=True), or SeesawLoss holding the case's cum_samples."""
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    c = kc.CASES[name]
    if c["kind"] == "sig":
        cw = kc.class_weight(name)
        kw = dict(use_sigmoid=True, loss_weight=c["lw"], ignore_index=c["ignore"], class_weight=None if cw is None else cw.tolist())
        kw.update(over)
        return CrossEntropyLoss(**kw)
    kw = dict(p=c["p"], q=c["q"], num_classes=c["C"], eps=kc.EPS, loss_weight=c["lw"], device=DEV)
    kw.update(over)
    m = SeesawLoss(**kw)
    m.cum_samples.copy_(T(kc.cum_before(name) if cum is None else cum))
    return m


def run(name, scores=None, labels=None, weights=None, upstream=None, crit=None):
    """head_cls_loss + backward on the case (or on replacements of its inputs): the device tensors."""
    from iif_amd.mmdet_bbox_head_loss import head_cls_loss
    x, lab, w = kc.inputs(name)
    c = kc.CASES[name]
    see = c["kind"] == "see"
    xs = (T(x, torch.bfloat16 if c["bf"] else None) if scores is None else scores).detach().requires_grad_(True)
    crit = crit or loss_module(name)
    out = head_cls_loss(crit, xs, T(lab) if labels is None else labels, T(w) if weights is None else weights)
    if see:
        assert set(out) == {"loss_cls_classes", "loss_cls_objectness", "acc_classes", "acc_objectness", "avg_factor"}
        losses, accs = (out["loss_cls_classes"], out["loss_cls_objectness"]), (out["acc_classes"], out["acc_objectness"])
    else:
        assert set(out) == {"loss_cls", "acc", "avg_factor"}
        losses, accs = (out["loss_cls"],), (out["acc"],)
    total = sum(losses)
    (total if upstream is None else upstream * total).backward()
    assert xs.grad.dtype == xs.dtype and out["avg_factor"].dim() == 0 and out["avg_factor"].is_cuda
    assert all(l.dim() == 0 for l in losses) and all(tuple(a.shape) == (1,) and a.is_cuda for a in accs)
    return dict(loss=torch.stack([l.detach() for l in losses]), acc=torch.cat([a.detach() for a in accs]), avg=out["avg_factor"].detach(),
                grad=xs.grad, x=xs, out=out, cum=crit.cum_samples.clone() if see else torch.zeros(0, device=DEV))


KEYS = ("loss", "acc", "avg", "grad", "cum")
_BASE = {}


def base(name):
    """The case run once, shared by the tests that only read it.  The three STATE cases are consecutive calls on ONE module."""
    if name not in _BASE:
        if name in kc.STATE:
            crit = loss_module(kc.STATE[0])
            for n in kc.STATE:
                _BASE[n] = run(n, crit=crit)
        else:
            _BASE[name] = run(name)
    return _BASE[name]


def bounds(ref, name):
    c = kc.CASES[name]
    rs, K = restated(name), kc.columns(name)
    sums = (rs["sum_abs_cls"], rs["sum_abs_obj"]) if c["kind"] == "see" else (rs["sum_abs"],)
    loss_tol = [max(4.0 * abs(float(a) - float(b)), (K + 16) * 2.0 ** -24 * s) for a, b, s in zip(ref[name + "_loss32"], ref[name + "_loss64"], sums)]
    gmax = float(ref[name + "_gmax64"])
    grad_tol = 4.0 * max(float(ref[name + "_e32_grad"]), 2.0 ** -24 * gmax) + (2.0 ** -7 * gmax if c["bf"] else 0.0)
    assert grad_tol <= (4.0 * max(float(ref["worst"][1]), 2.0 ** -24) + (2.0 ** -7 if c["bf"] else 0.0)) * gmax      # never wider than the fixture-wide reading
    return loss_tol, grad_tol, gmax


def check_against_reference(ref, name, r, what=""):
    rs = restated(name)
    loss_tol, grad_tol, gmax = bounds(ref, name)
    e_l = [abs(float(a) - float(b)) for a, b in zip(r["loss"], ref[name + "_loss64"])]
    e_g = float(np.abs(r["grad"].double().cpu().numpy() - rs["grad"]).max())
    frac = [e / t if t else 0.0 for e, t in zip(e_l, loss_tol)]
    print("%s%s: loss error %s = %s of its bound, gradient error %.3g (%.3g of the largest element) = %.3f of its bound"
          % (name, what, " ".join("%.3g" % e for e in e_l), " ".join("%.3f" % f for f in frac), e_g, e_g / gmax if gmax else 0.0,
             e_g / grad_tol if grad_tol else 0.0))
    for e, t in zip(e_l, loss_tol):
        assert e <= t, (name, e_l, loss_tol)
    assert e_g <= grad_tol, (name, e_g, grad_tol)


def check_integers(ref, name, r):
    rs = restated(name)
    assert float(r["avg"]) == float(ref[name + "_avg"]) == rs["avg"]
    assert np.array_equal(r["acc"].cpu().numpy(), ref[name + "_acc_valid"]), (name, r["acc"], ref[name + "_acc_valid"])
    if kc.CASES[name]["kind"] == "see":
        assert np.array_equal(r["cum"].cpu().numpy().view(np.int32), ref[name + "_cum"].view(np.int32)), name


# ---------------------------------------------------------------------------------------- 1: the reference's values
@pytest.mark.parametrize("name", list(kc.CASES))
def test_losses_gradient_avg_factor_accuracies_and_cum_samples(ref, name):
    r = base(name)
    check_against_reference(ref, name, r)
    check_integers(ref, name, r)
    x, lab, w = kc.inputs(name)
    if (w == 0).any():
        assert not r["grad"][T(w == 0)].any()                            # rows of weight zero: exact zeros
    c = kc.CASES[name]
    if c["pad"] == kc.PAD_ALL:
        assert not r["loss"].any() and not r["acc"].any() and float(r["avg"]) == 1.0 and not r["grad"].any()
        if c["kind"] == "see":
            assert np.array_equal(r["cum"].cpu().numpy(), kc.cum_before(name))
    if c["pad"] == kc.PAD_ONE:
        assert float(r["avg"]) == 1.0 and (r["acc"] == 100.0).all()
    if c["labels"] == "allbg":
        assert float(r["loss"][0]) == 0.0 and not r["grad"][:, :c["C"]].any() and float(r["acc"][0]) == 0.0      # seesaw_loss.py:249-250
    if c["kind"] == "see" and (w == 0).any() and c["pad"] == kc.PAD_MIXED:
        assert not np.array_equal(ref[name + "_cum"], ref[name + "_cum_padded"])       # what the reference adds for the padding rows


def test_return_dict_false_gives_the_sum(ref):
    from iif_amd.mmdet_bbox_head_loss import head_cls_loss
    name = "s257x80"
    x, lab, w = kc.inputs(name)
    xs = T(x).requires_grad_(True)
    out = head_cls_loss(loss_module(name, return_dict=False), xs, T(lab), T(w))
    assert set(out) == {"loss_cls", "acc_objectness", "acc_classes", "avg_factor"}
    b = base(name)
    assert torch.equal(out["loss_cls"].detach(), b["loss"][0] + b["loss"][1])
    out["loss_cls"].backward()
    assert torch.equal(xs.grad, b["grad"]) and torch.equal(torch.cat([out["acc_classes"], out["acc_objectness"]]), b["acc"])


def test_label_weights_none_means_all_ones():
    from iif_amd.mmdet_bbox_head_loss import head_cls_loss
    for name in ("g4x2", "s4x2"):
        x, lab, w = kc.inputs(name)
        assert (w == 1).all()
        out = head_cls_loss(loss_module(name), T(x), T(lab), None)
        keys = [k for k in out if k.startswith("loss")]
        assert torch.equal(torch.stack([out[k] for k in sorted(keys)]), torch.stack([base(name)["out"][k].detach() for k in sorted(keys)]))
        assert float(out["avg_factor"]) == float(len(lab))


# ---------------------------------------------------------------------------------------- 2: zero-weight rows are not read
@pytest.mark.parametrize("name", ["g257x80", "g65x1203b", "g63x2048", "s257x80", "s63x1203", "s65x2046"])
def test_nan_in_zero_weight_rows_changes_no_bit(ref, name):
    from iif_amd import custom
    x, lab, w = kc.inputs(name)
    try:
        custom.check_label_status()                                  # start clean, whatever ran before
    except IndexError:
        pass
    xs = base(name)["x"].detach().clone()
    xs[T(w == 0)] = float("nan")
    bad = lab.copy()
    bad[w == 0] = -12345                                             # on a live Seesaw row this would raise the flag
    r = run(name, scores=xs, labels=T(bad))
    for k in KEYS:
        assert torch.equal(r[k], base(name)[k]), (name, k)
    assert not r["grad"][T(w == 0)].any() and torch.isfinite(r["grad"].float()).all()
    custom.check_label_status()


# ---------------------------------------------------------------------------------------- 3: the existing kernels' bits
def _saved_gradient(losses):
    """The unit-scale gradient an autograd node of mmdet_bbox_head_loss saved (dscores / dscore of the C entry)."""
    return losses.grad_fn.saved_tensors[0]


@pytest.mark.parametrize("name", ["g4x2", "g257x1", "g64x2048", "g65x1203", "g257x80", "g63x1203"])
def test_sigmoid_gradient_is_the_bce_kernels(ref, name):
    from iif_amd import mmdet_bbox_head_loss as hl
    from iif_amd.mmdet_ce_loss import _launch_bce
    c = kc.CASES[name]
    x, lab, w = kc.inputs(name)
    w1 = np.where(w == 0, np.float32(0.25), w)                       # a batch without zero weights
    cw = kc.class_weight(name)
    cwt = None if cw is None else T(cw)
    ign = -100 if c["ignore"] is None else c["ignore"]
    xs = T(x).requires_grad_(True)
    loss, acc, avg = hl._HeadBceLoss.apply(xs, T(lab), T(w1), cwt, ign, c["lw"])
    _, _, dpred = _launch_bce(xs.detach(), T(lab), T(w1), ign, None, None, cwt, 1.0, True, False)
    d = _saved_gradient(loss)
    assert torch.equal(d, dpred) and d.abs().max() > 0
    # padded: the kept rows are those of the compacted call
    keep = T(w != 0)
    if not bool(keep.all()):
        lp, _, _ = hl._HeadBceLoss.apply(xs, T(lab), T(w), cwt, ign, c["lw"])
        xc = xs.detach()[keep].clone().requires_grad_(True)
        lc, ac, vc = hl._HeadBceLoss.apply(xc, T(lab)[keep], T(w)[keep], cwt, ign, c["lw"])
        assert torch.equal(_saved_gradient(lp)[keep], _saved_gradient(lc)) and not _saved_gradient(lp)[~keep].any()
        assert torch.equal(vc, base(name)["avg"])


@pytest.mark.parametrize("name", ["s4x2", "s64x2046", "s257x80", "s63x1203", "s65x2046", "s65x5pos"])
def test_seesaw_gradient_and_cum_samples_are_the_seesaw_kernels(ref, name):
    from iif_amd import mmdet_bbox_head_loss as hl
    from iif_amd.mmdet_seesaw_loss import _launch
    c = kc.CASES[name]
    C = c["C"]
    x, lab, w = kc.inputs(name)
    w1 = np.where(w == 0, np.float32(0.25), w)
    xs = T(x).requires_grad_(True)
    cum_a, cum_b = T(kc.cum_before(name)), T(kc.cum_before(name))
    out = hl._HeadSeesawLoss.apply(xs, T(lab), T(w1), cum_a, c["p"], c["q"], kc.EPS, c["lw"], False)
    _, _, d_old = _launch(xs.detach(), T(lab), T(w1), cum_b, True, c["p"], c["q"], kc.EPS, 1.0, False, 1.0, C, True)
    assert torch.equal(_saved_gradient(out[0]), d_old) and torch.equal(cum_a, cum_b) and d_old.abs().max() > 0
    keep = T(w != 0)
    if not bool(keep.all()):
        cum_p, cum_c = T(kc.cum_before(name)), T(kc.cum_before(name))
        op = hl._HeadSeesawLoss.apply(xs, T(lab), T(w), cum_p, c["p"], c["q"], kc.EPS, c["lw"], False)
        xc = xs.detach()[keep].clone().requires_grad_(True)
        oc = hl._HeadSeesawLoss.apply(xc, T(lab)[keep], T(w)[keep], cum_c, c["p"], c["q"], kc.EPS, c["lw"], False)
        assert torch.equal(_saved_gradient(op[0])[keep], _saved_gradient(oc[0])) and not _saved_gradient(op[0])[~keep].any()
        assert torch.equal(cum_p, cum_c) and torch.equal(cum_p, base(name)["cum"])
        for a, b in zip(op[2:], oc[2:]):
            assert torch.equal(a, b)                                 # both accuracies and avg_factor


def test_more_labels_than_one_count_block_takes():
    """N = 16400 rows: the count launch runs two blocks and passes the histogram and both row counts through its workspace."""
    from iif_amd import mmdet_bbox_head_loss as hl
    from iif_amd.mmdet_seesaw_loss import _launch
    N, C = 16400, 5
    x, lab, w = sc.make_inputs(N, C, 4)
    w[::3] = -w[::3]                                                 # negative weights count in the histogram, not in V
    cum0 = sc.make_cum(C, 4)
    xs = T(x).requires_grad_(True)
    cum = T(cum0)
    l_cls, l_obj, acc_obj, acc_cls, avg = hl._HeadSeesawLoss.apply(xs, T(lab), T(w), cum, 0.8, 2.0, kc.EPS, 1.0, False)
    rs = kc.restate_seesaw(x, lab, w, cum0, C, 0.8, 2.0, 1.0)
    assert float(avg) == rs["avg"] == float((w > 0).sum())
    assert np.array_equal(cum.cpu().numpy(), rs["cum"])
    assert np.array_equal(acc_obj.cpu().numpy(), rs["acc_obj"]) and np.array_equal(acc_cls.cpu().numpy(), rs["acc_cls"])
    for got, want, s in ((l_cls, rs["loss_cls"], rs["sum_abs_cls"]), (l_obj, rs["loss_obj"], rs["sum_abs_obj"])):
        assert abs(float(got) - want) <= (C + 2 + 16) * 2.0 ** -24 * s
    keep = T(w != 0)
    cum_b = T(cum0)
    _, _, d_old = _launch(xs.detach()[keep], T(lab)[keep], T(w)[keep], cum_b, True, 0.8, 2.0, kc.EPS, 1.0, False, 1.0, C, True)
    assert torch.equal(_saved_gradient(l_cls)[keep], d_old) and torch.equal(cum, cum_b)


# ---------------------------------------------------------------------------------------- 4: today's path
@pytest.mark.parametrize("name", ["g65x1203", "g257x80", "g65x1203b", "g63x1203", "s257x80", "s63x1203", "s5x80"])
def test_agrees_with_the_host_avg_factor_path(ref, name):
    """The chain that exists today - torch count, .item(), the module's own forward, autograd backward - against the float64
    reference within the bounds of check 1.  The Seesaw module counts every row it is given into cum_samples, so it gets the
    rows of weight != 0 (the contract's second part); the sigmoid module gets the padded batch."""
    x, lab, w = kc.inputs(name)
    see = kc.CASES[name]["kind"] == "see"
    crit = loss_module(name)
    keep = T(w != 0) if see else torch.ones(len(w), dtype=torch.bool, device=DEV)
    xs = base(name)["x"].detach()[keep].clone().requires_grad_(True)
    wt = T(w)
    avg = max(torch.sum(wt > 0).float().item(), 1.)
    out = crit(xs, T(lab)[keep], wt[keep], avg_factor=avg)
    losses = (out["loss_cls_classes"], out["loss_cls_objectness"]) if see else (out,)
    sum(losses).backward()
    grad = torch.zeros_like(base(name)["x"])
    grad[keep] = xs.grad
    assert avg == float(base(name)["avg"])
    check_against_reference(ref, name, dict(loss=torch.stack([l.detach() for l in losses]), grad=grad), " (host avg_factor path)")
    if see:
        assert torch.equal(crit.cum_samples, base(name)["cum"])


# ---------------------------------------------------------------------------------------- 5: determinism and reuse
@pytest.mark.parametrize("name", ["g257x80", "g65x1203b", "g3x5", "s257x80", "s65x2046", "s3x5"])
def test_two_calls_give_identical_bits(ref, name):
    a, b = run(name), run(name)                                      # (each on a fresh module: the same starting cum_samples)
    for k in KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], base(name)[k]), (name, k)


@pytest.mark.parametrize("name", ["g65x1203", "g257x80b", "s257x80"])
def test_backward_twice_and_an_upstream_factor(ref, name):
    from iif_amd.mmdet_bbox_head_loss import head_cls_loss
    x, lab, w = kc.inputs(name)
    xs = base(name)["x"].detach().clone().requires_grad_(True)
    out = head_cls_loss(loss_module(name), xs, T(lab), T(w))
    total = sum(v for k, v in out.items() if k.startswith("loss"))
    total.backward(retain_graph=True)
    g1 = xs.grad.clone()
    xs.grad = None
    total.backward()
    assert torch.equal(xs.grad, g1) and torch.equal(g1, base(name)["grad"])
    r3 = run(name, upstream=3.0)
    assert torch.equal(r3["loss"], base(name)["loss"])
    if xs.dtype == torch.float32:
        # one rounding of (3 lw / avg) u against two of 3 ((lw / avg) u): 2 ulp of the element
        assert float((r3["grad"] - 3.0 * g1).abs().max()) <= 4 * 2.0 ** -23 * float(g1.abs().max())
    else:
        assert float((r3["grad"].float() - 3.0 * g1.float()).abs().max()) <= 2.0 ** -7 * 3.0 * float(g1.float().abs().max())
    check_against_reference(ref, name, dict(loss=r3["loss"], grad=r3["grad"].double() / 3.0), " (upstream 3)")


def test_seesaw_backward_scales_each_loss_by_its_own_upstream(ref):
    from iif_amd.mmdet_bbox_head_loss import head_cls_loss
    name = "s257x80"
    x, lab, w = kc.inputs(name)
    C = kc.CASES[name]["C"]
    xs = T(x).requires_grad_(True)
    out = head_cls_loss(loss_module(name), xs, T(lab), T(w))
    (2.0 * out["loss_cls_classes"] + 0.5 * out["loss_cls_objectness"]).backward()
    g = base(name)["grad"]
    assert torch.equal(xs.grad[:, :C], 2.0 * g[:, :C]) and torch.equal(xs.grad[:, C:], 0.5 * g[:, C:])      # powers of two: exact
    xs.grad = None
    out2 = head_cls_loss(loss_module(name), xs, T(lab), T(w))
    out2["loss_cls_objectness"].backward()                           # the class loss unused: its columns get zeros
    assert not xs.grad[:, :C].any() and torch.equal(xs.grad[:, C:], g[:, C:])


def test_a_wider_pitch_is_read_in_place(ref):
    """ld > columns: a view into a wider buffer whose other columns hold NaN; the same bits as the dense case."""
    for name, pitch in (("g63x1203", 1208), ("g257x80", 83), ("g257x80b", 96), ("g65x1", 3), ("s257x80", 85), ("s63x1203", 1208)):
        x = base(name)["x"].detach()
        wide = torch.full((x.shape[0], pitch), float("nan"), dtype=x.dtype, device=DEV)
        wide[:, :x.shape[1]] = x
        r = run(name, scores=wide[:, :x.shape[1]])
        assert r["x"].stride(0) == pitch
        for k in KEYS:
            assert torch.equal(r[k], base(name)[k]), (name, k)


def test_an_empty_batch():
    from iif_amd.mmdet_bbox_head_loss import bbox_head_loss, head_cls_loss
    from iif_amd.mmdet_bbox_loss import L1Loss
    for name in ("g5x80", "s5x80"):
        K = kc.columns(name)
        xs = torch.zeros((0, K), device=DEV, requires_grad=True)
        lab, w = torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, device=DEV)
        crit = loss_module(name)
        out = head_cls_loss(crit, xs, lab, w)
        assert float(out["avg_factor"]) == 1.0
        for k, v in out.items():
            if k != "avg_factor":
                assert float(v.detach()) == 0.0, k
        sum(v for k, v in out.items() if k.startswith("loss")).backward()
        assert tuple(xs.grad.shape) == (0, K)
        if name[0] == "s":
            assert np.array_equal(crit.cum_samples.cpu().numpy(), kc.cum_before(name))
        # the reference adds no classification key for an empty cls_score (bbox_head.py:268)
        assert bbox_head_loss(crit, L1Loss(), xs, None, None, lab, w, None, None, kc.CASES[name]["C"]) == {}


def test_a_seesaw_label_outside_the_classes_contributes_nothing_and_is_reported(ref):
    from iif_amd import custom
    name = "s257x80"
    C = kc.CASES[name]["C"]
    x, lab, w = kc.inputs(name)
    try:
        custom.check_label_status()
    except IndexError:
        pass
    bad = lab.copy()
    rows = [0, 1]
    bad[rows] = [C + 1, -7]
    w2 = w.copy()
    w2[rows] = 1.0
    crit = loss_module(name)
    r = run(name, labels=T(bad), weights=T(w2), crit=crit)
    with pytest.raises(IndexError):
        custom.check_label_status()
    custom.check_label_status()                                      # reported once, then clean
    # the float64 restatement drops such rows from the losses and the histogram; they still count in avg_factor (weight > 0)
    rs = kc.restate_seesaw(x, bad, w2, kc.cum_before(name), C, kc.CASES[name]["p"], kc.CASES[name]["q"], kc.CASES[name]["lw"])
    assert float(r["avg"]) == rs["avg"] == float((w2 > 0).sum())
    assert np.array_equal(r["cum"].cpu().numpy(), rs["cum"]) and rs["cum"].sum() - kc.cum_before(name).sum() == float((w2 != 0).sum() - 2)
    loss_tol, grad_tol, gmax = bounds(ref, name)
    assert abs(float(r["loss"][0]) - rs["loss_cls"]) <= loss_tol[0] and abs(float(r["loss"][1]) - rs["loss_obj"]) <= loss_tol[1]
    assert float(np.abs(r["grad"].double().cpu().numpy() - rs["grad"]).max()) <= grad_tol
    assert not r["grad"][rows].any()
    # such a row is never a hit: the hits are those of the other rows, over the same avg_factor
    good = (w2 > 0) & (bad >= 0) & (bad <= C)
    acc_obj, acc_cls = sc.accuracy(x[good], bad[good], C)
    hits_obj = round(float(acc_obj) * int(good.sum()) / 100.0)
    assert float(r["acc"][1]) == float(np.float32(hits_obj) * np.float32(100.0 / rs["avg"])) and float(r["acc"][0]) == float(acc_cls)
    # in a row of weight zero the label is not read either
    w3 = w2.copy()
    w3[rows] = 0.0
    run(name, labels=T(bad), weights=T(w3))
    custom.check_label_status()


# ---------------------------------------------------------------------------------------- 6: no synchronisation
@pytest.mark.parametrize("kind", ["sigmoid", "seesaw"])
def test_nothing_synchronises_the_host(kind):
    """roi_stage_targets_padded -> a linear stand-in for the head -> bbox_head_loss -> backward(), two cascade rounds with
    refine_bboxes_padded in between, under torch's sync debug mode ('error'); mirrors
    test_bbox_head_loss_gpu.test_nothing_synchronises_the_host with the sigmoid CrossEntropyLoss (K columns) and with SeesawLoss
    (K + 2 columns)."""
    from iif_amd import custom
    from iif_amd.mmdet_bbox_head_loss import bbox_head_loss
    from iif_amd.mmdet_bbox_loss import SmoothL1Loss
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    from iif_amd.mmdet_roi_stage import refine_bboxes_padded, roi_stage_targets_padded
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    from . import assign_cases as ac
    from . import roi_stage_cases as rc
    from .test_roi_stage_gpu import parts
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    B, num, P, K = 2, 64, 40, rc.REFINE_CLASSES                 # fewer candidates than num: every image has padding rows
    cols = K if kind == "sigmoid" else K + 2
    shapes = [rc.IMG] * B
    props = torch.stack([T(ac.proposals(P, 9100 + b, rc.IMG[1], rc.IMG[0], 8, 120)) for b in range(B)])
    counts = torch.tensor([P, P - 15], dtype=torch.int64, device=DEV)
    gts = [T(ac.proposals(5, 9110 + b, rc.IMG[1], rc.IMG[0], 16, 160)) for b in range(B)]
    labs = [T(rc._u(5, 9120 + b, K)) for b in range(B)]
    stages = [parts(ac._with(rc.RCNN, pos=t, neg=t, min_pos=t), num, 0.25) for t in (0.5, 0.6)]
    coder = stages[0][2]
    gen = torch.Generator(device="cpu").manual_seed(7)
    heads = [(torch.randn(cols, 5, generator=gen).mul_(0.01).to(DEV).requires_grad_(True),
              torch.randn(4 * K, 5, generator=gen).mul_(0.001).to(DEV).requires_grad_(True)) for _ in range(2)]
    loss_bbox = SmoothL1Loss(beta=1.0)
    loss_cls = CrossEntropyLoss(use_sigmoid=True) if kind == "sigmoid" else SeesawLoss(num_classes=K, device=DEV)
    keys = {"loss_cls", "acc"} if kind == "sigmoid" else {"loss_cls_classes", "loss_cls_objectness", "acc_classes", "acc_objectness"}
    cums = []

    def rounds():
        out = []
        t = roi_stage_targets_padded(props, counts, gts, labs, *stages[0], K)
        for i in range(2):
            feat = t.rois / 100.0                                                # stands for the extractor and the shared layers
            cls_score, bbox_pred = feat @ heads[i][0].t(), feat @ heads[i][1].t()
            losses = bbox_head_loss(loss_cls, loss_bbox, cls_score, bbox_pred, t.rois, t.labels, t.label_weights, t.bbox_targets,
                                    t.bbox_weights, K)
            sum(v for k, v in losses.items() if k.startswith("loss")).backward()
            if kind == "seesaw":
                cums.append(loss_cls.cum_samples.clone())
            out.append((t, losses))
            if i == 0:
                labels = torch.where(t.labels < K, t.labels, torch.zeros_like(t.labels))          # stands for the argmax
                boxes, kept = refine_bboxes_padded(t.rois, labels, bbox_pred.detach(), t.pos_is_gt, t.counts, shapes, coder)
                t = roi_stage_targets_padded(boxes, kept, gts, labs, *stages[1], K)
        return out

    rounds()                                                                     # the library and the workspaces exist before the mode is on
    for h in heads:
        h[0].grad = h[1].grad = None
    del cums[:]
    if kind == "seesaw":
        loss_cls.cum_samples.zero_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = rounds()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    custom.check_label_status()
    cum = np.zeros(K + 1)
    for i, ((t, losses), h) in enumerate(zip(out, heads)):
        keep = t.label_weights > 0
        valid = int(keep.sum())
        assert 0 < valid < B * num                                               # there are padding rows, and they did not count
        assert set(losses) == keys | {"loss_bbox"}
        assert all(torch.isfinite(v).all().item() for v in losses.values())
        assert torch.isfinite(h[0].grad).all() and h[0].grad.abs().max() > 0 and torch.isfinite(h[1].grad).all()
        # the losses of the rows that count, by torch in float64, on the same scores
        z = ((t.rois / 100.0) @ h[0].detach().t())[keep].double()
        lab = t.labels[keep]
        if kind == "sigmoid":
            y = torch.nn.functional.one_hot(lab, K + 1)[:, :K].double()
            want = {"loss_cls": torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="sum") / valid}
            assert 0.0 <= float(losses["acc"]) <= 100.0
        else:
            cum += np.bincount(lab.cpu().numpy(), minlength=K + 1)
            assert np.array_equal(cums[i].cpu().numpy(), cum.astype(np.float32))  # the padding rows were not counted
            lc, lo, _ = sc.closed_form(z.cpu().numpy(), lab.cpu().numpy(), cum, K, avg_factor=float(valid))
            want = {"loss_cls_classes": lc, "loss_cls_objectness": lo}
        for k, v in want.items():
            assert abs(float(losses[k]) - float(v)) <= 1e-5 * float(v), (k, float(losses[k]), float(v))
        assert float(losses["loss_cls" if kind == "sigmoid" else "loss_cls_objectness"]) > 0
