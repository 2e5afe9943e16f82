"""FasaBBoxHead.loss without a host read (csrc/fasa_head.hip, csrc/head_loss.hip, iif_amd/mmdet_fasa_head_loss.py) on the MI355X.

Tolerances (none comes from what the kernels give):
  * fa_update_rows against fa_update on the compacted rows, fa_generate_padded against fa_generate: BIT FOR BIT (one shared
    __device__ function per formula, -ffp-contract=off), labels and counts exact;
  * the bank against float64: the bounds of tests/test_mmdet_fasa_gpu.py's update reference (fasa_head_cases.fasa_update_reference);
  * a summed loss, and a class's accumulator over that class's rows: max(4 x |float32 reference - float64 reference|,
    (C + 16) 2^-24 sum|term|), test_bbox_head_loss_gpu.py's bound; counts, avg_factor and the accuracy exact;
  * the gradient: 4 x max(the float32 reference's largest error, 2^-24 of the largest element), as there.
Measured on the MI355X, worst over the cases (pytest -s prints each): open accumulators - loss 0.054 of its bound, a class's
accumulator 0.085, gradient 0.614; the sequence - losses 0.002, bank mean 0.008 and variance 0.012 of the update bounds.
"""
import functools

import numpy as np
import pytest
import torch

from . import fasa_head_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = fc.U24
F64 = torch.float64


def bank_of(c, d, cfg=None, counts=None):
    from iif_amd.mmdet_fasa import FasaFeatureBank
    return FasaFeatureBank(c, d, [100] * c if counts is None else counts, dict(decay_ratio=0.1) if cfg is None else cfg, device=DEV)


def state_of(bank):
    return bank.feature_mean.data.clone(), bank.feature_std.data.clone(), bank.feature_used.data.clone()


def same_state(a, b):
    """Bit equality (NaN-safe: compared as integers)."""
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def padded(emb, pitch_extra=3):
    """emb in a buffer with a wider pitch, NaN in the pitch padding."""
    n, d = emb.shape
    buf = torch.full((n, d + pitch_extra), float("nan"), device=DEV)
    buf[:, :d] = emb.to(DEV)
    view = buf[:, :d]
    assert n == 1 or view.stride(0) == d + pitch_extra
    return view


# ---------------------------------------------------------------------------------------- 1: the bank update
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
@pytest.mark.parametrize("d", [1, 255, 257, 1024])
def test_update_rows_equals_update_on_the_compacted_rows(d, n):
    """Two consecutive updates (first sight, then the moving average and new classes); classes seen exactly once, label C and
    label -1 among the rows; row pitch D + 3 with NaN in the pitch padding AND NaN in the whole embedding of every row that is
    not positive - fa_update gets the clean compacted rows, so equal bits also say that those rows were not read."""
    C = fc.FASA_C
    rows_bank, ref_bank = bank_of(C, d), bank_of(C, d)
    for step in range(2):
        emb = torch.randn(n, d, generator=torch.Generator().manual_seed(7 * step + d)) * 1.5 + 0.3
        lab = fc.fasa_labels(n, step)
        pos = (lab >= 0) & (lab < C)
        assert pos.any() and (n < 63 or (not pos[0] and not pos[1]))
        dirty = emb.clone()
        dirty[~pos] = float("nan")
        rows_bank.fa_update_rows(padded(dirty), lab.to(DEV))
        ref_bank.fa_update(padded(emb[pos]), lab[pos].to(DEV))
        assert same_state(state_of(rows_bank), state_of(ref_bank)), (d, n, step)
    fu = rows_bank.feature_used.data
    assert 0 < int(fu.sum()) < C and torch.isfinite(rows_bank.feature_mean.data).all() and torch.isfinite(rows_bank.feature_std.data).all()


def test_update_rows_without_a_positive_row_changes_nothing():
    C, d, n = fc.FASA_C, 257, 257
    bank = bank_of(C, d)
    g = torch.Generator().manual_seed(5)
    bank.fa_update_rows(torch.randn(n, d, generator=g).to(DEV), fc.fasa_labels(n, 0).to(DEV))
    before = state_of(bank)
    lab = torch.full((n,), C, dtype=torch.int64)
    lab[::3] = -1
    lab[1::7] = C + 5
    bank.fa_update_rows(torch.full((n, d), float("nan"), device=DEV), lab.to(DEV))
    assert same_state(state_of(bank), before) and int(before[2].sum()) > 0
    fresh = bank_of(C, d)
    fresh.fa_update_rows(torch.full((n, d), float("nan"), device=DEV), lab.to(DEV))
    assert not fresh.feature_used.data.any() and not fresh.feature_mean.data.any() and not fresh.feature_std.data.any()


@pytest.mark.parametrize("n", [1024, 1025, 2500])
def test_update_rows_every_row_of_one_class(n):
    """At, one above and far above the 1024 row indices a block keeps in LDS: the rest of the class is found by walking on."""
    C, d = fc.FASA_C, 257
    rows_bank, ref_bank = bank_of(C, d), bank_of(C, d)
    for step in range(2):
        emb = torch.randn(n, d, generator=torch.Generator().manual_seed(40 + step)) + 0.5
        lab = torch.full((n,), 257, dtype=torch.int64)
        rows_bank.fa_update_rows(padded(emb), lab.to(DEV))
        ref_bank.fa_update(padded(emb), lab.to(DEV))
        assert same_state(state_of(rows_bank), state_of(ref_bank)), (n, step)
    assert rows_bank.feature_used.data.nonzero().reshape(-1).tolist() == [257]
    # the class's rows spread thinly over many more rows: the listed rows end long before the last one
    lab = torch.full((n,), C, dtype=torch.int64)
    lab[::2] = 3
    emb = torch.randn(n, d, generator=torch.Generator().manual_seed(44))
    dirty = emb.clone()
    dirty[1::2] = float("nan")
    rows_bank.fa_update_rows(padded(dirty), lab.to(DEV))
    ref_bank.fa_update(padded(emb[::2]), lab[::2].to(DEV))
    assert same_state(state_of(rows_bank), state_of(ref_bank))


def test_update_rows_within_the_float64_bound():
    """The float64 reference and bounds of test_mmdet_fasa_gpu.py on one case, two updates."""
    C, d, n = fc.FASA_C, 255, 257
    bank = bank_of(C, d)
    decay = float(torch.tensor(0.1, dtype=torch.float32))
    state = tuple(torch.zeros(C, d, dtype=F64) if i != 2 else torch.zeros(C, dtype=F64) for i in range(5))
    for step in range(2):
        emb = torch.randn(n, d, generator=torch.Generator().manual_seed(7 * step + d)) * 1.5 + 0.3
        lab = fc.fasa_labels(n, step)
        bank.fa_update_rows(padded(emb), lab.to(DEV))
        fc.fasa_update_reference(emb.to(F64), lab, decay, state)
    fm, fv, fu, bm, bv = state
    assert torch.equal(bank.feature_used.data.cpu().to(F64), fu) and 0 < fu.sum().item() < C
    em = (bank.feature_mean.data.cpu().to(F64) - fm).abs()
    ev = (bank.feature_std.data.cpu().to(F64) - fv).abs()
    print("\n  mean worst err/bound %.3f  var worst err/bound %.3f" % ((em / bm.clamp_min(1e-300)).max().item(),
                                                                      (ev / bv.clamp_min(1e-300)).max().item()))
    assert (em <= bm).all() and (ev <= bv).all()


# ---------------------------------------------------------------------------------------- 2: virtual embeddings
@pytest.fixture(scope="module")
def gen_bank():
    C, d = fc.FASA_C, 257
    bank = bank_of(C, d, dict(decay_ratio=0.1, loss_aug_weight=0.3))
    g = torch.Generator().manual_seed(11)
    bank.feature_mean.data.copy_(torch.randn(C, d, generator=g))
    bank.feature_std.data.copy_(torch.rand(C, d, generator=g) * 2)
    bank.prob_list.data.fill_(0.5)
    return bank, torch.randn(C, d, generator=g).to(DEV)


def generate_both(bank, normal, rand, used, capacity=None):
    C, d = bank.num_classes, bank.feat_dim
    bank.feature_used.data.copy_(used.to(DEV))
    e, l = bank.fa_generate(rand.to(DEV), normal)
    pe, pl, pw, cnt = bank.fa_generate_padded(rand.to(DEV), normal, capacity)
    K = C if capacity is None else capacity
    assert pe.shape == (K, d) and pe.dtype == torch.float32 and pl.shape == (K,) and pl.dtype == torch.int64
    assert pw.shape == (K,) and pw.dtype == torch.float32 and cnt.dim() == 0 and cnt.dtype == torch.int32 and cnt.is_cuda
    total = len(l)
    k = min(total, K)
    assert int(cnt) == k and int(bank.aug_dropped) == total - k
    if k:
        assert torch.equal(pl[:k], l[:k]) and torch.equal(pe[:k].view(torch.int32), e[:k].view(torch.int32))
    assert (pw[:k] == torch.tensor(0.3, dtype=torch.float32)).all()
    assert not pe[k:].any() and (pl[k:] == C).all() and not pw[k:].any()
    return pl[:k].tolist()


def test_generate_padded_equals_generate(gen_bank):
    bank, normal = gen_bank
    C = bank.num_classes
    ones = torch.ones(C)
    assert generate_both(bank, normal, torch.full((C,), 0.25), ones) == list(range(C))              # everything selected
    assert generate_both(bank, normal, torch.full((C,), 0.75), ones) == []                           # nothing selected
    assert generate_both(bank, normal, torch.full((C,), 0.5), ones) == []                            # rand == prob is not below it
    assert generate_both(bank, normal, torch.full((C,), 0.25), torch.zeros(C)) == []                 # nothing in use
    rand = torch.full((C,), 0.75)
    rand[250:262] = 0.25
    used = ones.clone()
    used[255] = 0
    assert generate_both(bank, normal, rand, used) == [c for c in range(250, 262) if c != 255]       # straddles 256
    rand = torch.full((C,), 0.25)
    rand[::3] = 0.75
    want = [c for c in range(C) if c % 3]
    assert generate_both(bank, normal, rand, ones) == want
    # capacity below, at and above the number selected
    assert generate_both(bank, normal, rand, ones, capacity=37) == want[:37]
    assert generate_both(bank, normal, rand, ones, capacity=1) == want[:1]
    assert generate_both(bank, normal, rand, ones, capacity=len(want)) == want
    assert generate_both(bank, normal, rand, ones, capacity=len(want) + 70) == want
    assert generate_both(bank, normal, torch.full((C,), 0.75), ones, capacity=5) == []


def test_generate_padded_draws_its_own_numbers(gen_bank):
    bank, _ = gen_bank
    bank.feature_used.data.fill_(1.0)
    e, l, w, cnt = bank.fa_generate_padded()
    k = int(cnt)
    assert 0 < k < bank.num_classes and (l[:k] < bank.num_classes).all() and (l[1:k] > l[:k - 1]).all() and torch.isfinite(e).all()


# ---------------------------------------------------------------------------------------- 3: open accumulators
def cums_inputs(n, ch):
    g = torch.Generator().manual_seed(100 * n + ch)
    x = torch.randn(n, ch, generator=g) * 2
    lab = torch.randint(0, ch, (n,), generator=g)
    if n >= 4:
        lab[: n // 4] = ch - 1                               # background, many rows of one class
        lab[n // 4: n // 2] = lab[n // 4]                    # and of a second one
    boost = torch.rand(n, generator=g) < 0.5
    x[torch.arange(n)[boost], lab[boost]] += 9.0
    w = torch.tensor([1.0, 0.0, 0.5, 2.0, 1.0, 0.0, 1.0, 1.0])[torch.randint(0, 8, (n,), generator=g)]
    if n >= 4:
        w[0], w[n - 1], w[n // 4] = 1.0, 0.0, 1.0
    else:
        w[0] = 1.0
    tab = (8 + torch.randint(0, 64, (ch,), generator=g)).float() / 16.0
    tab[-1] = 1.0
    return x, lab, w, tab


def cums_module(ch, tab, loss_weight=1.5):
    from iif_amd.mmdet_fasa import FasaIIFLoss
    crit = FasaIIFLoss(path=fc.LVIS_CSV, num_classes=ch - 1, loss_weight=loss_weight, device=DEV)
    crit.iif_weights = tab.to(DEV).unsqueeze(0)
    crit.open_cums()
    return crit


def run_cums(n, ch, scores=None, weights=None):
    from iif_amd.mmdet_fasa_head_loss import head_cls_loss_cums
    x, lab, w, tab = cums_inputs(n, ch)
    crit = cums_module(ch, tab)
    xs = (x.to(DEV) if scores is None else scores).detach().requires_grad_(True)
    wt = (w if weights is None else weights).to(DEV)
    out = head_cls_loss_cums(crit, xs, lab.to(DEV), wt)
    assert set(out) == {"loss_cls", "acc_classes", "avg_factor", "rows"}
    assert out["loss_cls"].dim() == 0 and tuple(out["acc_classes"].shape) == (1,) and out["avg_factor"].dim() == 0
    out["loss_cls"].backward()
    return dict(loss=out["loss_cls"].detach(), acc=out["acc_classes"], avg=out["avg_factor"], rows=out["rows"], grad=xs.grad,
                cl=crit.cum_losses.clone(), cn=crit.cum_labels.clone(), crit=crit, out=out)


@functools.lru_cache(maxsize=None)
def cums_references(n, ch):
    x, lab, w, tab = cums_inputs(n, ch)
    return _cums_references(n, ch, x, lab, w, tab)


def _cums_references(n, ch, x, lab, w, tab):
    """(numpy float64 restatement, then per dtype the REFERENCE's formulation - oracle.mmdet_iif's iif_cross_entropy with reduction
    'none' and fasa_accumulate, on the rows with w != 0 - in float64 and in float32: dict(loss, cl, grad))."""
    r64 = fc.cums_restate(x.numpy(), tab.numpy(), lab.numpy(), w.numpy(), 1.5)
    live = w != 0
    refs = {}
    for dt in (torch.float64, torch.float32):
        xs = x.to(dt).requires_grad_(True)
        cl, cn = torch.zeros(ch, dtype=dt), torch.zeros(ch)
        loss = torch.zeros((), dtype=dt)
        if live.any():
            rows = 1.5 * fc.M.iif_cross_entropy(xs[live], lab[live], tab.unsqueeze(0), weight=w[live].to(dt), reduction="none")
            loss = fc.M.fasa_accumulate(rows.detach(), lab[live], cl, cn)
            rows.mean().backward()
        refs[dt] = dict(loss=float(loss), cl=cl.double().numpy(), grad=torch.zeros(n, ch, dtype=F64) if xs.grad is None else xs.grad.double())
        assert np.array_equal(cn.numpy(), r64["cum_labels"])
    assert abs(refs[torch.float64]["loss"] - r64["loss"]) <= 1e-12 * abs(r64["loss"])
    assert np.abs(refs[torch.float64]["cl"] - r64["cum_losses"]).max() <= 1e-12 * max(np.abs(r64["cum_losses"]).max(), 1e-300)
    return r64, refs[torch.float64], refs[torch.float32]


@pytest.mark.parametrize("n", [1, 4, 65, 257])
@pytest.mark.parametrize("ch", [5, 301, 1204])
def test_open_accumulators_against_float64(ch, n):
    r = run_cums(n, ch)
    r64, t64, t32 = cums_references(n, ch)
    x, lab, w, tab = cums_inputs(n, ch)
    tol = max(4.0 * abs(t32["loss"] - t64["loss"]), (ch + 16) * U24 * r64["sum_abs"])
    err = abs(float(r["loss"]) - r64["loss"])
    ctol = np.maximum(4.0 * np.abs(t32["cl"] - t64["cl"]), (ch + 16) * U24 * r64["cls_abs"])
    cerr = np.abs(r["cl"].double().cpu().numpy() - r64["cum_losses"])
    gmax = float(t64["grad"].abs().max())
    gtol = 4.0 * max(float((t32["grad"] - t64["grad"]).abs().max()), U24 * gmax)
    gerr = float((r["grad"].double().cpu() - t64["grad"]).abs().max())
    print("\n  %dx%d: loss %.3f of its bound, accumulators %.3f, gradient %.3f"
          % (n, ch, err / tol, float((cerr / np.maximum(ctol, 1e-300)).max()), gerr / gtol))
    assert err <= tol and (cerr <= ctol).all() and gerr <= gtol
    assert float(r["avg"]) == r64["avg"] == max(int((w != 0).sum()), 1)
    assert np.array_equal(r["acc"].cpu().numpy(), np.float32(r64["acc"]).reshape(1))
    assert np.array_equal(r["cn"].cpu().numpy(), r64["cum_labels"])
    assert not r["rows"][(w == 0).to(DEV)].any() and not r["grad"][(w == 0).to(DEV)].any()
    # the stored rows are the terms: one rounding chain of the row's own nll
    assert np.abs(r["rows"].double().cpu().numpy() - r64["rows"]).max() <= (ch + 16) * U24 * max(np.abs(r64["rows"]).max(), 1e-300)
    # a second call adds the same counts and the same sums
    from iif_amd.mmdet_fasa_head_loss import head_cls_loss_cums
    again = head_cls_loss_cums(r["crit"], x.to(DEV), lab.to(DEV), w.to(DEV))
    assert torch.equal(again["loss_cls"], r["loss"]) and torch.equal(again["rows"], r["rows"])
    assert torch.equal(r["crit"].cum_labels, 2 * r["cn"]) and torch.equal(r["crit"].cum_losses, 2 * r["cl"])      # s + s is exact


@pytest.mark.parametrize("n,ch", [(65, 1204), (257, 5)])
def test_open_accumulators_do_not_read_rows_of_weight_zero(n, ch):
    x, lab, w, tab = cums_inputs(n, ch)
    base = run_cums(n, ch)
    xs = x.clone()
    xs[w == 0] = float("nan")
    r = run_cums(n, ch, scores=xs.to(DEV))
    for k in ("loss", "acc", "avg", "rows", "grad", "cl", "cn"):
        assert torch.equal(r[k], base[k]), k
    assert torch.isfinite(r["grad"]).all() and (w == 0).sum() > 0


def test_open_accumulators_with_every_weight_zero():
    n, ch = 65, 301
    r = run_cums(n, ch, scores=torch.full((n, ch), float("nan"), device=DEV), weights=torch.zeros(n))
    assert float(r["loss"]) == 0.0 and float(r["avg"]) == 1.0 and float(r["acc"]) == 0.0
    assert not r["cl"].any() and not r["cn"].any() and not r["grad"].any() and not r["rows"].any()


def test_closed_accumulators_and_other_criteria_take_their_own_paths():
    """fasa_cls_loss: closed -> head_cls_loss (bit-equal to it); the sigmoid mode -> the module's own forward, as the reference."""
    from iif_amd.mmdet_bbox_head_loss import head_cls_loss
    from iif_amd.mmdet_fasa import FasaIIFLoss
    from iif_amd.mmdet_fasa_head_loss import fasa_cls_loss
    n, ch = 65, 301
    x, lab, w, tab = cums_inputs(n, ch)
    crit = cums_module(ch, tab)
    crit.close_cums()
    a = fasa_cls_loss(crit, x.to(DEV), lab.to(DEV), w.to(DEV))
    b = head_cls_loss(crit, x.to(DEV), lab.to(DEV), w.to(DEV))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) and not crit.cum_labels.any()
    sig = FasaIIFLoss(use_sigmoid=True, path=fc.LVIS_CSV, num_classes=ch - 1, device=DEV)
    sig.iif_weights = tab.to(DEV).unsqueeze(0)                # (read only by the softmax criterion)
    out = fasa_cls_loss(sig, x.to(DEV), lab.to(DEV), w.to(DEV))
    avg = max(float((w > 0).sum()), 1.0)
    want = sig(x.to(DEV), lab.to(DEV), w.to(DEV), avg_factor=avg)
    assert out["avg_factor"] == avg and abs(float(out["loss_cls"]) - float(want)) <= 1e-6 * abs(float(want))
    soft = head_cls_loss(sig, x.to(DEV), lab.to(DEV), w.to(DEV))["loss_cls"]              # what taking it for an IIFLoss gives
    assert abs(float(soft) - float(want)) > 1e-3 * abs(float(want))


# ---------------------------------------------------------------------------------------- 4: the assembly against the reference
@pytest.fixture(scope="module")
def sequence(golden):
    """The fixture's sequence on the device, once: per call the losses (values and gradients), the bank state, the virtual rows."""
    from iif_amd.mmdet_bbox_loss import L1Loss
    from iif_amd.mmdet_fasa import FasaIIFLoss
    from iif_amd.mmdet_fasa_head_loss import fasa_bbox_head_loss
    g = golden("g37_fasa_head")
    rand, aug_labels, aug_normals = fc.fixture_draws(g)
    bank = bank_of(fc.C, fc.D, dict(fc.CFG), fc.instance_counts())
    assert float((bank.prob_list.data.cpu() - fc.prob_list()).abs().max()) <= 1e-6 * float(fc.prob_list().max())
    bank.prob_list.data.copy_(fc.prob_list().to(DEV))         # the reference's own float32 values: no draw sits on a rounding
    bank.epoch = fc.EPOCH
    crit = FasaIIFLoss(path=fc.LVIS_CSV, num_classes=fc.C, loss_weight=fc.CLS_LOSS_WEIGHT, device=DEV)
    reg = L1Loss(loss_weight=fc.BBOX_LOSS_WEIGHT)
    lin = torch.nn.Linear(fc.D, fc.C1).to(DEV)
    w, b = fc.fc_cls_params()
    with torch.no_grad():
        lin.weight.copy_(w.to(DEV))
        lin.bias.copy_(b.to(DEV))
    out = {}

    def call(step, training):
        i = {k: v.to(DEV) for k, v in fc.step_inputs(step).items()}
        xs, bp = i["cls_score"].requires_grad_(True), i["bbox_pred"].requires_grad_(True)
        kw = {}
        if training:
            kw = dict(rand=torch.from_numpy(rand[step]).to(DEV), normal=fc.normals_full(aug_labels[step], aug_normals[step]).to(DEV))
        losses = fasa_bbox_head_loss(bank, crit, reg, lin, xs, bp, None, i["labels"], i["label_weights"], i["bbox_targets"],
                                     i["bbox_weights"], i["embedding"] if training else None, fc.C, training=training,
                                     reg_class_agnostic=True, **kw)
        (losses["loss_cls"] + losses["loss_bbox"]).backward()
        return {k: v.detach() for k, v in losses.items()}, xs.grad, bp.grad, kw

    for step in range(fc.STEPS):
        losses, gx, gb, kw = call(step, True)
        pe, pl, pw, cnt = bank.fa_generate_padded(kw["rand"], kw["normal"])           # the same draws again: the rows the loss saw
        out[step] = dict(losses=losses, gx=gx, gb=gb, state=state_of(bank), aug=(pe, pl, pw, int(cnt)), lin_grad=lin.weight.grad.clone())
        lin.weight.grad = None
    crit.open_cums()
    losses, gx, gb, _ = call(fc.STEPS, False)
    out["val"] = dict(losses=losses, gx=gx, state=state_of(bank), cl=crit.cum_losses.clone(), cn=crit.cum_labels.clone())
    return g, out


def summed_loss_ok(got, g, key, terms):
    l32, l64 = float(g[key + "32"]), float(g[key + "64"])
    tol = max(4.0 * abs(l32 - l64), (terms + 16) * U24 * abs(l64))                     # every term is >= 0: sum|term| is the loss
    err = abs(float(got) - l64)
    print("  %s: error %.3g = %.3f of its bound" % (key, err, err / tol if tol else 0.0))
    return err <= tol


def test_sequence_losses_match_the_reference(sequence):
    g, out = sequence
    for step in range(fc.STEPS):
        losses = out[step]["losses"]
        assert set(losses) == {"loss_bbox", "loss_cls", "acc_classes"}
        assert summed_loss_ok(losses["loss_cls"], g, "s%d_loss_cls" % step, fc.C1)
        i = fc.step_inputs(step)
        assert summed_loss_ok(losses["loss_bbox"], g, "s%d_loss_bbox" % step, 4 * int(((i["labels"] >= 0) & (i["labels"] < fc.C)).sum()))
        assert np.array_equal(losses["acc_classes"].cpu().numpy(), g["s%d_acc_valid" % step])
        assert not out[step]["gx"][fc.PAD_FROM:].any() and torch.isfinite(out[step]["gx"]).all()      # padding rows: zero gradient
        pos = (i["labels"] >= 0) & (i["labels"] < fc.C)
        assert not out[step]["gb"][~pos.to(DEV)].any() and bool(out[step]["gb"].any()) == bool(pos.any())
        assert out[step]["lin_grad"].abs().max() > 0                                   # the virtual rows train fc_cls
    assert float(out[1]["losses"]["loss_bbox"]) == 0.0                                 # the step without a positive row
    losses = out["val"]["losses"]
    assert set(losses) == {"loss_bbox", "loss_cls", "acc_classes"}
    assert summed_loss_ok(losses["loss_cls"], g, "val_loss_cls", fc.C1)
    lab = fc.step_inputs(fc.STEPS)["labels"]
    assert summed_loss_ok(losses["loss_bbox"], g, "val_loss_bbox", 4 * int(((lab >= 0) & (lab < fc.C)).sum()))
    assert np.array_equal(losses["acc_classes"].cpu().numpy(), g["val_acc_valid"])
    assert np.array_equal(losses["acc_classes"].cpu().numpy(), g["val_acc_classes"])  # no padding: the reference's own figure


def test_sequence_bank_state_and_virtual_rows(sequence):
    g, out = sequence
    decay = float(torch.tensor(fc.CFG["decay_ratio"], dtype=torch.float32))           # the value the kernel is handed
    new = lambda: tuple(torch.zeros(fc.C, fc.D, dtype=F64) if i != 2 else torch.zeros(fc.C, dtype=F64) for i in range(5))      # noqa: E731
    state, ref_state = new(), new()
    for step in range(fc.STEPS):
        i = fc.step_inputs(step)
        fc.fasa_update_reference(i["embedding"].to(F64), i["labels"], decay, state, num_classes=fc.C)
        fc.fasa_update_reference(i["embedding"].to(F64), i["labels"], fc.CFG["decay_ratio"], ref_state, num_classes=fc.C)
        fm, fv, fu, bm, bv = state
        used = torch.from_numpy(g["s%d_used" % step])
        gm, gv, gu = (t.cpu() for t in out[step]["state"])
        assert torch.equal(gu.nonzero().reshape(-1), used) and torch.equal(fu.nonzero().reshape(-1), used)
        # the float64 reference with the bounds IS the reference's own float64 run when handed its decay, the double 0.1 ...
        r64m, r64v = torch.from_numpy(g["s%d_mean64" % step]), torch.from_numpy(g["s%d_var64" % step])
        assert (ref_state[0][used] - r64m).abs().max() <= 1e-12 * r64m.abs().max()
        assert (ref_state[1][used] - r64v).abs().max() <= 1e-12 * r64v.abs().max()
        # ... and the kernel is handed float32(0.1), as fa_update's is (test_mmdet_fasa_gpu.py): the same reference with that value
        em, ev = (gm.to(F64) - fm).abs(), (gv.to(F64) - fv).abs()
        print("  step %d: mean worst err/bound %.3f  var worst err/bound %.3f"
              % (step, (em / bm.clamp_min(1e-300)).max().item(), (ev / bv.clamp_min(1e-300)).max().item()))
        assert (em <= bm).all() and (ev <= bv).all()
        rest = torch.ones(fc.C, dtype=torch.bool)
        rest[used] = False
        assert not gm[rest].any() and not gv[rest].any()
        # the virtual rows, from the recorded draws: the reference's classes exactly, its float64 rows within the bank's bound
        pe, pl, pw, cnt = out[step]["aug"]
        drawn = torch.from_numpy(g["s%d_aug_labels" % step])
        assert cnt == len(drawn) and torch.equal(pl[:cnt].cpu(), drawn) and (pl[cnt:] == fc.C).all() and not pe[cnt:].any()
        assert (pw[:cnt] == torch.tensor(fc.CFG["loss_aug_weight"], dtype=torch.float32)).all() and not pw[cnt:].any()
        nrm = torch.from_numpy(g["s%d_aug_normals" % step]).to(F64)
        m, v, dm, dv = fm[drawn], fv[drawn], bm[drawn], bv[drawn]
        want = m + v.sqrt() * nrm
        tol = 16 * U24 * (m.abs() + (v.sqrt() * nrm).abs()) + dm + nrm.abs() * ((v + dv).sqrt() - (v - dv).clamp_min(0).sqrt())
        assert ((pe[:cnt].cpu().to(F64) - want).abs() <= tol).all()
    assert same_state(out["val"]["state"], out[fc.STEPS - 1]["state"])                 # validation leaves the bank alone


def test_sequence_accumulators(sequence):
    g, out = sequence
    i = fc.step_inputs(fc.STEPS)
    a = (i["cls_score"].numpy(), fc.table().numpy().reshape(-1), i["labels"].numpy(), i["label_weights"].numpy(), fc.CLS_LOSS_WEIGHT)
    r64 = fc.cums_restate(*a)
    assert np.abs(r64["cum_losses"] - g["val_cum_losses64"]).max() <= 1e-12 * np.abs(g["val_cum_losses64"]).max()
    assert np.array_equal(out["val"]["cn"].cpu().numpy(), g["val_cum_labels"])
    tol = np.maximum(4.0 * np.abs(g["val_cum_losses32"].astype(np.float64) - g["val_cum_losses64"]), (fc.C1 + 16) * U24 * r64["cls_abs"])
    # against the restatement, which the line above ties to the reference's float64 run: that run's log(sum exp) - z_l rounds a
    # confident single-row class (1e-17) to 0, the restatement's log1p form does not
    err = np.abs(out["val"]["cl"].double().cpu().numpy() - r64["cum_losses"])
    print("\n  accumulators: worst %.3f of its bound" % float((err / np.maximum(tol, 1e-300)).max()))
    assert (err <= tol).all() and (out["val"]["cl"].cpu().numpy()[g["val_cum_labels"] == 0] == 0).all()


# ---------------------------------------------------------------------------------------- 5: no synchronisation
def test_nothing_synchronises_the_host():
    """roi_stage_targets_padded -> a linear stand-in for the head -> fasa_bbox_head_loss -> backward(): one training step at
    epoch 1 (bank update, fresh draws, virtual rows) and one validation call with open accumulators, under torch's sync debug
    mode ('error')."""
    from iif_amd import custom
    from iif_amd.mmdet_bbox_loss import SmoothL1Loss
    from iif_amd.mmdet_fasa import FasaIIFLoss
    from iif_amd.mmdet_fasa_head_loss import fasa_bbox_head_loss
    from iif_amd.mmdet_roi_stage import roi_stage_targets_padded
    from . import assign_cases as ac
    from . import roi_stage_cases as rc
    from .test_roi_stage_gpu import parts
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    B, num, P, K, D = 2, 64, 40, rc.REFINE_CLASSES, 5           # fewer candidates than num: every image has padding rows
    props = torch.stack([torch.from_numpy(np.array(ac.proposals(P, 9100 + b, rc.IMG[1], rc.IMG[0], 8, 120))).to(DEV) for b in range(B)])
    counts = torch.tensor([P, P - 15], dtype=torch.int64, device=DEV)
    gts = [torch.from_numpy(np.array(ac.proposals(5, 9110 + b, rc.IMG[1], rc.IMG[0], 16, 160))).to(DEV) for b in range(B)]
    labs = [torch.from_numpy(np.array(rc._u(5, 9120 + b, K))).to(DEV) for b in range(B)]
    stage = parts(ac._with(rc.RCNN, pos=0.5, neg=0.5, min_pos=0.5), num, 0.25)
    gen = torch.Generator(device="cpu").manual_seed(7)
    w_cls = torch.randn(K + 1, D, generator=gen).mul_(0.01).to(DEV).requires_grad_(True)
    w_reg = torch.randn(4 * K, D, generator=gen).mul_(0.001).to(DEV).requires_grad_(True)
    crit = FasaIIFLoss(path=fc.LVIS_CSV, num_classes=K, device=DEV)
    crit.iif_weights = torch.ones(1, K + 1, device=DEV)
    val_crit = FasaIIFLoss(path=fc.LVIS_CSV, num_classes=K, device=DEV)
    val_crit.iif_weights = torch.ones(1, K + 1, device=DEV)
    val_crit.open_cums()
    reg = SmoothL1Loss(beta=1.0)
    bank = bank_of(K, D)
    bank.prob_list.data.fill_(0.5)
    fc_cls = lambda e: e @ w_cls.t()                                              # noqa: E731

    def step(training):
        t = roi_stage_targets_padded(props, counts, gts, labs, *stage, K)
        feat = t.rois / 100.0                                                     # stands for the extractor and the shared layers
        cls_score, bbox_pred = feat @ w_cls.t(), feat @ w_reg.t()
        losses = fasa_bbox_head_loss(bank, crit if training else val_crit, reg, fc_cls, cls_score, bbox_pred, t.rois, t.labels,
                                     t.label_weights, t.bbox_targets, t.bbox_weights, feat if training else None, K,
                                     training=training, epoch=1)
        (losses["loss_cls"] + losses["loss_bbox"]).backward()
        return t, losses

    step(True), step(False)                                                       # the library and the workspaces exist before the mode is on
    w_cls.grad = w_reg.grad = None
    val_crit.cum_losses.zero_(), val_crit.cum_labels.zero_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        (t, train), (tv, val) = step(True), step(False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    custom.check_label_status()
    valid = int((tv.label_weights > 0).sum())
    assert 0 < valid < B * num and 0 < int((t.label_weights > 0).sum()) < B * num  # there are padding rows
    for losses in (train, val):
        assert set(losses) == {"loss_cls", "acc_classes", "loss_bbox"}
        assert all(torch.isfinite(v).all().item() for v in losses.values()) and float(losses["loss_cls"]) > 0
    assert torch.isfinite(w_cls.grad).all() and w_cls.grad.abs().max() > 0 and torch.isfinite(w_reg.grad).all()
    pos = (t.labels >= 0) & (t.labels < K)
    assert pos.any() and (bank.feature_used.data[torch.unique(t.labels[pos])] == 1).all()
    assert float(val_crit.cum_labels.sum()) == valid                              # padding rows are in no accumulator
    keep = tv.label_weights > 0
    want = torch.nn.functional.cross_entropy(((tv.rois / 100.0) @ w_cls.detach().t())[keep].double(), tv.labels[keep])
    assert abs(float(val["loss_cls"]) - float(want)) <= 1e-5 * float(want)
