"""FASA pieces on the IIF path against the CPU restatement in oracle.mmdet_iif."""
import pytest
import torch

from oracle import mmdet_iif as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _csv(tmp_path, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    table = torch.rand(c + 1, generator=g) * 4 + 0.5
    table[-1] = 1.0
    path = tmp_path / "idf.csv"
    with open(path, "w") as f:
        f.write("idx,raw\n0,1.0\n")
        for i in range(c):
            f.write("%d,%.9g\n" % (i + 1, table[i].item()))
    return str(path), table


def test_fasa_iif_loss_cums(tmp_path):
    from iif_amd.mmdet_fasa import FasaIIFLoss
    c, n = 40, 300
    path, table = _csv(tmp_path, c)
    crit = FasaIIFLoss(num_classes=c, path=path, variant="raw", loss_weight=1.5, use_cums=True)
    assert crit.reduction == "none" and crit.reduction_old == "mean"
    g = torch.Generator().manual_seed(3)
    ref_cl, ref_cn = torch.zeros(c + 1), torch.zeros(c + 1)
    for step in range(3):
        x = torch.randn(n, c + 1, generator=g) * 2
        y = torch.randint(0, c + 1, (n,), generator=g)
        w = (torch.rand(n, generator=g) > 0.2).float()
        xd = x.to(DEV).requires_grad_(True)
        loss = crit(xd, y.to(DEV), w.to(DEV), avg_factor=float(max(w.sum().item(), 1)))
        loss.backward()
        xr = x.clone().requires_grad_(True)
        rows = 1.5 * M.iif_cross_entropy(xr, y, table.unsqueeze(0), weight=w, reduction="none", avg_factor=None)
        ref = M.fasa_accumulate(rows.detach(), y, ref_cl, ref_cn)
        rows.mean().backward()
        assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
        assert (xd.grad.cpu() - xr.grad).abs().max().item() <= 1e-5 * xr.grad.abs().max().item()
    assert torch.equal(crit.cum_labels.cpu(), ref_cn)                      # counts are integers: exact
    assert (crit.cum_losses.cpu() - ref_cl).abs().max().item() <= 1e-4 * ref_cl.abs().max().item()
    crit.close_cums()
    assert crit.reduction == "mean" and crit.cum_labels.abs().sum().item() == 0
    out = crit(torch.randn(5, c + 1, device=DEV), torch.randint(0, c + 1, (5,), device=DEV))
    assert out.dim() == 0


def test_feature_bank_update_and_generate():
    from iif_amd.mmdet_fasa import FasaFeatureBank
    c, d = 50, 192
    counts = [max(int(2000 * (0.9 ** i)), 1) for i in range(c)]
    bank = FasaFeatureBank(c, d, counts, dict(decay_ratio=0.1, instance_prob_scale=200.0), device=DEV)
    g = torch.Generator().manual_seed(8)
    fm, fv, fu = torch.zeros(c, d), torch.zeros(c, d), torch.zeros(c)
    for step in range(3):
        n = 97
        emb = torch.randn(n, d, generator=g) * 1.5 + 0.3
        lab = torch.randint(0, 30, (n,), generator=g)             # classes 30.. never seen
        bank.fa_update(emb.to(DEV), lab.to(DEV))
        M.fasa_update(emb, lab, fm, fv, fu, 0.1)
    assert torch.equal(bank.feature_used.cpu(), fu)
    assert (bank.feature_mean.cpu() - fm).abs().max().item() <= 1e-5
    assert (bank.feature_std.cpu() - fv).abs().max().item() <= 1e-4 * fv.abs().max().item()
    rand = torch.rand(c, generator=g)
    normal = torch.randn(c, d, generator=g)
    e, l = bank.fa_generate(rand.to(DEV), normal.to(DEV))
    re, rl = M.fasa_generate(rand, bank.prob_list.cpu(), fu, fm, fv, normal)
    assert len(rl) > 0 and l.cpu().tolist() == rl.tolist()
    assert (e.cpu() - re).abs().max().item() <= 1e-4
    # nothing selected -> the reference's empty lists
    e2, l2 = bank.fa_generate(torch.ones(c, device=DEV) * 2, normal.to(DEV))
    assert e2 == [] and l2 == []


def test_dynamic_sampling_runs():
    from iif_amd.mmdet_fasa import FasaFeatureBank
    c, d = 12, 16

    class L:
        cum_labels = torch.ones(c + 1, device=DEV) * 10
        cum_losses = torch.arange(c + 1, device=DEV).float()
    bank = FasaFeatureBank(c, d, [100] * c, device=DEV)
    bank.feature_mean.data.copy_(torch.randn(c, d, generator=torch.Generator().manual_seed(1)))
    p0 = bank.prob_list.data.clone()
    bank.dynamic_sampling(L)                                          # first call: t0 := t1, no change
    assert torch.equal(bank.prob_list.data, p0) and len(bank.group_cluster_list) >= 1
    L.cum_losses = L.cum_losses * 2                                    # losses rose -> probabilities go down
    bank.dynamic_sampling(L)
    assert (bank.prob_list.data <= p0 + 1e-9).all() and (bank.prob_list.data < p0).any()


# ------------------------------------------------------------------ strided loops of the update / generate kernels, float64
U24 = 2.0 ** -24
F64 = torch.float64
FASA_C = 300                                             # the select scan crosses a 256-class chunk


def _fasa_labels(n, step):
    """Labels of one update: classes seen exactly once (variance 0), the background label C and a negative label (both
    ignored), the rest spread over classes on both sides of the 256-class chunk boundary.  Step 1 revisits part of step 0's
    classes (the moving-average branch) and brings new ones (the first-sight branch)."""
    g = torch.Generator().manual_seed(1000 * step + n)
    if n == 1:
        return torch.tensor([7])                            # first sight, then the moving average of the same class
    pool = torch.cat([torch.arange(0, 24), torch.arange(250, 262)]) + 12 * step
    lab = pool[torch.randint(0, len(pool), (n,), generator=g)]
    lab[0], lab[1] = FASA_C, -1
    for i, c in enumerate((100 + step, 255, 256 + step, 299 - step)):         # exactly once each
        lab[2 + i] = c
    return lab


def _fasa_update_reference(emb, lab, decay, state):
    """One fa_update in float64 on (mean, var, used) and their error bounds, in place.  Bounds: the kernel sums a class's rows
    in row order in fp32, so a sum gets max((n + 16) 2^-24 S, 4 |float32 CPU sum - float64|); the mean divides it by the
    count; the centred sum of squares gets the same form plus count * (mean bound)^2 (the first-order effect of the mean's
    error cancels: the deviations sum to zero); every other step is one rounding of its own terms (16 * 2^-24 of their
    magnitudes); the moving average carries the bound of the state it blends."""
    fm, fv, fu, bm, bv = state
    n = emb.shape[0]
    e32 = emb.float()
    for c in torch.unique(lab).tolist():
        if c < 0 or c >= FASA_C:
            continue
        idx = torch.nonzero(lab == c).squeeze(1)
        m = len(idx)
        e = emb[idx]
        ssum = e.sum(0)
        b_sum = torch.maximum((n + 16) * U24 * e.abs().sum(0), 4 * (e32[idx].sum(0).to(F64) - ssum).abs())
        mean = ssum / m
        b_mean = b_sum / m + 16 * U24 * mean.abs()
        t = e - mean
        ss = (t * t).sum(0)
        t32 = e32[idx] - (e32[idx].sum(0) / m)
        b_ss = torch.maximum((n + 16) * U24 * ss, 4 * ((t32 * t32).sum(0).to(F64) - ss).abs()) + m * b_mean ** 2
        var = ss / (m - 1) if m > 1 else ss / m
        b_var = b_ss / max(m - 1, 1) + 16 * U24 * var
        if fu[c] > 0:
            bm[c] = decay * b_mean + (1 - decay) * bm[c] + 16 * U24 * (decay * mean.abs() + (1 - decay) * fm[c].abs())
            bv[c] = decay * b_var + (1 - decay) * bv[c] + 16 * U24 * (decay * var + (1 - decay) * fv[c])
            fm[c] = decay * mean + (1 - decay) * fm[c]
            fv[c] = decay * var + (1 - decay) * fv[c]
        else:
            fm[c], fv[c], bm[c], bv[c] = mean, var, b_mean, b_var
            fu[c] += 1


@pytest.mark.parametrize("n", [1, 257, 600])
@pytest.mark.parametrize("d", [1, 255, 256, 257, 1024])
def test_feature_bank_strides_against_float64(d, n):
    """D below / at / above one pass of the 256 threads and the model's 1024; n below and above one pass of the label count;
    embeddings with leading dimension D + 3 (NaN in the padding).  Measured on the MI355X, worst over the 15 cases: mean
    |error| / bound 0.043 (4.6e-7 absolute), variance 0.018 (2.4e-6); classes seen once: variance exactly 0; generate within
    16 * 2^-24 of its two terms, labels exact."""
    from iif_amd.mmdet_fasa import FasaFeatureBank
    C = FASA_C
    bank = FasaFeatureBank(C, d, [100] * C, dict(decay_ratio=0.1), device=DEV)
    decay = float(torch.tensor(0.1, dtype=torch.float32))                   # the value the kernel is handed
    state = (torch.zeros(C, d, dtype=F64), torch.zeros(C, d, dtype=F64), torch.zeros(C, dtype=F64),
             torch.zeros(C, d, dtype=F64), torch.zeros(C, d, dtype=F64))
    once = set()
    for step in range(2):
        g = torch.Generator().manual_seed(7 * step + d)
        emb = torch.randn(n, d, generator=g) * 1.5 + 0.3
        lab = _fasa_labels(n, step)
        buf = torch.full((n, d + 3), float("nan"), device=DEV)
        buf[:, :d] = emb.to(DEV)
        view = buf[:, :d]
        assert view.stride(0) == d + 3
        bank.fa_update(view, lab.to(DEV))
        if step == 0:
            once = {c for c in torch.unique(lab).tolist() if 0 <= c < C and int((lab == c).sum()) == 1}
            torch.cuda.synchronize()
            assert len(once) >= 1 and (bank.feature_std.data.cpu()[sorted(once)] == 0).all()   # seen once: variance exactly 0
        _fasa_update_reference(emb.to(F64), lab, decay, state)
    fm, fv, fu, bm, bv = state
    assert torch.equal(bank.feature_used.data.cpu().to(F64), fu)
    assert 0 < fu.sum().item() < C or n == 1
    gm, gv = bank.feature_mean.data.cpu().to(F64), bank.feature_std.data.cpu().to(F64)
    em, ev = (gm - fm).abs(), (gv - fv).abs()
    print("\n  mean worst err/bound %.3f (err %.2e)  var worst err/bound %.3f (err %.2e)" %
          ((em / bm.clamp_min(1e-300)).max().item(), em.max().item(), (ev / bv.clamp_min(1e-300)).max().item(), ev.max().item()))
    assert (em <= bm).all() and (ev <= bv).all()           # bound 0 for classes never seen: untouched, exactly zero
    # ---- generate, from the state the bank holds
    normal = torch.randn(C, d, generator=torch.Generator().manual_seed(99))
    bank.prob_list.data.fill_(0.5)
    want_all = gm + gv.sqrt() * normal.to(F64)
    b_all = 16 * U24 * (gm.abs() + (gv.sqrt() * normal.to(F64)).abs())

    def generate(rand, expect):
        e, l = bank.fa_generate(rand.to(DEV), normal.to(DEV))
        if not expect:
            assert e == [] and l == []
            return
        assert l.dtype == torch.int64 and l.cpu().tolist() == expect          # exact, ascending
        assert e.shape == (len(expect), d)
        assert ((e.cpu().to(F64) - want_all[expect]).abs() <= b_all[expect]).all()

    used = [c for c in range(C) if fu[c] > 0]
    generate(torch.full((C,), 0.25), used)                                     # everything that was ever seen
    generate(torch.full((C,), 0.75), [])                                       # nothing
    generate(torch.full((C,), 0.5), [])                                        # rand == prob is not below it
    rand = torch.full((C,), 0.75)
    rand[250:262] = 0.25
    generate(rand, [c for c in used if 250 <= c < 262])                        # straddles the 256-class chunk
    bank.feature_used.data.fill_(1.0)                                          # every class: slots on both sides of the chunk
    generate(torch.full((C,), 0.25), list(range(C)))
    rand = torch.full((C,), 0.25)
    rand[::3] = 0.75
    generate(rand, [c for c in range(C) if c % 3])
