"""Host side of the size-selected streaming paths (tests/stream_cases.py): the float64 references against torch autograd, and an
inventory through the planning query iif_stream_plan - every case lies on the side of its threshold that its name says, the
cases cover every answer the query can give, and the ragged cases are ragged.  A later change of a threshold fails here instead
of silently emptying a GPU test.  No device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ce_cases
from tests import stream_cases as S

F64 = torch.float64


def test_torch_hash_is_the_case_files_hash():
    for n, salt in ((1, 0), (1000, 3), (4097, 117), (50000, 7001)):
        ref = ce_cases._hash(n, salt).view(np.int64)
        assert np.array_equal(S.hash_t(n, salt).numpy(), ref)


def test_input_generators_produce_the_exact_sets():
    h = S.hash_t(200000, 5)
    a = S.act(h, 9) * 64
    assert a.abs().max() == 255 and torch.equal(a, a.round()) and a.unique().numel() == 511
    ca = S.coef_a(h, 3) * 8
    assert torch.equal(ca, ca.round()) and ca.abs().min() == 1 and ca.abs().max() == 16 and ca.unique().numel() == 32
    cb = S.coef_b(h, 11) * 64
    assert torch.equal(cb, cb.round()) and cb.min() == -64 and cb.max() == 64
    p = S.coef_pow2(h, 20)
    assert sorted(p.abs().unique().tolist()) == [0.125, 0.25, 0.5, 1.0, 2.0] and (p < 0).any() and (p > 0).any()
    e = S.excite(h, 30) * 16
    assert torch.equal(e, e.round()) and e.min() == 1 and e.max() == 16
    # the storage types hold them exactly, and the coefficients that the entry derives are exact too
    assert torch.equal(S.rnd(S.act(h, 9), S.BF16).double(), S.act(h, 9))
    d = S.channel_coefs(512, 100, "cpu")
    g32, iv32 = d["gamma"].float(), d["stats"][1].float()
    assert torch.equal((g32 * iv32).double(), d["k1"])
    tot = d["total"].float()
    assert torch.equal((tot[0].double() / S.COUNT).float().double(), d["k2"])
    assert torch.equal(((tot[1].double() / S.COUNT).float() * iv32).double(), d["k3"])


def test_exact_arithmetic_needs_fewer_than_24_bits():
    """fp32 evaluation in another order / with other contractions = the float64 value, for every expression of the cases."""
    d = S.bn_inputs(4099, 48, 900, "cpu")
    x, r, gy, st, st2 = (d[k].float() for k in ("x", "r", "gy", "stats", "stats2"))
    y64, _ = S.bn_apply_ref(d["x"], d["stats"], False, d["r"], d["stats2"])
    assert torch.equal(((st[2] * x + st[3]) + (st2[2] * r + st2[3])).double(), y64)
    assert torch.equal((torch.addcmul(st[3], st[2], x) + torch.addcmul(st2[3], st2[2], r)).double(), y64)
    dx64, _ = S.bn_bwd_apply_ref(d["gy"], d["x"], None, d["k1"], d["k2"], d["k3"], d["stats"][0])
    k1, k2, k3 = (d[k].float() for k in ("k1", "k2", "k3"))
    assert torch.equal((k1 * (gy - k2 - (x - st[0]) * k3)).double(), dx64)
    assert torch.equal((k1 * ((gy - k2) - (x - st[0]) * k3)).double(), dx64)
    h = S.hash_t(7 * 48, 901).view(7, 48)
    e, o = S.excite(h, 0), S.coef_b(h, 8)
    x3, r3 = d["x"][:7 * 11].view(7, 11, 48), d["r"][:7 * 11].view(7, 11, 48)
    y64, _ = S.se_apply_ref(x3, d["stats"], e, r3, d["stats2"])
    got = (st[2] * x3.float() + st[3]) * e.float()[:, None, :] + (st2[2] * r3.float() + st2[3])
    assert torch.equal(got.clamp_min(0).double(), y64)
    assert torch.equal((x3.float() * e.float()[:, None, :] + o.float()[:, None, :]).double(), S.se_form_ref(x3, e, o))


# ------------------------------------------------------------------------------------------------ (a) references
def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("res", ["none", "plain", "normalised"])
@pytest.mark.parametrize("relu", [True, False])
def test_bn_references_against_autograd(res, relu):
    m, c, eps = 37, 12, 1e-5
    x = _rand(m, c, seed=1).requires_grad_(True)
    r = _rand(m, c, seed=2).requires_grad_(True)
    gamma, beta = (_rand(c, seed=3) + 2).requires_grad_(True), _rand(c, seed=4).requires_grad_(True)
    gamma2, beta2 = _rand(c, seed=5) + 2, _rand(c, seed=6)
    gy = _rand(m, c, seed=7)
    y = F.batch_norm(x, None, None, gamma, beta, True, 0.1, eps)
    if res == "plain":
        y = y + r
    if res == "normalised":
        y = y + F.batch_norm(r, None, None, gamma2, beta2, True, 0.1, eps)
    if relu:
        y = F.relu(y)
    y.backward(gy)

    def stats_of(t, g, b):
        mean, invstd = t.mean(0), 1.0 / (t.var(0, unbiased=False) + eps).sqrt()
        return torch.stack([mean, invstd, g * invstd, b - mean * g * invstd])
    st = stats_of(x.detach(), gamma.detach(), beta.detach())
    st2 = stats_of(r.detach(), gamma2, beta2)
    y_ref, mask = S.bn_apply_ref(x.detach(), st, relu, None if res == "none" else r.detach(), st2 if res == "normalised" else None)
    assert (y_ref - y.detach()).abs().max() <= 1e-12
    mk = mask if relu else None
    dx, dgamma, dbeta, _ = S.bn_backward_ref(gy, x.detach(), mk, gamma.detach(), st[0], st[1])
    assert (dx - x.grad).abs().max() <= 1e-12 and (dgamma - gamma.grad).abs().max() <= 1e-12
    assert (dbeta - beta.grad).abs().max() <= 1e-12
    # the normalisation pass from its three coefficients is the same backward
    d = torch.where(mk, gy, torch.zeros_like(gy)) if relu else gy
    k1, k2, k3 = gamma.detach() * st[1], d.sum(0) / m, (d * (x.detach() - st[0]) * st[1]).sum(0) / m * st[1]
    dx2, gm = S.bn_bwd_apply_ref(gy, x.detach(), mk, k1, k2, k3, st[0])
    assert (dx2 - x.grad).abs().max() <= 1e-12
    if res == "plain":
        assert (gm - r.grad).abs().max() <= 1e-12
    # and the bound of dx vanishes with the coefficient errors, up to the arithmetic term
    assert (S.dx_bound(dx, d, x.detach(), gamma.detach(), st[0], st[1], 0.0, 0.0, S.FP32) <= 1e-5 * (1 + dx.abs().max())).all()


def test_se_references_against_autograd():
    n, hw, c = 3, 10, 8
    x = _rand(n, hw, c, seed=1).requires_grad_(True)
    r = _rand(n, hw, c, seed=2)
    e = torch.rand(n, c, dtype=F64, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    st = _rand(4, c, seed=4)
    o = st[2] * x + st[3]
    y = F.relu(o * e[:, None, :] + r)
    gy = _rand(n, hw, c, seed=5)
    y_ref, mask = S.se_apply_ref(x.detach(), st, e.detach(), r)
    assert torch.equal(y_ref, y.detach())
    # gradient with respect to the BN output o, the excitation held fixed: g e (the offset row is the squeeze's share)
    (go,) = torch.autograd.grad(y, o, gy)
    gm = torch.where(mask, gy, torch.zeros_like(gy))
    assert (S.se_form_ref(gm, e.detach(), torch.zeros(n, c, dtype=F64)) - go).abs().max() <= 1e-12
    off = _rand(n, c, seed=6)
    assert torch.equal(S.se_form_ref(gm, e.detach(), off), go + off[:, None, :])


@pytest.mark.parametrize("k,stride,pad,shape", [(3, 2, 1, (2, 7, 9, 4)), (3, 1, 1, (1, 5, 6, 3)), (2, 2, 0, (2, 6, 8, 2))])
def test_maxpool_references_against_autograd(k, stride, pad, shape):
    x = _rand(*shape, seed=k).requires_grad_(True)                      # no ties
    y = F.max_pool2d(x.permute(0, 3, 1, 2), k, stride, pad).permute(0, 2, 3, 1)
    gy = _rand(*y.shape, seed=9)
    y.backward(gy)
    y_ref, code = S.maxpool_ref(x.detach(), k, stride, pad)
    assert torch.equal(y_ref, y.detach())
    assert torch.equal(S.gather_at_code(x.detach(), code, k, stride, pad), y_ref)
    assert (S.maxpool_scatter(gy, code, shape[1:3], k, stride, pad) - x.grad).abs().max() <= 1e-12
    # ties: the first maximum in scan order, as torch
    ones = torch.ones(1, 6, 6, 8, dtype=F64, requires_grad=True)
    F.max_pool2d(ones.permute(0, 3, 1, 2), 3, 2, 1).sum().backward()
    _, code = S.maxpool_ref(ones.detach(), 3, 2, 1)
    assert torch.equal(S.maxpool_scatter(torch.ones(1, 3, 3, 8, dtype=F64), code, (6, 6), 3, 2, 1), ones.grad)


def test_stem_pool_and_fused_backward_references_against_autograd():
    n, h, w, c, eps = 2, 7, 9, 4, 1e-5
    x = _rand(n, h, w, c, seed=1).requires_grad_(True)
    gamma, beta = (_rand(c, seed=2) + 2).requires_grad_(True), _rand(c, seed=3).requires_grad_(True)
    act = F.relu(F.batch_norm(x.permute(0, 3, 1, 2), None, None, gamma, beta, True, 0.1, eps))
    y = F.max_pool2d(act, 3, 2, 1).permute(0, 2, 3, 1)
    gp = _rand(*y.shape, seed=4)
    y.backward(gp)
    xd = x.detach().reshape(-1, c)
    mean, invstd = xd.mean(0), 1.0 / (xd.var(0, unbiased=False) + eps).sqrt()
    st = torch.stack([mean, invstd, gamma.detach() * invstd, beta.detach() - mean * gamma.detach() * invstd])
    y_ref, code, px = S.stem_pool_ref(x.detach(), st, torch.float64)
    assert (y_ref - y.detach()).abs().max() <= 1e-12
    assert ((st[2] * px + st[3]).clamp_min(0) - y_ref).abs().max() <= 1e-12
    dx, dgamma, dbeta, _ = S.pool_fused_ref(gp, code, x.detach(), st, gamma.detach(), None)
    assert (dx.view(n, h, w, c) - x.grad).abs().max() <= 1e-12
    assert (dgamma - gamma.grad).abs().max() <= 1e-12 and (dbeta - beta.grad).abs().max() <= 1e-12


def test_optimiser_and_layout_references_against_torch():
    g = torch.Generator().manual_seed(3)
    for nesterov in (False, True):
        p = torch.randn(101, dtype=F64, generator=g)
        q = p.clone().requires_grad_(True)
        opt = torch.optim.SGD([q], lr=0.1, momentum=0.9, weight_decay=1e-3, nesterov=nesterov)
        buf = torch.zeros_like(p)
        for _ in range(3):
            gr = torch.randn(101, dtype=F64, generator=g)
            q.grad = gr.clone()
            opt.step()
            S.sgd_ref(p, gr, buf, 0.1, 0.9, 1e-3, nesterov)
        assert (p - q.detach()).abs().max() <= 1e-13
    for momentum in (0.0, 0.9):
        for centered in (False, True):
            p = torch.randn(101, dtype=F64, generator=g)
            q = p.clone().requires_grad_(True)
            opt = torch.optim.RMSprop([q], lr=0.01, alpha=0.9, eps=0.0316, weight_decay=1e-3, momentum=momentum, centered=centered)
            sq, buf, ga = torch.zeros_like(p), torch.zeros_like(p) if momentum else None, torch.zeros_like(p) if centered else None
            for _ in range(3):
                gr = torch.randn(101, dtype=F64, generator=g)
                q.grad = gr.clone()
                opt.step()
                S.rmsprop_ref(p, gr, sq, buf, ga, 0.01, 0.9, 0.0316, 1e-3, momentum)
            assert (p - q.detach()).abs().max() <= 1e-13
    img = torch.randn(2, 3, 9, 11, dtype=F64, generator=g)
    wt = torch.randn(5, 3, 7, 7, dtype=F64, generator=g)
    cols = S.im2col_ref(img, 7, 7, 2, 3, 160)
    w2 = torch.zeros(5, 160, dtype=F64)
    w2[:, :147] = wt.permute(0, 2, 3, 1).reshape(5, 147)
    assert ((cols @ w2.t()).permute(0, 3, 1, 2) - F.conv2d(img, wt, None, 2, 3)).abs().max() <= 1e-12
    assert not cols[..., 147:].any()


# ------------------------------------------------------------------------------------------------ (b), (c) inventory
def test_bn_cases_sit_where_their_names_say_and_cover_the_query():
    seen_u, ragged = set(), set()
    for name, (m, c, u, rem, cvec) in S.BN_CASES.items():
        tv = S.bn_vectors(name)
        assert tv == m * (c // 8) == S.bn_shape(name, S.FP32)[0] * (S.bn_shape(name, S.FP32)[1] // 4)
        blocks, qu, nts, trips = S.plan("bn", tv)
        assert (qu, nts, trips) == (u, 0, 1), (name, qu, nts, trips)
        assert blocks == -(-tv // (256 * u))
        assert tv % (256 * u) == rem and c // 8 == cvec and (256 % cvec == 0) == (not name.endswith("_nf"))
        seen_u.add(qu)
        if rem % 256 != 0:                                   # (c) neither a whole trip nor whole 256-vector sub-trips
            ragged.add(qu)
        assert m * c * 2 <= 40e6                             # no tensor above about 40 MB
    assert seen_u == {1, 2, 4} and ragged == {1, 2, 4}
    for name in S.BN_TABLE:
        assert S.BN_CASES[name][3] % 256 != 0, name          # every case of the table is ragged
    # a tail inside the first sub-trip, in the second, and (U = 4) in the third: every `base + 256 u < total` outcome
    assert S.BN_CASES["u2_a"][3] < 256 < S.BN_CASES["u2_b"][3] < 512 < S.BN_CASES["u4_b"][3] < 768
    # each case lies within 1 024 vectors of its threshold, and the query changes its answer exactly there
    step = {2: 2 * 256 * 2048, 4: 4 * 256 * 2048}
    for name in ("u2_a", "u2_b", "u4_a", "u4_b", "u2_nf", "u4_nf"):
        u = S.BN_CASES[name][2]
        assert step[u] <= S.bn_vectors(name) < step[u] + 1024, name
        assert S.plan("bn", step[u] - 1)[1] == u // 2 and S.plan("bn", step[u])[1] == u
    assert step[2] - 256 < S.bn_vectors("u1_top") < step[2]
    assert S.plan("bn", S.bn_vectors("u1_top") + 64)[1] == 2


def test_grid_stride_cases_are_past_their_caps_and_ragged():
    trips_seen = set()
    for name, (family, work, cap) in S.grid_cases().items():
        blocks, u, nts, trips = S.plan(family, work)
        per = 1 if family == "stem_rows" else 256
        # (the option-A forward shares its tensor with the backward, whose cin items are the ones just past the cap)
        assert blocks * per == cap and trips == (3 if name == "shortcut_fwd" else 2), (name, blocks, trips)
        assert cap < work < cap + cap // 8 or name == "shortcut_fwd", (name, work)
        # ragged: the last block of the second trip is partly idle (the two shapes the issue fixes are whole blocks)
        assert work % 256 != 0 or name in ("se_stream", "avgpool_bwd", "stem_pool_rows"), (name, work)
        # one item fewer than the cap is a single trip of fewer blocks: the side the older tests are on
        b1, _, _, t1 = S.plan(family, cap - per)
        assert t1 == 1 and b1 == cap // per - 1
        trips_seen.update((t1, trips))
    assert trips_seen == {1, 2, 3}
    assert S.N_OPT % 4 == 3                                  # a three-element scalar tail behind the f32x4 body
    assert S.plan("grid", 1000)[3] == 1 and S.plan("grid", 10007 // 4 + 1)[3] == 1 and S.plan("rms", (2 ** 20 + 5) // 4 + 1)[3] == 1


def test_pool_fused_cases_cover_every_answer_of_the_query():
    answers = set()
    classes = set()
    for name, (n, h, w, c, dts, want, klass) in S.POOL_FUSED_CASES.items():
        cv = c // S.vec(S.DTYPES[dts])
        assert 256 % cv == 0 and 2 * c <= 256
        groups, rpb, remap, last = S.plan("pool_fused", n * h, w, cv)
        got = (remap, rpb > 8, last < rpb)
        assert got == want, (name, groups, rpb, remap, last)
        assert remap == (1 if groups % 8 == 0 else 0) and groups == -(-(n * h) // rpb) and 1 <= last <= rpb
        nvec_last = last * w * cv
        assert klass == ("lt256" if nvec_last < 256 else "mid" if nvec_last <= 512 else "long"), (name, nvec_last)
        answers.add(got)
        classes.add(klass)
        if name == "remap_on":
            assert groups >= 16
        if name == "wide_row":
            assert w * cv > 512
    assert {a[0] for a in answers} == {0, 1} and {a[1] for a in answers} == {False, True} and {a[2] for a in answers} == {False, True}
    assert classes == {"lt256", "mid", "long"}
    assert any(h % 2 and w % 2 for (_, h, w, _, _, _, _) in S.POOL_FUSED_CASES.values())
    assert any(c == 128 for (_, _, _, c, _, _, _) in S.POOL_FUSED_CASES.values())
    assert any(d == "f32" for (_, _, _, _, d, _, _) in S.POOL_FUSED_CASES.values())


def test_planning_query_rejects_bad_arguments():
    L = S._lib.lib()
    out = np.zeros(4, dtype=np.int32)
    assert L.iif_stream_plan(0, 100, 0, 0, None) == -1
    assert L.iif_stream_plan(0, 0, 0, 0, out.ctypes.data) == -1
    assert L.iif_stream_plan(9, 100, 0, 0, out.ctypes.data) == -1
    assert L.iif_stream_plan(5, 100, 0, 8, out.ctypes.data) == -1
