"""The RPN head's backward at the sampled pixels (csrc/rpn_head_sampled.hip, iif_amd/mmdet_rpn_head.py) on the MI355X.

  1. Against the reference's own runs (tests/golden/g39_rpn_head_sampled.npz): the maps equal the modules' own forward bit for
     bit; every gradient within max(4 x the float32 reference's own error against its float64 run on that case, 2^-24 x the
     largest element) of the float64 value; ``d feats`` exactly 0 wherever the float64 gradient is 0.
  2. Against dense torch autograd of the same modules in float64 (CPU), on hand-made samples: corners and edges, the 1x1 and 2x2
     levels, two anchors on one pixel, a fully sampled 3x3 block, an image with counts (0, 0), an empty batch, 1 .. 65 active
     slots, A in {1, 3, 9}, three channel pairs, both memory formats and a mix.  Bound per element, first order in u = 2^-24:
     (n + 5 A + 48) u T, where T is the sum of the absolute values of the element's terms (from a float64 autograd run on
     absolute values with the true ReLU mask) and n the length of the longest summation chain the element passes (active slots
     for the parameters, 9 Co for ``d feats``); 5 A covers the chain behind ``dh`` and 48 the 16 ulp allowed to ``rpn_loss``'s own
     gradients plus the roundings of the products.  T = 0 demands an exact zero.
  3. the same bits from call to call; 4. no synchronisation; 5. the hidden activation is not kept; 6. frozen parameters get no
     gradient and a weight that is not 16-byte aligned gives the aligned one's bits.
"""
import types

import numpy as np
import pytest
import torch

from . import rpn_head_cases as hc

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def T(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV, dtype=dtype)


def N_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ref(golden):
    g = golden("g39_rpn_head_sampled")
    hc.check_generator(g)
    return g


def generator(A=3):
    from iif_amd.mmdet_anchor import AnchorGenerator
    kw = dict(hc.GEN)
    if A == 1:
        kw["ratios"] = [1.0]
    elif A == 9:
        kw["scales"] = [2, 4, 8]
    gen = AnchorGenerator(**kw)
    assert gen.num_base_anchors == [A] * len(hc.STRIDES)
    return gen


def targets_of(pos, neg, counts, pos_bt, A, pos_weight=-1.0):
    """An ``RPNStageTargets`` around given lists (numpy, padded with -1)."""
    from iif_amd.mmdet_rpn_stage import RPNStageTargets
    grid, level_counts = generator(A)._grid(hc.FEATMAPS, "test")
    nts = sum(max(int(p), 1) + max(int(n), 1) for p, n in counts)
    return RPNStageTargets(T(pos, torch.int64), T(neg, torch.int64), T(counts, torch.int64), T(np.where(pos >= 0, 0, -1), torch.int64),
                           T(pos_bt, torch.float32), torch.tensor(float(nts), dtype=torch.float32, device=DEV), list(level_counts),
                           [tuple(f) for f in hc.FEATMAPS], grid, float(pos_weight))


def modules(params, dtype=torch.float32, device=DEV):
    w_conv, b_conv, w_cls, b_cls, w_reg, b_reg = params
    co, ci = w_conv.shape[:2]
    conv = torch.nn.Conv2d(ci, co, 3, padding=1)
    cls = torch.nn.Conv2d(co, w_cls.shape[0], 1)
    reg = torch.nn.Conv2d(co, w_reg.shape[0], 1)
    with torch.no_grad():
        for p, v in zip((conv.weight, conv.bias, cls.weight, cls.bias, reg.weight, reg.bias), params):
            p.copy_(torch.from_numpy(v.copy()))
    return tuple(m.to(device=device, dtype=dtype) for m in (conv, cls, reg))


def losses(kind):
    from iif_amd.mmdet_bbox_loss import L1Loss, SmoothL1Loss
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    return CrossEntropyLoss(use_sigmoid=True, loss_weight=1.0), (L1Loss() if kind == "l1" else SmoothL1Loss(beta=hc.BETA))


def as_format(x, fmt):
    return x.contiguous(memory_format=torch.channels_last if fmt == "cl" else torch.contiguous_format)


def run_sampled(t, feats, params, kind, pos_weight, formats):
    """Forward, ``rpn_loss``, backward on the sampled path: ``(loss [2, L], parameter gradients, d feats, maps)`` as numpy."""
    from iif_amd.mmdet_rpn_head import rpn_head_forward_sampled, rpn_sampled_pixels
    from iif_amd.mmdet_rpn_stage import rpn_loss
    conv, cls, reg = modules(params)
    xs = [as_format(T(x), f).requires_grad_(True) for x, f in zip(feats, formats)]
    sample = rpn_sampled_pixels(t)
    # torch's deterministic convolutions for both forwards: its default 1x1 channels_last convolution at 128 and more input
    # channels does not give the same bits twice, so "the modules' own forward" would not even equal itself
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        scores, deltas = rpn_head_forward_sampled(xs, conv, cls, reg, sample)
        with torch.no_grad():
            for x, s, d in zip(xs, scores, deltas):                         # the modules' own forward, bit for bit
                h = torch.relu(conv(x))
                assert torch.equal(s.view(torch.int32), cls(h).view(torch.int32)) and torch.equal(d.view(torch.int32), reg(h).view(torch.int32))
                assert s.stride() == cls(h).stride()
    ce, box = losses(kind)
    out = rpn_loss(scores, deltas, t, ce, box, pos_weight=pos_weight)
    (sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"])).backward()
    for x in xs:
        assert x.grad.shape == x.shape and x.grad.stride() == x.stride()    # the input's memory format
    val = np.array([[float(v.detach()) for v in out["loss_rpn_cls"]], [float(v.detach()) for v in out["loss_rpn_bbox"]]], dtype=np.float64)
    pg = [N_(p.grad) for p in (conv.weight, conv.bias, cls.weight, cls.bias, reg.weight, reg.bias)]
    return val, pg, [N_(x.grad) for x in xs], sample


# ------------------------------------------------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("fmt", ["nchw", "cl"])
@pytest.mark.parametrize("name", list(hc.CASES))
def test_gradients_against_the_reference(ref, name, fmt):
    c = hc.CASES[name]
    pre = name + "_"
    t = targets_of(ref[pre + "pos"].astype(np.int64), ref[pre + "neg"].astype(np.int64), ref[pre + "counts"], ref[pre + "pos_bt"], 3,
                   c["pos_weight"])
    assert float(t.num_total_samples) == float(ref[pre + "nts"])
    feats, params = hc.features(c["ci"], c["salt"]), hc.parameters(c["ci"], c["co"], 3, c["salt"])
    val, pg, dfeat, sample = run_sampled(t, feats, params, c["kind"], c["pos_weight"], [fmt] * len(feats))
    slots, owner = hc.sample_slots(ref[pre + "pos"].astype(np.int64), ref[pre + "neg"].astype(np.int64), ref[pre + "counts"], 3)
    assert np.array_equal(N_(sample.slots), slots) and np.array_equal(N_(sample.owner), owner)
    # the loss: rpn_loss's rule (its terms are non-negative: sum |term| / nts is the loss itself)
    l32, l64 = ref[pre + "loss32"].astype(np.float64), ref[pre + "loss64"]
    n_terms = int(ref[pre + "counts"].sum())
    assert (np.abs(val - l64) <= np.maximum(4 * np.abs(l32 - l64), (4 * n_terms + 16) * U * np.abs(l64))).all(), (val, l64)
    got = dict(zip(hc.PARAM_NAMES, pg))
    got["feat"] = np.concatenate([g.reshape(-1) for g in dfeat])
    worst = {}
    for key, g in got.items():
        fx = "dfeat" if key == "feat" else "d_" + key
        g32, g64 = ref[pre + fx + "32"].astype(np.float64), ref[pre + fx + "64"]
        assert g.shape == g64.shape, key
        bound = max(4.0 * float(np.abs(g32 - g64).max()), U * float(np.abs(g64).max()))
        err = float(np.abs(g.astype(np.float64) - g64).max())
        worst[key] = err / bound
        print("rpn_head %-10s %-4s d %-6s: max |g - g64| %.3g, bound %.3g (reference's own error %.3g)"
              % (name, fmt, key, err, bound, float(np.abs(g32 - g64).max())))
    assert not got["feat"][ref[pre + "dfeat64"] == 0].any()                 # exact zeros off the active pixels' neighbourhoods
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------ 2. float64 autograd
def flat_index(A, l, y, x, a):
    return int(hc.level_starts(A)[l]) + (y * hc.FEATMAPS[l][1] + x) * A + a


def lists_of(entries, A, nep, num, salt):
    """``entries[b]``: ``(level, y, x, a, is_pos)``.  Padded ascending lists, counts and hash targets in (-1, 1)."""
    Bn = len(entries)
    pos, neg = np.full((Bn, nep), -1, np.int64), np.full((Bn, num), -1, np.int64)
    counts = np.zeros((Bn, 2), np.int64)
    for b, es in enumerate(entries):
        p = sorted(flat_index(A, l, y, x, a) for l, y, x, a, is_pos in es if is_pos)
        n = sorted(flat_index(A, l, y, x, a) for l, y, x, a, is_pos in es if not is_pos)
        assert len(set(p + n)) == len(p) + len(n) and len(p) <= nep and len(n) <= num
        pos[b, :len(p)], neg[b, :len(n)], counts[b] = p, n, (len(p), len(n))
    bt = ((hc._u(Bn * nep * 4, salt, 1 << 12).astype(np.float32) / np.float32(1 << 11)) - np.float32(1)).reshape(Bn, nep, 4)
    bt[pos < 0] = 0
    return pos, neg, counts, bt


def spread(n, A, salt):
    """``n`` distinct pixels over both images and levels 0 to 2, every fourth a positive."""
    pix = [(b, l, y, x) for b in range(hc.B) for l in range(3) for y in range(hc.FEATMAPS[l][0]) for x in range(hc.FEATMAPS[l][1])]
    order = np.argsort(hc._u(len(pix), salt, 1 << 30), kind="stable")[:n]
    entries = [[] for _ in range(hc.B)]
    for k, i in enumerate(order):
        b, l, y, x = pix[i]
        entries[b].append((l, y, x, k % A, k % 4 == 0))
    return entries


def sample_entries(kind, A):
    H, W = hc.FEATMAPS[0]
    last = A - 1
    if kind == "borders":                                # each corner and each edge of level 0, the 2x2 and the 1x1 level
        e0 = [(0, 0, 0, 0, True), (0, 0, W - 1, last, False), (0, H - 1, 0, 0, False), (0, H - 1, W - 1, last, True),
              (0, 0, W // 2, 0, False), (0, H - 1, W // 2, last, True), (0, H // 2, 0, 0, True), (0, H // 2, W - 1, last, False),
              (3, 0, 0, 0, True), (3, 0, 1, last, False), (3, 1, 0, 0, False), (3, 1, 1, last, True), (4, 0, 0, 0, False)]
        e1 = [(1, 2, 3, 0, True), (2, 1, 2, last, False), (4, 0, 0, last, True)]
        return [e0, e1]
    if kind == "shared":                                 # two (three) sampled anchors on one pixel; its neighbour; the other image alone
        e0 = [(0, 5, 7, 0, True), (0, 5, 7, last, False), (0, 5, 8, 0, False), (1, 0, 0, 0, False), (1, 0, 0, last, True)]
        if A >= 3:
            e0.append((0, 5, 7, 1, False))
        return [e0, [(0, 5, 7, 0, False)]]
    if kind == "block3x3":                               # every d feats pixel of the block's middle has nine contributors
        e0 = [(1, y, x, (y + x) % A, (y + x) % 2 == 0) for y in (2, 3, 4) for x in (3, 4, 5)]
        return [e0, []]                                  # the second image: counts (0, 0)
    if kind == "none":
        return [[], []]
    raise KeyError(kind)


def reference64(feats, params, pos, neg, counts, bt, A, pos_weight, beta):
    """Dense float64 autograd on the CPU: the gradients, and per gradient element the sum of the absolute values of its terms."""
    import torch.nn.functional as Fn
    conv, cls, reg = modules(params, torch.float64, "cpu")
    xs = [torch.from_numpy(x.copy()).double().requires_grad_(True) for x in feats]
    pre = [conv(x) for x in xs]
    hs = [torch.relu(p) for p in pre]
    scores, deltas = [cls(h) for h in hs], [reg(h) for h in hs]
    for m in scores + deltas:
        m.retain_grad()
    Bn = feats[0].shape[0]
    s = torch.cat([m.permute(0, 2, 3, 1).reshape(Bn, -1) for m in scores], 1)
    d = torch.cat([m.permute(0, 2, 3, 1).reshape(Bn, -1, 4) for m in deltas], 1)
    nts = float(sum(max(int(p), 1) + max(int(n), 1) for p, n in counts))
    total = torch.zeros((), dtype=torch.float64)
    for b in range(Bn):
        p, n = torch.from_numpy(pos[b, :counts[b, 0]]), torch.from_numpy(neg[b, :counts[b, 1]])
        w = 1.0 if pos_weight <= 0 else pos_weight
        total = total + w * Fn.binary_cross_entropy_with_logits(s[b, p], torch.ones(p.numel(), dtype=torch.float64), reduction="sum")
        total = total + Fn.binary_cross_entropy_with_logits(s[b, n], torch.zeros(n.numel(), dtype=torch.float64), reduction="sum")
        diff = (d[b, p] - torch.from_numpy(bt[b, :counts[b, 0]]).double()).abs()
        if beta > 0:
            diff = torch.where(diff < beta, 0.5 * diff * diff / beta, diff - 0.5 * beta)
        total = total + diff.sum()
    (total / nts).backward()
    plist = (conv.weight, conv.bias, cls.weight, cls.bias, reg.weight, reg.bias)
    grads = [p.grad.numpy().copy() for p in plist] + [x.grad.numpy().copy() for x in xs]
    # the same network on absolute values with the true ReLU mask, fed the absolute map gradients
    aconv, acls, areg = modules([np.abs(v) for v in params], torch.float64, "cpu")
    axs = [torch.from_numpy(np.abs(x)).double().requires_grad_(True) for x in feats]
    ahs = [aconv(x) * (p.detach() > 0).double() for x, p in zip(axs, pre)]
    amaps = [acls(h) for h in ahs] + [areg(h) for h in ahs]
    aplist = (aconv.weight, aconv.bias, acls.weight, acls.bias, areg.weight, areg.bias)
    sums = torch.autograd.grad(amaps, list(aplist) + axs, grad_outputs=[m.grad.abs() for m in scores + deltas])
    return grads, [v.numpy() for v in sums]


SAMPLES = [
    # name, sample, A, (ci, co), formats, loss kind, pos_weight
    ("borders-a3", "borders", 3, (64, 64), "nchw", "l1", -1.0),
    ("borders-a1-cl", "borders", 1, (64, 64), "cl", "sl1", 2.0),
    ("borders-a9-mixed", "borders", 9, (64, 128), "mixed", "l1", -1.0),
    ("shared-mixed", "shared", 3, (64, 64), "mixed", "sl1", 2.0),
    ("shared-a9-256", "shared", 9, (256, 256), "cl", "l1", -1.0),
    ("block3x3-256", "block3x3", 3, (256, 256), "nchw", "l1", -1.0),
    ("block3x3-cl", "block3x3", 3, (64, 128), "cl", "sl1", -1.0),
    ("none", "none", 3, (64, 64), "nchw", "l1", -1.0),
] + [("active-%d" % n, n, 3, (64, 64), ("nchw", "cl", "mixed")[i % 3], "l1", -1.0) for i, n in enumerate((1, 31, 32, 33, 63, 64, 65))]


def formats_of(kind):
    L = len(hc.FEATMAPS)
    return [("nchw", "cl")[l % 2] for l in range(L)] if kind == "mixed" else [kind] * L


@pytest.mark.parametrize("case", SAMPLES, ids=[s[0] for s in SAMPLES])
def test_gradients_against_float64_autograd(case):
    name, what, A, (ci, co), fmt, kind, pos_weight = case
    salt = 9950 + 7 * SAMPLES.index(case)
    entries = spread(what, A, salt) if isinstance(what, int) else sample_entries(what, A)
    nep, num = 64, 128
    pos, neg, counts, bt = lists_of(entries, A, nep, num, salt + 1)
    feats, params = hc.features(ci, salt + 2), hc.parameters(ci, co, A, salt + 2)
    t = targets_of(pos, neg, counts, bt, A, pos_weight)
    val, pg, dfeat, sample = run_sampled(t, feats, params, kind, pos_weight, formats_of(fmt))
    slots, owner = hc.sample_slots(pos, neg, counts, A)
    assert np.array_equal(N_(sample.slots), slots) and np.array_equal(N_(sample.owner), owner)
    active = int((slots[:, 1] >= 0).sum())
    if isinstance(what, int):
        assert active == what
    if what == "shared":
        assert active < int(counts.sum())
    if what == "block3x3":
        assert counts[1].tolist() == [0, 0]
    grads, sums = reference64(feats, params, pos, neg, counts, bt, A, pos_weight, 0.0 if kind == "l1" else hc.BETA)
    chain = [active] * 6 + [9 * co] * len(feats)
    worst = 0.0
    for k, (g, g64, t_abs, n) in enumerate(zip(pg + dfeat, grads, sums, chain)):
        assert g.shape == g64.shape
        bound = (n + 5 * A + 48) * U * t_abs
        err = np.abs(g.astype(np.float64) - g64)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert not g[t_abs == 0].any(), k                                   # exact zeros where no term exists
        assert (err <= bound).all(), (name, k, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
    print("rpn_head %-18s: %3d active slots, worst error / bound %.3f" % (name, active, worst))
    if what == "none":
        assert active == 0 and all(not g.any() for g in pg + dfeat)
    else:
        assert all(np.abs(g).max() > 0 for g in pg)


# ------------------------------------------------------------------------------------------------------------ 3. the same bits
def test_two_calls_give_the_same_bits():
    A, ci, co = 3, 64, 128
    pos, neg, counts, bt = lists_of(spread(65, A, 9990), A, 64, 128, 9991)
    feats, params = hc.features(ci, 9992), hc.parameters(ci, co, A, 9992)
    t = targets_of(pos, neg, counts, bt, A)
    runs = [run_sampled(t, feats, params, "sl1", 2.0, formats_of("mixed")) for _ in range(2)]
    groups = [r[1] + [np.concatenate([g.reshape(-1) for g in r[2]])] for r in runs]
    assert len(groups[0]) == 7
    for a, b in zip(*groups):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------------------ 4. no synchronisation
def test_forward_train_backward_and_proposals_never_synchronise():
    from iif_amd import mmdet_nms
    from iif_amd.mmdet_assigner import MaxIoUAssigner
    from iif_amd.mmdet_rpn_head import rpn_head_forward_train
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    name = "boxes_l1"
    c = hc.CASES[name]
    gen = generator(3)
    p, n, min_pos, assign_all, _, _, mlq = hc.RUN
    asg = MaxIoUAssigner(p, n, min_pos_iou=min_pos, gt_max_assign_all=assign_all, match_low_quality=mlq)
    smp = RandomSampler(hc.NUM, hc.FRAC, neg_pos_ub=hc.UB, add_gt_as_proposals=False)
    coder = DeltaXYWHBBoxCoder(hc.MEANS, hc.STDS)
    ce, box = losses("sl1")
    head = modules(hc.parameters(c["ci"], c["co"], 3, c["salt"]))
    gts = [T(g) for g in hc.case_gts(name)]
    metas = [dict(pad_shape=hc.PAD_SHAPES[b], img_shape=hc.IMG_SHAPES[b]) for b in range(hc.B)]
    anchors = gen.grid_anchors(hc.FEATMAPS, device=DEV)
    cfg = types.SimpleNamespace(nms_pre=64, max_per_img=32, min_bbox_size=0, nms=dict(type="nms", iou_threshold=0.7))
    rpn_coder = types.SimpleNamespace(means=hc.MEANS, stds=hc.STDS, clip_border=True, add_ctr_clamp=False, ctr_clamp=32)

    def inputs():
        return [T(x).requires_grad_(True) for x in hc.features(c["ci"], c["salt"])]

    def step(xs):
        for m in head:
            m.zero_grad(set_to_none=True)
        out, scores, deltas = rpn_head_forward_train(head, gen, asg, smp, coder, ce, box, xs, gts, metas, allowed_border=0, pos_weight=2.0)
        assert sorted(out) == ["loss_rpn_bbox", "loss_rpn_cls"] and not scores[0].requires_grad and not deltas[0].requires_grad
        (sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"])).backward()
        return mmdet_nms.rpn_proposals_padded(scores, deltas, anchors, [s[:2] for s in hc.IMG_SHAPES], cfg, rpn_coder)

    step(inputs())                                       # once before the mode is on: the library loads, caches warm
    xs = inputs()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dets, counts = step(xs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(counts.sum()) > 0 and all(torch.isfinite(x.grad).all() for x in xs) and float(xs[0].grad.abs().sum()) > 0
    assert all(m.weight.grad is not None and m.bias.grad is not None and m.weight.grad.abs().sum() > 0 for m in head)


# ------------------------------------------------------------------------------------------------------------ 5. memory
def test_hidden_activation_is_not_kept():
    from iif_amd.mmdet_rpn_head import rpn_head_forward_sampled, rpn_sampled_pixels
    A, ci, co = 3, 64, 256
    pos, neg, counts, bt = lists_of(sample_entries("borders", A), A, 64, 128, 9995)
    t = targets_of(pos, neg, counts, bt, A)
    sample = rpn_sampled_pixels(t)
    conv, cls, reg = modules(hc.parameters(ci, co, A, 9996))
    xs = [T(x).requires_grad_(True) for x in hc.features(ci, 9996)]
    hidden = [4 * hc.B * co * H * W for H, W in hc.FEATMAPS]               # bytes of each level's hidden activation
    maps = sum(4 * hc.B * 5 * A * H * W for H, W in hc.FEATMAPS)

    def held(fn):
        fn()                                             # warm: workspaces, kernels
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated()
        del out
        return after - before

    sampled = held(lambda: rpn_head_forward_sampled(xs, conv, cls, reg, sample))

    def plain():
        hs = [torch.relu(conv(x)) for x in xs]
        return [cls(h) for h in hs], [reg(h) for h in hs]
    dense = held(plain)
    print("rpn_head forward keeps %d bytes (maps %d), the plain modules %d (hidden activations %d)" % (sampled, maps, dense, sum(hidden)))
    assert dense >= sum(hidden)                          # autograd keeps every level's hidden activation
    assert sampled < hidden[0]                           # nothing of the size of the (12, 16) level's is alive
    assert sampled <= maps + 512 * 2 * len(hc.FEATMAPS)  # the maps themselves, in the allocator's 512-byte blocks


# ------------------------------------------------------------------------------------------------------------ 6. frozen, misaligned
def test_frozen_parameters_and_a_misaligned_weight():
    """Parameters that require no gradient get none and ``d feats`` keeps its bits; an ``rpn_conv`` weight that is a view at an odd
    offset of a flat arena (not 16-byte aligned) gives the bits of the aligned one."""
    from iif_amd.mmdet_rpn_head import rpn_head_forward_sampled, rpn_sampled_pixels
    from iif_amd.mmdet_rpn_stage import rpn_loss
    A, ci, co = 3, 64, 64
    pos, neg, counts, bt = lists_of(sample_entries("shared", A), A, 64, 128, 9997)
    t = targets_of(pos, neg, counts, bt, A)
    sample = rpn_sampled_pixels(t)
    feats, params = hc.features(ci, 9998), hc.parameters(ci, co, A, 9998)
    ce, box = losses("l1")

    def run(frozen, misaligned):
        head = modules(params)
        if misaligned:
            w = head[0].weight
            arena = torch.zeros((w.numel() + 5,), dtype=torch.float32, device=DEV)
            view = arena[1:1 + w.numel()].view(w.shape)
            view.copy_(w.detach())
            head[0].weight.data = view
            assert head[0].weight.data_ptr() % 16 == 4
        for m in head:
            m.requires_grad_(not frozen)
        xs = [T(x).requires_grad_(True) for x in feats]
        with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            scores, deltas = rpn_head_forward_sampled(xs, *head, sample)
        out = rpn_loss(scores, deltas, t, ce, box)
        (sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"])).backward()
        return [x.grad for x in xs], [p.grad for m in head for p in (m.weight, m.bias)]

    base_x, base_p = run(False, False)
    frozen_x, frozen_p = run(True, False)
    assert all(g is None for g in frozen_p) and all(g is not None for g in base_p)
    odd_x, odd_p = run(False, True)
    for a, b, c in zip(base_x, frozen_x, odd_x):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    for a, c in zip(base_p, odd_p):
        assert torch.equal(a.view(torch.int32), c.contiguous().view(torch.int32))
