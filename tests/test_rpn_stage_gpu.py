"""The RPN head's training side (csrc/rpn_stage.hip, iif_amd/mmdet_anchor.py, iif_amd/mmdet_rpn_stage.py) on the MI355X.

  1. ``grid_anchors`` / ``grid_priors`` / ``valid_flags`` against the reference's own runs (tests/golden/g34_rpn_stage.npz), bits;
  2. ``rpn_stage_targets`` / ``rpn_stage_dense`` against the fixture: integers, weights, ``dx, dy`` exactly, ``dw, dh`` within twice
     the float32 reference's own error against the float64 continuation (test_roi_stage_gpu.py's rule);
  3. against the per-image chain on the device, bit for bit (``log`` columns included);
  4. ``rpn_loss``: each per-level value within max(4 x the float32 reference's own error, (T + 16) 2^-24 sum |term|) of the
     fixture's float64 value (T the level's non-zero terms: the first-order summation bound plus slack for exp / log1p);
     gradients exactly zero where nothing was sampled and within 16 float32 ulp of the float64 value elsewhere;
  5. sparse reads; 6. the dense losses on ``rpn_stage_dense``; 7. the same bits from call to call; 8. no synchronisation.
"""
import types

import numpy as np
import pytest
import torch

from . import assign_cases as ac
from . import rpn_stage_cases as rc
from . import targets_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


def T(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV, dtype=dtype)


def N_(t):
    return t.detach().cpu().numpy()


def raw(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def ref(golden):
    g = golden("g34_rpn_stage")
    rc.check_generator(g)
    return g


@pytest.fixture(scope="module")
def ulps(golden):
    return golden("g26_targets")["coder_ref_ulps"]


def parts(run=rc.RUN, num=rc.NUM, frac=rc.FRAC, ub=rc.UB, means=rc.MEANS, stds=rc.STDS):
    from iif_amd.mmdet_assigner import MaxIoUAssigner
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler
    pos, neg, min_pos, assign_all, _, _, mlq = run
    return (MaxIoUAssigner(pos, neg, min_pos_iou=min_pos, gt_max_assign_all=assign_all, match_low_quality=mlq),
            RandomSampler(num, frac, neg_pos_ub=ub, add_gt_as_proposals=False), DeltaXYWHBBoxCoder(means, stds))


def fpn_generator():
    from iif_amd.mmdet_anchor import AnchorGenerator
    return AnchorGenerator(**rc.GEN_CASES[rc.FPN][0])


_runs = {}


def case_run(ref, name):
    """The fixture case on the device, once: ``(targets, keys [B, A] numpy)``."""
    if name not in _runs:
        from iif_amd.mmdet_rpn_stage import rpn_stage_targets
        c = rc.CASES[name]
        _, _, flat = rc.fpn_anchors()
        gts = rc.case_gts(name)
        keys = []
        for b in range(2):
            inside = rc.fpn_inside(b, c["border"])
            gi = rc.targets_np(flat, inside, gts[b], np.zeros(flat.shape[0], np.int32), rc.run_of(name))[4]
            keys.append(rc.fixture_keys(ref, name, b, gi, inside))
        keys = np.stack(keys)
        asg, smp, coder = parts(rc.run_of(name))
        t = rpn_stage_targets(rc.FEATMAPS, fpn_generator(), rc.PAD_SHAPES, rc.IMG_SHAPES, [T(g) for g in gts], asg, smp, coder,
                              allowed_border=c["border"], pos_weight=c["pos_weight"], keys=T(keys))
        _runs[name] = (t, keys)
    return _runs[name]


# ------------------------------------------------------------------------------------------------------------ 1. the generator
@pytest.mark.parametrize("name", list(rc.GEN_CASES))
def test_generator_equals_the_reference_bit_for_bit(ref, name):
    from iif_amd.mmdet_anchor import AnchorGenerator
    kw, featmaps = rc.GEN_CASES[name]
    gen = AnchorGenerator(**kw)
    want = ref["gen_%s_anchors" % name]
    sizes = [h * w * n for (h, w), n in zip(featmaps, gen.num_base_anchors)]
    for fn in (gen.grid_anchors, gen.grid_priors):
        out = fn(featmaps, device=DEV)
        assert [o.shape for o in out] == [(s, 4) for s in sizes] and all(o.dtype == torch.float32 for o in out)
        assert np.array_equal(rc.bits(N_(torch.cat(out))), rc.bits(want))
    for k, pad in enumerate(rc.GEN_PAD_SHAPES):
        out = gen.valid_flags(featmaps, pad, device=DEV)
        assert [o.shape for o in out] == [(s,) for s in sizes] and all(o.dtype == torch.bool for o in out)
        assert np.array_equal(np.packbits(N_(torch.cat(out))), ref["gen_%s_flags%d" % (name, k)]), pad


# ------------------------------------------------------------------------------------------------------------ 2. the fixture
@pytest.mark.parametrize("name", list(rc.CASES))
def test_targets_equal_the_reference(ref, ulps, name):
    from iif_amd.mmdet_rpn_stage import rpn_stage_dense
    t, _ = case_run(ref, name)
    pre = "t_%s_" % name
    counts = ref[pre + "counts"]
    assert t.pos_inds.dtype == torch.int64 and tuple(t.pos_inds.shape) == (2, rc.NEP) and tuple(t.neg_inds.shape) == (2, rc.NUM)
    assert np.array_equal(N_(t.counts), counts) and t.counts.dtype == torch.int64
    assert np.array_equal(N_(t.pos_inds), ref[pre + "pos"]) and np.array_equal(N_(t.neg_inds), ref[pre + "neg"])
    assert np.array_equal(N_(t.pos_assigned_gt_inds), ref[pre + "pos_gt"])
    assert t.num_total_samples.dtype == torch.float32 and float(t.num_total_samples) == float(ref[pre + "nts"])
    assert t.num_level_anchors == [a.shape[0] for a in rc.fpn_anchors()[1]] and t.featmap_sizes == [tuple(f) for f in rc.FEATMAPS]
    got, want = N_(t.pos_bbox_targets), ref[pre + "pos_bt"]
    assert np.array_equal(rc.bits(got[..., :2]), rc.bits(want[..., :2]))
    _, _, flat = rc.fpn_anchors()
    gts = rc.case_gts(name)
    per_image = []
    for b in range(2):
        kp, kn = counts[b]
        assert not got[b, kp:].any()
        pos = ref[pre + "pos"][b, :kp].astype(np.int64)
        if kp:
            exact, kinds, err = tc.encode_check(got[b, :kp], flat[pos], gts[b][ref[pre + "pos_gt"][b, :kp]], rc.MEANS, rc.STDS)
            assert exact and kinds and err <= 2 * ulps[0], (b, err)
        per_image.append((pos, ref[pre + "neg"][b, :kn].astype(np.int64), want[b, :kp]))
    dense = rpn_stage_dense(t, num_classes=1)
    want_dense = rc.dense_np(t.num_level_anchors, per_image, rc.CASES[name]["pos_weight"])
    mine_dense = rc.dense_np(t.num_level_anchors, [(p, n, got[b, :p.size]) for b, (p, n, _) in enumerate(per_image)],
                             rc.CASES[name]["pos_weight"])
    for f, (outs, wants, mines) in enumerate(zip(dense, want_dense, mine_dense)):
        for l, (o, w, m) in enumerate(zip(outs, wants, mines)):
            o = N_(o)
            assert o.shape == w.shape and o.dtype == w.dtype, (f, l)
            if f == 2:                                  # targets: dx, dy exactly; dw, dh are pos_bbox_targets' (checked above)
                assert np.array_equal(rc.bits(o[..., :2]), rc.bits(w[..., :2])) and np.array_equal(rc.bits(o), rc.bits(m)), l
            else:
                assert np.array_equal(o, w), (f, l)


# ------------------------------------------------------------------------------------------------------------ 3. the chain
def row_generator(valid):
    """One level, one base anchor (8 x 8, stride 4), a row of ``valid + 3`` cells of which ``valid`` are valid for the pad shape."""
    from iif_amd.mmdet_anchor import AnchorGenerator
    return AnchorGenerator([4], [1.0], [2]), [(1, valid + 3)], (4, 4 * valid, 3)


def row_gts(G, valid, salt):
    if G == 0:
        return np.zeros((0, 4), dtype=np.float32)
    x1 = rc._u(G, salt, 4 * (valid + 3) * 4).astype(np.float32) / np.float32(4) - np.float32(6)
    y1 = rc._u(G, salt + 1, 24).astype(np.float32) / np.float32(2) - np.float32(8)
    w = rc._u(G, salt + 2, 40).astype(np.float32) / np.float32(4) + np.float32(4)
    h = rc._u(G, salt + 3, 40).astype(np.float32) / np.float32(4) + np.float32(4)
    g = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)
    g[0] = (np.float32(4 * (valid - 1)) - 2, -4, np.float32(4 * (valid - 1)) + 2, 4)          # half of the last valid anchor
    return g


def assert_equals_chain(t, gen, featmaps, pad_shapes, img_shapes, gts, asg, smp, coder, keys, border):
    from iif_amd.mmdet_targets import anchor_inside_flags
    B, nep, num = len(gts), int(smp.num * smp.pos_fraction), int(smp.num)
    flat = torch.cat(gen.grid_anchors(featmaps, device=DEV))
    total = 0
    for b in range(B):
        valid = torch.cat(gen.valid_flags(featmaps, pad_shapes[b], device=DEV))
        inside = anchor_inside_flags(flat, valid, img_shapes[b][:2], border)
        sel = inside.nonzero().flatten()
        if sel.numel() == 0:
            kp = kn = 0
        else:
            a = flat[inside]
            ar = asg.assign(a, gts[b], None, None)
            p = smp.sample_padded(ar, a, gts[b], keys=keys[b][inside].contiguous())
            kp, kn = p.counts.tolist()
            pos_c = p.pos_inds[:kp]
            assert torch.equal(t.pos_inds[b, :kp], sel[pos_c]) and torch.equal(t.neg_inds[b, :kn], sel[p.neg_inds[:kn]]), b
            gi = ar.gt_inds[pos_c] - 1
            assert torch.equal(t.pos_assigned_gt_inds[b, :kp], gi), b
            if kp:
                enc = coder.encode(a[pos_c], gts[b][gi])
                assert torch.equal(raw(t.pos_bbox_targets[b, :kp]), raw(enc)), b
        assert t.counts[b].tolist() == [kp, kn], b
        assert (t.pos_inds[b, kp:] == -1).all() and (t.neg_inds[b, kn:] == -1).all() and (t.pos_assigned_gt_inds[b, kp:] == -1).all()
        assert not t.pos_bbox_targets[b, kp:].any()
        total += max(kp, 1) + max(kn, 1)
    assert float(t.num_total_samples) == float(total)


@pytest.mark.parametrize("G", [0, 1, 7, 257])
@pytest.mark.parametrize("valid", [1, 255, 256, 257, 4097])
def test_rows_equal_the_chain_bit_for_bit(valid, G):
    from iif_amd.mmdet_rpn_stage import rpn_stage_targets
    gen, featmaps, pad = row_generator(valid)
    gts = [T(row_gts(G, valid, 9700 + valid + G))]
    A = valid + 3
    for i, (assign_all, num) in enumerate(((True, 64), (False, 16))):
        asg, smp, coder = parts(ac._with(rc.RUN, assign_all=assign_all), num=num, means=tc.MEANS[1], stds=tc.STDS[1])
        keys = T(tc.free_keys(A, 9800 + valid + G + i)).reshape(1, A)
        t = rpn_stage_targets(featmaps, gen, [pad], [pad], gts, asg, smp, coder, allowed_border=-1, keys=keys)
        assert_equals_chain(t, gen, featmaps, [pad], [pad], gts, asg, smp, coder, keys, -1)


def test_row_with_every_key_in_one_bin_equals_the_chain():
    """tc.one_bin_keys on a row of A = 4100 anchors: two sweep tiles of the select, every candidate a boundary candidate, tied keys."""
    from iif_amd.mmdet_rpn_stage import rpn_stage_targets
    valid = tc.ONE_BIN_N - 3
    gen, featmaps, pad = row_generator(valid)
    gts = [T(row_gts(257, valid, 9650))]
    keys = T(tc.one_bin_keys()).reshape(1, tc.ONE_BIN_N)
    for num, frac, ub in tc.ONE_BIN_BUDGETS:
        asg, smp, coder = parts(num=num, frac=frac, ub=ub, means=tc.MEANS[1], stds=tc.STDS[1])
        t = rpn_stage_targets(featmaps, gen, [pad], [pad], gts, asg, smp, coder, allowed_border=-1, keys=keys)
        assert_equals_chain(t, gen, featmaps, [pad], [pad], gts, asg, smp, coder, keys, -1)


@pytest.mark.parametrize("border", [-1, 0])
def test_three_images_and_equal_keys_equal_the_chain(border):
    from iif_amd.mmdet_rpn_stage import rpn_stage_targets
    gen = fpn_generator()
    pads = [(96, 128, 3), (64, 96, 3), (33, 50, 3)]
    imgs = [(90, 121, 3), (60, 93, 3), (30, 47, 3)]
    gts = [T(rc.gt_boxes("crowd", 0)), T(rc.gt_boxes("edge", 1)), T(rc.gt_boxes("few", 1)[2:])]
    A = sum(a.shape[0] for a in rc.fpn_anchors()[1])
    asg, smp, coder = parts(num=64)
    for keys in (T(np.stack([tc.free_keys(A, 9900 + b) for b in range(3)])), torch.full((3, A), 12345, dtype=torch.int32, device=DEV)):
        t = rpn_stage_targets(rc.FEATMAPS, gen, pads, imgs, gts, asg, smp, coder, allowed_border=border, keys=keys)
        assert_equals_chain(t, gen, rc.FEATMAPS, pads, imgs, gts, asg, smp, coder, keys, border)
    assert int(t.counts[0, 0]) == 32                    # the crowded image fills its budget, equal keys: the lowest indices


def test_image_without_valid_anchor_has_zero_counts():
    from iif_amd.mmdet_rpn_stage import rpn_stage_targets
    gen = fpn_generator()
    asg, smp, coder = parts()
    gts = [T(rc.gt_boxes("few", 0)), T(rc.gt_boxes("few", 0))]
    t = rpn_stage_targets(rc.FEATMAPS, gen, [(96, 128, 3), (64, 96, 3)], [(90, 121, 3), (8, 8, 3)], gts, asg, smp, coder, allowed_border=0)
    assert t.counts[1].tolist() == [0, 0] and int(t.counts[0].sum()) == rc.NUM
    assert float(t.num_total_samples) == float(max(int(t.counts[0, 0]), 1) + max(int(t.counts[0, 1]), 1) + 2)


# ------------------------------------------------------------------------------------------------------------ 4. the loss
def losses(kind):
    from iif_amd.mmdet_bbox_loss import L1Loss, SmoothL1Loss
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    return CrossEntropyLoss(use_sigmoid=True, loss_weight=1.0), (L1Loss() if kind == "l1" else SmoothL1Loss(beta=rc.BETA))


def run_loss(t, scores, deltas, kind, pos_weight, channels_last):
    from iif_amd.mmdet_rpn_stage import rpn_loss
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    s = [T(x).contiguous(memory_format=fmt).requires_grad_(True) for x in scores]
    d = [T(x).contiguous(memory_format=fmt).requires_grad_(True) for x in deltas]
    ce, reg = losses(kind)
    out = rpn_loss(s, d, t, ce, reg, pos_weight=pos_weight)
    assert sorted(out) == ["loss_rpn_bbox", "loss_rpn_cls"] and len(out["loss_rpn_cls"]) == len(scores)
    (sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"])).backward()
    for x in s + d:
        assert x.grad.shape == x.shape and x.grad.stride() == x.stride()                     # the input's memory format
    val = np.array([[float(v.detach()) for v in out["loss_rpn_cls"]], [float(v.detach()) for v in out["loss_rpn_bbox"]]], dtype=np.float32)
    return val, [N_(x.grad) for x in s], [N_(x.grad) for x in d]


def loss_bounds(ref, name, kind):
    """Per level [2, L]: max(4 x |loss32 - loss64| of the reference, (T + 16) 2^-24 sum |term|)."""
    counts = ref["t_%s_counts" % name]
    per_image = [(ref["t_%s_pos" % name][b, :counts[b, 0]].astype(np.int64), ref["t_%s_neg" % name][b, :counts[b, 1]].astype(np.int64),
                  ref["t_%s_pos_bt" % name][b, :counts[b, 0]]) for b in range(2)]
    scores, deltas = rc.maps(name)
    level_counts = [a.shape[0] for a in rc.fpn_anchors()[1]]
    cls, box, nts = rc.loss_terms_np(scores, deltas, per_image, level_counts, rc.CASES[name]["pos_weight"], 0.0 if kind == "l1" else rc.BETA)
    l32, l64 = ref["l_%s_%s_loss32" % (name, kind)].astype(np.float64), ref["l_%s_%s_loss64" % (name, kind)]
    summ = np.array([[(np.count_nonzero(t) + 16) * EPS * np.abs(t).sum() / nts for t in grp] for grp in (cls, box)])
    return np.maximum(4 * np.abs(l32 - l64), summ), np.abs(l32 - l64), summ


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("kind", ["l1", "sl1"])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_loss_and_gradients_against_float64(ref, name, kind, channels_last):
    t, _ = case_run(ref, name)
    scores, deltas = rc.maps(name)
    pw = rc.CASES[name]["pos_weight"]
    val, gs, gd = run_loss(t, scores, deltas, kind, pw, channels_last)
    l64 = ref["l_%s_%s_loss64" % (name, kind)]
    bound, ref_err, summ = loss_bounds(ref, name, kind)
    err = np.abs(val.astype(np.float64) - l64)
    print("rpn_loss %-9s %-3s %s: max |v - v64| / bound %.3f (reference's own error / bound %.3f)"
          % (name, kind, "NHWC" if channels_last else "NCHW", float((err / np.maximum(bound, 1e-300)).max()),
             float((ref_err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), (err, bound)
    fs, fd = rc.flat_maps(gs, gd)
    entry = np.concatenate([ref["t_%s_pos" % name], ref["t_%s_neg" % name]], axis=1).astype(np.int64)
    counts = ref["t_%s_counts" % name]
    g64c, g64b = ref["l_%s_%s_gcls64" % (name, kind)], ref["l_%s_%s_gbox64" % (name, kind)]
    worst = 0.0
    for b in range(2):
        live = entry[b] >= 0
        pos = entry[b, :counts[b, 0]]
        for got, want in ((fs[b, entry[b, live]], g64c[b, live]), (fd[b, pos], g64b[b, :counts[b, 0]])):
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            e = np.abs(got.astype(np.float64) - want) / ulp
            worst = max(worst, float(e.max(initial=0.0)))
        rest_s, rest_d = fs[b].copy(), fd[b].copy()
        rest_s[entry[b, live]] = 0
        rest_d[pos] = 0
        assert not rest_s.any() and not rest_d.any()                                         # exactly zero where nothing was sampled
    print("rpn_loss %-9s %-3s %s: gradients within %.2f float32 ulp of float64" % (name, kind, "NHWC" if channels_last else "NCHW", worst))
    assert worst <= 16


# ------------------------------------------------------------------------------------------------------------ 5. sparse reads
@pytest.mark.parametrize("channels_last", [False, True])
def test_unsampled_positions_are_never_read(ref, channels_last):
    name = "crowded"
    t, _ = case_run(ref, name)
    scores, deltas = rc.maps(name)
    clean = run_loss(t, scores, deltas, "sl1", 2.0, channels_last)
    fs, fd = rc.flat_maps(scores, deltas)
    keep_s, keep_d = np.zeros(fs.shape, bool), np.zeros(fd.shape[:2], bool)
    for b in range(2):
        kp, kn = ref["t_%s_counts" % name][b]
        keep_s[b, ref["t_%s_pos" % name][b, :kp]] = keep_s[b, ref["t_%s_neg" % name][b, :kn]] = True
        keep_d[b, ref["t_%s_pos" % name][b, :kp]] = True
    cuts = np.cumsum(t.num_level_anchors)[:-1]
    nan_s = [np.where(k.reshape(2, H, W, 3).transpose(0, 3, 1, 2), x, np.float32("nan")).astype(np.float32)
             for k, x, (H, W) in zip(np.split(keep_s, cuts, axis=1), scores, rc.FEATMAPS)]
    nan_d = [np.where(np.repeat(k.reshape(2, H, W, 3), 4, axis=3).transpose(0, 3, 1, 2), x, np.float32("nan")).astype(np.float32)
             for k, x, (H, W) in zip(np.split(keep_d, cuts, axis=1), deltas, rc.FEATMAPS)]
    assert np.isnan(nan_s[0]).any() and np.isnan(nan_d[0]).any()
    dirty = run_loss(t, nan_s, nan_d, "sl1", 2.0, channels_last)
    assert np.array_equal(rc.bits(clean[0]), rc.bits(dirty[0]))
    for a, b in zip(clean[1] + clean[2], dirty[1] + dirty[2]):
        assert np.array_equal(rc.bits(a), rc.bits(b))


# ------------------------------------------------------------------------------------------------------------ 6. the dense losses
@pytest.mark.parametrize("kind", ["l1", "sl1"])
@pytest.mark.parametrize("name", ["crowded", "empty"])
def test_dense_losses_agree(ref, name, kind):
    from iif_amd.mmdet_rpn_stage import rpn_loss, rpn_stage_dense
    t, _ = case_run(ref, name)
    scores, deltas = rc.maps(name)
    ce, reg = losses(kind)
    s, d = [T(x) for x in scores], [T(x) for x in deltas]
    out = rpn_loss(s, d, t, ce, reg, pos_weight=rc.CASES[name]["pos_weight"])
    labels, lw, bt, bw = rpn_stage_dense(t, num_classes=1)
    avg = float(t.num_total_samples)                                                         # the host read of the dense chain
    bound, _, _ = loss_bounds(ref, name, kind)
    for l in range(len(scores)):
        cls = ce(s[l].permute(0, 2, 3, 1).reshape(-1, 1), labels[l].reshape(-1), lw[l].reshape(-1), avg_factor=avg)
        box = reg(d[l].permute(0, 2, 3, 1).reshape(-1, 4), bt[l].reshape(-1, 4), bw[l].reshape(-1, 4), avg_factor=avg)
        assert abs(float(cls) - float(out["loss_rpn_cls"][l])) <= bound[0, l], l
        assert abs(float(box) - float(out["loss_rpn_bbox"][l])) <= bound[1, l], l


# ------------------------------------------------------------------------------------------------------------ 7. the same bits
def test_two_calls_give_the_same_bits(ref):
    from iif_amd.mmdet_rpn_stage import rpn_stage_dense, rpn_stage_targets
    name = "crowded"
    first, keys = case_run(ref, name)
    c = rc.CASES[name]
    asg, smp, coder = parts(rc.run_of(name))
    again = rpn_stage_targets(rc.FEATMAPS, fpn_generator(), rc.PAD_SHAPES, rc.IMG_SHAPES, [T(g) for g in rc.case_gts(name)], asg, smp,
                              coder, allowed_border=c["border"], pos_weight=c["pos_weight"], keys=T(keys))
    for a, b in zip(first[:6], again[:6]):
        assert torch.equal(raw(a), raw(b))
    for a, b in zip(rpn_stage_dense(first), rpn_stage_dense(again)):
        assert all(torch.equal(raw(x), raw(y)) for x, y in zip(a, b))
    scores, deltas = rc.maps(name)
    r1, r2 = (run_loss(t, scores, deltas, "sl1", 2.0, False) for t in (first, again))
    assert np.array_equal(rc.bits(r1[0]), rc.bits(r2[0]))
    assert all(np.array_equal(rc.bits(a), rc.bits(b)) for a, b in zip(r1[1] + r1[2], r2[1] + r2[2]))


# ------------------------------------------------------------------------------------------------------------ 8. no synchronisation
def test_training_front_end_never_synchronises(ref):
    from iif_amd import mmdet_nms
    from iif_amd.mmdet_roi_stage import roi_stage_targets_padded
    from iif_amd.mmdet_rpn_stage import rpn_loss, rpn_stage_targets
    from . import nms_cases as nc
    from . import roi_stage_cases as rsc
    from .test_roi_stage_gpu import parts as roi_parts
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    name = "crowded"
    gen = fpn_generator()
    asg, smp, coder = parts(rc.run_of(name))
    gts = [T(g) for g in rc.case_gts(name)]
    scores, deltas = rc.maps(name)
    ce, reg = losses("sl1")
    c = nc.RPN_CASES["fpn5"]
    cls, regm, anchors = nc.rpn_inputs("fpn5")
    tcls, treg, tanc = ([T(x) for x in v] for v in (cls, regm, anchors))
    cfg = types.SimpleNamespace(nms_pre=c["nms_pre"], max_per_img=c["max_per_img"], min_bbox_size=c["min_size"],
                                nms=dict(type="nms", iou_threshold=c["thr"]))
    rpn_coder = types.SimpleNamespace(means=nc.MEANS, stds=nc.STDS, clip_border=True, add_ctr_clamp=False, ctr_clamp=32)
    B2 = len(c["shapes"])
    gts2 = [T(ac.proposals(5, 8970 + b, 120, 100, 8, 60)) for b in range(B2)]
    labs2 = [T(rsc._u(5, 8980 + b, rsc.REFINE_CLASSES)) for b in range(B2)]
    roi = roi_parts(rsc.RCNN, 64, 0.25)

    def step():
        s = [T(x).requires_grad_(True) for x in scores]
        d = [T(x).requires_grad_(True) for x in deltas]
        return s, d

    s, d = step()                                        # once before the mode is on: the library loads, caches warm
    t = rpn_stage_targets(rc.FEATMAPS, gen, rc.PAD_SHAPES, rc.IMG_SHAPES, gts, asg, smp, coder, allowed_border=0, pos_weight=2.0)
    out = rpn_loss(s, d, t, ce, reg, pos_weight=2.0)
    (sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"])).backward()
    dets, counts = mmdet_nms.rpn_proposals_padded(tcls, treg, tanc, c["shapes"], cfg, rpn_coder)
    roi_stage_targets_padded(dets, counts, gts2, labs2, *roi, rsc.REFINE_CLASSES)
    s, d = step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t = rpn_stage_targets(rc.FEATMAPS, gen, rc.PAD_SHAPES, rc.IMG_SHAPES, gts, asg, smp, coder, allowed_border=0, pos_weight=2.0)
        out = rpn_loss(s, d, t, ce, reg, pos_weight=2.0)
        (sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"])).backward()
        dets, counts = mmdet_nms.rpn_proposals_padded(tcls, treg, tanc, c["shapes"], cfg, rpn_coder)
        r = roi_stage_targets_padded(dets, counts, gts2, labs2, *roi, rsc.REFINE_CLASSES)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(t.counts.sum()) > 0 and all(torch.isfinite(x.grad).all() for x in s + d) and int(r.counts.sum()) > 0
