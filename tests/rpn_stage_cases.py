"""Cases and the numpy restatement for the RPN head's training side (iif_amd/mmdet_anchor.py, iif_amd/mmdet_rpn_stage.py): anchors
and flags (core/anchor/anchor_generator.py), the masked assignment and key sampling of anchor_head.py:210-268 in the FLAT index
space, the dense unmap of ``get_targets`` + ``images_to_levels``, and the loss terms of anchor_head.py:373-421.

The inputs are functions of the case name alone (hash streams), so the fixture tests/golden/g34_rpn_stage.npz holds only what the
reference produced; ``input_checksums`` ties the two together.
"""
import numpy as np

from . import assign_cases as ac
from . import targets_cases as tc
from .ce_cases import _hash

F = np.float32
bits = ac.bits

# ---------------------------------------------------------------------------------------------------------------- generators
# name -> constructor arguments and the feature-map sizes the tests ask for
GEN_CASES = {
    "fpn": (dict(strides=[4, 8, 16, 32, 64], ratios=[0.5, 1.0, 2.0], scales=[8]), [(24, 32), (12, 16), (6, 8), (3, 4), (2, 2)]),
    "offset": (dict(strides=[8, 16], ratios=[0.5, 1.0, 2.0], scales=[4, 8], center_offset=0.5), [(5, 7), (3, 4)]),
    "ratio_major": (dict(strides=[8, 16], ratios=[0.5, 1.0, 2.0], scales=[2, 4, 8], scale_major=False), [(5, 7), (3, 4)]),
    "octave": (dict(strides=[8, 16, 32], ratios=[0.5, 1.0, 2.0], octave_base_scale=4, scales_per_octave=3), [(6, 5), (3, 3), (2, 1)]),
    "nonsquare": (dict(strides=[(4, 8), (8, 16)], ratios=[1.0, 3.0], scales=[8], base_sizes=[6, 12]), [(7, 9), (4, 5)]),
    "centers": (dict(strides=[16], ratios=[1.0], scales=[1.0], base_sizes=[9], centers=[(3.5, 1.25)]), [(2, 3)]),
}
GEN_PAD_SHAPES = ((96, 128), (64, 96), (33, 50), (1, 1))

FPN = "fpn"
FEATMAPS = GEN_CASES[FPN][1]
PAD_SHAPES = ((96, 128, 3), (64, 96, 3))
IMG_SHAPES = ((90, 121, 3), (60, 93, 3))
NUM, FRAC, UB = 256, 0.5, -1
NEP = int(NUM * FRAC)
MEANS, STDS = (0., 0., 0., 0.), (1., 1., 1., 1.)
RUN = ac.RPN                                    # (0.7, 0.3, 0.3, gt_max_assign_all, -1, True, match_low_quality)
BETA = 1.0 / 9.0

# name -> the two images' ground truth, allowed_border, pos_weight, gt_max_assign_all
CASES = {
    "crowded": dict(images=("crowd", "few"), border=-1, pos_weight=-1.0, assign_all=True),
    "empty": dict(images=("none", "few"), border=0, pos_weight=2.0, assign_all=False),
    "tie_all": dict(images=("tie", "edge"), border=0, pos_weight=-1.0, assign_all=True),
    "tie_first": dict(images=("tie", "edge"), border=-1, pos_weight=2.0, assign_all=False),
}


def run_of(name):
    r = list(RUN)
    r[3] = CASES[name]["assign_all"]
    return tuple(r)


def _u(n, salt, mod):
    return (_hash(n, salt) % np.uint64(mod)).astype(np.int64)


def base_anchors_np(strides, ratios, scales=None, base_sizes=None, scale_major=True, octave_base_scale=None, scales_per_octave=None,
                    centers=None, center_offset=0.):
    """anchor_generator.py:131-194 in numpy float32, operation by operation: a list of ``[A_l, 4]``."""
    strides = [s if isinstance(s, tuple) else (s, s) for s in strides]
    base_sizes = [min(s) for s in strides] if base_sizes is None else base_sizes
    if scales is None:
        scales = np.array([2 ** (i / scales_per_octave) for i in range(scales_per_octave)]) * octave_base_scale
    scales = np.asarray(scales, dtype=np.float32)
    ratios = np.asarray(ratios, dtype=np.float32)
    out = []
    for i, bs in enumerate(base_sizes):
        if centers is None:
            xc, yc = center_offset * bs, center_offset * bs
        else:
            xc, yc = centers[i]
        hr = np.sqrt(ratios)
        wr = (F(1) / hr).astype(np.float32)
        if scale_major:
            ws = ((F(bs) * wr)[:, None] * scales[None, :]).reshape(-1)
            hs = ((F(bs) * hr)[:, None] * scales[None, :]).reshape(-1)
        else:
            ws = ((F(bs) * scales)[:, None] * wr[None, :]).reshape(-1)
            hs = ((F(bs) * scales)[:, None] * hr[None, :]).reshape(-1)
        ws, hs = ws.astype(np.float32), hs.astype(np.float32)
        out.append(np.stack([F(xc) - F(0.5) * ws, F(yc) - F(0.5) * hs, F(xc) + F(0.5) * ws, F(yc) + F(0.5) * hs], axis=-1).astype(np.float32))
    return out


def grid_anchors_np(base, strides, featmaps):
    """anchor_generator.py:239-272: per level ``[H W A, 4]`` = base[a] + (x sx, y sy, x sx, y sy)."""
    out = []
    for b, s, (H, W) in zip(base, strides, featmaps):
        sw, sh = s if isinstance(s, tuple) else (s, s)
        xx = np.tile(np.arange(W) * sw, H)
        yy = np.repeat(np.arange(H) * sh, W)
        shifts = np.stack([xx, yy, xx, yy], axis=-1).astype(np.float32)
        out.append((b[None, :, :] + shifts[:, None, :]).reshape(-1, 4).astype(np.float32))
    return out


def valid_flags_np(strides, featmaps, num_base, pad_shape):
    """anchor_generator.py:383-440 per level."""
    out = []
    h, w = pad_shape[:2]
    for s, (H, W), nb in zip(strides, featmaps, num_base):
        sw, sh = s if isinstance(s, tuple) else (s, s)
        vh, vw = min(int(np.ceil(h / sh)), H), min(int(np.ceil(w / sw)), W)
        v = (np.arange(W) < vw)[None, :] & (np.arange(H) < vh)[:, None]
        out.append(np.repeat(v.reshape(-1), nb))
    return out


def inside_flags_np(anchors, valid, img_shape, border):
    """core/anchor/utils.py:21-47."""
    if border < 0:
        return valid
    h, w = img_shape[:2]
    a = anchors
    return valid & (a[:, 0] >= F(-border)) & (a[:, 1] >= F(-border)) & (a[:, 2] < F(w + border)) & (a[:, 3] < F(h + border))


def fpn_anchors():
    kw = GEN_CASES[FPN][0]
    base = base_anchors_np(**kw)
    per_level = grid_anchors_np(base, kw["strides"], FEATMAPS)
    return base, per_level, np.concatenate(per_level)


def fpn_inside(img, border):
    """bool [A]: the candidates of image ``img`` (0 / 1) under ``allowed_border``."""
    kw = GEN_CASES[FPN][0]
    base, per_level, flat = fpn_anchors()
    valid = np.concatenate(valid_flags_np(kw["strides"], FEATMAPS, [b.shape[0] for b in base], PAD_SHAPES[img]))
    return inside_flags_np(flat, valid, IMG_SHAPES[img], border)


# ---------------------------------------------------------------------------------------------------------------- ground truth
def gt_boxes(kind, img):
    """float32 [G, 4] of one image.  'crowd': about 300 boxes that nearly coincide with anchors of the image's valid area (far
    more positives than num_expected_pos); 'few': three boxes; 'none': no box; 'tie': a box midway between two neighbouring
    anchors - an exact IoU tie for the gt's maximum - plus two ordinary ones; 'edge': a box centred beyond the padded area of
    the SMALLER image, whose best anchor overall is not valid there, plus an ordinary one."""
    _, _, flat = fpn_anchors()
    if kind == "none":
        return np.zeros((0, 4), dtype=np.float32)
    if kind == "crowd":
        ok = np.nonzero(fpn_inside(img, 0))[0]
        pick = ok[np.unique(_u(300, 9100 + img, ok.size))]
        jit = (_u(pick.size * 4, 9110 + img, 5).reshape(-1, 4).astype(np.float32) - F(2)) * F(0.25)
        return (flat[pick] + jit).astype(np.float32)
    if kind == "few":
        return np.array([[10.5, 8.25, 40.0, 30.5], [30.0, 20.0, 75.5, 58.0], [2.0, 3.0, 20.0, 50.0]], dtype=np.float32)
    if kind == "tie":
        # the ratio-1 anchor of level 0 at cell (x, y) is [4 x - 16, 4 y - 16, 4 x + 16, 4 y + 16]; the 20 x 20 box lies inside
        # several of them, and each such overlap is 400 / 1024: the same bits, below pos_iou_thr and above min_pos_iou
        return np.array([[32.0, 26.0, 52.0, 46.0], [50.0, 40.0, 110.0, 84.0], [5.0, 60.0, 30.0, 88.0]], dtype=np.float32)
    if kind == "edge":
        return np.array([[78.0, 20.0, 122.0, 42.0], [20.0, 10.0, 52.0, 44.0]], dtype=np.float32)
    raise KeyError(kind)


def case_gts(name):
    return [gt_boxes(k, i) for i, k in enumerate(CASES[name]["images"])]


def maps(name):
    """(scores, deltas): per level float32 ``[B, A_l / (H W), H, W]`` and ``[B, 4 A_l / (H W), H, W]``, values in (-4, 4) / (-1, 1)."""
    salt = 9300 + 10 * list(CASES).index(name)
    scores, deltas = [], []
    for l, (H, W) in enumerate(FEATMAPS):
        n = 2 * 3 * H * W
        scores.append(((_u(n, salt + l, 1 << 16).astype(np.float32) / F(1 << 13)) - F(4)).reshape(2, 3, H, W))
        deltas.append(((_u(4 * n, salt + 5 + l, 1 << 16).astype(np.float32) / F(1 << 15)) - F(1)).reshape(2, 12, H, W))
    return scores, deltas


def key_salt(name, img):
    return 9500 + 8 * list(CASES).index(name) + 4 * img


def fixture_keys(g, name, img, gt_inds_compact, inside):
    """int32 [A] flat keys of image ``img`` from the fixture's ranks (compact index space) - hash keys where the anchor takes
    no part."""
    pre = "t_%s_%d_rank" % (name, img)
    kc = tc.keys_from_ranks(gt_inds_compact, {0: g[pre + "0"], 1: g[pre + "1"]}, key_salt(name, img))
    keys = tc.free_keys(inside.size, key_salt(name, img) + 3)
    keys[inside] = kc
    return keys


def input_checksums():
    out = {}
    for name in CASES:
        s, d = maps(name)
        out["in_%s" % name] = np.array([ac.bit_sum(np.concatenate([g.reshape(-1) for g in case_gts(name)] + [np.zeros(1, np.float32)])),
                                        ac.bit_sum(np.concatenate([x.reshape(-1) for x in s + d]))], dtype=np.uint64)
    return out


def check_generator(g):
    for key, v in input_checksums().items():
        assert np.array_equal(v, g[key]), "input generator drifted from the fixture: " + key


# ---------------------------------------------------------------------------------------------------------------- targets
def targets_np(flat, inside, gts, keys, run, num=NUM, frac=FRAC, ub=UB, means=MEANS, stds=STDS):
    """Masked assignment and key sampling of one image in the FLAT index space: ``(pos_inds, neg_inds, pos_gt, pos_targets,
    gt_inds_compact)``; ``keys`` is flat ``[A]``."""
    sel = np.nonzero(inside)[0]
    if sel.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, np.zeros((0, 4), dtype=np.float32), z
    gi = ac.assign_np(flat[sel], gts, None, None, run)[0]
    pos_c, neg_c = tc.sample_np(gi, keys[sel], num, frac, ub)
    pos_gt = gi[pos_c] - 1
    bt = tc.bbox2delta_np(flat[sel][pos_c], gts[pos_gt], means, stds) if pos_c.size else np.zeros((0, 4), dtype=np.float32)
    return sel[pos_c], sel[neg_c], pos_gt, bt, gi


def dense_np(level_counts, per_image, pos_weight, num_classes=1):
    """``get_targets`` after ``images_to_levels`` from per-image ``(pos_inds, neg_inds, pos_targets)``: four per-level lists."""
    B, A = len(per_image), sum(level_counts)
    labels = np.full((B, A), num_classes, dtype=np.int64)
    lw = np.zeros((B, A), dtype=np.float32)
    bt = np.zeros((B, A, 4), dtype=np.float32)
    bw = np.zeros((B, A, 4), dtype=np.float32)
    for b, (pos, neg, t) in enumerate(per_image):
        labels[b, pos] = 0
        lw[b, pos] = 1.0 if pos_weight <= 0 else pos_weight
        lw[b, neg] = 1.0
        bt[b, pos] = t
        bw[b, pos] = 1.0
    cuts = np.cumsum(level_counts)[:-1]
    return tuple(np.split(x, cuts, axis=1) for x in (labels, lw, bt, bw))


def flat_maps(scores, deltas):
    """anchor_head.py:402-409: ``[B, A]`` scores and ``[B, A, 4]`` deltas over the concatenated levels."""
    s = np.concatenate([x.transpose(0, 2, 3, 1).reshape(x.shape[0], -1) for x in scores], axis=1)
    d = np.concatenate([x.transpose(0, 2, 3, 1).reshape(x.shape[0], -1, 4) for x in deltas], axis=1)
    return s, d


def loss_terms_np(scores, deltas, per_image, level_counts, pos_weight, beta, dtype=np.float64):
    """Per level the UNSCALED terms: ``(cls_terms, box_terms)`` lists of 1-D arrays in ``dtype`` (w BCE_with_logits at the
    sampled anchors; L1 / SmoothL1 at the positives' deltas), and ``num_total_samples``."""
    s, d = flat_maps(scores, deltas)
    s, d = s.astype(dtype), d.astype(dtype)
    starts = np.concatenate([[0], np.cumsum(level_counts)])
    cls = [[] for _ in level_counts]
    box = [[] for _ in level_counts]
    nts = 0
    for b, (pos, neg, t) in enumerate(per_image):
        nts += max(pos.size, 1) + max(neg.size, 1)
        for idx, tgt, w in ((pos, 1.0, 1.0 if pos_weight <= 0 else pos_weight), (neg, 0.0, 1.0)):
            x = s[b, idx]
            term = (np.maximum(x, 0) - x * dtype(tgt) + np.log1p(np.exp(-np.abs(x)))) * dtype(w)
            lv = np.searchsorted(starts, idx, side="right") - 1
            for l in range(len(level_counts)):
                cls[l].append(term[lv == l])
        diff = np.abs(d[b, pos] - t.astype(dtype))
        if beta > 0:
            diff = np.where(diff < dtype(beta), dtype(0.5) * diff * diff / dtype(beta), diff - dtype(0.5 * beta))
        lv = np.searchsorted(starts, pos, side="right") - 1
        for l in range(len(level_counts)):
            box[l].append(diff[lv == l].reshape(-1))
    return [np.concatenate(c) for c in cls], [np.concatenate(c) for c in box], nts
