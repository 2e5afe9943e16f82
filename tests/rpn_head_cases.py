"""Cases for the RPN head's sampled backward (iif_amd/mmdet_rpn_head.py, csrc/rpn_head_sampled.hip).

Inputs are closed integer formulas of a salt (hash streams), restated here for the fixture's maker and the tests alike, so
tests/golden/g39_rpn_head_sampled.npz holds results only; ``input_checksums`` ties the two together.  Features and parameters lie
on a dyadic grid: features are multiples of 1/8 in [-1, 1), ``rpn_conv``'s weights multiples of 2^-12 in [-1/8, 1/8) and its bias
multiples of 1/16, so every partial sum of the 3x3 convolution is a multiple of 2^-15 below 2^9 (up to 256 input channels): the
ReLU's input is exact in float32 in any summation order, and float32 and float64 agree on every sign.  ``rpn_cls`` / ``rpn_reg``
weights are multiples of 2^-10 in [-1/2, 1/2).  The weights use 10-bit integers so that no sum of products of them cancels to an
exact zero by accident: a ``d feats`` element of the float64 run is 0 only where no sampled pixel reaches it (the maker asserts it).
"""
import numpy as np

from . import assign_cases as ac
from .ce_cases import _hash

F = np.float32

STRIDES = [8, 16, 32, 64, 128]
FEATMAPS = [(12, 16), (6, 8), (3, 4), (2, 2), (1, 1)]
B = 2
PIXELS = sum(h * w for h, w in FEATMAPS)
GEN = dict(strides=STRIDES, ratios=[0.5, 1.0, 2.0], scales=[4])
PAD_SHAPES = ((96, 128, 3), (64, 96, 3))
IMG_SHAPES = ((90, 121, 3), (60, 93, 3))
NUM, FRAC, UB = 64, 0.5, -1
NEP = int(NUM * FRAC)
MEANS, STDS = (0., 0., 0., 0.), (1., 1., 1., 1.)
BETA = 1.0 / 9.0
RUN = ac.RPN

# the fixture's cases: ground truth of the two images, allowed_border, pos_weight, the box loss, channels, input salt
CASES = {
    "boxes_l1": dict(images=("many", "few"), border=-1, pos_weight=-1.0, kind="l1", ci=24, co=40, salt=9900),
    "empty_sl1": dict(images=("none", "few"), border=0, pos_weight=2.0, kind="sl1", ci=24, co=40, salt=9910),
}


def _u(n, salt, mod):
    return (_hash(n, salt) % np.uint64(mod)).astype(np.int64)


def gt_boxes(kind):
    if kind == "none":
        return np.zeros((0, 4), dtype=np.float32)
    if kind == "few":
        return np.array([[10.5, 8.25, 40.0, 30.5], [30.0, 20.0, 75.5, 58.0], [2.0, 3.0, 20.0, 50.0]], dtype=np.float32)
    if kind == "many":
        # boxes close to anchors of levels 0 to 2 (32, 64 and 128 pixels), several on neighbouring cells
        return np.array([[16.0, 24.0, 48.0, 56.0], [25.0, 25.0, 56.0, 55.0], [60.0, 10.0, 105.0, 34.0], [0.0, 30.0, 64.0, 92.0],
                         [70.0, 40.0, 118.0, 88.0], [5.0, 5.0, 28.0, 50.0], [40.0, 60.0, 72.0, 90.0], [2.0, 2.0, 120.0, 88.0]],
                        dtype=np.float32)
    raise KeyError(kind)


def case_gts(name):
    return [gt_boxes(k) for k in CASES[name]["images"]]


def features(ci, salt, featmaps=FEATMAPS, batch=B):
    """Per level float32 ``[batch, ci, H, W]``: multiples of 1/8 in [-1, 1)."""
    return [((_u(batch * ci * H * W, salt + l, 16) - 8).astype(np.float32) / F(8)).reshape(batch, ci, H, W)
            for l, (H, W) in enumerate(featmaps)]


def parameters(ci, co, A, salt):
    """``(w_conv [co, ci, 3, 3], b_conv [co], w_cls [A, co, 1, 1], b_cls [A], w_reg [4 A, co, 1, 1], b_reg [4 A])`` float32."""
    def grid(shape, s, mod, div):
        n = int(np.prod(shape))
        return ((_u(n, salt + s, mod) - mod // 2).astype(np.float32) / F(div)).reshape(shape)
    return (grid((co, ci, 3, 3), 20, 1024, 4096), grid((co,), 21, 16, 16), grid((A, co, 1, 1), 22, 1024, 1024), grid((A,), 23, 16, 16),
            grid((4 * A, co, 1, 1), 24, 1024, 1024), grid((4 * A,), 25, 16, 16))


PARAM_NAMES = ("w_conv", "b_conv", "w_cls", "b_cls", "w_reg", "b_reg")


def input_checksums():
    out = {}
    for name, c in CASES.items():
        parts = [g.reshape(-1) for g in case_gts(name)] + [x.reshape(-1) for x in features(c["ci"], c["salt"])] + \
                [p.reshape(-1) for p in parameters(c["ci"], c["co"], 3, c["salt"])]
        out["in_%s" % name] = np.array([ac.bit_sum(np.concatenate(parts))], dtype=np.uint64)
    return out


def check_generator(g):
    for key, v in input_checksums().items():
        assert np.array_equal(v, g[key]), "input generator drifted from the fixture: " + key


# ---------------------------------------------------------------------------------------------------------------- the sample
def level_starts(A, featmaps=FEATMAPS):
    return np.concatenate([[0], np.cumsum([h * w * A for h, w in featmaps])]).astype(np.int64)


def decode_pixels(idx, A, featmaps=FEATMAPS):
    """Flat anchor indices (order ``(level, y, x, a)``) -> ``(level, y, x)`` arrays: ``(idx - level_start) // A``."""
    idx = np.asarray(idx, dtype=np.int64)
    starts = level_starts(A, featmaps)
    lv = np.searchsorted(starts, idx, side="right") - 1
    cell = (idx - starts[lv]) // A
    W = np.array([w for _, w in featmaps], dtype=np.int64)[lv]
    return lv, cell // W, cell % W


def sample_slots(pos, neg, counts, A, featmaps=FEATMAPS):
    """The owner rule in numpy.  ``pos [B, nep]`` / ``neg [B, num]`` padded with -1, ``counts [B, 2]``: ``(slots [S, 4], owner
    [B, P])`` with slot ``e = b (nep + num) + r`` (positives first), ``slots[e] = (b, level, y, x)`` if ``e`` is the lowest slot
    on its pixel and ``(0, -1, 0, 0)`` otherwise; ``owner`` -1 where nothing was sampled."""
    Bn, nep = pos.shape
    num = neg.shape[1]
    P = sum(h * w for h, w in featmaps)
    pix0 = np.concatenate([[0], np.cumsum([h * w for h, w in featmaps])])
    slots = np.zeros((Bn * (nep + num), 4), dtype=np.int32)
    slots[:, 1] = -1
    owner = np.full((Bn, P), -1, dtype=np.int32)
    for b in range(Bn):
        for r in range(nep + num):
            is_pos = r < nep
            k = r if is_pos else r - nep
            if k >= counts[b, 0 if is_pos else 1]:
                continue
            idx = pos[b, k] if is_pos else neg[b, k]
            l, y, x = (int(v[0]) for v in decode_pixels([idx], A, featmaps))
            p = pix0[l] + y * featmaps[l][1] + x
            if owner[b, p] < 0:                                         # slots are visited in ascending order: the first one owns
                e = b * (nep + num) + r
                owner[b, p] = e
                slots[e] = (b, l, y, x)
    return slots, owner
