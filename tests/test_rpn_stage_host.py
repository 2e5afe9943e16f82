"""Host-side checks of the RPN head's training side (iif_amd/mmdet_anchor.py, iif_amd/mmdet_rpn_stage.py): no device work.

  * the numpy restatement of tests/rpn_stage_cases.py reproduces the reference's runs (tests/golden/g34_rpn_stage.npz);
  * the header prototypes and ``_lib.SIGNATURES`` agree in argument count;
  * every limit and unsupported option raises its error before anything touches the device;
  * ``AnchorGenerator.base_anchors`` equal the reference's bit for bit.
"""
import os
import re
import types

import numpy as np
import pytest
import torch

from . import rpn_stage_cases as rc
from . import targets_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_grid_anchors", "iif_grid_valid_flags", "iif_rpn_stage_workspace_bytes", "iif_rpn_stage_targets", "iif_rpn_stage_dense",
           "iif_rpn_loss_fwd", "iif_rpn_loss_bwd")


@pytest.fixture(scope="module")
def ref(golden):
    g = golden("g34_rpn_stage")
    rc.check_generator(g)
    return g


@pytest.fixture(scope="module")
def ulps(golden):
    return golden("g26_targets")["coder_ref_ulps"]


def case_lists(ref, name):
    """Per image ``(pos, neg, reference targets)`` of a fixture case, and the level counts."""
    counts = ref["t_%s_counts" % name]
    per_image = []
    for b in range(2):
        kp, kn = counts[b]
        per_image.append((ref["t_%s_pos" % name][b, :kp].astype(np.int64), ref["t_%s_neg" % name][b, :kn].astype(np.int64),
                          ref["t_%s_pos_bt" % name][b, :kp]))
    return per_image, [a.shape[0] for a in rc.fpn_anchors()[1]]


@pytest.mark.parametrize("name", list(rc.GEN_CASES))
def test_generator_restatement_and_base_anchors(ref, name):
    from iif_amd.mmdet_anchor import AnchorGenerator
    kw, featmaps = rc.GEN_CASES[name]
    gen = AnchorGenerator(**kw)
    base = rc.base_anchors_np(**kw)
    assert gen.num_levels == len(featmaps) and gen.num_base_anchors == [b.shape[0] for b in base]
    for l, b in enumerate(base):
        want = ref["gen_%s_base%d" % (name, l)]
        assert np.array_equal(rc.bits(b), rc.bits(want)), l
        assert np.array_equal(rc.bits(gen.base_anchors[l].numpy()), rc.bits(want)), l           # bit for bit
    anchors = np.concatenate(rc.grid_anchors_np(base, kw["strides"], featmaps))
    assert np.array_equal(rc.bits(anchors), rc.bits(ref["gen_%s_anchors" % name]))
    for k, pad in enumerate(rc.GEN_PAD_SHAPES):
        flags = np.concatenate(rc.valid_flags_np(kw["strides"], featmaps, gen.num_base_anchors, pad))
        assert np.array_equal(np.packbits(flags), ref["gen_%s_flags%d" % (name, k)]), pad
    assert repr(gen).startswith("AnchorGenerator(\n    strides=[(") and "center_offset=" in repr(gen)


def test_generator_constructor_errors():
    from iif_amd.mmdet_anchor import AnchorGenerator
    with pytest.raises(ValueError):
        AnchorGenerator([4], [1.0], [8], center_offset=1.5)
    with pytest.raises(AssertionError):
        AnchorGenerator([4], [1.0], [8], centers=[(0, 0)], center_offset=0.5)
    with pytest.raises(AssertionError):
        AnchorGenerator([4, 8], [1.0], [8], centers=[(0, 0)])
    with pytest.raises(AssertionError):
        AnchorGenerator([4, 8], [1.0], [8], base_sizes=[4])
    with pytest.raises(AssertionError):
        AnchorGenerator([4], [1.0], scales=[8], octave_base_scale=4, scales_per_octave=3)
    with pytest.raises(AssertionError):
        AnchorGenerator([4], [1.0])
    with pytest.raises(NotImplementedError):
        AnchorGenerator([4], [1.0], [8]).sparse_priors(None, (1, 1), 0)
    with pytest.raises(ValueError):                                             # nine levels: before any device work
        AnchorGenerator([4] * 9, [1.0], [8]).grid_anchors([(1, 1)] * 9, device="cuda")
    with pytest.raises(ValueError):                                             # 18 base anchors
        AnchorGenerator([4], [1.0] * 6, [1, 2, 3]).valid_flags([(1, 1)], (4, 4), device="cuda")


@pytest.mark.parametrize("name", list(rc.CASES))
def test_targets_restatement_reproduces_the_fixture(ref, ulps, name):
    c = rc.CASES[name]
    _, per_level, flat = rc.fpn_anchors()
    counts = ref["t_%s_counts" % name]
    nts = 0
    for b, gts in enumerate(rc.case_gts(name)):
        inside = rc.fpn_inside(b, c["border"])
        gi = rc.targets_np(flat, inside, gts, np.zeros(flat.shape[0], np.int32), rc.run_of(name))[4]
        keys = rc.fixture_keys(ref, name, b, gi, inside)
        pos, neg, pos_gt, bt, _ = rc.targets_np(flat, inside, gts, keys, rc.run_of(name))
        kp, kn = counts[b]
        assert (pos.size, neg.size) == (kp, kn)
        assert np.array_equal(pos, ref["t_%s_pos" % name][b, :kp]) and (ref["t_%s_pos" % name][b, kp:] == -1).all()
        assert np.array_equal(neg, ref["t_%s_neg" % name][b, :kn]) and (ref["t_%s_neg" % name][b, kn:] == -1).all()
        assert np.array_equal(pos_gt, ref["t_%s_pos_gt" % name][b, :kp])
        want = ref["t_%s_pos_bt" % name][b, :kp]
        assert np.array_equal(rc.bits(bt[:, :2]), rc.bits(want[:, :2]))
        if kp:
            exact, kinds, err = tc.encode_check(bt, flat[pos], gts[pos_gt], rc.MEANS, rc.STDS)
            assert exact and kinds and err <= 2 * ulps[0]
        nts += max(kp, 1) + max(kn, 1)
    assert nts == int(ref["t_%s_nts" % name])


@pytest.mark.parametrize("kind,beta", [("l1", 0.0), ("sl1", rc.BETA)])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_loss_restatement_reproduces_the_fixture(ref, name, kind, beta):
    per_image, level_counts = case_lists(ref, name)
    scores, deltas = rc.maps(name)
    cls, box, nts = rc.loss_terms_np(scores, deltas, per_image, level_counts, rc.CASES[name]["pos_weight"], beta)
    assert nts == int(ref["t_%s_nts" % name])
    mine = np.array([[t.sum() / nts for t in cls], [t.sum() / nts for t in box]])
    assert np.allclose(mine, ref["l_%s_%s_loss64" % (name, kind)], rtol=1e-12, atol=1e-15)


def test_header_and_ctypes_table_agree_in_argument_count():
    from iif_amd import _lib
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[name]), (name, len(args), len(_lib.SIGNATURES[name]))
    import ctypes
    assert ctypes.sizeof(_lib.RpnGrid) == 4 + 5 * 32 + 8 * 16 * 4 * 4 and ctypes.sizeof(_lib.RpnLossLevel) == 4 * 8 + 16 * 8


def _parts(num=256, frac=0.5, add_gt=False, ign=-1):
    from iif_amd.mmdet_assigner import MaxIoUAssigner
    from iif_amd.mmdet_targets import DeltaXYWHBBoxCoder, RandomSampler
    return (MaxIoUAssigner(0.7, 0.3, min_pos_iou=0.3, ignore_iof_thr=ign), RandomSampler(num, frac, add_gt_as_proposals=add_gt),
            DeltaXYWHBBoxCoder(rc.MEANS, rc.STDS))


def test_limits_and_unsupported_options_raise_before_device_work():
    """CPU tensors throughout: reaching the device checks would raise ``IIFNativeError`` instead of the stated error."""
    from iif_amd.mmdet_anchor import AnchorGenerator
    from iif_amd.mmdet_bbox_loss import L1Loss
    from iif_amd.mmdet_ce_loss import CrossEntropyLoss
    from iif_amd.mmdet_rpn_stage import rpn_loss, rpn_stage_targets
    gen = AnchorGenerator(**rc.GEN_CASES[rc.FPN][0])
    gt = torch.zeros((1, 4))

    def call(B=2, gen=gen, featmaps=rc.FEATMAPS, parts=None, **kw):
        asg, smp, coder = parts or _parts()
        return rpn_stage_targets(featmaps, gen, [rc.PAD_SHAPES[0]] * B, [rc.IMG_SHAPES[0]] * B, [gt] * B, asg, smp, coder, **kw)
    for B in (0, 17):
        with pytest.raises(ValueError, match="per-image chain"):
            call(B=B)
    with pytest.raises(ValueError, match="per-image chain"):
        call(parts=_parts(num=1025))
    with pytest.raises(ValueError, match="per-image chain"):
        call(gen=AnchorGenerator([4] * 9, [1.0], [8]), featmaps=[(1, 1)] * 9)
    with pytest.raises(ValueError, match="per-image chain"):
        call(gen=AnchorGenerator([4], [1.0] * 17, [8]), featmaps=[(1, 1)])
    with pytest.raises(ValueError, match="per-image chain"):
        call(gen=AnchorGenerator([1], [1.0] * 16, [8]), featmaps=[(16384, 16384)])          # 2^32 anchors
    with pytest.raises(ValueError, match="add_gt_as_proposals"):
        call(parts=_parts(add_gt=True))
    asg, smp, coder = _parts()
    with pytest.raises(NotImplementedError, match="RandomSampler"):
        call(parts=(asg, types.SimpleNamespace(num=256, pos_fraction=0.5, add_gt_as_proposals=False, neg_pos_ub=-1), coder))
    with pytest.raises(NotImplementedError, match="ignore"):
        call(parts=_parts(ign=0.5), gt_bboxes_ignore_list=[torch.ones((1, 4))] * 2)
    with pytest.raises(ValueError, match="keys"):
        call(keys=torch.zeros((2, 5), dtype=torch.int32))
    targets = types.SimpleNamespace(featmap_sizes=rc.FEATMAPS)
    ce, l1 = CrossEntropyLoss(use_sigmoid=True), L1Loss()
    for bad in (CrossEntropyLoss(use_sigmoid=False), CrossEntropyLoss(use_sigmoid=True, reduction="sum"),
                CrossEntropyLoss(use_sigmoid=True, class_weight=[1.0]), torch.nn.BCEWithLogitsLoss()):
        with pytest.raises(NotImplementedError, match="rpn_stage_dense"):
            rpn_loss([], [], targets, bad, l1)
    for bad in (L1Loss(reduction="sum"), torch.nn.MSELoss()):
        with pytest.raises(NotImplementedError, match="rpn_stage_dense"):
            rpn_loss([], [], targets, ce, bad)
