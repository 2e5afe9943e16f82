#!/usr/bin/env python3
"""Generate tests/golden/gNN_targets.npz (the next free number) by RUNNING THE REFERENCE's RandomSampler, DeltaXYWHBBoxCoder,
anchor_inside_flags, unmap, AnchorHead._get_targets_single and BBoxHead._get_target_single on the CPU in float32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_targets.py <reference checkout>

``core/bbox/coder/delta_xywh_bbox_coder.py``, ``core/bbox/samplers/{base_sampler,random_sampler,sampling_result}.py``,
``core/bbox/assigners/assign_result.py``, ``core/anchor/utils.py``, ``core/utils/misc.py``, ``models/dense_heads/anchor_head.py``
and ``models/roi_heads/bbox_heads/bbox_head.py`` are imported as they are.  mmcv / mmdet are not needed: the process gets
placeholder modules - registries whose ``register_module`` returns the class, ``mmcv.jit`` / ``force_fp32`` / ``auto_fp16`` as
identity decorators, ``BaseModule`` as ``torch.nn.Module``, ``demodata.ensure_rng`` returning None.  The two head methods are
called unbound on a stand-in ``self`` whose assigner returns a prepared AssignResult (the reference's class) and whose sampler
and coder are the reference's.  Nothing from the reference is written to the repository except outputs (data).

The sampler is tied to the reference through KEYS: ``torch.randperm`` is wrapped to record the permutations the reference drew,
and tests/targets_cases.keys_from_ranks turns their inverses into keys under which "keep the k smallest (key, index) pairs"
selects the reference's ``gallery[perm[:k]]``.  The fixture stores the keys in that form (one rank per member of a class the
reference drew for; the rest of a key is the hash's) and the reference's sorted index lists.

For every case the generator asserts that the numpy restatements of tests/targets_cases.py reproduce the reference: bit for bit
everywhere except the log / exp columns, there bit for bit too where numpy's float32 log / exp agree with torch's and otherwise
within the reference's own measured error plus the same again (targets_cases.encode_check / decode_check).  It prints the
reference's maximum errors on that scale (float32 ulps against the float64 continuation) and stores them as ``coder_ref_ulps``.
"""
import glob
import importlib
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import targets_cases as tc          # noqa: E402

torch.set_num_threads(8)
T = torch.from_numpy


class _Registry:
    def register_module(self, name=None, force=False, module=None):
        if module is not None:
            return module
        return lambda cls: cls


def _pkg(name, path=None, **names):
    m = types.ModuleType(name)
    m.__path__ = [path] if path else []
    for k, v in names.items():
        setattr(m, k, v)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    return m


def _identity_decorator(*args, **kwargs):
    return lambda f: f


def reference(ref_root):
    mm = os.path.join(ref_root, "instance_segmentation", "mmdet")
    bbox = os.path.join(mm, "core", "bbox")
    imp = importlib.import_module
    try:
        import six  # noqa: F401
    except ImportError:
        _pkg("six")
        _pkg("six.moves", map=map, zip=zip)
    _pkg("mmcv", jit=_identity_decorator)
    _pkg("mmcv.runner", force_fp32=_identity_decorator, auto_fp16=_identity_decorator, BaseModule=torch.nn.Module)
    _pkg("mmdet")
    _pkg("mmdet.utils", os.path.join(mm, "utils"))
    imp("mmdet.utils.util_mixins")
    core = _pkg("mmdet.core")
    _pkg("mmdet.core.mask")
    _pkg("mmdet.core.mask.structures", BitmapMasks=type("BitmapMasks", (), {}), PolygonMasks=type("PolygonMasks", (), {}))
    _pkg("mmdet.core.utils", os.path.join(mm, "core", "utils"))
    misc = imp("mmdet.core.utils.misc")
    _pkg("mmdet.core.anchor", os.path.join(mm, "core", "anchor"))
    autils = imp("mmdet.core.anchor.utils")
    _pkg("mmdet.core.bbox")
    _pkg("mmdet.core.bbox.builder", BBOX_ASSIGNERS=_Registry(), BBOX_SAMPLERS=_Registry(), BBOX_CODERS=_Registry())
    _pkg("mmdet.core.bbox.demodata", ensure_rng=lambda rng=None: None)
    _pkg("mmdet.core.bbox.assigners", os.path.join(bbox, "assigners"))
    ar = imp("mmdet.core.bbox.assigners.assign_result")
    _pkg("mmdet.core.bbox.samplers", os.path.join(bbox, "samplers"))
    rs = imp("mmdet.core.bbox.samplers.random_sampler")
    _pkg("mmdet.core.bbox.coder", os.path.join(bbox, "coder"))
    cd = imp("mmdet.core.bbox.coder.delta_xywh_bbox_coder")
    for k in ("build_anchor_generator", "build_assigner", "build_bbox_coder", "build_sampler", "multiclass_nms"):
        setattr(core, k, None)
    core.anchor_inside_flags = autils.anchor_inside_flags
    core.images_to_levels = autils.images_to_levels
    core.multi_apply = misc.multi_apply
    core.unmap = misc.unmap
    _pkg("mmdet.models")
    _pkg("mmdet.models.builder", HEADS=_Registry(), build_loss=None)
    _pkg("mmdet.models.losses", accuracy=None)
    _pkg("mmdet.models.utils", build_linear_layer=None)
    _pkg("mmdet.models.dense_heads", os.path.join(mm, "models", "dense_heads"))
    _pkg("mmdet.models.dense_heads.dense_test_mixins", BBoxTestMixin=type("BBoxTestMixin", (), {}))
    ah = imp("mmdet.models.dense_heads.anchor_head")
    _pkg("mmdet.models.roi_heads")
    _pkg("mmdet.models.roi_heads.bbox_heads", os.path.join(mm, "models", "roi_heads", "bbox_heads"))
    bh = imp("mmdet.models.roi_heads.bbox_heads.bbox_head")
    return types.SimpleNamespace(AssignResult=ar.AssignResult, RandomSampler=rs.RandomSampler, Coder=cd.DeltaXYWHBBoxCoder,
                                 bbox2delta=cd.bbox2delta, delta2bbox=cd.delta2bbox, inside_flags=autils.anchor_inside_flags,
                                 AnchorHead=ah.AnchorHead, BBoxHead=bh.BBoxHead)


class PermRecorder:
    """Wraps torch.randperm while active; ``perms`` holds what it returned, in call order."""

    def __enter__(self):
        self.perms = []
        self._orig = torch.randperm

        def randperm(n, *a, **kw):
            p = self._orig(n, *a, **kw)
            self.perms.append(p.numpy().copy())
            return p
        torch.randperm = randperm
        return self

    def __exit__(self, *exc):
        torch.randperm = self._orig

    def by_class(self, n_pos, n_neg, num, frac, n_pos_kept):
        """{0: perm over the positives or None, 1: over the negatives or None} from the order of the draws."""
        q = list(self.perms)
        out = {0: None, 1: None}
        if n_pos > int(num * frac):
            out[0] = q.pop(0)
            assert out[0].size == n_pos
        if q:
            out[1] = q.pop(0)
            assert out[1].size == n_neg
        assert not q
        return out


def next_path():
    nums = [int(m.group(1)) for f in glob.glob(os.path.join(HERE, "g*_*")) for m in [re.match(r"g(\d+)_", os.path.basename(f))] if m]
    mine = glob.glob(os.path.join(HERE, "g*_targets.npz"))
    if mine:
        return mine[0]                               # regenerate in place
    return os.path.join(HERE, "g%d_targets.npz" % (max(nums) + 1))


def same_bits(a, b):
    return np.array_equal(tc.bits(a), tc.bits(b))


def run_sampler(R, gi, bboxes, gts, gt_labels, cand_labels, num, frac, ub, add_gt, salt):
    """The reference's sample() -> (SamplingResult, ranks, keys, gt_inds after add_gt)."""
    asr = R.AssignResult(gts.shape[0], T(gi.copy()), torch.zeros(gi.size), None if cand_labels is None else T(cand_labels.copy()))
    smp = R.RandomSampler(num, frac, neg_pos_ub=ub, add_gt_as_proposals=add_gt)
    with PermRecorder() as rec:
        res = smp.sample(asr, T(bboxes.copy()), T(gts.copy()), None if gt_labels is None else T(gt_labels.copy()))
    gi2 = asr.gt_inds.numpy().copy()
    perms = rec.by_class(int((gi2 > 0).sum()), int((gi2 == 0).sum()), num, frac, res.pos_inds.numel())
    ranks = tc.ranks_from_perms(gi2, perms)
    keys = tc.keys_from_ranks(gi2, ranks, salt)
    pos, neg = tc.sample_np(gi2, keys, num, frac, ub)
    assert np.array_equal(pos, res.pos_inds.numpy()) and np.array_equal(neg, res.neg_inds.numpy()), "selection rule != reference"
    return res, ranks, keys, gi2


def main():
    R = reference(sys.argv[1])
    torch.manual_seed(20261018)
    out = dict(tc.input_checksums())

    # ---- sampler
    for name, (N, P, I, num, frac, ub, front) in tc.SAMPLER_CASES.items():
        gi = tc.sampler_gt_inds(name)
        n = gi.size
        salt = tc.key_salt("s", name)
        bboxes = np.zeros((n, 4), dtype=np.float32)
        bboxes[:, 0] = np.arange(n)
        gts = np.zeros((tc.G_DEFAULT, 4), dtype=np.float32)
        labs = np.arange(tc.G_DEFAULT, dtype=np.int64)
        res, ranks, keys, gi2 = run_sampler(R, gi, bboxes, gts, labs if front else None, None, num, frac, ub, bool(front), salt)
        assert gi2.size == N and (gi2 > 0).sum() == P and (gi2 < 0).sum() == I
        pos, neg = res.pos_inds.numpy(), res.neg_inds.numpy()
        # SamplingResult's other fields are plain gathers of the index lists
        allb = np.concatenate([gts, bboxes]) if front else bboxes
        assert np.array_equal(res.pos_bboxes.numpy(), allb[pos]) and np.array_equal(res.neg_bboxes.numpy(), allb[neg])
        assert np.array_equal(res.pos_is_gt.numpy(), (pos < front).astype(np.uint8)) and res.num_gts == tc.G_DEFAULT
        assert np.array_equal(res.pos_assigned_gt_inds.numpy(), gi2[pos] - 1)
        assert np.array_equal(res.pos_gt_bboxes.numpy(), gts[gi2[pos] - 1]) and np.array_equal(res.bboxes.numpy(), allb[np.concatenate([pos, neg])])
        out["s_%s_rank0" % name], out["s_%s_rank1" % name] = ranks[0], ranks[1]
        out["s_%s_pos" % name] = pos.astype(np.int32)
        out["s_%s_neg" % name] = neg.astype(np.int32)
        print("sampler %-9s N %6d: %4d of %4d positives, %4d of %6d negatives" % (name, N, pos.size, P, neg.size, (gi2 == 0).sum()))

    # ---- coder
    worst = {"enc": 0.0, "dec": 0.0, "enc_np": 0.0, "dec_np": 0.0}
    pending = []
    for name, (n, means, stds) in tc.ENCODE_CASES.items():
        p5, g = tc.encode_inputs(name)
        ref = R.bbox2delta(T(p5[:, :4].copy()), T(g.copy()), means, stds).numpy()
        assert same_bits(ref, R.Coder(means, stds).encode(T(p5[:, :4].copy()), T(g.copy())).numpy())
        exact, kinds, err = tc.encode_check(ref, p5[:, :4], g, means, stds)
        assert exact and kinds, name
        worst["enc"] = max(worst["enc"], err)
        mine = tc.bbox2delta_np(p5[:, :4], g, means, stds)
        pending.append(("enc", name, same_bits(ref, mine), tc.encode_check(mine, p5[:, :4], g, means, stds)))
        if n <= 65:
            out["e_%s_out" % name] = ref
        else:
            out["e_%s_head" % name] = ref[:16]
            out["e_%s_xy_bitsum" % name] = tc.bit_sum(ref[:, :2][np.isfinite(ref[:, :2])])
            out["e_%s_kinds" % name] = tc._kind(ref).astype(np.int8)
    for name, (n, K, means, stds, max_shape, clip_border, ctr, ctr_clamp) in tc.DECODE_CASES.items():
        rois, d = tc.decode_inputs(name)
        args = (means, stds, max_shape, tc.WH_RATIO_CLIP, clip_border, ctr, ctr_clamp)
        ref = R.delta2bbox(T(rois.copy()), T(d.copy()), *args).numpy()
        assert same_bits(ref, R.Coder(means, stds, clip_border, ctr, ctr_clamp).decode(T(rois.copy()), T(d.copy()), max_shape, tc.WH_RATIO_CLIP).numpy())
        ok, kinds, err = tc.decode_check(ref, rois, d, *args)
        assert ok and kinds, name
        worst["dec"] = max(worst["dec"], err)
        mine = tc.delta2bbox_np(rois, d, *args)
        pending.append(("dec", name, same_bits(ref, mine), tc.decode_check(mine, rois, d, *args)))
        gx, gy, pw, ph, dw, dh = tc.decode_parts_np(rois, d, means, stds, tc.WH_RATIO_CLIP, ctr, ctr_clamp)
        mr = np.float32(np.abs(np.log(tc.WH_RATIO_CLIP)))
        hits = (int((dw == mr).sum() + (dh == mr).sum()), int((dw == -mr).sum() + (dh == -mr).sum()))
        if n >= 63:
            assert hits[0] > 0 and (ctr or hits[1] > 0), (name, hits)
        if n * K <= 65 * 3:
            out["d_%s_out" % name] = ref
        else:
            out["d_%s_head" % name] = ref[:16]
        out["d_%s_clipped" % name] = np.array([int((ref == 0).sum()), int(sum((ref[:, i::2] == m).sum() for i, m in ((0, 1333.0), (1, 800.0))))])
    for kind, name, bitwise, (ok, kinds, err) in pending:
        assert ok and kinds, (kind, name)
        worst[kind + "_np"] = max(worst[kind + "_np"], err)
        assert bitwise or err <= 2 * worst[kind], (kind, name, err, worst[kind])
    out["coder_ref_ulps"] = np.array([worst["enc"], worst["dec"]], dtype=np.float64)
    print("coder: the reference's own maximum error against the float64 continuation: encode %.4f ulp, decode %.4f ulp "
          "(numpy's restatement: %.4f, %.4f)" % (worst["enc"], worst["dec"], worst["enc_np"], worst["dec_np"]))

    # ---- anchor targets
    anchors, gts, glab, gi_full, inside = tc.anchor_inputs()
    num, frac, ub = tc.ANCHOR_SAMPLER
    for name, (with_labels, pos_weight, decoded, masked, means, stds) in tc.ANCHOR_CASES.items():
        salt = tc.key_salt("a", name)
        border = 0 if masked else -1
        valid = torch.ones(tc.A_TARGETS, dtype=torch.bool)
        ins = R.inside_flags(T(anchors.copy()), valid, tc.IMG_SHAPE, border).numpy()
        if masked:
            assert np.array_equal(ins, inside) and 0 < inside.sum() < tc.A_TARGETS
        gi = gi_full[ins]

        class Assigner:
            def assign(self, a, g, gi_ignore, labels):
                assert a.shape[0] == gi.size and labels is None
                return R.AssignResult(g.shape[0], T(gi.copy()), torch.zeros(gi.size), None)
        me = types.SimpleNamespace(train_cfg=types.SimpleNamespace(allowed_border=border, pos_weight=pos_weight), assigner=Assigner(),
                                   sampler=R.RandomSampler(num, frac, neg_pos_ub=ub, add_gt_as_proposals=False), sampling=True,
                                   num_classes=tc.ANCHOR_CLASSES, reg_decoded_bbox=decoded, bbox_coder=R.Coder(means, stds))
        with PermRecorder() as rec:
            labels, lw, bt, bw, pos_t, neg_t, sres = R.AnchorHead._get_targets_single(
                me, T(anchors.copy()), valid, T(gts.copy()), None, T(glab.copy()) if with_labels else None,
                dict(img_shape=tc.IMG_SHAPE + (3,)))
        perms = rec.by_class(int((gi > 0).sum()), int((gi == 0).sum()), num, frac, pos_t.numel())
        ranks = tc.ranks_from_perms(gi, perms)
        keys = tc.keys_from_ranks(gi, ranks, salt)
        n_lab, n_lw, n_bt, n_bw, pos, neg = tc.anchor_targets_np(anchors, gts, glab if with_labels else None, gi_full, keys,
                                                                 ins if masked else None, tc.ANCHOR_CLASSES, pos_weight, decoded, means, stds)
        assert np.array_equal(pos, pos_t.numpy()) and np.array_equal(neg, neg_t.numpy()), name
        assert np.array_equal(n_lab, labels.numpy()) and same_bits(n_lw, lw.numpy()) and same_bits(n_bw, bw.numpy()), name
        bt = bt.numpy()
        assert same_bits(n_bt[:, :2], bt[:, :2]), name
        if not same_bits(n_bt, bt):
            sel = np.nonzero(ins)[0][pos]
            e = tc.encode_check(n_bt[sel], anchors[sel], gts[gi[pos] - 1], means, stds)
            assert e[0] and e[1] and e[2] <= 2 * worst["enc"], (name, e)
        sel = np.nonzero(ins)[0][pos]
        out["a_%s_rank0" % name], out["a_%s_rank1" % name] = ranks[0], ranks[1]
        out["a_%s_pos" % name] = pos.astype(np.int32)
        out["a_%s_neg" % name] = neg.astype(np.int32)
        out["a_%s_labels_pos" % name] = labels.numpy()[sel].astype(np.int32)
        out["a_%s_bt_pos" % name] = bt[sel]
        out["a_%s_sums" % name] = np.array([tc.bit_sum(lw.numpy()), tc.bit_sum(bw.numpy()), np.uint64(labels.numpy().sum())], dtype=np.uint64)
        print("anchor targets %-9s: %d anchors take part, %d positives, %d negatives" % (name, gi.size, pos.size, neg.size))

    # ---- RoI targets
    for name, (case, means, stds, pos_weight) in tc.ROI_CASES.items():
        b, g, lab, gi, cand_lab, (num, frac, ub, front) = tc.roi_inputs(name)
        salt = tc.key_salt("r", name)
        res, ranks, keys, gi2 = run_sampler(R, gi, b, g, lab, cand_lab, num, frac, ub, bool(front), salt)
        me = types.SimpleNamespace(num_classes=tc.ROI_CLASSES, reg_decoded_bbox=False, bbox_coder=R.Coder(means, stds))
        labels, lw, bt, bw = R.BBoxHead._get_target_single(me, res.pos_bboxes, res.neg_bboxes, res.pos_gt_bboxes, res.pos_gt_labels,
                                                           types.SimpleNamespace(pos_weight=pos_weight))
        pos, neg = res.pos_inds.numpy(), res.neg_inds.numpy()
        allb = np.concatenate([g, b]) if front else b
        alll = np.concatenate([lab, cand_lab]) if front else cand_lab
        n_rois, n_lab, n_lw, n_bt, n_bw, n_pg = tc.roi_targets_np(allb, g, gi2, alll, pos, neg, num, tc.ROI_CLASSES, pos_weight, means, stds)
        k = pos.size + neg.size
        assert np.array_equal(n_lab[:k], labels.numpy()) and same_bits(n_lw[:k], lw.numpy()) and same_bits(n_bw[:k], bw.numpy()), name
        assert same_bits(n_rois[:k, 1:], res.bboxes.numpy()) and np.array_equal(n_pg[:pos.size], res.pos_assigned_gt_inds.numpy())
        bt = bt.numpy()
        assert same_bits(n_bt[:k, :2], bt[:, :2]), name
        if not same_bits(n_bt[:k], bt):
            e = tc.encode_check(n_bt[:pos.size], allb[pos], g[gi2[pos] - 1], means, stds)
            assert e[0] and e[1] and e[2] <= 2 * worst["enc"], (name, e)
        assert (name == "nopos") == (pos.size == 0)
        out["r_%s_rank0" % name], out["r_%s_rank1" % name] = ranks[0], ranks[1]
        out["r_%s_pos" % name] = pos.astype(np.int32)
        out["r_%s_neg" % name] = neg.astype(np.int32)
        out["r_%s_labels" % name] = labels.numpy().astype(np.int32)
        out["r_%s_lw" % name] = lw.numpy()
        out["r_%s_bt_pos" % name] = bt[:pos.size]
        print("roi targets %-6s: %d positives, %d negatives of %d rows" % (name, pos.size, neg.size, num))

    path = next_path()
    np.savez_compressed(path, **out)
    print("wrote %s: %.1f KB" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
