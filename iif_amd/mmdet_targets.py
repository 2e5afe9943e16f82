"""mmdet's ``RandomSampler``, ``DeltaXYWHBBoxCoder`` and the two target builders on the gfx950 kernels (csrc/targets.hip):
the steps between ``MaxIoUAssigner`` (mmdet_assigner.py) and the losses.

Mirror of instance_segmentation/mmdet/core/bbox/samplers/base_sampler.py:9-102, random_sampler.py:8-82, sampling_result.py:7-55,
core/bbox/coder/delta_xywh_bbox_coder.py:11-272, core/anchor/utils.py:21-47, dense_heads/anchor_head.py:172-268 and
roi_heads/bbox_heads/bbox_head.py:122-261 (constructors, attributes, assertions, empty-input results).

  * ``bbox2delta`` / ``delta2bbox`` / ``DeltaXYWHBBoxCoder``: ``iif_bbox2delta`` / ``iif_delta2bbox``, one launch each.
  * ``RandomSampler``: ``iif_random_sample``.  ``sample_padded`` gives fixed-shape index lists, device counts and dense flags
    in four enqueued operations (the key draw and the entry's three) without a host synchronisation; ``sample`` gives the
    reference's ``SamplingResult`` at the cost of ONE host read (the two counts).
  * ``anchor_targets_single``: assign, sample, ``iif_anchor_targets``; without a mask it never synchronises.
  * ``bbox_targets``: ``BBoxHead.get_targets`` on padded samplings (``iif_roi_targets``, no synchronisation, ``rois``
    included) or on ``SamplingResult``s (exact sizes).

Deliberately not offered: ``PseudoSampler``, OHEM and the other samplers; batch dimensions and a tensor-valued ``max_shape``
in the coder; a mask inside the assigner itself (``MaxIoUAssigner.assign`` still takes none: the synchronisation-free masked RPN
path is ``mmdet_rpn_stage.rpn_stage_targets``, whose own assignment passes carry the mask for all images at once, while
``anchor_targets_single`` stays the per-image chain); the ONNX export branches.  When mmdet is importable the classes register themselves as ``RandomSampler`` / ``DeltaXYWHBBoxCoder``.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .mmdet_assigner import _boxes


def _f4(v, what):
    v = tuple(float(x) for x in v)
    if len(v) != 4:
        raise AssertionError("%s: four values expected (got %d)" % (what, len(v)))
    return (ctypes.c_float * 4)(*v)


# ------------------------------------------------------------------------------------------------------------ coder
def bbox2delta(proposals, gt, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """delta_xywh_bbox_coder.py:98-141 for float32 ``[n, 4]`` boxes (``[n, 5]`` rows are read in place): ``[n, 4]`` deltas.
    ``dx, dy`` are the reference's float32 numbers bit for bit, ``dw, dh`` up to the rounding of ``log``."""
    assert proposals.size(0) == gt.size(0)
    means, stds = _f4(means, "means"), _f4(stds, "stds")
    p, n, ldp = _boxes(proposals, "proposals")
    g, _, ldg = _boxes(gt, "gt")
    _lib.require_gpu(proposals, gt)
    out = torch.empty((n, 4), dtype=torch.float32, device=proposals.device)
    if n == 0:
        return out
    rc = _lib.lib().iif_bbox2delta(_lib.ptr(p), ldp, _lib.ptr(g), ldg, n, means, stds, _lib.ptr(out),
                                   _lib.stream_ptr())
    _lib.check(rc, "iif_bbox2delta")
    return out


def delta2bbox(rois, deltas, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), max_shape=None, wh_ratio_clip=16 / 1000,
               clip_border=True, add_ctr_clamp=False, ctr_clamp=32):
    """delta_xywh_bbox_coder.py:144-272 for ``rois [n, 4]`` and ``deltas [n, 4 K]`` (float32): ``[n, 4 K]`` boxes.
    ``max_shape`` is a sequence ``(H, W[, C])`` or None; batch dimensions and a tensor ``max_shape`` are not offered."""
    if isinstance(max_shape, torch.Tensor):
        raise NotImplementedError("delta2bbox: a tensor-valued max_shape is not offered; pass (H, W)")
    if deltas.dim() != 2:
        raise NotImplementedError("delta2bbox: [n, 4 K] deltas only, no batch dimensions (got %s)" % (tuple(deltas.shape),))
    if deltas.dtype != torch.float32:
        raise NotImplementedError("delta2bbox: float32 deltas only (got %s)" % deltas.dtype)
    if deltas.requires_grad:
        raise RuntimeError("delta2bbox: the native coder has no autograd; detach the deltas")
    means, stds = _f4(means, "means"), _f4(stds, "stds")
    r, n, ldr = _boxes(rois, "rois")
    assert deltas.size(0) == n
    assert deltas.size(1) % 4 == 0
    K = deltas.size(1) // 4
    _lib.require_gpu(rois, deltas)
    out = torch.empty((n, 4 * K), dtype=torch.float32, device=deltas.device)
    if n == 0 or K == 0:
        return out
    d = deltas if deltas.stride(1) == 1 and (n == 1 or deltas.stride(0) >= 4 * K) else deltas.contiguous()
    ldd = d.stride(0) if n > 1 else 4 * K
    max_ratio = float(np.abs(np.log(wh_ratio_clip)))
    clip = bool(clip_border) and max_shape is not None
    mh, mw = (float(max_shape[0]), float(max_shape[1])) if clip else (0.0, 0.0)
    rc = _lib.lib().iif_delta2bbox(_lib.ptr(r), ldr, _lib.ptr(d), ldd, n, K, means, stds, max_ratio,
                                   int(bool(add_ctr_clamp)), float(ctr_clamp), int(clip), mh, mw, _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "iif_delta2bbox")
    return out


class DeltaXYWHBBoxCoder:
    """delta_xywh_bbox_coder.py:11-95: the reference's arguments, defaults and attribute names."""

    def __init__(self, target_means=(0., 0., 0., 0.), target_stds=(1., 1., 1., 1.), clip_border=True, add_ctr_clamp=False,
                 ctr_clamp=32):
        self.means = target_means
        self.stds = target_stds
        self.clip_border = clip_border
        self.add_ctr_clamp = add_ctr_clamp
        self.ctr_clamp = ctr_clamp

    def encode(self, bboxes, gt_bboxes):
        assert bboxes.size(0) == gt_bboxes.size(0)
        assert bboxes.size(-1) == gt_bboxes.size(-1) == 4
        return bbox2delta(bboxes, gt_bboxes, self.means, self.stds)

    def decode(self, bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000):
        assert pred_bboxes.size(0) == bboxes.size(0)
        if pred_bboxes.ndim == 3:
            raise NotImplementedError("DeltaXYWHBBoxCoder.decode: batch dimensions are not offered on the native path")
        return delta2bbox(bboxes, pred_bboxes, self.means, self.stds, max_shape, wh_ratio_clip, self.clip_border,
                          self.add_ctr_clamp, self.ctr_clamp)


# ------------------------------------------------------------------------------------------------------------ sampler
class SamplingResult:
    """The fields of sampling_result.py:26-55 at their exact sizes: ``pos_inds``, ``neg_inds``, ``pos_bboxes``, ``neg_bboxes``,
    ``pos_is_gt``, ``num_gts``, ``pos_assigned_gt_inds``, ``pos_gt_bboxes``, ``pos_gt_labels`` (None without assigned labels)
    and the property ``bboxes``.  Every field but the index lists is a gather through them."""

    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags):
        gts = gt_bboxes.reshape(-1, 4)
        labels = assign_result.labels
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.num_gts = gt_bboxes.shape[0]
        self.pos_bboxes, self.neg_bboxes = bboxes.index_select(0, pos_inds), bboxes.index_select(0, neg_inds)
        self.pos_is_gt = gt_flags.index_select(0, pos_inds)
        self.pos_assigned_gt_inds = assign_result.gt_inds.index_select(0, pos_inds) - 1
        # no ground truth: no positives either (the reference asserts it), and nothing to index
        self.pos_gt_bboxes = gts.index_select(0, self.pos_assigned_gt_inds) if gts.numel() else gts.new_empty((0, 4))
        self.pos_gt_labels = None if labels is None else labels.index_select(0, pos_inds)

    @property
    def bboxes(self):
        """Positive boxes, then negative boxes."""
        return torch.cat([self.pos_bboxes, self.neg_bboxes], dim=0)


class PaddedSampling:
    """What ``RandomSampler.sample_padded`` returns; every tensor lives on the device and has a shape known in advance.

    ``pos_inds [num_expected_pos]`` / ``neg_inds [num]``: the sampled candidates, ascending, unused tails -1;
    ``counts [2]``: how many of each; ``flags [N]`` int8: 0 not sampled, 1 positive, 2 negative.  ``bboxes`` (with the
    ground-truth boxes in front under ``add_gt_as_proposals``), ``gt_bboxes``, ``assign_result`` and ``gt_flags`` are what the
    reference hands to ``SamplingResult``."""

    def __init__(self, pos_inds, neg_inds, counts, flags, bboxes, gt_bboxes, assign_result, gt_flags, num):
        self.pos_inds, self.neg_inds, self.counts, self.flags = pos_inds, neg_inds, counts, flags
        self.bboxes, self.gt_bboxes, self.assign_result, self.gt_flags = bboxes, gt_bboxes, assign_result, gt_flags
        self.num = num
        self.num_gts = gt_bboxes.shape[0]


class RandomSampler:
    """base_sampler.py:12-23 + random_sampler.py:21-30: ``num``, ``pos_fraction``, ``neg_pos_ub``, ``add_gt_as_proposals``.

    The sample is drawn on the device: one int32 key per candidate from torch's DEVICE generator (``torch.manual_seed``
    governs it), and a class that has more members than its budget keeps the members with the smallest ``(key, index)``
    pairs.  That is a uniform sample without replacement, but it CANNOT reproduce the reference's CPU ``torch.randperm`` stream
    for a given seed.  Equal int32 keys go to the lower index: at N = 268 569 a draw holds a handful of tied pairs (N^2 / 2^32
    on average), which tilts those pairs, and nothing else, towards the lower index.  ``rng`` is accepted and unused."""

    def __init__(self, num, pos_fraction, neg_pos_ub=-1, add_gt_as_proposals=True, **kwargs):
        self.num = num
        self.pos_fraction = pos_fraction
        self.neg_pos_ub = neg_pos_ub
        self.add_gt_as_proposals = add_gt_as_proposals
        self.pos_sampler = self
        self.neg_sampler = self

    def sample_padded(self, assign_result, bboxes, gt_bboxes, gt_labels=None, keys=None):
        """base_sampler.py:68-98 without a host synchronisation: a ``PaddedSampling``.  ``keys``: int32 ``[N]`` >= 0 on the
        device (N counts the ground-truth boxes in front under ``add_gt_as_proposals``), or None to draw them."""
        if len(bboxes.shape) < 2:
            bboxes = bboxes[None, :]
        bboxes = bboxes[:, :4]
        _lib.require_gpu(bboxes, gt_bboxes, gt_labels, assign_result.gt_inds, keys)
        dev = bboxes.device
        gt_flags = bboxes.new_zeros((bboxes.shape[0],), dtype=torch.uint8)
        if self.add_gt_as_proposals and len(gt_bboxes) > 0:
            if gt_labels is None:
                raise ValueError("gt_labels must be given when add_gt_as_proposals is True")
            bboxes = torch.cat([gt_bboxes, bboxes], dim=0)
            assign_result.add_gt_(gt_labels)
            gt_ones = bboxes.new_ones(gt_bboxes.shape[0], dtype=torch.uint8)
            gt_flags = torch.cat([gt_ones, gt_flags])
        gt_inds = assign_result.gt_inds
        if gt_inds.dtype != torch.int64 or not gt_inds.is_contiguous():
            gt_inds = gt_inds.to(torch.int64).contiguous()
        N = gt_inds.numel()
        assert N == bboxes.shape[0]
        num = int(self.num)
        num_expected_pos = int(self.num * self.pos_fraction)
        assert 0 <= num_expected_pos <= num
        if keys is None:
            keys = torch.randint(0, 2 ** 31, (N,), dtype=torch.int32, device=dev)
        else:
            if keys.dtype != torch.int32 or keys.numel() != N:
                raise ValueError("keys: one int32 per candidate expected (%d candidates, got %s %s)" % (N, keys.dtype, tuple(keys.shape)))
            keys = keys.contiguous()
        pos_inds = torch.empty((num_expected_pos,), dtype=torch.int64, device=dev)
        neg_inds = torch.empty((num,), dtype=torch.int64, device=dev)
        counts = torch.empty((2,), dtype=torch.int64, device=dev)
        flags = torch.empty((N,), dtype=torch.int8, device=dev)
        ws_bytes = 4 * N + 65536
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)                      # this call's own
        rc = _lib.lib().iif_random_sample(_lib.ptr(gt_inds), _lib.ptr(keys), N, num_expected_pos, num, float(self.neg_pos_ub),
                                          _lib.ptr(pos_inds), _lib.ptr(neg_inds), _lib.ptr(counts), _lib.ptr(flags),
                                          _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
        _lib.check(rc, "iif_random_sample")
        return PaddedSampling(pos_inds, neg_inds, counts, flags, bboxes, gt_bboxes, assign_result, gt_flags, num)

    def sample(self, assign_result, bboxes, gt_bboxes, gt_labels=None, keys=None, **kwargs):
        """base_sampler.py:35-102: the reference's ``SamplingResult``.  One host read (the two counts), no other
        synchronisation."""
        p = self.sample_padded(assign_result, bboxes, gt_bboxes, gt_labels, keys=keys)
        n_pos, n_neg = p.counts.tolist()
        return SamplingResult(p.pos_inds[:n_pos], p.neg_inds[:n_neg], p.bboxes, gt_bboxes, assign_result, p.gt_flags)


# ------------------------------------------------------------------------------------------------------------ targets
def anchor_inside_flags(flat_anchors, valid_flags, img_shape, allowed_border=0):
    """core/anchor/utils.py:21-47: ``valid_flags`` and "the anchor lies within ``allowed_border`` pixels of the image";
    a negative border checks nothing and returns ``valid_flags`` itself."""
    if allowed_border < 0:
        return valid_flags
    img_h, img_w = img_shape[:2]
    x1, y1, x2, y2 = flat_anchors[:, :4].unbind(dim=1)
    inside = (x1 >= -allowed_border) & (y1 >= -allowed_border) & (x2 < img_w + allowed_border) & (y2 < img_h + allowed_border)
    return valid_flags & inside


def _coder_norm(coder):
    return _f4(coder.means, "target_means"), _f4(coder.stds, "target_stds")


def anchor_targets_single(flat_anchors, gt_bboxes, gt_bboxes_ignore, gt_labels, assigner, sampler, coder, num_classes,
                          pos_weight=-1, inside_flags=None, reg_decoded_bbox=False):
    """anchor_head.py:210-268 with ``unmap_outputs=True``: ``(labels [A], label_weights [A], bbox_targets [A, 4],
    bbox_weights [A, 4], counts [2])``, all on the device; ``counts`` holds the sampled positives and negatives.

    ``gt_labels`` None is the RPN (positives get label 0, the assigner sees no labels: the reference's ``self.sampling``
    branch).  ``inside_flags`` None: every anchor takes part (``allowed_border=-1`` with all flags valid, which the caller
    knows from integers) and nothing synchronises the host.  With a mask the anchors are compacted with torch indexing - one
    synchronisation, as in the reference - and the kernel unmaps through an index; a mask without a set flag returns
    ``(None,) * 5`` (:213-214).  The sampler must not add the ground truth as proposals (the reference's anchor heads
    configure ``add_gt_as_proposals=False``)."""
    a, A, lda = _boxes(flat_anchors, "flat_anchors")
    g, G, ldg = _boxes(gt_bboxes, "gt_bboxes")
    _lib.require_gpu(flat_anchors, gt_bboxes, gt_labels, inside_flags)
    if sampler.add_gt_as_proposals:
        raise ValueError("anchor_targets_single: the sampler must have add_gt_as_proposals=False")
    dev = flat_anchors.device
    compact = None
    anchors = flat_anchors
    if inside_flags is not None:
        inside = inside_flags.type(torch.bool)
        anchors = flat_anchors[inside, :]                                       # the synchronisation
        if anchors.shape[0] == 0:
            return (None,) * 5
        compact = torch.cumsum(inside, 0) - 1
        compact = torch.where(inside, compact, torch.full_like(compact, -1))
    assign_result = assigner.assign(anchors, gt_bboxes, gt_bboxes_ignore, None)
    p = sampler.sample_padded(assign_result, anchors, gt_bboxes)
    lab = None if gt_labels is None else gt_labels.reshape(-1).to(torch.int64).contiguous()
    labels = torch.empty((A,), dtype=torch.int64, device=dev)
    label_weights = torch.empty((A,), dtype=torch.float32, device=dev)
    bbox_targets = torch.empty((A, 4), dtype=torch.float32, device=dev)
    bbox_weights = torch.empty((A, 4), dtype=torch.float32, device=dev)
    if A == 0:
        return labels, label_weights, bbox_targets, bbox_weights, p.counts
    means, stds = _coder_norm(coder)
    gt_inds = p.assign_result.gt_inds
    rc = _lib.lib().iif_anchor_targets(_lib.ptr(a), lda, A, _lib.ptr(p.flags), _lib.ptr(gt_inds), gt_inds.numel(), _lib.ptr(g), ldg, G,
                                       _lib.ptr(lab), _lib.ptr(compact), int(num_classes), float(pos_weight),
                                       int(bool(reg_decoded_bbox)), means, stds, _lib.ptr(labels), _lib.ptr(label_weights),
                                       _lib.ptr(bbox_targets), _lib.ptr(bbox_weights), _lib.stream_ptr())
    _lib.check(rc, "iif_anchor_targets")
    return labels, label_weights, bbox_targets, bbox_weights, p.counts


def _roi_targets_padded(p, gt_bboxes, img_index, coder, num_classes, pos_weight, reg_decoded_bbox):
    b, N, ldb = _boxes(p.bboxes, "bboxes")
    g, G, ldg = _boxes(gt_bboxes, "gt_bboxes")
    dev = p.bboxes.device
    cap = int(p.num)
    rois = torch.empty((cap, 5), dtype=torch.float32, device=dev)
    labels = torch.empty((cap,), dtype=torch.int64, device=dev)
    label_weights = torch.empty((cap,), dtype=torch.float32, device=dev)
    bbox_targets = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    bbox_weights = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    pos_gt = torch.empty((cap,), dtype=torch.int64, device=dev)
    if cap:
        means, stds = _coder_norm(coder)
        lab = p.assign_result.labels
        if lab is not None:
            lab = lab.to(torch.int64).contiguous()
        gt_inds = p.assign_result.gt_inds.to(torch.int64).contiguous()
        rc = _lib.lib().iif_roi_targets(_lib.ptr(b), ldb, N, _lib.ptr(gt_inds), _lib.ptr(lab), _lib.ptr(g), ldg, G,
                                        _lib.ptr(p.pos_inds), _lib.ptr(p.neg_inds), _lib.ptr(p.counts), cap, p.pos_inds.numel(),
                                        int(img_index), int(num_classes), float(pos_weight), int(bool(reg_decoded_bbox)), means,
                                        stds, _lib.ptr(rois), _lib.ptr(labels), _lib.ptr(label_weights), _lib.ptr(bbox_targets),
                                        _lib.ptr(bbox_weights), _lib.ptr(pos_gt), _lib.stream_ptr())
        _lib.check(rc, "iif_roi_targets")
    return rois, labels, label_weights, bbox_targets, bbox_weights, pos_gt


def _roi_targets_exact(res, coder, num_classes, pos_weight, reg_decoded_bbox):
    """bbox_head.py:155-186 on a ``SamplingResult``: positives first, then negatives; the encode is the native one."""
    pos, neg = res.pos_bboxes, res.neg_bboxes
    num_pos, num_neg = pos.size(0), neg.size(0)
    labels = pos.new_full((num_pos + num_neg,), num_classes, dtype=torch.long)
    targets = pos.new_zeros((num_pos + num_neg, 4))
    if num_pos > 0:
        labels[:num_pos] = res.pos_gt_labels
        targets[:num_pos] = res.pos_gt_bboxes if reg_decoded_bbox else coder.encode(pos, res.pos_gt_bboxes)
    label_weights = torch.cat([pos.new_full((num_pos,), 1.0 if pos_weight <= 0 else pos_weight), pos.new_ones((num_neg,))])
    bbox_weights = torch.cat([pos.new_ones((num_pos, 4)), pos.new_zeros((num_neg, 4))])
    return labels, label_weights, targets, bbox_weights


def bbox_targets(samplings, gt_bboxes_list, gt_labels_list, coder, num_classes, pos_weight=-1, reg_decoded_bbox=False,
                 concat=True):
    """bbox_head.py:188-261 (``BBoxHead.get_targets``): ``(labels, label_weights, bbox_targets, bbox_weights)``.

    ``samplings`` are ``PaddedSampling``s - one launch per image, no host synchronisation, every image contributes
    ``sampler.num`` rows (padding rows: zero box, background label, zero weights) and the tuple ends with ``rois [.., 5]``
    (``bbox2roi`` of the same rows) and ``pos_assigned_gt_inds`` - or ``SamplingResult``s, for the reference's exact sizes.
    ``gt_labels_list`` is accepted for the reference's signature; the labels come from the assignment, as there."""
    assert len(samplings) == len(gt_bboxes_list)
    padded = [isinstance(s, PaddedSampling) for s in samplings]
    if any(padded) and not all(padded):
        raise ValueError("bbox_targets: padded samplings and SamplingResults cannot be mixed")
    if all(padded) and samplings:
        cols = [_roi_targets_padded(s, g, i, coder, num_classes, pos_weight, reg_decoded_bbox)
                for i, (s, g) in enumerate(zip(samplings, gt_bboxes_list))]
        rois, labels, label_weights, targets, weights, pos_gt = (list(c) for c in zip(*cols))
        out = [labels, label_weights, targets, weights, rois, pos_gt]
    else:
        cols = [_roi_targets_exact(s, coder, num_classes, pos_weight, reg_decoded_bbox) for s in samplings]
        out = [list(c) for c in zip(*cols)] if cols else [[], [], [], []]
    if concat:
        out = [torch.cat(c, 0) for c in out]
    return tuple(out)


def register_into_mmdet():
    """Register the native classes as mmdet's ``RandomSampler`` / ``DeltaXYWHBBoxCoder`` if mmdet is importable."""
    try:
        from mmdet.core.bbox.builder import BBOX_CODERS, BBOX_SAMPLERS
    except Exception:
        return False
    BBOX_SAMPLERS.register_module(name="RandomSampler", force=True, module=RandomSampler)
    BBOX_CODERS.register_module(name="DeltaXYWHBBoxCoder", force=True, module=DeltaXYWHBBoxCoder)
    return True


register_into_mmdet()
