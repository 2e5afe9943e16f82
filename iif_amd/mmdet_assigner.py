"""mmdet's ``MaxIoUAssigner`` and ``bbox_overlaps`` / ``BboxOverlaps2D`` on the gfx950 kernels (csrc/assign.hip).

Mirror of instance_segmentation/mmdet/core/bbox/assigners/max_iou_assigner.py:10-213, assigners/assign_result.py and
iou_calculators/iou2d_calculator.py:22-261 (constructors, attributes, signatures, empty-input results).

  * ``bbox_overlaps`` / ``BboxOverlaps2D``: ``iif_bbox_overlaps``, one launch; 'iou' / 'iof' / 'giou', pairwise or aligned,
    4- or 5-column float32 boxes read in place.  The reference's float32 numbers bit for bit.
  * ``MaxIoUAssigner.assign``: ``iif_max_iou_assign``.  The ``[G, N]`` overlap matrix (and the reference's nine temporaries
    of that size) is never stored: the three result vectors and a workspace of ``8 (G + 1)`` bytes are all that is
    allocated, the loop over the ground-truth boxes runs inside the kernel, and nothing synchronises the host.

Deliberately not offered: the calculator's ``dtype='fp16'`` mode, leading batch dimensions, ``assign_wrt_overlaps`` (its
argument is the matrix this module exists to avoid) and autograd through the overlaps.  When mmdet is importable the classes
register themselves as ``MaxIoUAssigner`` / ``BboxOverlaps2D``.
"""
import torch

from . import _lib

_MODES = {"iou": 0, "iof": 1, "giou": 2}


def _boxes(t, what):
    """``t`` as float32 rows of at least four unit-stride columns that the kernels read in place: (tensor, rows, pitch)."""
    if t.dim() != 2:
        raise NotImplementedError("%s: [n, 4] or [n, 5] boxes only, no batch dimensions (got %s)" % (what, tuple(t.shape)))
    if t.size(0) and t.size(-1) not in (4, 5):
        raise AssertionError("%s: boxes have 4 columns, or 5 with a score (got %s)" % (what, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise NotImplementedError("%s: float32 boxes only (got %s)" % (what, t.dtype))
    if t.requires_grad:
        raise RuntimeError("%s: the native overlaps have no autograd; detach the boxes" % what)
    n = t.size(0)
    if n == 0:
        return t, 0, 4
    if t.stride(1) != 1 or (n > 1 and t.stride(0) < 4):
        t = t[:, :4].contiguous()
    return t, n, (t.stride(0) if n > 1 else 4)


def bbox_overlaps(bboxes1, bboxes2, mode="iou", is_aligned=False, eps=1e-6):
    """iou2d_calculator.py:75-261 for float32 ``[m, 4]`` / ``[n, 4]`` boxes (a fifth column is ignored): ``[m, n]``, or
    ``[m]`` when ``is_aligned``.  Empty inputs give the reference's empty shapes.  No batch dimensions, no autograd."""
    assert mode in _MODES, "Unsupported mode %s" % (mode,)
    b1, m, ld1 = _boxes(bboxes1, "bboxes1")
    b2, n, ld2 = _boxes(bboxes2, "bboxes2")
    if is_aligned:
        assert m == n
    _lib.require_gpu(bboxes1, bboxes2)
    out = torch.empty((m,) if is_aligned else (m, n), dtype=torch.float32, device=bboxes1.device)
    if m * n == 0:
        return out
    rc = _lib.lib().iif_bbox_overlaps(_lib.ptr(b1), ld1, m, _lib.ptr(b2), ld2, n, _MODES[mode], int(bool(is_aligned)),
                                      float(eps), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "iif_bbox_overlaps")
    return out


class BboxOverlaps2D:
    """iou2d_calculator.py:22-72.  ``dtype='fp16'`` (the reference's memory saver) is not implemented: use the assigner,
    which needs no matrix at all."""

    def __init__(self, scale=1., dtype=None):
        self.scale = scale
        self.dtype = dtype

    def __call__(self, bboxes1, bboxes2, mode="iou", is_aligned=False):
        assert bboxes1.size(-1) in [0, 4, 5]
        assert bboxes2.size(-1) in [0, 4, 5]
        if self.dtype == "fp16":
            raise NotImplementedError("BboxOverlaps2D(dtype='fp16') is not implemented on the native path")
        return bbox_overlaps(bboxes1, bboxes2, mode, is_aligned)

    def __repr__(self):
        return self.__class__.__name__ + "(scale=%s, dtype=%s)" % (self.scale, self.dtype)


class AssignResult:
    """assign_result.py: ``num_gts``, ``gt_inds`` (0 background, -1 ignored, i + 1 = gt i), ``max_overlaps``, ``labels``."""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts = num_gts
        self.gt_inds = gt_inds
        self.max_overlaps = max_overlaps
        self.labels = labels
        self._extra_properties = {}

    @property
    def num_preds(self):
        return len(self.gt_inds)

    def set_extra_property(self, key, value):
        assert key not in self.info
        self._extra_properties[key] = value

    def get_extra_property(self, key):
        return self._extra_properties.get(key, None)

    @property
    def info(self):
        basic_info = {"num_gts": self.num_gts, "num_preds": self.num_preds, "gt_inds": self.gt_inds,
                      "max_overlaps": self.max_overlaps, "labels": self.labels}
        basic_info.update(self._extra_properties)
        return basic_info

    def __repr__(self):
        lab = None if self.labels is None else tuple(self.labels.shape)
        return "<AssignResult(num_gts=%r, gt_inds.shape=%r, max_overlaps.shape=%r, labels.shape=%r)>" % (
            self.num_gts, tuple(self.gt_inds.shape), tuple(self.max_overlaps.shape), lab)

    def add_gt_(self, gt_labels):
        """The ground-truth boxes as leading proposals (the samplers' ``add_gt_as_proposals``): plain concatenation."""
        k = len(gt_labels)
        self_inds = torch.arange(1, k + 1, dtype=torch.long, device=gt_labels.device)
        self.gt_inds = torch.cat([self_inds, self.gt_inds])
        self.max_overlaps = torch.cat([self.max_overlaps.new_ones(k), self.max_overlaps])
        if self.labels is not None:
            self.labels = torch.cat([gt_labels, self.labels])


class MaxIoUAssigner:
    """max_iou_assigner.py:10-59: the reference's arguments and defaults.

    ``gpu_assign_thr`` is accepted and has no effect: it moved the work to the CPU to keep the ``[G, N]`` matrices out of
    device memory, and this assigner never allocates them.  ``iou_calculator`` must be (a config of) ``BboxOverlaps2D``
    without ``dtype='fp16'``: the kernel computes the overlaps itself.  ``assign_wrt_overlaps`` is not offered."""

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True, ignore_iof_thr=-1,
                 ignore_wrt_candidates=True, match_low_quality=True, gpu_assign_thr=-1,
                 iou_calculator=dict(type="BboxOverlaps2D")):
        self.pos_iou_thr = pos_iou_thr
        self.neg_iou_thr = neg_iou_thr
        self.min_pos_iou = min_pos_iou
        self.gt_max_assign_all = gt_max_assign_all
        self.ignore_iof_thr = ignore_iof_thr
        self.ignore_wrt_candidates = ignore_wrt_candidates
        self.gpu_assign_thr = gpu_assign_thr
        self.match_low_quality = match_low_quality
        if isinstance(iou_calculator, dict):
            cfg = dict(iou_calculator)
            if cfg.pop("type", None) not in ("BboxOverlaps2D", BboxOverlaps2D):
                raise NotImplementedError("MaxIoUAssigner runs BboxOverlaps2D inside its kernel; got %r" % (iou_calculator,))
            iou_calculator = BboxOverlaps2D(**cfg)
        if type(iou_calculator) is not BboxOverlaps2D or iou_calculator.dtype == "fp16":
            raise NotImplementedError("MaxIoUAssigner runs the float32 BboxOverlaps2D inside its kernel; got %r" % (iou_calculator,))
        self.iou_calculator = iou_calculator

    def _neg_range(self):
        """Step 2's interval (:173-179): a float t is [0, t), a tuple is itself, anything else marks nothing."""
        if isinstance(self.neg_iou_thr, float):
            return 0.0, self.neg_iou_thr
        if isinstance(self.neg_iou_thr, tuple):
            assert len(self.neg_iou_thr) == 2
            return float(self.neg_iou_thr[0]), float(self.neg_iou_thr[1])
        return 0.0, 0.0

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        """max_iou_assigner.py:61-126 + :128-213 in at most three enqueued operations, without a host synchronisation.
        ``bboxes`` ``[N, 4]`` or ``[N, 5]``, ``gt_bboxes`` ``[G, 4]``, float32 on the GPU; returns an ``AssignResult``
        whose ``labels`` is None when ``gt_labels`` is None."""
        b, N, ldb = _boxes(bboxes, "bboxes")
        g, G, ldg = _boxes(gt_bboxes, "gt_bboxes")
        ig, I, ldi = (None, 0, 4) if gt_bboxes_ignore is None else _boxes(gt_bboxes_ignore, "gt_bboxes_ignore")
        neg_lo, neg_hi = self._neg_range()
        _lib.require_gpu(bboxes, gt_bboxes, gt_bboxes_ignore, gt_labels)
        dev = bboxes.device
        if gt_labels is not None and gt_labels.numel() != G:
            raise ValueError("one label per ground-truth box expected: %d boxes, %d labels" % (G, gt_labels.numel()))
        if G == 0 or N == 0:                                         # decided from the shapes (:146-162)
            gt_inds = torch.full((N,), 0 if G == 0 else -1, dtype=torch.long, device=dev)
            max_overlaps = torch.zeros((N,), dtype=torch.float32, device=dev)
            labels = None if gt_labels is None else torch.full((N,), -1, dtype=torch.long, device=dev)
            return AssignResult(G, gt_inds, max_overlaps, labels=labels)
        gt_inds = torch.empty((N,), dtype=torch.long, device=dev)
        max_overlaps = torch.empty((N,), dtype=torch.float32, device=dev)
        lab = labels = None
        if gt_labels is not None:
            lab = gt_labels.reshape(-1).to(torch.int64).contiguous()
            labels = torch.empty((N,), dtype=torch.long, device=dev)
        ws = torch.empty((G + 1,), dtype=torch.int64, device=dev) if self.match_low_quality else None      # this call's own
        rc = _lib.lib().iif_max_iou_assign(
            _lib.ptr(b), ldb, N, _lib.ptr(g), ldg, G, _lib.ptr(ig), ldi, I, float(self.pos_iou_thr), neg_lo, neg_hi,
            float(self.min_pos_iou), float(self.ignore_iof_thr), int(bool(self.gt_max_assign_all)),
            int(bool(self.ignore_wrt_candidates)), int(bool(self.match_low_quality)), _lib.ptr(lab), _lib.ptr(gt_inds),
            _lib.ptr(max_overlaps), _lib.ptr(labels), _lib.ptr(ws), 8 * (G + 1) if ws is not None else 0, _lib.stream_ptr())
        _lib.check(rc, "iif_max_iou_assign")
        return AssignResult(G, gt_inds, max_overlaps, labels=labels)

    def assign_wrt_overlaps(self, overlaps, gt_labels=None):
        raise NotImplementedError("assign_wrt_overlaps takes the [G, N] overlap matrix that this assigner never forms; "
                                  "call assign(bboxes, gt_bboxes, ...)")


def register_into_mmdet():
    """Register the native classes as mmdet's ``MaxIoUAssigner`` / ``BboxOverlaps2D`` if mmdet is importable."""
    try:
        from mmdet.core.bbox.builder import BBOX_ASSIGNERS
        from mmdet.core.bbox.iou_calculators.builder import IOU_CALCULATORS
    except Exception:
        return False
    BBOX_ASSIGNERS.register_module(name="MaxIoUAssigner", force=True, module=MaxIoUAssigner)
    IOU_CALCULATORS.register_module(name="BboxOverlaps2D", force=True, module=BboxOverlaps2D)
    return True


register_into_mmdet()
