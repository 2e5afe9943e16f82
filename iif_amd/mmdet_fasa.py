"""FASA (feature augmentation and sampling adaptation) pieces that sit on the IIF classifier path, on the
gfx950 kernels.

Mirrors, from instance_segmentation/mmdet:
  * ``FasaIIFLoss`` (models/losses/fasa_iif_loss.py:12-208): the IIF cross entropy plus, while ``use_cums`` is
    open, per-class accumulators of the row losses and label counts (:154-160);
  * the feature bank of ``ConvFCFASABBoxHead`` (models/roi_heads/bbox_heads/fasa_bbox_head.py:35-66,118-215):
    ``fa_update`` (per-class running mean / variance of positive embeddings), ``fa_generate`` (virtual
    embeddings for under-sampled classes) and the once-per-epoch ``dynamic_sampling`` (host-side,
    AffinityPropagation over class means).

The reference walks ``torch.unique(labels)`` on the host (one device sync per class and step); here each of
those is one launch with no host round trip, except the row count of ``fa_generate`` (one sync, as the
reference's ``len(embedding_list)``).  ``fa_update_rows`` and ``fa_generate_padded`` are the forms without any host read, for
the padded pipeline (``mmdet_fasa_head_loss.fasa_bbox_head_loss``).
"""
import torch
import torch.nn as nn

from . import _lib
from .loss_reduction import register_losses
from .mmdet_iif_loss import IIFLoss


class FasaIIFLoss(IIFLoss):
    """fasa_iif_loss.py:12-208.  ``use_sigmoid`` / ``use_mask`` replace the IIF cross entropy by mmdet's
    ``binary_cross_entropy`` / ``mask_cross_entropy`` (fasa_iif_loss.py:35-40), here the native ones of
    ``mmdet_ce_loss``; the class counters work on either."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction="mean", class_weight=None, loss_weight=1.0,
                 use_cums=False, num_classes=1203, path="./lvis_files/idf_1204.csv", variant="raw", device="cuda"):
        assert (use_sigmoid is False) or (use_mask is False)
        super().__init__(use_sigmoid=False, reduction=reduction, class_weight=class_weight, ignore_index=None,
                         loss_weight=loss_weight, num_classes=num_classes, path=path, variant=variant, device=device)
        self.use_sigmoid = use_sigmoid
        self.use_mask = use_mask
        if use_sigmoid or use_mask:
            # imported here: the module registers CrossEntropyLoss into mmdet, which a plain IIF user has not asked for
            from .mmdet_ce_loss import binary_cross_entropy, mask_cross_entropy
            self.cls_criterion = binary_cross_entropy if use_sigmoid else mask_cross_entropy
        self._device = device
        self.use_cums = use_cums
        if self.use_cums:
            self.open_cums()

    def open_cums(self):
        self.use_cums = True
        self.reduction_old = self.reduction
        self.reduction = "none"
        self.cum_losses = torch.zeros(self.num_classes + 1, device=self._device)
        self.cum_labels = torch.zeros(self.num_classes + 1, device=self._device)

    def close_cums(self):
        self.use_cums = False
        self.reduction = self.reduction_old
        self.cum_losses = torch.zeros(self.num_classes + 1, device=self._device)
        self.cum_labels = torch.zeros(self.num_classes + 1, device=self._device)

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        loss_cls = super().forward(cls_score, label, weight=weight, avg_factor=avg_factor,
                                   reduction_override=reduction_override, **kwargs)
        if self.use_cums:
            rows = loss_cls.detach().float()
            if rows.dim() > 1:                      # the sigmoid criterion's [N, C] element losses: a row's sum
                rows = rows.sum(dim=1)
            rows = rows.contiguous()
            lb = label.reshape(-1).to(torch.int64).contiguous()
            _lib.check(_lib.lib().iif_class_accumulate(_lib.ptr(rows), _lib.ptr(lb), rows.numel(), self.num_classes + 1,
                                                       _lib.ptr(self.cum_losses), _lib.ptr(self.cum_labels),
                                                       _lib.stream_ptr()), "iif_class_accumulate")
            loss_cls = loss_cls.mean()
        return loss_cls


class FasaFeatureBank(nn.Module):
    """State and methods ``ConvFCFASABBoxHead`` adds to the stock bbox head (fasa_bbox_head.py:35-66,118-215).
    ``instance_counts``: per-class training instance counts (the reference's LVIS_INSTANCES table)."""

    def __init__(self, num_classes, feat_dim, instance_counts, fasa_cfg=None, device="cuda"):
        super().__init__()
        cfg = fasa_cfg or {}
        self.num_classes, self.feat_dim = num_classes, feat_dim
        self.feature_mean = nn.Parameter(torch.zeros(num_classes, feat_dim, device=device), requires_grad=False)
        self.feature_std = nn.Parameter(torch.zeros(num_classes, feat_dim, device=device), requires_grad=False)   # a variance
        self.feature_used = nn.Parameter(torch.zeros(num_classes, device=device), requires_grad=False)
        self.decay_ratio = cfg.get("decay_ratio", 0.1)
        self.loss_aug_weight = cfg.get("loss_aug_weight", 0.1)
        self.dynamic_up = cfg.get("dynamic_up", 1.1)
        self.dynamic_down = cfg.get("dynamic_down", 0.9)
        counts = torch.as_tensor(instance_counts, dtype=torch.float32, device=device)
        prob = 1 / counts
        prob = cfg.get("instance_prob_scale", 1) * torch.pow(prob / prob.sum(), cfg.get("instance_prob_power", 1))
        self.prob_list = nn.Parameter(prob.clamp(0, 1), requires_grad=False)
        self.cum_loss_perclass_t0 = torch.zeros(num_classes + 1, device=device)
        self.cum_loss_perclass_t1 = torch.zeros(num_classes + 1, device=device)
        self.group_cluster_list = []
        self.epoch = 0
        self._slots = torch.zeros(num_classes, dtype=torch.int32, device=device)
        self._count = torch.zeros(1, dtype=torch.int32, device=device)

    def fa_update(self, embedding, labels):
        """fasa_bbox_head.py:118-147, all classes in one launch."""
        if len(labels) == 0:
            return
        _lib.require_gpu(embedding, labels)
        e = embedding.detach().float()
        if e.stride(1) != 1:
            e = e.contiguous()
        lb = labels.reshape(-1).to(torch.int64).contiguous()
        _lib.check(_lib.lib().iif_fasa_update(_lib.ptr(e), _lib.ptr(lb), e.shape[0], e.shape[1], e.stride(0), self.num_classes,
                                              float(self.decay_ratio), _lib.ptr(self.feature_mean.data),
                                              _lib.ptr(self.feature_std.data), _lib.ptr(self.feature_used.data),
                                              _lib.stream_ptr()), "iif_fasa_update")

    def fa_generate(self, rand=None, normal=None):
        """fasa_bbox_head.py:149-172.  ``rand`` [C] / ``normal`` [C, D] default to fresh torch draws (the
        reference draws ``torch.rand(C)`` and one ``torch.normal`` per selected class)."""
        dev = self.feature_mean.device
        if rand is None:
            rand = torch.rand(self.num_classes, device=dev)
        if normal is None:
            normal = torch.randn(self.num_classes, self.feat_dim, device=dev)
        out = torch.empty(self.num_classes, self.feat_dim, device=dev)
        labels = torch.empty(self.num_classes, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().iif_fasa_generate(_lib.ptr(rand.float().contiguous()), _lib.ptr(self.prob_list.data),
                                                _lib.ptr(self.feature_used.data), _lib.ptr(self.feature_mean.data),
                                                _lib.ptr(self.feature_std.data), _lib.ptr(normal.float().contiguous()),
                                                self.num_classes, self.feat_dim, _lib.ptr(self._slots), _lib.ptr(self._count),
                                                _lib.ptr(out), _lib.ptr(labels), _lib.stream_ptr()), "iif_fasa_generate")
        k = int(self._count.item())
        if k == 0:
            return [], []
        return out[:k], labels[:k]

    # ---- the padded pipeline (mmdet_fasa_head_loss.fasa_bbox_head_loss): no host read
    MAX_ROWS = 65535            # IIF_FASA_ROWS_MAX_ROWS
    MAX_CLASSES = 4096          # IIF_FASA_ROWS_MAX_CLASSES

    def fa_update_rows(self, embedding, labels):
        """``fa_update(embedding[pos], labels[pos])`` with ``pos = (labels >= 0) & (labels < num_classes)`` selected on
        the device (fasa_bbox_head.py:258-262 without its two boolean indexings): the padded rows of
        ``roi_stage_targets_padded`` go in as they are.  ``feature_mean``, ``feature_std`` and ``feature_used`` end
        with the bits ``fa_update`` gives on the compacted rows; the embedding of a row that is not positive is never
        read; two launches, no atomics.  ``embedding`` [N, D] float32 with any row pitch >= D, ``labels`` [N].

        Raises ``ValueError`` for more than 65535 rows or more than 4096 classes: compact the rows and call
        ``fa_update``, which has no such limit."""
        if embedding.dim() != 2 or embedding.shape[1] != self.feat_dim or labels.numel() != embedding.shape[0]:
            raise ValueError("fa_update_rows: embedding [N, %d] and N labels expected, got %s and %d labels"
                             % (self.feat_dim, tuple(embedding.shape), labels.numel()))
        n = embedding.shape[0]
        if n > self.MAX_ROWS or self.num_classes > self.MAX_CLASSES:
            raise ValueError("fa_update_rows: at most %d rows and %d classes (got %d rows, %d classes); compact the positive "
                             "rows and call fa_update instead" % (self.MAX_ROWS, self.MAX_CLASSES, n, self.num_classes))
        if n == 0:
            return
        _lib.require_gpu(embedding, labels)
        e = embedding.detach()
        if e.dtype != torch.float32:
            e = e.float()
        if e.stride(1) != 1 or (n > 1 and e.stride(0) < e.shape[1]):
            e = e.contiguous()
        lb = labels.reshape(-1).to(torch.int64).contiguous()
        if getattr(self, "_present", None) is None or self._present.device != e.device:
            self._present = torch.zeros(self.num_classes, dtype=torch.int32, device=e.device)
        _lib.check(_lib.lib().iif_fasa_update_rows(_lib.ptr(e), _lib.ptr(lb), n, e.shape[1], e.stride(0) if n > 1 else e.shape[1],
                                                   self.num_classes, float(self.decay_ratio), _lib.ptr(self.feature_mean.data),
                                                   _lib.ptr(self.feature_std.data), _lib.ptr(self.feature_used.data),
                                                   _lib.ptr(self._present), _lib.stream_ptr()), "iif_fasa_update_rows")

    def fa_generate_padded(self, rand=None, normal=None, capacity=None):
        """``fa_generate`` with a fixed shape and no host read: ``(embedding [K, D] float32, labels [K] int64,
        weights [K] float32, count)`` with ``K = capacity`` (default ``num_classes``) and ``count`` a 0-d int32 device
        tensor.  Rows below ``count`` hold what ``fa_generate`` returns for the same draws - the same classes in
        ascending order, the same bits - with weight ``loss_aug_weight``; the rows from ``count`` on hold zeros, label
        ``num_classes`` and weight 0, which ``head_cls_loss`` does not read.  One launch (plus the two draws when
        ``rand`` [C] / ``normal`` [C, D] are not given).

        With ``capacity`` below the number of classes drawn the lowest ``capacity`` classes are kept, ``count ==
        capacity``, and ``self.aug_dropped`` (0-d int32 device tensor, rewritten by every call) holds the number of
        classes dropped; it is 0 otherwise, always so at the default capacity.  This is the one deliberate difference
        from the reference.  ``capacity < 1`` raises ``ValueError``."""
        K = self.num_classes if capacity is None else int(capacity)
        if K < 1:
            raise ValueError("fa_generate_padded: capacity must be at least 1, got %r" % (capacity,))
        dev = self.feature_mean.device
        if rand is None:
            rand = torch.rand(self.num_classes, device=dev)
        if normal is None:
            normal = torch.randn(self.num_classes, self.feat_dim, device=dev)
        if rand.numel() != self.num_classes or tuple(normal.shape) != (self.num_classes, self.feat_dim):
            raise ValueError("fa_generate_padded: rand [%d] and normal [%d, %d] expected, got %s and %s"
                             % (self.num_classes, self.num_classes, self.feat_dim, tuple(rand.shape), tuple(normal.shape)))
        _lib.require_gpu(rand, normal, self.feature_mean)
        out = torch.empty(K, self.feat_dim, device=dev)
        labels = torch.empty(K, dtype=torch.int64, device=dev)
        weights = torch.empty(K, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().iif_fasa_generate_padded(
            _lib.ptr(rand.reshape(-1).float().contiguous()), _lib.ptr(self.prob_list.data), _lib.ptr(self.feature_used.data),
            _lib.ptr(self.feature_mean.data), _lib.ptr(self.feature_std.data), _lib.ptr(normal.float().contiguous()),
            self.num_classes, self.feat_dim, K, float(self.loss_aug_weight), _lib.ptr(out), _lib.ptr(labels), _lib.ptr(weights),
            _lib.ptr(count), _lib.stream_ptr()), "iif_fasa_generate_padded")
        self.aug_dropped = count[1]
        return out, labels, weights, count[0]

    def dynamic_sampling(self, loss_cls, training=False):
        """fasa_bbox_head.py:174-215: once per epoch, in eval mode.  Host-side (AffinityPropagation)."""
        if training:
            return
        import torch.distributed as dist
        from sklearn.cluster import AffinityPropagation

        def reduce_mean(t):                       # mmdet/core/utils/dist_utils.py:67-73
            if not (dist.is_available() and dist.is_initialized()):
                return t
            t = t.clone()
            dist.all_reduce(t.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
            return t
        cum_labels = reduce_mean(loss_cls.cum_labels)
        cum_losses = reduce_mean(loss_cls.cum_losses)
        self.cum_loss_perclass_t1 = cum_losses / cum_labels.sum()
        if self.cum_loss_perclass_t0.sum() == 0:
            self.cum_loss_perclass_t0[:] = self.cum_loss_perclass_t1[:]
        fm = self.feature_mean.data
        mean_xy = torch.matmul(fm, fm.T)
        sq = torch.sum(fm.square(), dim=1)
        distance = (sq.unsqueeze(1) - 2 * mean_xy + sq.unsqueeze(0)).cpu().numpy()
        clustering = AffinityPropagation(random_state=1, affinity="precomputed").fit(distance)
        self.group_cluster_list = [[i for i, v in enumerate(clustering.labels_) if v == g]
                                   for g in range(max(clustering.labels_) + 1)]
        for group in self.group_cluster_list:
            delta = self.cum_loss_perclass_t1[group].sum() - self.cum_loss_perclass_t0[group].sum()
            if delta > 0:
                self.prob_list.data[group] = (self.prob_list.data[group] * self.dynamic_down).clamp(0, 1)
            if delta < 0:
                self.prob_list.data[group] = (self.prob_list.data[group] * self.dynamic_up).clamp(0, 1)
        self.cum_loss_perclass_t0[:] = self.cum_loss_perclass_t1[:]


def register_into_mmdet():
    return register_losses({"FasaIIFLoss": FasaIIFLoss})


register_into_mmdet()
