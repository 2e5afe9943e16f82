"""``FCNMaskHead.get_targets`` + ``FCNMaskHead.loss`` on the padded rows of the padded RoI pipeline, without a host read.

The reference (instance_segmentation/mmdet/models/roi_heads/mask_heads/fcn_mask_head.py:138-177) builds the mask targets of the
sampled positives, returns ``mask_pred.sum()`` when there are none and otherwise ``mask_cross_entropy`` at each RoI's label (or
at channel 0 of a ``class_agnostic`` head), a mean over the positives.  The number of positives is a host number there.
``mmdet_roi_stage.roi_stage_targets_padded`` emits a fixed number of rows instead - ``pos_rois``, ``pos_gt_inds`` and
``pos_labels``, padded with image index -1 and label ``num_classes`` - so that nothing has to be read back;
``SingleRoIExtractor`` and ``mask_targets_padded`` write zero rows for the padding.  ``mask_head_loss`` closes that path:

  ``mask_targets_padded``            the targets of every row, one launch
  ``predictor.loss(valid_rows=True)`` the class-selected loss; a padded row is skipped - its features and targets are not read - and
                                     the divisor ``max(1, K) * H * W`` comes from the count ``K`` of real rows, taken on the device

``predictor`` is any of ``ClassSelectedMaskPredictor`` (mmdet_mask_predictor.py), ``ClassSelectedNormedMaskPredictor``
(mmdet_normed_mask_predictor.py) and ``FusedMaskHeadTail`` (mmdet_mask_tail.py, which takes the 14 x 14 input of ``upsample``).
No positives in the whole batch: the loss is exactly 0 and every gradient exact zeros, where the reference returns the sum of an
empty tensor.  With device-resident masks (``DeviceBitmapMasks`` or uint8 / bool tensors) the forward and the backward make no
host read: they run under ``torch.cuda.set_sync_debug_mode("error")``.

Not offered here: ``class_weight`` / ``loss_weight`` on the mask loss, the 3x3 ``convs`` in front (plain ``nn.Conv2d`` modules do
that), a registered RoI head class.
"""
from .mmdet_mask_target import mask_targets_padded

__all__ = ["mask_head_loss"]


def mask_head_loss(predictor, feats, pos_rois, pos_gt_inds, pos_labels, gt_masks_list, mask_size):
    """``dict(loss_mask=...)``, shape ``(1,)``.  ``feats [K, C, h, w]``: the mask head's features of the ``K`` padded rows, the
    input of ``predictor``; ``pos_rois [K, 5]`` (image index or -1, x1, y1, x2, y2), ``pos_gt_inds [K]`` and ``pos_labels [K]``
    (``num_classes`` on a padded row) as ``roi_stage_targets_padded`` returns them; ``gt_masks_list``: one item per image, as
    ``mask_targets_padded`` takes them; ``mask_size``: the side(s) of the predicted masks (28 for the default head).  Argument
    mistakes are reported by ``mask_targets_padded`` and by the predictor, with their errors."""
    targets = mask_targets_padded(pos_rois, pos_gt_inds, gt_masks_list, mask_size)
    return predictor.loss(feats, pos_labels, targets, valid_rows=True)
