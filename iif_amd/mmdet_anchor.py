"""mmdet's ``AnchorGenerator`` on the gfx950 kernels (csrc/rpn_stage.hip): every level of ``grid_anchors`` / ``grid_priors`` /
``valid_flags`` in ONE launch into one buffer, returned as per-level views.

Mirror of instance_segmentation/mmdet/core/anchor/anchor_generator.py:11-457: the constructor's arguments, assertions and
``ValueError``, the attributes ``strides`` (as pairs), ``base_sizes``, ``scales``, ``ratios``, ``scale_major``, ``centers``,
``center_offset``, ``num_base_anchors`` / ``num_base_priors``, ``num_levels``, ``base_anchors`` and ``__repr__``.

  * ``base_anchors`` are tiny: they are computed once on the host with the reference's own sequence of float32 torch operations
    (``sqrt``, ``1 /``, the two multiplication orders, ``+- 0.5 *``), so they are the reference's numbers bit for bit.
  * Anchor ``(l, y, x, a)`` is ``base[l][a] + (x sx, y sy, x sx, y sy)``: one float32 add per coordinate, the reference's.
  * The flag of ``valid_flags`` is ``x < min(ceil(w / sx), W_l) and y < min(ceil(h / sy), H_l)``, on integers.

Limits of the single launch: at most 8 levels, 16 base anchors per level, integer strides, fewer than 2^31 anchors.
Deliberately not offered: ``SSDAnchorGenerator``, ``LegacyAnchorGenerator``, ``YOLOAnchorGenerator``, ``sparse_priors``.  When
mmdet is importable the class registers itself as ``AnchorGenerator``.
"""
import ctypes

import numpy as np
import torch
from torch.nn.modules.utils import _pair

from . import _lib

__all__ = ["AnchorGenerator", "MAX_LEVELS", "MAX_BASE_ANCHORS"]

MAX_LEVELS, MAX_BASE_ANCHORS = 8, 16


class AnchorGenerator:
    """anchor_generator.py:61-113: the reference's arguments, defaults and attribute names."""

    def __init__(self, strides, ratios, scales=None, base_sizes=None, scale_major=True, octave_base_scale=None,
                 scales_per_octave=None, centers=None, center_offset=0.):
        octave = octave_base_scale is not None and scales_per_octave is not None
        if center_offset != 0:
            assert centers is None, "centers (%s) cannot be combined with a non-zero center_offset" % (centers,)
        if not 0 <= center_offset <= 1:
            raise ValueError("center_offset must lie in [0, 1] (got %s)" % (center_offset,))
        assert centers is None or len(centers) == len(strides), "one centre per stride expected (got %s, %s)" % (strides, centers)
        assert octave != (scales is not None), "give either scales or octave_base_scale with scales_per_octave, not both"
        self.strides = [_pair(s) for s in strides]
        self.base_sizes = list(base_sizes) if base_sizes is not None else [min(s) for s in self.strides]
        assert len(self.base_sizes) == len(self.strides), "one base size per stride expected (got %s, %s)" % (self.strides, self.base_sizes)
        if scales is None:
            # float64 on the host, rounded to float32 once by torch.Tensor: the reference's numbers
            scales = np.array([2 ** (i / scales_per_octave) for i in range(scales_per_octave)]) * octave_base_scale
        self.scales = torch.Tensor(scales)
        self.ratios = torch.Tensor(ratios)
        self.octave_base_scale, self.scales_per_octave = octave_base_scale, scales_per_octave
        self.scale_major, self.centers, self.center_offset = scale_major, centers, center_offset
        self.base_anchors = self.gen_base_anchors()

    @property
    def num_base_priors(self):
        return [int(b.size(0)) for b in self.base_anchors]

    num_base_anchors = num_base_priors

    @property
    def num_levels(self):
        return len(self.strides)

    def gen_base_anchors(self):
        centers = self.centers if self.centers is not None else [None] * len(self.base_sizes)
        return [self.gen_single_level_base_anchors(size, self.scales, self.ratios, c) for size, c in zip(self.base_sizes, centers)]

    def gen_single_level_base_anchors(self, base_size, scales, ratios, center=None):
        """``[len(ratios) len(scales), 4]`` float32 on the host.  The order of the float32 operations is the reference's
        (anchor_generator.py:151-194), which is what makes the bits equal: sqrt, reciprocal, (size * ratio) * scale or
        (size * scale) * ratio, then centre -/+ 0.5 * extent."""
        cx, cy = center if center is not None else (self.center_offset * base_size, self.center_offset * base_size)
        rh = torch.sqrt(ratios)
        rw = 1 / rh
        if self.scale_major:
            first_w, first_h, second = base_size * rw, base_size * rh, scales
        else:
            first_w, first_h, second = base_size * scales, base_size * scales, None
        if second is not None:
            ws = (first_w[:, None] * second[None, :]).view(-1)
            hs = (first_h[:, None] * second[None, :]).view(-1)
        else:
            ws = (first_w[:, None] * rw[None, :]).view(-1)
            hs = (first_h[:, None] * rh[None, :]).view(-1)
        half_w, half_h = 0.5 * ws, 0.5 * hs
        return torch.stack([cx - half_w, cy - half_h, cx + half_w, cy + half_h], dim=-1)

    # ---- the launch's description of the grid
    def _grid(self, featmap_sizes, what):
        """(``_lib.RpnGrid``, anchors per level) for these feature-map sizes; raises before any device work."""
        assert self.num_levels == len(featmap_sizes)
        if self.num_levels > MAX_LEVELS:
            raise ValueError("%s: %d levels; the single launch takes at most %d - generate such a grid per level with torch "
                             "operations" % (what, self.num_levels, MAX_LEVELS))
        g = _lib.RpnGrid()
        g.num_levels = self.num_levels
        counts = []
        for l, ((sw, sh), base) in enumerate(zip(self.strides, self.base_anchors)):
            if int(sw) != sw or int(sh) != sh or sw < 1 or sh < 1:
                raise ValueError("%s: integer strides >= 1 expected (got %s)" % (what, (sw, sh)))
            nb = int(base.size(0))
            if not 1 <= nb <= MAX_BASE_ANCHORS:
                raise ValueError("%s: %d base anchors on level %d; the single launch takes 1 .. %d" % (what, nb, l, MAX_BASE_ANCHORS))
            H, W = int(featmap_sizes[l][0]), int(featmap_sizes[l][1])
            if not (0 <= H <= 65535 and 0 <= W <= 65535) or W * int(sw) >= 2 ** 24 or H * int(sh) >= 2 ** 24:
                raise ValueError("%s: feature map %s with stride %s is out of range" % (what, (H, W), (sw, sh)))
            g.W[l], g.H[l], g.num_base[l], g.stride_w[l], g.stride_h[l] = W, H, nb, int(sw), int(sh)
            vals = base.to(torch.float32).reshape(-1).tolist()              # a host tensor: no device read
            for a in range(nb):
                for j in range(4):
                    g.base[l][a][j] = vals[4 * a + j]
            counts.append(H * W * nb)
        if sum(counts) >= 2 ** 31 - 4:
            raise ValueError("%s: %d anchors; the single launch takes fewer than 2^31" % (what, sum(counts)))
        return g, counts

    def _valid_sizes(self, featmap_sizes, pad_shape):
        """anchor_generator.py:398-402 per level: ``[(valid_w, valid_h)]``."""
        out = []
        h, w = pad_shape[:2]
        for (sw, sh), (feat_h, feat_w) in zip(self.strides, featmap_sizes):
            out.append((min(int(np.ceil(w / sw)), int(feat_w)), min(int(np.ceil(h / sh)), int(feat_h))))
        return out

    @staticmethod
    def _device(device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.IIFNativeError("iif_amd runs on MI355X only: AnchorGenerator got device %s (no CPU fallback)" % (dev,))
        return dev

    def grid_priors(self, featmap_sizes, device="cuda"):
        """anchor_generator.py:216-272: a list of ``[H_l W_l A_l, 4]`` float32 tensors, views of one buffer, one launch."""
        g, counts = self._grid(featmap_sizes, "grid_priors")
        dev = self._device(device)
        out = torch.empty((sum(counts), 4), dtype=torch.float32, device=dev)
        if sum(counts):
            with torch.cuda.device(dev):
                rc = _lib.lib().iif_grid_anchors(ctypes.byref(g), _lib.ptr(out), _lib.stream_ptr())
            _lib.check(rc, "iif_grid_anchors")
        return list(torch.split(out, counts, 0))

    def grid_anchors(self, featmap_sizes, device="cuda"):
        """anchor_generator.py:309-381: the same values as ``grid_priors``."""
        return self.grid_priors(featmap_sizes, device)

    def valid_flags(self, featmap_sizes, pad_shape, device="cuda"):
        """anchor_generator.py:383-440: a list of bool ``[H_l W_l A_l]`` tensors, views of one buffer, one launch."""
        g, counts = self._grid(featmap_sizes, "valid_flags")
        dev = self._device(device)
        valid = self._valid_sizes(featmap_sizes, pad_shape)
        for (vw, vh), (feat_h, feat_w) in zip(valid, featmap_sizes):
            assert vh <= feat_h and vw <= feat_w
        wh = (ctypes.c_int32 * (2 * len(valid)))(*[max(int(v), 0) for pair in valid for v in pair])
        out = torch.empty((sum(counts),), dtype=torch.uint8, device=dev)
        if sum(counts):
            with torch.cuda.device(dev):
                rc = _lib.lib().iif_grid_valid_flags(ctypes.byref(g), wh, _lib.ptr(out), _lib.stream_ptr())
            _lib.check(rc, "iif_grid_valid_flags")
        return list(torch.split(out.view(torch.bool), counts, 0))

    def sparse_priors(self, *args, **kwargs):
        raise NotImplementedError("AnchorGenerator.sparse_priors is not offered on the native path")

    def __repr__(self):
        """The reference's text (its missing comma after ``num_levels`` included)."""
        fields = [("strides", self.strides, ","), ("ratios", self.ratios, ","), ("scales", self.scales, ","),
                  ("base_sizes", self.base_sizes, ","), ("scale_major", self.scale_major, ","),
                  ("octave_base_scale", self.octave_base_scale, ","), ("scales_per_octave", self.scales_per_octave, ","),
                  ("num_levels", self.num_levels, ""), ("centers", self.centers, ","), ("center_offset", self.center_offset, ")")]
        return type(self).__name__ + "(\n" + "\n".join("    %s=%s%s" % f for f in fields)


def register_into_mmdet():
    """Register the native class as mmdet's ``AnchorGenerator`` if mmdet is importable."""
    try:
        from mmdet.core.anchor.builder import PRIOR_GENERATORS
    except Exception:
        return False
    PRIOR_GENERATORS.register_module(name="AnchorGenerator", force=True, module=AnchorGenerator)
    return True


register_into_mmdet()
