#!/usr/bin/env python3
"""Generate tests/golden/gNN_roi_extract.npz (the next free number) by RUNNING THE REFERENCE's SingleRoIExtractor on the CPU,
once in float64 and once in float32, forward and (through torch autograd) backward.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_roi_extract.py <reference checkout>

``models/roi_heads/roi_extractors/base_roi_extractor.py`` and ``single_level_roi_extractor.py`` are imported as they are, under
placeholder ``mmcv`` / ``mmdet`` modules (the helpers of make_golden_targets.py).  The reference has no RoIAlign of its own - it
imports mmcv's compiled operator - so the placeholder's ``mmcv.ops.RoIAlign`` is the small torch module below: the definition
in include/iif_amd.h (mmcv's, pool_mode 'avg') evaluated with differentiable torch gathers, vectorised over a roi's samples.
One extension: a batch index outside [0, N) gives a zero row (mmcv would read out of bounds).  Levels, rescaling, the scatter
into the output and the per-level gradients - the reference's ``feats[i].sum() * 0.`` terms included - therefore come from the
reference's own ``forward`` and from autograd.  Nothing from the reference is written to the repository except outputs (data).

Asserted before anything is stored:
  * the torch placeholder and the numpy restatement of tests/roi_align_cases.py (the plain loop over samples) agree in float64
    to 1e-12, outputs and gradients, and on every level;
  * for a linear field f = a x + b y + c and rois inside the map every bin equals f at its centre
    x1 s - 0.5 + (pw + 0.5) bin_w (likewise y) to 1e-13 (a few float64 roundings at |f| < 16): this pins the ``aligned``
    half-pixel shift independently of anyone's memory of mmcv;
  * for every roi log2 of the level quotient is, in float64, at least 1e-4 from an integer - except rois built on exact
    thresholds (scale = finest_scale 2^k exactly), where the + 1e-6 puts the level unambiguously up;
  * the float32 and the float64 evaluation make the same discrete decisions for every roi (level, grid counts, dropped
    samples, cells); no bin is excluded from any comparison.
Stored per case: the rois, input checksums, ``target_lvls`` (-1 where the scale is NaN: the reference's value there is the
undefined conversion of NaN to an integer, which matches no level), checksums of the float64 output and level gradients
(the arrays themselves for roi_align_cases.FULL_CASE), and ``ref_f32_err_out`` / ``ref_f32_err_grad``: the float32 run's largest
error against float64 divided by max|f| and by the largest float64 gradient of that level.
"""
import glob
import importlib
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from tests import roi_align_cases as rc                                      # noqa: E402
from make_golden_targets import _Registry, _identity_decorator, _pkg        # noqa: E402

torch.set_num_threads(8)


class RoIAlign(torch.nn.Module):
    """The placeholder for mmcv.ops.RoIAlign (see the module docstring)."""

    def __init__(self, output_size, spatial_scale=1.0, sampling_ratio=0, pool_mode='avg', aligned=True, use_torchvision=False):
        super().__init__()
        assert pool_mode == 'avg'
        self.output_size = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
        self.spatial_scale, self.sampling_ratio, self.aligned = float(spatial_scale), int(sampling_ratio), aligned

    @staticmethod
    def _axis(start, bin_, grid, P, size, dt):
        p = torch.arange(P, dtype=dt)[:, None]
        i = torch.arange(grid, dtype=dt)[None, :]
        y = start + p * bin_ + (i + 0.5) * bin_ / grid
        kept = ~((y < -1.0) | (y > size))
        y = torch.where(kept, y.clamp(min=0), torch.zeros_like(y))
        low = y.long()
        edge = low >= size - 1
        low = torch.where(edge, torch.full_like(low, size - 1), low)
        high = torch.where(edge, low, low + 1)
        y = torch.where(edge, low.to(dt), y)
        l = y - low.to(dt)
        return kept.reshape(-1), low.reshape(-1), high.reshape(-1), l.reshape(-1), (1.0 - l).reshape(-1)

    def forward(self, input, rois):
        dt = input.dtype
        N, C, H, W = input.shape
        PH, PW = self.output_size
        s = torch.tensor(self.spatial_scale, dtype=dt)
        off = 0.5 if self.aligned else 0.0
        rows = []
        for k in range(rois.size(0)):
            r = rois[k].to(dt)
            b = float(r[0])
            zero = input.new_zeros((C, PH, PW))
            if not 0 <= b < N:
                rows.append(zero)
                continue
            start_w, start_h = r[1] * s - off, r[2] * s - off
            end_w, end_h = r[3] * s - off, r[4] * s - off
            roi_w, roi_h = end_w - start_w, end_h - start_h
            if not self.aligned:
                roi_w, roi_h = roi_w.clamp(min=1.0), roi_h.clamp(min=1.0)
            bin_h, bin_w = roi_h / PH, roi_w / PW
            gh = self.sampling_ratio if self.sampling_ratio > 0 else int(torch.ceil(roi_h / PH))
            gw = self.sampling_ratio if self.sampling_ratio > 0 else int(torch.ceil(roi_w / PW))
            if gh <= 0 or gw <= 0:
                rows.append(zero)
                continue
            ky, yl, yh, ly, hy = self._axis(start_h, bin_h, gh, PH, H, dt)
            kx, xl, xh, lx, hx = self._axis(start_w, bin_w, gw, PW, W, dt)
            f = input[int(b)]
            val = ((hy[:, None] * hx[None, :]) * f[:, yl[:, None], xl[None, :]] + (hy[:, None] * lx[None, :]) * f[:, yl[:, None], xh[None, :]]
                   + (ly[:, None] * hx[None, :]) * f[:, yh[:, None], xl[None, :]] + (ly[:, None] * lx[None, :]) * f[:, yh[:, None], xh[None, :]])
            val = val * (ky[:, None] & kx[None, :]).to(dt)
            rows.append(val.view(C, PH, gh, PW, gw).sum((2, 4)) / max(gh * gw, 1))
        return torch.stack(rows) if rows else input.new_zeros((0, C, PH, PW))


class _BaseModule(torch.nn.Module):
    def __init__(self, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg


def reference(ref_root):
    mm = os.path.join(ref_root, "instance_segmentation", "mmdet")
    mmcv = _pkg("mmcv")
    _pkg("mmcv.ops", RoIAlign=RoIAlign)
    _pkg("mmcv.runner", force_fp32=_identity_decorator, BaseModule=_BaseModule)
    assert mmcv.ops.RoIAlign is RoIAlign
    _pkg("mmdet")
    _pkg("mmdet.models")
    _pkg("mmdet.models.builder", ROI_EXTRACTORS=_Registry())
    _pkg("mmdet.models.roi_heads")
    _pkg("mmdet.models.roi_heads.roi_extractors", os.path.join(mm, "models", "roi_heads", "roi_extractors"))
    m = importlib.import_module("mmdet.models.roi_heads.roi_extractors.single_level_roi_extractor")
    return m.SingleRoIExtractor


def run_reference(Extractor, name, dt):
    """(out [K, PH, PW, C], levels, gradients [N, H, W, C] per level) of the reference in precision dt, as numpy arrays."""
    kind, C, out, sr, aligned, finest, factor, lv = rc.CASES[name]
    ext = Extractor(dict(type='RoIAlign', output_size=out, sampling_ratio=sr, aligned=aligned), C,
                    [rc.STRIDES[i] for i in lv], finest_scale=finest)
    rois = torch.from_numpy(rc.rois(name).copy()).to(dt)
    feats = [torch.from_numpy(f).to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for f in rc.features(name)]
    gout = torch.from_numpy(rc.grad_out(name, rois.size(0))).to(dt).permute(0, 3, 1, 2)
    with np.errstate(all="ignore"):
        res = ext(feats, rois, roi_scale_factor=factor)
        res.backward(gout)
        if len(lv) > 1:
            scale = torch.sqrt((rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]))
            lvls = ext.map_roi_levels(rois, len(lv)).numpy().copy()
            lvls[torch.isnan(scale).numpy()] = -1
        else:
            lvls = np.zeros(rois.size(0), dtype=np.int64)
    return (res.detach().permute(0, 2, 3, 1).numpy(), lvls, [f.grad.permute(0, 2, 3, 1).numpy() for f in feats])


def check_linear_field():
    H, W, s = 50, 68, 0.25
    a, b, c = 0.125, -0.0625, 3.0
    ys, xs = torch.arange(H, dtype=torch.float64)[:, None], torch.arange(W, dtype=torch.float64)[None, :]
    field = (a * xs + b * ys + c).expand(1, 1, H, W)
    rois = torch.tensor([[0, 10.25, 20.5, 30.75, 44.0], [0, 41.3, 30.7, 190.9, 175.2], [0, 8.0, 8.0, 260.0, 190.0]], dtype=torch.float64)
    worst = 0.0
    for out in ((7, 7), (14, 14), (2, 3)):
        got = RoIAlign(out, s, 0, 'avg', True)(field, rois)
        for k in range(rois.size(0)):
            x1, y1, x2, y2 = (float(v) for v in rois[k, 1:])
            bw, bh = (x2 - x1) * s / out[1], (y2 - y1) * s / out[0]
            cx = x1 * s - 0.5 + (np.arange(out[1]) + 0.5) * bw
            cy = y1 * s - 0.5 + (np.arange(out[0]) + 0.5) * bh
            assert cx.min() - bw / 2 >= 0 and cx.max() + bw / 2 <= W - 1 and cy.min() - bh / 2 >= 0 and cy.max() + bh / 2 <= H - 1
            want = a * cx[None, :] + b * cy[:, None] + c
            worst = max(worst, float(np.abs(got[k, 0].numpy() - want).max()))
    print("linear field: bin = f(centre) to %.2e" % worst)
    assert worst <= 1e-13


def main():
    Extractor = reference(sys.argv[1])
    check_linear_field()
    store = dict(rc.input_checksums())
    for name in rc.CASES:
        geo = rc.case_geometry(name)
        rois = rc.rois(name)
        out64, lv64, g64 = run_reference(Extractor, name, torch.float64)
        out32, lv32, g32 = run_reference(Extractor, name, torch.float32)
        assert out32.dtype == np.float32 and out64.dtype == np.float64
        assert np.array_equal(lv32, lv64), name
        # the restatement against the reference, float64
        mine, mlv, mg = rc.reference64(name)
        assert np.array_equal(mlv, lv64), (name, mlv, lv64)
        assert np.abs(mine - out64).max(initial=0) <= 1e-12, (name, np.abs(mine - out64).max())
        for a, b in zip(mg, g64):
            assert np.abs(a - b).max() <= 1e-12, (name, np.abs(a - b).max())
        # decisions and level margins
        for k in range(rois.shape[0]):
            assert rc.decisions_equal(rc.decisions(rois[k], rc.F32, **geo), rc.decisions(rois[k], rc.F64, **geo)), (name, k)
            area = (float(rois[k, 3]) - float(rois[k, 1])) * (float(rois[k, 4]) - float(rois[k, 2]))
            if len(geo["sizes"]) > 1 and area > 0:
                q0 = np.sqrt(area) / geo["finest_scale"]
                t0, t = np.log2(q0), np.log2(q0 + float(np.float32(1e-6)))
                exact = t0 == np.round(t0)
                assert exact or abs(t - np.round(t)) >= 1e-4, (name, k, t)
                if exact:
                    assert lv32[k] == min(max(int(t0), 0), len(geo["sizes"]) - 1), (name, k)
        fmax = max(float(np.abs(f).max()) for f in rc.features(name))
        err_out = float(np.abs(out32.astype(np.float64) - out64).max(initial=0)) / fmax
        err_grad = [float(np.abs(a.astype(np.float64) - b).max()) / float(np.abs(b).max()) if np.abs(b).max() > 0 else 0.0
                    for a, b in zip(g32, g64)]
        for a, b in zip(g32, g64):
            assert not a[b == 0].any(), name                 # float32 leaves zero what float64 leaves zero
        store["c_%s_lvls" % name] = lv64
        store["c_%s_out_sum" % name] = rc.checksum(out64)
        store["c_%s_grad_sums" % name] = np.stack([rc.checksum(g) for g in g64])
        store["c_%s_ref_f32_err_out" % name] = np.array(err_out)
        store["c_%s_ref_f32_err_grad" % name] = np.array(err_grad)
        if name == rc.FULL_CASE:
            store["c_%s_out" % name] = out64
            for i, g in enumerate(g64):
                store["c_%s_grad%d" % (name, i)] = g
        print("%-26s K %3d  levels used %s  ref f32 err: out %.2e  grad %s" % (
            name, rois.shape[0], sorted(set(lv64.tolist())), err_out, " ".join("%.2e" % e for e in err_grad)))
    taken = [int(m.group(1)) for f in glob.glob(os.path.join(HERE, "g*.npz")) for m in [re.match(r"g(\d+)_", os.path.basename(f))] if m]
    mine = [f for f in glob.glob(os.path.join(HERE, "g*_roi_extract.npz"))]
    path = mine[0] if mine else os.path.join(HERE, "g%d_roi_extract.npz" % (max(taken) + 1))
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
