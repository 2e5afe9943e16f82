"""SingleRoIExtractor / RoIAlign (iif_amd.mmdet_roi_extractor, csrc/roi_align.hip), the part that needs no device: the fixture
tests/golden/g27_roi_extract.npz against the input generators and the numpy restatement of tests/roi_align_cases.py, the
separable form the kernel uses against the loop over samples, the Python surface's constructors, attributes and errors, and the
two C entry points in header, library and ctypes table with their argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from . import roi_align_cases as rc
from iif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_roi_extract_forward", "iif_roi_extract_backward")
FIXTURE = "g27_roi_extract"


def close(a, b, tol=1e-12):
    """Checksums agree to tol relative to the sum of magnitudes (the second figure)."""
    return bool(np.all(np.abs(np.asarray(a) - np.asarray(b)) <= tol * max(1.0, float(np.asarray(b).ravel()[1]))))


def test_fixture_inputs_regenerate(golden):
    rc.check_generator(golden(FIXTURE))


@pytest.mark.parametrize("name", list(rc.CASES))
def test_restatement_reproduces_the_fixture(golden, name):
    """Levels exactly, float64 outputs and gradients to 1e-12 (full arrays where stored, checksums elsewhere)."""
    g = golden(FIXTURE)
    out, lvls, grads = rc.reference64(name)
    assert np.array_equal(lvls, g["c_%s_lvls" % name])
    assert close(rc.checksum(out), g["c_%s_out_sum" % name])
    sums = g["c_%s_grad_sums" % name]
    assert sums.shape == (len(grads), 3)
    for i, gr in enumerate(grads):
        assert close(rc.checksum(gr), sums[i]), i
        used = (lvls == i).any()
        assert used or not gr.any()                       # a level no roi maps to: all zero
    if name == rc.FULL_CASE:
        assert np.abs(out - g["c_%s_out" % name]).max() <= 1e-12
        for i, gr in enumerate(grads):
            assert np.abs(gr - g["c_%s_grad%d" % (name, i)]).max() <= 1e-12


@pytest.mark.parametrize("name", list(rc.CASES))
def test_separable_form_equals_the_sample_loop(name):
    """sum_py sum_px Wy[py] Wx[px] f[py, px] / count against the four-corner loop, float64, degenerate rois included."""
    geo = rc.case_geometry(name)
    out, _, _ = rc.reference64(name)
    sep, touched = rc.forward_separable_np(rc.features(name), rc.rois(name), rc.F64, **geo)
    assert np.abs(sep - out).max() <= 1e-12
    assert touched >= 1


def test_separable_form_touches_fewer_pixels():
    """A 5 x 4 grid: at most (5 + 2)(4 + 2) distinct pixels against 4 * 20 corner visits; 2 x 2: 9 or fewer... against 16."""
    geo = dict(sizes=((50, 68),), scales=(0.25,), out=(7, 7), sampling_ratio=0, aligned=True, finest_scale=56, factor=None, N=1)
    f = [np.ones((1, 50, 68, 1), dtype=np.float32)]
    for roi, grid, bound in (((0, 10.0, 20.0, 118.0, 152.0), (5, 4), 42), ((0, 10.0, 20.0, 62.0, 70.0), (2, 2), 16)):
        r = np.array([roi], dtype=np.float32)
        d = rc.decisions(r[0], rc.F64, **geo)
        assert (d[2], d[3]) == grid
        _, touched = rc.forward_separable_np(f, r, rc.F64, **geo)
        assert touched <= bound and touched < 4 * grid[0] * grid[1]


def test_cases_are_what_they_are_there_for(golden):
    g = golden(FIXTURE)
    lv = g["c_kinds_c3_lvls"]
    kinds = rc.rois("kinds_c3")
    assert lv.tolist() == [0, 1, 2, 3, 1, 1, 0, 0, 0, 0, 0, -1, 0, 0, 3, 0, 1, 1, 2, 3, 1, 1, 0, 3]
    assert kinds[20, 0] == -1 and kinds[21, 0] == rc.N_IMG
    out, _, grads = rc.reference64("kinds_c3")
    for k in (10, 11, 12, 13, 20, 21):                      # negative sides (aligned), NaN scale, zero size / width, padding rows
        assert not out[k].any(), k
    assert all(out[k].any() for k in range(24) if k not in (10, 11, 12, 13, 20, 21))
    assert g["c_thresholds56_c1_lvls"].tolist() == [0, 1, 1, 2, 3, 0, 1, 2]
    assert set(g["c_all_on_level2_c64_lvls"].tolist()) == {2} and set(g["c_same64_c64_lvls"].tolist()) == {1}
    assert sorted(set(g["c_rand300_c3_lvls"].tolist())) == [0, 1, 2, 3]
    # the unaligned variant gives the negative-sided and the zero-size rows a one-pixel roi
    out_u, _, _ = rc.reference64("kinds_c3_unaligned")
    assert out_u[10].any() and out_u[12].any() and not out_u[11].any()
    # the whole map at 2 x 3 on one level: the largest grid
    d = rc.decisions(rc.rois("one_level_c3")[-1], rc.F32, **rc.case_geometry("one_level_c3"))
    assert (d[2], d[3]) == (25, 23)
    for name in rc.CASES:
        e = float(g["c_%s_ref_f32_err_out" % name])
        assert 0 < e < 1e-4, (name, e)
        assert (g["c_%s_ref_f32_err_grad" % name] < 1e-4).all()


# ------------------------------------------------------------------------------------------------------------ Python surface
def test_constructors_and_attributes_mirror_the_reference():
    from iif_amd import mmdet_roi_extractor as M
    r = M.RoIAlign(7)
    assert (r.output_size, r.spatial_scale, r.sampling_ratio, r.pool_mode, r.aligned, r.use_torchvision) == ((7, 7), 1.0, 0, 'avg', True, False)
    r = M.RoIAlign((2, 3), spatial_scale=0.125, sampling_ratio=2, pool_mode='avg', aligned=False, use_torchvision=True)
    assert (r.output_size, r.spatial_scale, r.sampling_ratio, r.aligned, r.use_torchvision) == ((2, 3), 0.125, 2, False, True)
    assert "output_size=(2, 3)" in repr(r) and "aligned=False" in repr(r)
    e = M.SingleRoIExtractor(dict(type='RoIAlign', output_size=7, sampling_ratio=0), out_channels=256, featmap_strides=[4, 8, 16, 32])
    assert isinstance(e.roi_layers, torch.nn.ModuleList) and len(e.roi_layers) == 4 and all(isinstance(l, M.RoIAlign) for l in e.roi_layers)
    assert e.roi_layers[0].output_size == (7, 7) and [l.spatial_scale for l in e.roi_layers] == [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    assert (e.out_channels, e.featmap_strides, e.num_inputs, e.fp16_enabled, e.finest_scale, e.init_cfg) == (256, [4, 8, 16, 32], 4, False, 56, None)
    e = M.SingleRoIExtractor(dict(type='RoIAlign', output_size=14, sampling_ratio=0), 256, [4, 8, 16, 32], finest_scale=28)
    assert e.finest_scale == 28 and e.roi_layers[3].output_size == (14, 14)
    for word in ("pool_mode='max'", "float32", "GenericRoIExtractor", "ONNX", "gradient with respect to", "channels_last", "more than 8 levels"):
        assert word in M.__doc__, word


def test_level_mapping_and_rescaling_methods_follow_the_reference(golden):
    from iif_amd.mmdet_roi_extractor import SingleRoIExtractor
    g = golden(FIXTURE)
    e = SingleRoIExtractor(dict(type='RoIAlign', output_size=7, sampling_ratio=0), 3, [4, 8, 16, 32], finest_scale=16)
    rois = torch.from_numpy(rc.rois("kinds_c3").copy())
    lv, want = e.map_roi_levels(rois, 4).numpy(), g["c_kinds_c3_lvls"]
    assert np.array_equal(lv[want >= 0], want[want >= 0])
    got = e.roi_rescale(rois[:4], 1.5).numpy()
    geo = rc.case_geometry("kinds_c3_scaled")
    for k in range(4):
        _, _, lvl, _, sh, sw, bh, bw, _, _, _ = rc.roi_geometry(rois[k].numpy(), rc.F32, **geo)
        s = np.float32(geo["scales"][lvl])
        assert np.float32(got[k, 1] * s - np.float32(0.5)) == sw and np.float32(got[k, 2] * s - np.float32(0.5)) == sh


def test_error_conventions():
    from iif_amd import mmdet_roi_extractor as M
    x, rois = torch.zeros(1, 3, 8, 8), torch.tensor([[0., 1., 1., 5., 5.]])
    with pytest.raises(NotImplementedError):
        M.RoIAlign(7, pool_mode='max')
    with pytest.raises(NotImplementedError):
        M.roi_align(x, rois, 7, pool_mode='max')
    with pytest.raises(NotImplementedError):
        M.roi_align(x.half(), rois, 7)
    with pytest.raises(NotImplementedError):
        M.roi_align(x.double(), rois, 7)
    with pytest.raises(NotImplementedError):
        M.GenericRoIExtractor(dict(type='RoIAlign', output_size=7), 3, [4])
    with pytest.raises(NotImplementedError):
        M.SingleRoIExtractor(dict(type='RoIPool', output_size=7), 3, [4])
    with pytest.raises(NotImplementedError):
        M.SingleRoIExtractor(dict(type='RoIAlign', output_size=7), 3, [4] * 9)
    with pytest.raises(NotImplementedError):
        M.SingleRoIExtractor(dict(type='RoIAlign', output_size=7, pool_mode='max'), 3, [4])
    with pytest.raises(NotImplementedError):
        M.extract_forward([x] * 9, rois, 7, [1.0] * 9)
    e = M.SingleRoIExtractor(dict(type='RoIAlign', output_size=7), 3, [4, 8])
    with pytest.raises(NotImplementedError):
        e([x, torch.zeros(1, 4, 4, 4)], rois)                                     # different C
    with pytest.raises(NotImplementedError):
        e([x, torch.zeros(2, 3, 4, 4)], rois)                                     # different N
    with pytest.raises(AssertionError):
        e([x, x, x], rois)                                                        # more levels than strides
    with pytest.raises(AssertionError):
        M.roi_align(x, torch.zeros(1, 4), 7)
    with pytest.raises(RuntimeError):
        M.roi_align(x, rois.clone().requires_grad_(True), 7)
    # CPU tensors are rejected, not emulated
    for call in (lambda: M.roi_align(x, rois, 7), lambda: M.RoIAlign(7)(x, rois), lambda: e([x, x[:, :, :4, :4]], rois),
                 lambda: M.extract_forward([x], rois, 7, [1.0]), lambda: M.extract_backward([x.shape], rois, torch.zeros(1, 3, 7, 7), 7, [1.0])):
        with pytest.raises(_lib.IIFNativeError):
            call()


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_entry_points_in_header_library_and_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code)
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        proto = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name])
    fields = re.search(r"typedef struct iif_roi_level \{(.*?)\}", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", fields).strip() == "void* ptr; int32_t H, W; float spatial_scale;"
    assert [f[0] for f in _lib.RoiLevel._fields_] == ["ptr", "H", "W", "spatial_scale"] and ctypes.sizeof(_lib.RoiLevel) == 24


def test_entry_points_check_arguments_before_launching():
    """Bad arguments return -1 before anything touches the device."""
    L = _lib.lib()
    one = 64            # a non-null, aligned stand-in: the checks below fail before any pointer is used

    def levels(n=4, ptr=one, H=8, W=8, s=0.25):
        arr = (_lib.RoiLevel * max(n, 1))()
        for l in arr:
            l.ptr, l.H, l.W, l.spatial_scale = ptr, H, W, s
        return arr

    def fwd(**kw):
        return L.iif_roi_extract_forward(kw.get("levels", levels()), kw.get("L", 4), kw.get("N", 2), kw.get("C", 3), kw.get("rois", one),
                                         kw.get("ld", 5), kw.get("K", 3), kw.get("ph", 7), kw.get("pw", 7), 0, 1, kw.get("finest", 56.0),
                                         kw.get("factor", 0.0), kw.get("out", one), 0, kw.get("lvl", None), None)
    assert fwd(levels=None) == -1 and fwd(rois=None) == -1 and fwd(out=None) == -1
    assert fwd(levels=levels(ptr=None)) == -1 and fwd(levels=levels(ptr=66)) == -1 and fwd(rois=66) == -1 and fwd(out=66) == -1 and fwd(lvl=66) == -1
    assert fwd(L=0) == -1 and fwd(L=9) == -1 and fwd(N=0) == -1 and fwd(C=0) == -1 and fwd(K=-1) == -1 and fwd(ld=4) == -1
    assert fwd(ph=0) == -1 and fwd(pw=-1) == -1 and fwd(ph=1025) == -1
    assert fwd(levels=levels(H=0)) == -1 and fwd(levels=levels(W=-3)) == -1 and fwd(levels=levels(s=0.0)) == -1
    assert fwd(finest=0.0) == -1 and fwd(finest=float("nan")) == -1 and fwd(factor=float("nan")) == -1
    assert fwd(L=1, finest=0.0, K=0) == 0                      # one level: no mapping, finest_scale is not read
    assert fwd(K=0, rois=None, out=None, levels=levels(ptr=None)) == 0

    def bwd(**kw):
        return L.iif_roi_extract_backward(kw.get("levels", levels(ptr=1024)), kw.get("L", 4), kw.get("N", 2), kw.get("C", 3),
                                          kw.get("rois", one), kw.get("ld", 5), kw.get("K", 3), kw.get("ph", 7), kw.get("pw", 7), 0, 1,
                                          kw.get("finest", 56.0), 0.0, kw.get("gout", one), 0, kw.get("arena", 1024),
                                          kw.get("bytes", 2 * 8 * 8 * 3 * 4), None)
    assert bwd(levels=None) == -1 and bwd(rois=None) == -1 and bwd(gout=None) == -1 and bwd(arena=None) == -1
    assert bwd(L=0) == -1 and bwd(L=9) == -1 and bwd(N=0) == -1 and bwd(C=0) == -1 and bwd(K=-1) == -1 and bwd(ld=4) == -1
    assert bwd(ph=0) == -1 and bwd(gout=66) == -1 and bwd(levels=levels(ptr=1026)) == -1 and bwd(finest=-1.0) == -1
    assert bwd(bytes=2 * 8 * 8 * 3 * 4 - 4) == -1              # a level's gradient reaches past the arena
    assert bwd(levels=levels(ptr=512)) == -1 and bwd(bytes=0) == -1
    assert bwd(K=0, rois=None, gout=None, arena=None) == 0
