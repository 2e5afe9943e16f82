"""SingleRoIExtractor / RoIAlign on the MI355X: iif_amd.mmdet_roi_extractor against the reference's own float64 run
(tests/golden/g27_roi_extract.npz; the numpy restatement of tests/roi_align_cases.py, which test_roi_extract_host.py and the
fixture's generator tie to it, regenerates the arrays the fixture keeps only as checksums).

Levels are compared exactly.  Outputs are measured as max|got - float64| / max|f| and each level's gradient as
max|got - float64| / max|float64 gradient of that level|; the kernel is allowed 4 x the float32 REFERENCE's own figure on the same
scale (``ref_f32_err_out`` / ``ref_f32_err_grad`` of the case, measured by the fixture's generator): the factor covers the
different summation order of the separable form and the arrival order of the atomics.  Every position the float64 gradient leaves
at zero must be exactly zero.  Each test prints its ratios (measured / reference figure)."""
import numpy as np
import pytest
import torch

from . import roi_align_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = "g27_roi_extract"
FACTOR = 4.0


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ref(golden):
    g = golden(FIXTURE)
    rc.check_generator(g)
    return g


def inputs(name, channels_last=True):
    """(feats as [N, C, H, W] device tensors in the asked layout, rois, grad_out [K, C, PH, PW] NCHW-contiguous)."""
    feats = [T(f).permute(0, 3, 1, 2) for f in rc.features(name)]
    if not channels_last:
        feats = [f.contiguous() for f in feats]
    rois = T(rc.rois(name))
    gout = T(rc.grad_out(name, rois.size(0))).permute(0, 3, 1, 2).contiguous()
    return feats, rois, gout


def call_args(name):
    geo = rc.case_geometry(name)
    return dict(output_size=geo["out"], spatial_scales=geo["scales"], sampling_ratio=geo["sampling_ratio"], aligned=geo["aligned"],
                finest_scale=geo["finest_scale"], roi_scale_factor=geo["factor"])


def check_out(ref, name, got_nchw, what):
    want, _, _ = rc.reference64(name)
    fmax = max(float(np.abs(f).max()) for f in rc.features(name))
    got = N_(got_nchw).transpose(0, 2, 3, 1).astype(np.float64)
    err = float(np.abs(got - want).max(initial=0)) / fmax
    allowed = float(ref["c_%s_ref_f32_err_out" % name])
    print("%s %s: out err %.3e, reference float32 %.3e, ratio %.2f" % (name, what, err, allowed, err / allowed))
    assert err <= FACTOR * allowed, (name, what, err, allowed)
    assert not got[~want.any(axis=(1, 2, 3))].any()                      # zero rows are exactly zero


def check_grads(ref, name, grads, what):
    _, _, want = rc.reference64(name)
    allowed = ref["c_%s_ref_f32_err_grad" % name]
    assert len(grads) == len(want)
    for i, (g, w) in enumerate(zip(grads, want)):
        assert g.shape == (w.shape[0], w.shape[3], w.shape[1], w.shape[2]) and g.is_contiguous(memory_format=torch.channels_last)
        got = N_(g).transpose(0, 2, 3, 1).astype(np.float64)
        assert not got[w == 0].any(), (name, what, i)                   # exactly zero where float64 is
        top = float(np.abs(w).max())
        if top == 0:
            assert allowed[i] == 0
            continue
        err = float(np.abs(got - w).max()) / top
        print("%s %s: level %d grad err %.3e, reference float32 %.3e, ratio %.2f" % (name, what, i, err, allowed[i], err / max(allowed[i], 1e-30)))
        assert err <= FACTOR * allowed[i], (name, what, i, err, allowed[i])


@pytest.mark.parametrize("name", list(rc.CASES))
def test_entries_against_the_float64_reference(ref, name):
    """Both entries, channels-last features, both output / grad_out layouts; levels exact."""
    from iif_amd.mmdet_roi_extractor import extract_backward, extract_forward
    feats, rois, gout = inputs(name)
    kw = call_args(name)
    out, lvls = extract_forward(feats, rois, return_levels=True, **kw)
    assert out.is_contiguous() and lvls.dtype == torch.int32
    assert np.array_equal(N_(lvls), ref["c_%s_lvls" % name])
    check_out(ref, name, out, "nchw")
    out_cl = extract_forward(feats, rois, channels_last_out=True, **kw)
    assert out_cl.shape == out.shape and (out_cl.is_contiguous(memory_format=torch.channels_last) or out.size(1) == 1)
    check_out(ref, name, out_cl, "channels-last out")
    shapes = [f.shape for f in feats]
    check_grads(ref, name, extract_backward(shapes, rois, gout, **kw), "nchw grad_out")
    check_grads(ref, name, extract_backward(shapes, rois, gout.contiguous(memory_format=torch.channels_last), **kw), "channels-last grad_out")


@pytest.mark.parametrize("name", ["kinds_c3", "kinds_c65_unaligned_sr2", "kinds_c3_scaled", "all_on_level2_c64", "one_level_c3"])
@pytest.mark.parametrize("channels_last", [True, False])
def test_module_under_autograd_equals_the_entries(ref, name, channels_last):
    """SingleRoIExtractor.forward / backward on NCHW-contiguous and channels-last features: the entries' results bit for bit in the
    forward, the same atomic sums (4 x the reference's float32 figure) in the backward; rois get no gradient."""
    from iif_amd.mmdet_roi_extractor import SingleRoIExtractor, extract_forward
    _, C, out_size, sr, aligned, finest, factor, lv = rc.CASES[name]
    feats, rois, gout = inputs(name, channels_last)
    leaves = [f.detach().requires_grad_(True) for f in feats]
    ext = SingleRoIExtractor(dict(type='RoIAlign', output_size=out_size, sampling_ratio=sr, aligned=aligned), C,
                             [rc.STRIDES[i] for i in lv], finest_scale=finest)
    out = ext(leaves, rois, roi_scale_factor=factor)
    assert out.shape == (rois.size(0), C) + tuple(out_size) and out.is_contiguous()
    if len(lv) > 1:                          # (one level: the module, like the reference, ignores the factor; none is set there)
        assert torch.equal(out.detach().view(torch.int32), extract_forward(feats, rois, **call_args(name)).view(torch.int32))
    check_out(ref, name, out, "module")
    out.backward(gout)
    assert rois.grad is None and all(l.grad is not None and l.grad.shape == l.shape for l in leaves)
    check_grads(ref, name, [l.grad.contiguous(memory_format=torch.channels_last) for l in leaves], "module")
    _, lvls, _ = rc.reference64(name)
    for i, l in enumerate(leaves):
        if len(lv) > 1 and not (lvls == i).any():
            assert not l.grad.any().item()                               # a level no roi maps to: exactly zero


def test_roi_align_is_the_one_level_case(ref):
    from iif_amd.mmdet_roi_extractor import RoIAlign, roi_align
    name = "one_level_c3"
    feats, rois, gout = inputs(name)
    x = feats[0].detach().requires_grad_(True)
    layer = RoIAlign((2, 3), spatial_scale=0.25, sampling_ratio=0)
    out = layer(x, rois)
    check_out(ref, name, out, "RoIAlign")
    out.backward(gout)
    check_grads(ref, name, [x.grad], "RoIAlign")
    again = roi_align(feats[0], rois, (2, 3), 0.25, 0, 'avg', True)
    assert torch.equal(out.detach().view(torch.int32), again.view(torch.int32))


def test_no_rois_gives_the_reference_empty_result():
    from iif_amd.mmdet_roi_extractor import SingleRoIExtractor
    feats = [torch.randn(2, 3, h, w, device=DEV, requires_grad=True) for h, w in rc.LEVELS]
    ext = SingleRoIExtractor(dict(type='RoIAlign', output_size=7, sampling_ratio=0), 3, [4, 8, 16, 32])
    out = ext(feats, torch.zeros((0, 5), device=DEV))
    assert out.shape == (0, 3, 7, 7) and out.dtype == torch.float32
    out.sum().backward()
    assert all(f.grad is not None and not f.grad.any().item() for f in feats)


def test_padded_rois_read_in_place(ref):
    """rois as a column slice of a wider buffer (pitch 8): no copy is needed, the same result."""
    from iif_amd.mmdet_roi_extractor import extract_forward
    name = "kinds_c3"
    feats, rois, _ = inputs(name)
    wide = torch.full((rois.size(0), 8), float("nan"), device=DEV)
    wide[:, :5] = rois
    kw = call_args(name)
    assert torch.equal(extract_forward(feats, wide[:, :5], **kw).view(torch.int32), extract_forward(feats, rois, **kw).view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ host synchronisation
def test_forward_and_backward_do_not_synchronise_the_host(ref):
    """SingleRoIExtractor forward + backward on channels-last features under torch's sync debug mode ('error')."""
    from iif_amd.mmdet_roi_extractor import SingleRoIExtractor
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "this torch build has no sync debug mode: the check cannot run"
    name = "rand300_c3"
    feats, rois, gout = inputs(name)
    leaves = [f.detach().requires_grad_(True) for f in feats]
    ext = SingleRoIExtractor(dict(type='RoIAlign', output_size=7, sampling_ratio=0), 3, list(rc.STRIDES), finest_scale=16)
    ext([f.detach() for f in feats], rois)                                  # the library is loaded before the mode is on
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ext(leaves, rois)
        out.backward(gout)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    check_out(ref, name, out, "sync-free")
    check_grads(ref, name, [l.grad for l in leaves], "sync-free")
