"""Host-side checks of the fused mask head tail (iif_amd/mmdet_mask_tail.py, csrc/mask_tail.hip): no device.

  * the float64 restatement of tests/mask_tail_cases.py reproduces the REFERENCE's own FCNMaskHead.forward + .loss
    (tests/golden/g32_mask_tail.npz, written by tests/golden/make_golden_mask_tail.py) to 1e-12, all five gradients;
  * on every grid case the ReLU's input is exact in float32 (equal to float64 bit for bit, in two summation orders), so no sign
    tie separates the GPU kernels from the restatement;
  * the float32 reference path (conv_transpose2d, relu, F.conv2d, oracle.mmdet_iif.mask_cross_entropy) stays within 2.5e-6 of
    the restatement on cases a, b, c, d, f, g, which gives the GPU tests' 1e-5 a margin of 4x (case e is printed: its GPU
    tolerance is max(1e-5, 4 * e32));
  * the module contract and the argument checks of the C entries (they return before any launch).
"""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from iif_amd import _lib
from tests import mask_tail_cases as mtc

GOLDEN_CASES = ("multi", "soft", "agnostic")


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_restatement_reproduces_the_reference_head(golden, name):
    g = golden("g32_mask_tail")
    get = lambda k, p="f64": torch.from_numpy(g["%s_%s_%s" % (name, k, p)])          # noqa: E731
    labels = get("labels")
    c = get("weight").shape[0]
    if c == 1:                                                                  # the class_agnostic head: FCNMaskHead.loss passes zeros
        labels = torch.zeros_like(labels)
    r = mtc.restate64(get("f"), get("up_weight"), get("up_bias"), get("weight"), get("bias"), labels, get("targets"))
    assert abs(float(r["loss"]) - float(get("loss"))) <= 1e-12 * abs(float(get("loss")))
    assert _rel(r["df"], get("df")) <= 1e-12
    assert _rel(r["dup_weight"], get("dup_weight")) <= 1e-12
    assert _rel(r["dup_bias"], get("dup_bias")) <= 1e-12
    assert _rel(r["dweight"], get("dweight").reshape(c, -1)) <= 1e-12
    assert _rel(r["dbias"], get("dbias")) <= 1e-12
    assert get("df").abs().max() > 0 and get("dup_weight").abs().max() > 0
    # the fixture's inputs sit on the grid: the float32 run saw the same values
    for k in ("f", "up_weight", "up_bias"):
        assert torch.equal(get(k), get(k, "f32").double())


@pytest.mark.parametrize("name", mtc.GRID_CASES)
def test_pre_is_exact_in_float32_on_the_grid_cases(name):
    """float32 pre == float64 pre bit for bit, with ci in ascending and in descending order: whatever order a kernel sums in,
    it sees the same sign.  Exact zeros exist, so the pre > 0 rule is exercised."""
    f, up_weight, up_bias = mtc.inputs(name)[:3]
    pre64 = mtc.reference64(name)["pre"]
    pre32 = F.conv_transpose2d(f, up_weight, up_bias, stride=2)
    assert torch.equal(pre32.double(), pre64)
    rev = torch.arange(f.shape[1] - 1, -1, -1)                                  # the same sum with ci descending
    pre_rev = F.conv_transpose2d(f[:, rev].contiguous(), up_weight[rev].contiguous(), up_bias, stride=2)
    assert torch.equal(pre_rev.double(), pre64)
    assert f.bfloat16().float().equal(f)
    if name == "a":
        zeros = int((pre64 == 0).sum())
        print("case a: %d exact zeros of pre among %d" % (zeros, pre64.numel()))
        assert zeros > 0


@pytest.mark.parametrize("name", mtc.GRID_CASES)
def test_float32_reference_error_leaves_the_gpu_tolerance_a_margin(name):
    e = mtc.e32(name)
    print(name, {k: "%.2e" % v for k, v in e.items()})
    if name != "e":
        for k, v in e.items():
            assert v <= 2.5e-6, (name, k, v)
    for k in mtc.GRADS:
        assert mtc.grad_tol(name, k) >= 1e-5


def test_module_matches_the_reference_state_dict_and_round_trips():
    from iif_amd.mmdet_mask_tail import FusedMaskHeadTail
    for ci, co, c, agnostic in ((256, 256, 1203, False), (16, 8, 5, False), (256, 256, 80, True)):
        m = FusedMaskHeadTail(ci, co, c, class_agnostic=agnostic)
        ref = nn.ModuleDict(dict(upsample=nn.ConvTranspose2d(ci, co, 2, stride=2), conv_logits=nn.Conv2d(co, 1 if agnostic else c, 1)))
        want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
        assert set(want) == {"upsample.weight", "upsample.bias", "conv_logits.weight", "conv_logits.bias"}
        m.load_state_dict(ref.state_dict())                          # a reference checkpoint's mask_head.* loads unchanged
        u, cl = m.to_modules()
        for a, b in ((u, ref["upsample"]), (cl, ref["conv_logits"])):
            assert type(a) is type(b) and torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
        assert u.kernel_size == (2, 2) and u.stride == (2, 2)
        again = FusedMaskHeadTail.from_modules(ref["upsample"], ref["conv_logits"])
        assert again.class_agnostic == agnostic or not agnostic
        assert torch.equal(again.upsample.weight, ref["upsample"].weight) and torch.equal(again.conv_logits.bias, ref["conv_logits"].bias)
    good_u, good_c = nn.ConvTranspose2d(4, 4, 2, stride=2), nn.Conv2d(4, 3, 1)
    for bad_u in (nn.ConvTranspose2d(4, 4, 4, stride=2, padding=1), nn.ConvTranspose2d(4, 4, 2, stride=1), nn.Conv2d(4, 4, 1),
                  nn.ConvTranspose2d(4, 4, 2, stride=2, groups=2), nn.ConvTranspose2d(4, 4, 3, stride=3)):
        with pytest.raises(NotImplementedError):
            FusedMaskHeadTail.from_modules(bad_u, good_c)
    with pytest.raises(NotImplementedError):
        FusedMaskHeadTail.from_modules(good_u, nn.Conv2d(4, 3, 3))
    with pytest.raises(ValueError):
        FusedMaskHeadTail.from_modules(good_u, nn.Conv2d(5, 3, 1))


def test_module_initialisation_is_the_references():
    """kaiming_normal_(mode='fan_out', nonlinearity='relu') on both layers, zero biases (fcn_mask_head.py:115-125).  fan_out of
    the ConvTranspose2d weight [Ci, Co, 2, 2] is Ci * 4 as torch computes it; of the 1x1 convolution C."""
    from iif_amd.mmdet_mask_tail import FusedMaskHeadTail
    torch.manual_seed(5)
    m = FusedMaskHeadTail(256, 256, 1203)
    assert not m.upsample.bias.any() and not m.conv_logits.bias.any()
    for w, std in ((m.upsample.weight, (2.0 / (256 * 4)) ** 0.5), (m.conv_logits.weight, (2.0 / 1203) ** 0.5)):
        w = w.detach().double()
        n = w.numel()
        assert abs(float(w.mean())) <= 5 * std / n ** 0.5
        assert abs(float(w.std()) / std - 1) <= 5 / (2 * n) ** 0.5   # five standard errors of a normal sample's deviation
        assert float(w.abs().max()) <= 7 * std
    torch.manual_seed(5)                                             # and it IS that initialiser: the same draws in the same order
    u, c = nn.ConvTranspose2d(256, 256, 2, stride=2), nn.Conv2d(256, 1203, 1)
    torch.manual_seed(5)
    for layer in (u, c):
        nn.init.kaiming_normal_(layer.weight, mode="fan_out", nonlinearity="relu")
    assert torch.equal(m.upsample.weight.detach(), u.weight.detach()) and torch.equal(m.conv_logits.weight.detach(), c.weight.detach())


def test_cpu_tensors_shapes_and_dtypes_raise(monkeypatch):
    from iif_amd import mmdet_mask_tail as mt
    f = torch.zeros(2, 4, 3, 3)
    uw = torch.zeros(4, 6, 2, 2)
    ub = torch.zeros(6)
    w = torch.zeros(5, 6, 1, 1)
    b = torch.zeros(5)
    lb = torch.zeros(2, dtype=torch.int64)
    t = torch.zeros(2, 6, 6)
    with pytest.raises(_lib.IIFNativeError):
        mt.upsampled_class_mask_logits(f, uw, ub, w, b, lb)
    with pytest.raises(_lib.IIFNativeError):
        mt.upsampled_class_mask_loss(f, uw, ub, w, b, lb, t)
    with pytest.raises(_lib.IIFNativeError):
        mt.upsampled_class_mask_loss(f[:0], uw, ub, w, b, lb[:0], t[:0])
    m = mt.FusedMaskHeadTail(4, 6, 5)
    with pytest.raises(_lib.IIFNativeError):
        m(f, lb)
    with pytest.raises(_lib.IIFNativeError):
        m.loss(f, lb, t)
    # shapes and dtypes, with the device check out of the way
    monkeypatch.setattr(_lib, "require_gpu", lambda *a: None)
    for bad in ((f[0], uw, ub, w, b, lb), (f, uw[:3], ub, w, b, lb), (f, torch.zeros(4, 6, 3, 3), ub, w, b, lb), (f, uw, ub[:5], w, b, lb),
                (f, uw, ub, w[:, :5], b, lb), (f, uw, ub, torch.zeros(5, 6, 3, 3), b, lb), (f, uw, ub, torch.zeros(5, 6, 1), b, lb),
                (f, uw, ub, w, b[:4], lb), (f, uw, ub, w, b, lb[:1]), (torch.zeros(2, 4, 33, 32), uw, ub, w, b, lb),
                (torch.zeros(2, 1025, 1, 1), torch.zeros(1025, 6, 2, 2), ub, w, b, lb),
                (f, torch.zeros(4, 1025, 2, 2), torch.zeros(1025), torch.zeros(5, 1025), b, lb)):
        with pytest.raises(ValueError):
            mt._prep(*bad)
    for bad in ((f.half(), uw, ub, w, b, lb), (f.double(), uw, ub, w, b, lb), (f, uw.double(), ub, w, b, lb), (f, uw, ub.bfloat16(), w, b, lb),
                (f, uw, ub, w.double(), b, lb), (f, uw, ub, w, b.bfloat16(), lb), (f.bfloat16(), uw.bfloat16(), ub, w, b, lb),
                (f, uw, ub, w, b, lb.float())):
        with pytest.raises(NotImplementedError):
            mt._prep(*bad)
    out = mt._prep(f.bfloat16().to(memory_format=torch.channels_last), uw, None, w.reshape(5, 6), None, lb.int())
    assert out[0].is_contiguous() and out[5].dtype == torch.int64 and out[6:] == (2, 5, 4, 6, 3, 3)
    wide = torch.zeros(5, 9, 1, 1)[:, :6]                          # a row-strided view is read in place
    assert mt._ld(mt._prep(f, uw, ub, wide, b, lb)[3]) == 9
    off = torch.zeros(4 * 6 * 4 + 1)[1:].reshape(4, 6, 2, 2)       # a contiguous up_weight that is not 16-byte aligned is copied
    assert off.data_ptr() % 16 and mt._prep(f, off, ub, w, b, lb)[1].data_ptr() % 16 == 0


def test_c_entries_reject_bad_arguments_before_any_launch():
    """As the iif_slab_sum checks of tests/test_cabi.py: host buffers stand in for device memory, nothing may be launched."""
    L = _lib.lib()
    raw = (ctypes.c_float * 64)()
    p = ctypes.addressof(raw)
    p += (-p) % 16
    F32 = _lib.IIF_F32
    geo = (("n", 2), ("c", 3), ("ci", 4), ("co", 4), ("h", 2), ("w", 2))
    call = lambda fn, spec: (lambda **k: fn(*[k.get(a, d) for a, d in spec]))        # noqa: E731
    fwd = call(L.iif_mask_tail_fwd, (("f", p), ("dtype", F32), ("up_weight", p), ("up_bias", p), ("weight", p), ("ld_w", 4), ("bias", p),
                                     ("labels", p), ("target", p)) + geo + (("z", p), ("g0", p), ("rows", p), ("loss", p),
                                                                            ("status", p), ("stream", None)))
    rows = call(L.iif_mask_tail_bwd_rows, (("f", p), ("dtype", F32), ("up_weight", p), ("up_bias", p), ("g", p), ("up", None),
                                           ("labels", p)) + geo + (("signs", p), ("rows", p), ("stream", None)))
    dfe = call(L.iif_mask_tail_bwd_input, (("g", p), ("up", None), ("up_weight", p), ("weight", p), ("ld_w", 4), ("labels", p),
                                           ("signs", p)) + geo + (("df", p), ("dtype", F32), ("stream", None)))
    par = call(L.iif_mask_tail_bwd_params, (("f", p), ("dtype", F32), ("g", p), ("up", None), ("weight", p), ("ld_w", 4), ("labels", p),
                                            ("signs", p)) + geo + (("partial", p), ("dup_weight", p), ("dup_bias", p), ("stream", None)))
    for entry, ptrs in ((fwd, ("f", "up_weight", "weight", "labels", "status", "rows", "loss")),
                        (rows, ("f", "up_weight", "g", "labels", "signs")),
                        (dfe, ("g", "up_weight", "weight", "labels", "signs", "df")),
                        (par, ("f", "g", "weight", "labels", "signs", "partial"))):
        for name in ptrs:
            assert entry(**{name: None}) == -1, name
        assert entry(ci=0) == -1 and entry(ci=1025) == -1
        assert entry(co=0) == -1 and entry(co=1025) == -1
        assert entry(h=0) == -1 and entry(w=0) == -1 and entry(h=33, w=32) == -1
        assert entry(n=-1) == -1 and entry(n=65536) == -1
        assert entry(c=0) == -1 and entry(c=-3) == -1
        assert entry(dtype=7) == -1
        assert entry(n=0) == 0                                        # nothing to do: IIF_OK, nothing enqueued
    assert fwd(ld_w=3) == -1 and dfe(ld_w=3) == -1 and par(ld_w=3) == -1     # rows that overlap
    assert fwd(z=None, target=None) == -1                             # nothing asked for
    assert fwd(target=None) == -1                                     # g0 without a target
    assert par(dup_weight=None, dup_bias=None) == -1
    assert dfe(up_weight=p + 4) == -2                                 # IIF_EUNSUPPORTED: up_weight rows are read 16 bytes at a time
    cls = call(L.iif_mask_tail_bwd_classes, (("rows", p), ("labels", p), ("n", 2), ("c", 3), ("co", 4), ("dweight", p), ("dbias", p),
                                             ("stream", None)))
    assert cls(rows=None) == -1 and cls(labels=None) == -1 and cls(dweight=None, dbias=None) == -1
    assert cls(n=-1) == -1 and cls(n=65536) == -1 and cls(c=0) == -1 and cls(co=0) == -1 and cls(co=1025) == -1
    assert cls(n=0) == 0
    # the RoI ranges of dup_weight: at most 16, never more than RoIs, every range non-empty
    for n, ci, co in ((1, 3, 3), (3, 256, 256), (70, 256, 256), (256, 256, 256), (65535, 1024, 1024), (5, 300, 130)):
        s = L.iif_mask_tail_splits(n, ci, co)
        per = -(-n // s)
        assert 1 <= s <= min(n, 16) and (s - 1) * per < n <= s * per
    assert L.iif_mask_tail_splits(0, 4, 4) == 0
