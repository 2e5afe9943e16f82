"""The fused inference forward without a device: the three C entries (iif_conv_igemm_affine, iif_conv_affine_ok,
iif_bn_fold) are declared, exported and bound, their argument checks return before any HIP call, and
NativeResNet.eval_route - the walk the plan takes its eval routing from - lists every convolution after the stem of the
supported networks as fused (a route that quietly falls back must not pass)."""
import ctypes
import os
import re

import pytest
import torch

from iif_amd import _lib, ops, per_shot_acc, resnet_cifar, resnet_pytorch, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
ENTRIES = {"iif_conv_igemm_affine": 9, "iif_conv_affine_ok": 3, "iif_bn_fold": 4, "iif_conv_affine_route": 4}


def test_entries_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(cdll, name), name
    assert re.search(r"typedef struct iif_bn_fold_desc", hdr)


def _net(arch, dt=torch.bfloat16):
    if hasattr(resnet_cifar, arch):
        return getattr(resnet_cifar, arch)(num_classes=10, device="cpu", compute_dtype=dt)
    return getattr(resnet_pytorch, arch)(num_classes=10, device="cpu", compute_dtype=dt, pretrained="None")


def _conv_descs(net, n, h, w):
    """(name, descriptor arguments, has_res, has_res_affine) of every convolution after the stem, derived here from the
    module tree alone (not from eval_route): geometry per group as the engine's grouped layers run (64-channel chunks)."""
    c1 = net.conv1
    hh, ww = ops.conv_out_hw(h, w, c1.k, c1.k, c1.stride, c1.pad)
    if net.style == "imagenet":
        hh, ww = (hh + 2 - 3) // 2 + 1, (ww + 2 - 3) // 2 + 1
    out = []
    for si, st in enumerate(net._stages):
        for bi, blk in enumerate(st):
            hi, wi = hh, ww
            pairs = blk.units()
            for ui, (cv, _) in enumerate(pairs):
                oh, ow = ops.conv_out_hw(hi, wi, cv.k, cv.k, cv.stride, cv.pad)
                g = cv.cin // cv.chunk if cv.groups > 1 else 1
                ldw = cv.k * cv.k * cv.chunk if cv.groups > 1 else net._offsets[(id(cv), "weight")][2]
                closing = ui == len(pairs) - 1
                out.append(("layer%d.%d.conv%d" % (si + 1, bi, ui + 1),
                            (n, hi, wi, cv.cin // g, oh, ow, cv.cout // g, cv.k, cv.k, cv.stride, cv.pad, ldw), g,
                            closing, closing and blk.downsample is not None))
                hi, wi = oh, ow
            hh, ww = hi, wi
    return out


NETS = [("resnet50", 256, 224), ("resnet32", 128, 32), ("resnext50_32x4d", 128, 224)]


@pytest.mark.parametrize("arch,n,hw", NETS)
def test_every_convolution_after_the_stem_has_a_fused_instance(arch, n, hw):
    net = _net(arch)
    descs = _conv_descs(net, n, hw, hw)
    assert len(descs) == {"resnet50": 48, "resnet32": 30, "resnext50_32x4d": 48}[arch]
    for name, geo, g, has_res, has_aff2 in descs:
        assert ops.conv_affine_ok(*geo, torch.bfloat16, g, has_res, has_aff2), name
        assert not ops.conv_affine_ok(*geo, torch.float32, g, has_res, has_aff2), name        # fp32 descriptors: never
    # a normalised residual needs a residual
    name, geo, g, _, _ = descs[-1]
    assert not ops.conv_affine_ok(*geo, torch.bfloat16, g, False, True)


@pytest.mark.parametrize("arch,n,hw", NETS)
def test_eval_route_fuses_everything_but_the_stem(arch, n, hw):
    net = _net(arch)
    route = net.eval_route(n, hw, hw)
    assert [name for name, _ in route][0] == "conv1"
    convs = 1 + sum(len(b.units()) + (b.downsample is not None) for st in net._stages for b in st)
    assert len(route) == convs
    for name, r in route:
        assert r in ("fused", "raw") or r.startswith("unfused: "), (name, r)
    unfused = [name for name, r in route if r.startswith("unfused")]
    assert unfused in ([], ["conv1"]), unfused
    raw = [name for name, r in route if r == "raw"]
    assert raw == [name for name, _ in route if name.endswith(".downsample")]
    assert sum(r == "fused" for _, r in route) == len(_conv_descs(net, n, hw, hw)) + (arch == "resnet32")
    # the names are the modules' names
    mods = dict(net.named_modules())
    for name, _ in route:
        assert (name if not name.endswith(".downsample") else name + ".0") in mods, name


def test_eval_route_of_se_resnet50_keeps_the_block_closing_units():
    net = _net("se_resnet50")
    route = net.eval_route(256, 224, 224)
    unfused = [name for name, r in route if r.startswith("unfused")]
    closing = ["layer%d.%d.conv3" % (si + 1, bi) for si, st in enumerate(net._stages) for bi in range(len(st))]
    assert len(closing) == 16 and unfused == ["conv1"] + closing
    assert sum(r == "fused" for _, r in route) == 32 and sum(r == "raw" for _, r in route) == 4


def test_eval_route_fp32_and_dma_limit_keep_todays_route(monkeypatch):
    route = _net("resnet50", torch.float32).eval_route(8, 64, 64)
    assert all(r == "raw" or r.startswith("unfused") for _, r in route)
    from iif_amd import resnet_engine
    monkeypatch.setattr(resnet_engine, "_DMA_LIMIT", 1 << 16)
    route = _net("resnet50").eval_route(8, 64, 64)
    assert all(r == "raw" or r.startswith("unfused") for _, r in route)


def test_flag_default_and_setter():
    net = _net("resnet20")
    assert net.fused_eval is False
    assert net.set_fused_eval(True) is net and net.fused_eval is True
    net.set_fused_eval(False)
    assert net.fused_eval is False


def test_parsers_accept_fused_eval():
    for mod in (train, per_shot_acc):
        p = mod.get_args_parser()
        assert p.parse_args([]).fused_eval is False
        assert p.parse_args(["--fused-eval"]).fused_eval is True


def test_enable_fused_eval_prints_the_route_summary(capsys):
    args = train.get_args_parser().parse_args(["--fused-eval", "--model", "resnet32", "--dset_name", "cifar100", "-b", "128"])
    net = _net("resnet32")
    train.enable_fused_eval(net, args)
    assert net.fused_eval and "fused 31 of 31 units" in capsys.readouterr().out
    args = train.get_args_parser().parse_args(["--model", "resnet32"])
    net = _net("resnet32")
    train.enable_fused_eval(net, args)
    assert not net.fused_eval and capsys.readouterr().out == ""


# ------------------------------------------------------------------ argument checks (nothing is launched)
def _desc(dtype=_lib.IIF_BF16, **kw):
    f = dict(n=2, hs=8, ws=8, cs=64, hd=8, wd=8, cd=64, r=3, s=3, stride=1, pad=1, transposed=0, ldw=576, dtype=dtype,
             dst_dtype=dtype, groups=1)
    f.update(kw)
    return _lib.ConvDesc(*[f[k] for k in ("n", "hs", "ws", "cs", "hd", "wd", "cd", "r", "s", "stride", "pad", "transposed",
                                          "ldw", "dtype", "dst_dtype", "groups")], None, 0)


def _affine(d=None, src=0x10000, wgt=0x20000, dst=0x30000, res=0, res_affine=0, affine=0x40000, bits=0):
    d = d if d is not None else _desc()
    return _lib.lib().iif_conv_igemm_affine(ctypes.byref(d), src, wgt, dst, res, res_affine, affine, bits, 0)


def test_affine_entry_rejects_bad_arguments():
    assert _lib.lib().iif_conv_igemm_affine(None, 0x10000, 0x20000, 0x30000, 0, 0, 0x40000, 0, 0) == EINVAL
    for kw in (dict(src=0), dict(wgt=0), dict(dst=0), dict(affine=0), dict(res_affine=0x50000)):       # (res_affine without res)
        assert _affine(**kw) == EINVAL, kw
    assert _affine(d=_desc(transposed=1)) == EINVAL
    for kw in (dict(src=0x10008), dict(wgt=0x20004), dict(dst=0x30002), dict(res=0x50008), dict(affine=0x40002),
               dict(res=0x50000, res_affine=0x60001)):
        assert _affine(**kw) == EUNSUPPORTED, kw
    for d in (_desc(dtype=_lib.IIF_F32), _desc(cd=60), _desc(cs=60, ldw=540), _desc(stride=3), _desc(ldw=64)):
        assert _affine(d=d) == EUNSUPPORTED
        assert _lib.lib().iif_conv_affine_ok(ctypes.byref(d), 0, 0) == 0
    assert _lib.lib().iif_conv_affine_ok(None, 0, 0) == 0
    assert _lib.lib().iif_conv_affine_ok(ctypes.byref(_desc()), 1, 1) == 1
    assert _lib.lib().iif_conv_affine_ok(ctypes.byref(_desc()), 0, 1) == 0


def test_bn_fold_entry_rejects_bad_arguments():
    f = _lib.lib().iif_bn_fold
    assert f(0, 4, 1e-5, 0) == EINVAL
    assert f(0x10000, 0, 1e-5, 0) == EINVAL
    assert f(0x10000, -3, 1e-5, 0) == EINVAL
    assert f(0x10000, 4, -1e-5, 0) == EINVAL
    assert f(0x10000, 4, float("nan"), 0) == EINVAL
    assert f(0x10004, 4, 1e-5, 0) == EUNSUPPORTED


def test_bn_fold_table_layout_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    body = re.search(r"typedef struct iif_bn_fold_desc \{(.*?)\} iif_bn_fold_desc;", hdr, re.S).group(1)
    assert re.findall(r"\b(gamma|beta|running_mean|running_var|stats|c|reserved)\b\s*[;,]", body) == [
        "gamma", "beta", "running_mean", "running_var", "stats", "c", "reserved"]
