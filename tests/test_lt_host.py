"""List-dataset device input without a device: the host draws (RandomResizedCrop box, flip, jitter order and factors) and
their keys, the evaluation geometry against TensorTransform, the packed batch layout, ColorJitter's split into
factors / apply, the CLI refusals of --device-augment, get_data's choice of loader, and the argument checks of
iif_lt_augment (which return before any HIP call)."""
import ctypes
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from iif_amd import _lib, augment, initialisers, lt_device, train
from iif_amd.imbalanced_dataset import TensorTransform, eval_geometry, mean_std_hue

from .lt_cases import oracle, smooth_image, write_npy_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


# ---------------------------------------------------------------------------------------------------------- draws
def _box_ok(h, w, box):
    top, left, ch, cw = box
    assert 0 <= top and top + ch <= h and 0 <= left and left + cw <= w and ch > 0 and cw > 0
    if (ch, cw) == (min(h, w), min(h, w)) and (top, left) == ((h - ch) // 2, (w - cw) // 2):
        return "fallback"
    # the drawn area (0.08 .. 1 of the image) and ratio (3/4 .. 4/3) before rounding to whole pixels
    assert (cw + 0.5) * (ch + 0.5) >= 0.08 * h * w and (cw - 0.5) * (ch - 0.5) <= h * w
    assert (cw + 0.5) / (ch - 0.5 if ch > 0.5 else 1e-9) >= 3 / 4 and (cw - 0.5) / (ch + 0.5) <= 4 / 3
    return "drawn"


@pytest.mark.parametrize("shape", [(375, 500), (500, 333), (256, 256), (40, 41), (10, 1000), (1000, 10), (1, 1)])
def test_boxes_inside_the_image_with_area_and_ratio_in_range(shape):
    h, w = shape
    kinds = set()
    for pos in range(300):
        box, flip, _, _ = lt_device.draw(h, w, lt_device.uniforms(7, 1, 0, pos))
        kinds.add(_box_ok(h, w, box))
    if shape in ((10, 1000), (1000, 10)):
        assert kinds == {"fallback"}                 # no box of ratio <= 4/3 and area >= 8 % fits: the centre square
    elif min(shape) > 1:
        assert "drawn" in kinds


def test_draws_are_deterministic_per_key_and_differ_across_epochs_and_ranks():
    cj = augment.ColorJitter(0.4, 0.4, 0.4, 0.25)

    def d(seed, epoch, rank, pos):
        box, flip, order, f = lt_device.draw(400, 300, lt_device.uniforms(seed, epoch, rank, pos), cj)
        return box, flip, tuple(order), f
    a = [d(3, 2, 1, p) for p in range(64)]
    assert a == [d(3, 2, 1, p) for p in range(64)]
    assert len(set(a)) == 64                                       # positions differ
    for other in ([d(3, 3, 1, p) for p in range(64)], [d(3, 2, 0, p) for p in range(64)], [d(4, 2, 1, p) for p in range(64)]):
        assert sum(x == y for x, y in zip(a, other)) == 0
    u = lt_device.uniforms(3, 2, 1, 5)
    assert u.shape == (lt_device.N_SLOTS,) and (u >= 0).all() and (u < 1).all()


def test_jitter_draws_cover_every_order_and_the_factor_ranges():
    cj = augment.ColorJitter(0.4, 0.4, 0.4, 0.25)
    orders, fs = set(), []
    for pos in range(2000):
        _, _, order, f = lt_device.draw(50, 60, lt_device.uniforms(1, 0, 0, pos), cj)
        assert sorted(order) == [0, 1, 2, 3]
        orders.add(tuple(order))
        fs.append(f)
    fs = np.asarray(fs)
    assert len(orders) == 24
    assert (fs[:, :3] >= 0.6).all() and (fs[:, :3] <= 1.4).all() and (np.abs(fs[:, 3]) <= 0.25).all()
    _, _, _, f = lt_device.draw(50, 60, lt_device.uniforms(1, 0, 0, 0), augment.ColorJitter(0.4, 0.4, 0.4, 0.0))
    assert f[3] is None                                            # hue 0 (all but iNaturalist): no shift drawn


def test_flip_is_a_fair_coin():
    n = 4000
    flips = sum(lt_device.draw(64, 64, lt_device.uniforms(9, 0, 0, p))[1] for p in range(n))
    assert abs(flips - n / 2) < 5 * math.sqrt(n / 4)


def test_colour_jitter_call_is_factors_then_apply():
    x = torch.rand(3, 9, 11, generator=torch.Generator().manual_seed(0))
    for hue in (0.0, 0.25):
        cj = augment.ColorJitter(0.4, 0.4, 0.4, hue)
        for s in range(5):
            g1, g2 = torch.Generator().manual_seed(s), torch.Generator().manual_seed(s)
            got = cj(x.clone(), g1)
            order = torch.randperm(4, generator=g2).tolist()
            want = cj.apply(x.clone(), order, *cj.factors(lambda: torch.rand((), generator=g2).item()))
            assert torch.equal(got, want)


def test_dataset_constants():
    assert mean_std_hue("inat18") == ((0.466, 0.471, 0.380), (0.195, 0.194, 0.192), 0.25)
    for name in ("imagenet_lt", "places_lt"):
        assert mean_std_hue(name) == ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 0.0)
    ld = [0, 1]                                                   # any sized dataset
    assert lt_device.DeviceLTLoader(ld, 1, dset_name="inat18", device="cpu").jitter.hue == 0.25
    assert lt_device.DeviceLTLoader(ld, 1, dset_name="places_lt", device="cpu").jitter.hue == 0.0
    assert lt_device.DeviceLTLoader(ld, 1, train=False, device="cpu").flags == 0


# ------------------------------------------------------------------------------------------------ evaluation geometry
@pytest.mark.parametrize("shape", [(300, 200, 3), (200, 300, 3), (250, 250, 3), (37, 90, 3), (64, 32)])
@pytest.mark.parametrize("dset", ["imagenet_lt", "inat18"])
def test_eval_geometry_equals_tensor_transform(shape, dset):
    img = smooth_image(shape[0], shape[1], 3)
    if len(shape) == 2:
        img = img[:, :, 0]
    size = 32
    region, words, rec = lt_device.eval_sample(img, size)
    h, w = shape[:2]
    nh, nw, top, left = eval_geometry(h, w, size)
    assert words == (h, w, nh, nw, top, left, 0) and rec is None and min(nh, nw) == round(size * 256 / 224)
    mean, std, _ = mean_std_hue(dset)
    want = TensorTransform(dset, False, size)(img)
    assert torch.equal(oracle(region, words, None, mean, std, size), want)


# ---------------------------------------------------------------------------------------------------------- packing
def test_pack_ragged_grey_and_rgba():
    imgs = [smooth_image(30, 41, 1), smooth_image(17, 5, 2)[:, :, 0], smooth_image(22, 33, 3, channels=4),
            smooth_image(8, 9, 4, channels=1), smooth_image(60, 61, 5)]
    cj = augment.ColorJitter(0.4, 0.4, 0.4, 0.25)
    samples = []
    for i, im in enumerate(imgs):
        region, words, rec = lt_device.train_sample(im, 16, lt_device.uniforms(0, 0, 0, i), cj)
        assert region.dtype == np.uint8 and region.ndim == 3 and region.shape[2] == 3 and region.flags.c_contiguous
        samples.append((region, words, rec, 10 + i))
    buf = lt_device.pack(samples)
    assert buf.dtype == torch.uint8 and buf.dim() == 1
    pool, desc, jit, tgt = lt_device.unpack(buf, len(samples))
    assert tgt.tolist() == [10, 11, 12, 13, 14]
    end = 0
    for i, (region, words, rec, _) in enumerate(samples):
        off = int(desc[i, 0])
        assert off % 16 == 0 and off >= end
        end = off + region.nbytes
        assert tuple(desc[i, 1:].tolist()) == tuple(words) and words[:2] == region.shape[:2]
        assert np.array_equal(pool[off:end].numpy(), region.reshape(-1))
        assert np.array_equal(jit[i].numpy().view(np.uint32), rec)
    assert end <= pool.numel()
    grey = lt_device.to_hwc3(imgs[1])
    assert np.array_equal(grey[:, :, 0], imgs[1]) and np.array_equal(grey[:, :, 2], imgs[1])
    assert np.array_equal(lt_device.to_hwc3(imgs[2]), imgs[2][:, :, :3])
    with pytest.raises(TypeError):
        lt_device.to_hwc3(np.zeros((4, 4, 3), np.float32))


def test_jitter_record_words():
    rec = lt_device.jitter_record([2, 0, 3, 1], 1.2, 0.7, None, None)
    assert rec[0] == 2 | (0 << 2) | (3 << 4) | (1 << 6)
    f = rec[1:].view(np.float32)
    assert f.tolist() == np.asarray([1.2, 1.0 - 1.2, 0.7, 1.0 - 0.7, 1.0, 0.0, 0.0], np.float32).tolist()


def test_eval_sample_ships_the_whole_image_and_train_only_the_box():
    img = smooth_image(300, 400, 0)
    region, words, _ = lt_device.eval_sample(img, 224)
    assert region.shape == (300, 400, 3)
    box, _, _, _ = lt_device.draw(300, 400, lt_device.uniforms(0, 0, 0, 3))
    region, words, _ = lt_device.train_sample(img, 224, lt_device.uniforms(0, 0, 0, 3))
    top, left, ch, cw = box
    assert np.array_equal(region, img[top:top + ch, left:left + cw]) and words[2:6] == (224, 224, 0, 0)


# ------------------------------------------------------------------------------------------------------------ wiring
def _args(tmp_path, **kw):
    train_txt, eval_txt = write_npy_tree(str(tmp_path), [(40 + i, 50, 3) for i in range(13)],
                                         [0] * 2 + [1] * 7 + [2] * 4, eval_count=5)
    a = dict(dset_name="places_lt", data_path=str(tmp_path), train_txt=train_txt, eval_txt=eval_txt, image_size=32,
             rand_number=0, sampler="random", distributed=False, batch_size=4, workers=0, device="cpu")
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_get_data_keeps_the_host_loader_without_the_flag(tmp_path):
    args = _args(tmp_path)
    ds, C, loader, loader_test, sampler = initialisers.get_data(args)
    assert isinstance(loader, torch.utils.data.DataLoader) and isinstance(ds.transform, TensorTransform)
    args.device_augment = False
    assert isinstance(initialisers.get_data(args)[2], torch.utils.data.DataLoader)


def test_get_data_takes_the_device_loader_with_the_flag(tmp_path):
    args = _args(tmp_path, device_augment=True, sampler="upsampling")
    ds, C, loader, loader_test, sampler = initialisers.get_data(args)
    assert isinstance(loader, lt_device.DeviceLTLoader) and sampler is loader and ds.transform is None
    assert isinstance(loader_test, lt_device.DeviceLTLoader) and not loader_test.train
    assert ds.cls_num_list[:3] == [7, 4, 2] and C == len(ds.cls_num_list) == 365 and loader.flags == lt_device.JITTER and loader.mode == "upsampling"
    assert len(loader) == 21 // 4 and len(loader_test) == 2
    assert loader_test.dataset.targets == [2, 2, 0, 0, 0]


def test_cli_refusals():
    ns = dict(device_augment=True, data_path="/data", dset_name="places_lt", auto_augment=None)
    train.check_device_augment(types.SimpleNamespace(**ns))                   # accepted
    for kw in ({"data_path": ""}, {"auto_augment": "imagenet"}, {"auto_augment": "randaugment"}, {"auto_augment": "cifar"}):
        with pytest.raises(SystemExit):
            train.check_device_augment(types.SimpleNamespace(**dict(ns, **kw)))
    train.check_device_augment(types.SimpleNamespace(**dict(ns, dset_name="cifar100", auto_augment="cifar")))   # no-op there
    train.check_device_augment(types.SimpleNamespace(**dict(ns, device_augment=False, data_path="")))
    args = train.get_args_parser().parse_args(["--dset_name", "inat18", "--device-augment"])
    assert args.device_augment is True
    assert train.get_args_parser().parse_args([]).device_augment is False


@pytest.mark.parametrize("extra,msg", [([], "needs --data-path"), (["--data-path", "/x", "--auto-augment", "imagenet"],
                                                                     "stays on the host")])
def test_cli_refuses_before_touching_a_device(extra, msg):
    r = subprocess.run([sys.executable, "-m", "iif_amd.train", "--dset_name", "places_lt", "--device-augment"] + extra,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and msg in r.stderr, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbol_in_header_and_ctypes_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    assert re.search(r"int iif_lt_augment\(", text) and re.search(r"#define IIF_LT_JITTER %du" % lt_device.JITTER, text)
    assert len(_lib.SIGNATURES["iif_lt_augment"]) == 10
    assert hasattr(_lib.lib(), "iif_lt_augment")


def test_argument_checks_return_einval_without_a_device():
    f = _lib.lib().iif_lt_augment
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)                       # never dereferenced as device memory: every call returns before any launch

    def call(pool=p, nbytes=64, desc=p, jitter=p, batch=2, size=8, ms=p, flags=1, out=p):
        return f(pool, nbytes, desc, jitter, batch, size, ms, flags, out, None)
    for kw in ({"pool": 0}, {"desc": 0}, {"ms": 0}, {"out": 0}, {"jitter": 0}, {"nbytes": -1}, {"batch": -1}, {"size": 0},
               {"size": -3}, {"size": 16385}, {"flags": 2}, {"flags": 0x81}):
        assert call(**kw) == EINVAL, kw
    assert call(batch=0) == 0 and call(batch=0, jitter=0, flags=0) == 0          # nothing to do, no launch
