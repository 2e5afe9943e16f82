"""iif_lt_augment_policy and DeviceLTLoader(policy=...) on the MI355X, against a torch oracle: the geometry of
tests/lt_cases.oracle (interpolate(antialias=True), window, flip), clamp(0, 1), augment.apply_op_signed per applied op,
Normalize.  Every op at every magnitude and sign at identity geometry; the 25 ImageNet sub-policies and RandAugment with
real resizes at S = 224; two ops whose pixels pass between sweeps; bad descriptors and op codes; the loader; the CLI.

A last-ulp difference between the kernel's resize (or its double-summed grey mean) and torch's can move a uint8 quantiser
(Posterize, Solarize, Equalize) by one level.  Where the geometry is a real resize, the ops are therefore also checked
against an oracle that starts from the kernel's own geometry (the same launch with no op and mean 0, std 1, which returns
the clamped resampled image exactly), and that geometry against torch's."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from iif_amd import augment, cifar, lt_device
from iif_amd.imbalanced_dataset import LT_Dataset, mean_std_hue

from .lt_cases import smooth_image, write_npy_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5                                    # max abs error on the [0, 1] scale
LEVEL = 1.0 / 255.0
MEAN, STD = mean_std_hue("imagenet_lt")[:2]
QUANTISERS = ("Posterize", "Solarize", "Equalize")


def _geometry(region, words, size):
    h, w, rh, rw, oy, ox, flip = [int(v) for v in words]
    t = torch.from_numpy(np.ascontiguousarray(region)).permute(2, 0, 1).float() / 255.0
    t = torch.nn.functional.interpolate(t[None], size=(rh, rw), mode="bilinear", align_corners=False, antialias=True)[0]
    t = t[:, oy:oy + size, ox:ox + size]
    return (t.flip(-1) if flip else t).clamp(0.0, 1.0)


def _ops_oracle(t, ops, mean=MEAN, std=STD):
    """augment.apply_op_signed for each applied op slot on a clamped [0, 1] image, then Normalize."""
    for op in ops:
        if op is not None:
            t = augment.apply_op_signed(t, op[0], op[1], op[2])
    return (t - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)


def _launch(items, size, mean=MEAN, std=STD, desc_override=None, ops_override=None):
    """items: [(region, words, [op slot, op slot])]; the kernel's images on the CPU."""
    samples = [(r, w, None, 0, lt_device.policy_record(ops, size)) for r, w, ops in items]
    B = len(items)
    pool, desc, _, _, rec = lt_device.unpack(lt_device.pack(samples).to(DEV), B, policy=True)
    if desc_override is not None:
        desc = desc_override(desc.clone())
    if ops_override is not None:
        rec = ops_override(rec.clone())
    out = lt_device.lt_augment_policy(pool, desc, rec, size, mean, std)
    torch.cuda.synchronize()
    return out.cpu()


def _kernel_geometry(items, size):
    """The kernel's clamped resampled images: no op, mean 0, std 1."""
    return _launch([(r, w, [None, None]) for r, w, _ in items], size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _err01(got, want):
    return (got - want).abs() * torch.tensor(STD).view(1, 3, 1, 1)


def _identity_items(size, seed):
    items = []
    for k, name in enumerate(cifar.OPS):
        img = smooth_image(size, size, seed + k)
        img = (20 + img.astype(np.int64) * 180 // 255).astype(np.uint8)    # not full range: AutoContrast stretches it
        for mag in range(10):
            for sign in (-1.0, 1.0):
                slot = (name, mag, sign)
                ops = [slot, None] if (mag + int(sign > 0)) % 2 == 0 else [None, slot]
                items.append((img, (size, size, size, size, 0, 0, mag & 1), ops))
    return items


# ------------------------------------------------------------------------------------------------ one op at a time
@pytest.mark.parametrize("size", [48, 37])
def test_every_op_magnitude_and_sign_at_identity_geometry(size):
    items = _identity_items(size, 3)
    got = _launch(items, size)
    want = torch.stack([_ops_oracle(_geometry(r, w, size), ops) for r, w, ops in items])
    err = _err01(got, want).flatten(1).max(1).values
    worst = {}
    for i, (_, _, ops) in enumerate(items):
        name = (ops[0] or ops[1])[0]
        worst[name] = max(worst.get(name, 0.0), float(err[i]))
        if name in QUANTISERS:                             # uint8 levels / 255: bit for bit
            assert torch.equal(got[i], want[i]), (i, ops)
    print("max abs error on [0, 1] per op:", {k: "%.2g" % v for k, v in worst.items()})
    assert torch.isfinite(got).all() and float(err.max()) <= TOL, worst


def test_no_op_gives_the_values_of_iif_lt_augment():
    items = []
    for k, ((h, w), (rh, rw), (oy, ox)) in enumerate([((300, 400), (224, 224), (0, 0)), ((90, 120), (224, 224), (0, 0)),
                                                       ((375, 500), (256, 341), (16, 58))]):
        items.append((smooth_image(h, w, 40 + k), (h, w, rh, rw, oy, ox, k & 1), [None, None]))
    got = _kernel_geometry(items, 224)
    pool, desc, jit, _ = lt_device.unpack(lt_device.pack([(r, w, None, 0) for r, w, _ in items]).to(DEV), len(items))
    ref = lt_device.lt_augment(pool, desc, None, 224, (0.0,) * 3, (1.0,) * 3, 0).clamp(0.0, 1.0).cpu()
    assert torch.equal(got, ref)
    want = torch.stack([_geometry(r, w, 224) for r, w, _ in items])
    assert float((got - want).abs().max()) <= TOL


# ------------------------------------------------------------------------------------------ whole policies at S = 224
def _resized_items(n, seed, ops_of):
    rng = np.random.RandomState(seed)
    items = []
    for k in range(n):
        h, w = int(rng.randint(256, 501)), int(rng.randint(256, 501))
        img = smooth_image(h, w, seed + k)
        region, words, _ = lt_device.train_sample(img, 224, lt_device.uniforms(seed, 0, 0, k))
        items.append((region, words, ops_of(k)))
    return items


def _check_policy_batch(items, strict):
    """Against the oracle on the kernel's geometry: strict -> at least 99 % of the images within TOL, the rest within one
    uint8 level; otherwise (a grey mean / blur summed in another order can feed a quantiser) 99 % of each image's values
    within TOL.  Against torch's geometry: 99 % of each image's values within TOL."""
    got = _launch(items, 224)
    geo = _kernel_geometry(items, 224)
    want = torch.stack([_ops_oracle(geo[i], ops) for i, (_, _, ops) in enumerate(items)])
    err = _err01(got, want).flatten(1)
    worst = err.max(1).values
    print("images within TOL: %d / %d, worst %.3g" % (int((worst <= TOL).sum()), len(items), float(worst.max())))
    assert torch.isfinite(got).all()
    if strict:
        assert int((worst <= TOL).sum()) >= 0.99 * len(items) and float(worst.max()) <= LEVEL + TOL, worst.tolist()
    else:
        assert float((err <= TOL).float().mean(1).min()) >= 0.99
    aten = torch.stack([_ops_oracle(_geometry(r, w, 224), ops) for r, w, ops in items])
    frac = (_err01(got, aten).flatten(1) <= TOL).float().mean(1)
    print("values within TOL of the ATen-geometry oracle: worst image %.5f" % float(frac.min()))
    assert float(frac.min()) >= 0.99


def test_all_25_imagenet_sub_policies_at_224():
    subs = augment._P["imagenet"]

    def ops_of(k):
        sub = subs[k % 25]
        signs = (1.0 if k & 1 else -1.0, 1.0 if k & 2 else -1.0)
        return [(sub[0], sub[2], signs[0]), (sub[3], sub[5], signs[1])]
    _check_policy_batch(_resized_items(50, 11, ops_of), strict=True)


def test_randaugment_batch_at_224():
    def ops_of(k):
        return lt_device.draw_policy("randaugment", lt_device.policy_uniforms(5, 0, 0, k))
    _check_policy_batch(_resized_items(48, 12, ops_of), strict=False)


@pytest.mark.parametrize("pair", [("Equalize", "Rotate"), ("Rotate", "Equalize"), ("Rotate", "Sharpness"),
                                  ("Sharpness", "ShearX"), ("TranslateX", "TranslateY"), ("AutoContrast", "Contrast"),
                                  ("Equalize", "Equalize"), ("ShearY", "AutoContrast"), ("Solarize", "Rotate")])
def test_two_ops_whose_pixels_pass_between_sweeps(pair):
    def ops_of(k):
        return [(pair[0], 3 + k % 7, 1.0 if k & 1 else -1.0), (pair[1], 9 - k % 5, 1.0 if k & 2 else -1.0)]
    _check_policy_batch(_resized_items(6, 20 + len(pair[0]) + 3 * len(pair[1]), ops_of), strict=True)


# ------------------------------------------------------------------------------------------------------- bad inputs
def test_bad_descriptor_or_op_code_gives_a_zero_image():
    img = smooth_image(60, 70, 1)
    items = [(img, (60, 70, 32, 32, 0, 0, k & 1), [("Rotate", 5, 1.0), ("Equalize", 0, 1.0)]) for k in range(6)]

    def bad_desc(d):
        d[1, 3] = 31                                       # rh < oy + S
        return d

    def bad_ops(r):
        r[3, 0, 0] = 14                                    # one past Invert
        r[4, 1, 0] = 0x7F
        return r
    got = _launch(items, 32, desc_override=bad_desc, ops_override=bad_ops)
    assert all(torch.count_nonzero(got[i]) == 0 for i in (1, 3, 4))
    want = torch.stack([_ops_oracle(_geometry(r, w, 32), ops) for r, w, ops in items])
    keep = [0, 2, 5]
    assert float(_err01(got[keep], want[keep]).max()) <= TOL


# ------------------------------------------------------------------------------------------------------------ loader
@pytest.fixture(scope="module")
def npy_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("ltp")
    rng = np.random.RandomState(2)
    shapes = [(int(rng.randint(40, 120)), int(rng.randint(40, 120)), 3) for _ in range(29)]
    train_txt, eval_txt = write_npy_tree(str(root), shapes, [i % 4 for i in range(29)], eval_count=9)
    return str(root), train_txt


@pytest.mark.parametrize("policy", ["imagenet", "randaugment"])
def test_loader_repeats_per_seed_and_matches_the_oracle(npy_tree, policy):
    root, train_txt = npy_tree
    ds = LT_Dataset(root, train_txt, 4)

    def run(workers):
        ld = lt_device.DeviceLTLoader(ds, 8, train=True, size=40, seed=6, workers=workers, device=DEV, policy=policy)
        ld.set_epoch(2)
        out = [(x.cpu(), t.cpu()) for x, t in ld]
        torch.cuda.synchronize()
        return ld, out
    ld, a = run(2)
    _, b = run(0)
    assert len(a) == len(ds) // 8 and ld.jitter is None
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    idx = ld.indices(2)
    items = []
    for p in range(8):
        i = int(idx[p])
        img = lt_device.to_hwc3(ds.loader(ds.img_path[i]))
        region, words, _ = lt_device.train_sample(img, 40, lt_device.uniforms(6, 2, 0, p))
        items.append((region, words, lt_device.draw_policy(policy, lt_device.policy_uniforms(6, 2, 0, p))))
        assert int(a[0][1][p]) == ds.targets[i]
    geo = _kernel_geometry(items, 40)
    want = torch.stack([_ops_oracle(geo[k], ops) for k, (_, _, ops) in enumerate(items)])
    frac = (_err01(a[0][0], want).flatten(1) <= TOL).float().mean(1)
    assert float(frac.min()) >= 0.99, frac.tolist()


# --------------------------------------------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("policy", ["imagenet", "randaugment"])
def test_train_cli_device_policy(tmp_path, policy):
    rng = np.random.RandomState(3)
    shapes = [(int(rng.randint(60, 140)), int(rng.randint(60, 140)), 3) for _ in range(48)]
    train_txt, eval_txt = write_npy_tree(str(tmp_path), shapes, [i % 6 for i in range(48)], eval_count=16)
    r = subprocess.run([sys.executable, "-m", "iif_amd.train", "--dset_name", "places_lt", "--data-path", str(tmp_path),
                        "--train-txt", train_txt, "--eval-txt", eval_txt, "--device-augment", "--device-policy",
                        "--auto-augment", policy, "--model", "resnet18", "--image-size", "64", "-b", "8", "-j", "2",
                        "--epochs", "1", "--max-iters", "3"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    out = r.stdout + r.stderr
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert re.search(r"\* Acc@1 \S+ Acc@5", out)
