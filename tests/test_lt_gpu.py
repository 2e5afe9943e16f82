"""iif_lt_augment and DeviceLTLoader on the MI355X: every stage image by image against a torch oracle built from the same
descriptors (tests/lt_cases.py: interpolate(antialias=True), the window, the flip, augment.ColorJitter.apply, Normalize),
malformed descriptors, determinism per (seed, epoch, rank), two ranks, and the training CLI end to end on a .npy tree."""
import os
import re
import subprocess
import sys
from itertools import permutations

import numpy as np
import pytest
import torch

from iif_amd import augment, lt_device
from iif_amd.imbalanced_dataset import LT_Dataset, mean_std_hue

from .lt_cases import oracle, smooth_image, write_npy_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL, TOL_HUE = 1e-5, 2e-5             # max abs error on the [0, 1] scale
IMNET = mean_std_hue("imagenet_lt")[:2]
INAT = mean_std_hue("inat18")[:2]


def _launch(items, size, jitter=False, mean_std=IMNET, desc_override=None):
    """items: [(region, words, jitter tuple or None)]; returns (kernel images, oracle images) on the CPU."""
    samples = [(r, w, lt_device.jitter_record(*j) if j is not None else None, 0) for r, w, j in items]
    buf = lt_device.pack(samples)
    B = len(items)
    dev = buf.to(DEV)
    pool, desc, jit, _ = lt_device.unpack(dev, B)
    if desc_override is not None:
        desc = desc_override(desc.clone())
    out = lt_device.lt_augment(pool, desc, jit if jitter else None, size, *mean_std, lt_device.JITTER if jitter else 0)
    torch.cuda.synchronize()
    want = torch.stack([oracle(r, w, j if jitter else None, *mean_std, size) for r, w, j in items])
    return out.cpu(), want


def _err01(got, want, mean_std=IMNET):
    """max abs error on the [0, 1] scale, per image."""
    std = torch.tensor(mean_std[1]).view(1, 3, 1, 1)
    return ((got - want).abs() * std).flatten(1).max(1).values


def _check(got, want, tol, mean_std=IMNET):
    e = _err01(got, want, mean_std)
    print("max abs error on [0, 1]: %.3g" % float(e.max()))
    assert torch.isfinite(got).all() and float(e.max()) <= tol, e.tolist()


# ---------------------------------------------------------------------------------------------------------- geometry
GEOMETRY = [   # (region h, w), (rh, rw), (oy, ox)
    ((20, 30), (48, 48), (0, 0)),           # upscale
    ((5, 7), (48, 48), (0, 0)),             # ~8x upscale of a tiny region
    ((96, 100), (48, 48), (0, 0)),          # ~2x downscale
    ((480, 500), (48, 48), (0, 0)),         # ~10x downscale
    ((60, 200), (48, 48), (0, 0)),          # non-square region, different scales per axis
    ((1, 1), (48, 48), (0, 0)),             # a single pixel
    ((120, 90), (64, 55), (9, 3)),          # a window inside a non-square resize (the evaluation form)
    ((48, 48), (48, 48), (0, 0)),           # identity
]


@pytest.mark.parametrize("flip", [0, 1])
def test_resample_against_interpolate_antialias(flip):
    items = []
    for k, ((h, w), (rh, rw), (oy, ox)) in enumerate(GEOMETRY):
        items.append((smooth_image(h, w, k), (h, w, rh, rw, oy, ox, flip), None))
    got, want = _launch(items, 48)
    _check(got, want, TOL)


def test_large_image_at_224():
    img = smooth_image(900, 1200, 11)
    items = [(img, (900, 1200, 224, 224, 0, 0, 0), None), (img[100:800, 200:1100], (700, 900, 224, 224, 0, 0, 1), None),
             (img[:375, :500], (375, 500, 256, 341, 16, 58, 0), None)]
    got, want = _launch(items, 224)
    _check(got, want, TOL)


# ------------------------------------------------------------------------------------------------------------ colour
ALONE = [([0, 1, 2, 3], 1.35, None, None, None), ([0, 1, 2, 3], 0.62, None, None, None),
         ([1, 0, 2, 3], None, 1.38, None, None), ([1, 0, 2, 3], None, 0.61, None, None),
         ([2, 0, 1, 3], None, None, 1.4, None), ([2, 0, 1, 3], None, None, 0.6, None),
         ([3, 0, 1, 2], None, None, None, 0.21), ([3, 0, 1, 2], None, None, None, -0.25), ([3, 0, 1, 2], None, None, None, 0.0)]


def _jitter_items(jits, size=40, seed=0):
    items = []
    for k, j in enumerate(jits):
        h, w = 50 + 7 * (k % 5), 45 + 11 * (k % 3)
        items.append((smooth_image(h, w, seed + k), (h, w, size, size, 0, 0, k & 1), j))
    return items


def test_each_colour_op_alone():
    got, want = _launch(_jitter_items(ALONE), 40, jitter=True)
    hue = torch.tensor([j[4] is not None for j in ALONE])
    e = _err01(got, want)
    print("max abs error on [0, 1]: %.3g without hue, %.3g hue" % (float(e[~hue].max()), float(e[hue].max())))
    assert float(e[~hue].max()) <= TOL and float(e[hue].max()) <= TOL_HUE


@pytest.mark.parametrize("hue", [None, 0.13])
def test_all_24_orders_with_contrast(hue):
    jits = [(list(o), 1.25, 0.7, 1.3, hue) for o in permutations(range(4))]
    got, want = _launch(_jitter_items(jits, seed=30), 40, jitter=True)
    _check(got, want, TOL if hue is None else TOL_HUE)


def test_hue_with_the_inaturalist_constants():
    cj = augment.ColorJitter(0.4, 0.4, 0.4, mean_std_hue("inat18")[2])
    items = []
    for pos in range(24):
        img = smooth_image(70 + pos, 90 - pos, 100 + pos)
        region, words, rec = lt_device.train_sample(img, 32, lt_device.uniforms(5, 0, 0, pos), cj)
        _, _, order, f = lt_device.draw(img.shape[0], img.shape[1], lt_device.uniforms(5, 0, 0, pos), cj)
        items.append((region, words, (order, *f)))
    got, want = _launch(items, 32, jitter=True, mean_std=INAT)
    _check(got, want, TOL_HUE, INAT)


# --------------------------------------------------------------------------------------------- eval, mixed, malformed
def test_eval_path():
    items = []
    for k, (h, w) in enumerate([(300, 200), (200, 300), (250, 250), (40, 90), (500, 375)]):
        region, words, _ = lt_device.eval_sample(smooth_image(h, w, 50 + k), 64)
        items.append((region, words, None))
    got, want = _launch(items, 64)
    _check(got, want, TOL)


def test_mixed_size_training_batch():
    cj = augment.ColorJitter(0.4, 0.4, 0.4, 0.0)
    shapes = [(375, 500), (500, 333), (64, 48), (1200, 900), (10, 1000), (256, 256), (31, 17), (333, 500)]
    items = []
    for pos, (h, w) in enumerate(shapes):
        img = smooth_image(h, w, 70 + pos)
        u = lt_device.uniforms(2, 1, 0, pos)
        region, words, _ = lt_device.train_sample(img, 96, u, cj)
        _, _, order, f = lt_device.draw(h, w, u, cj)
        items.append((region, words, (order, *f)))
    got, want = _launch(items, 96, jitter=True)
    _check(got, want, TOL)


def test_malformed_descriptors_give_zeros():
    base = (smooth_image(40, 50, 1), (40, 50, 32, 32, 0, 0, 0), ([1, 0, 2, 3], 1.1, 0.8, 1.2, None))
    items = [base] * 10

    def corrupt(d):
        d[1, 0] = 1 << 40                      # offset past the pool
        d[2, 1] = 0                            # height 0
        d[3, 2] = -5                           # negative width
        d[4, 3] = 31                           # rh < oy + S
        d[5, 6] = 1                            # ox + S > rw
        d[6, 5] = -1                           # negative window origin
        d[7, 0] = -16                          # negative offset
        d[8, 1] = 10 ** 6                      # a region larger than the pool
        return d
    got, want = _launch(items, 32, jitter=True, desc_override=corrupt)
    assert all(torch.count_nonzero(got[i]) == 0 for i in range(1, 9))
    _check(got[[0, 9]], want[[0, 9]], TOL)


# ------------------------------------------------------------------------------------------------------------ loader
@pytest.fixture(scope="module")
def npy_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("lt")
    rng = np.random.RandomState(0)
    shapes = [(int(rng.randint(40, 120)), int(rng.randint(40, 120)), 3) for _ in range(37)]
    shapes[3], shapes[8] = (60, 70), (50, 40, 4)            # a grey and an RGBA image
    labels = [i % 5 for i in range(37)]
    train_txt, eval_txt = write_npy_tree(str(root), shapes, labels, eval_count=11)
    return str(root), train_txt, eval_txt


def _collect(loader):
    out = [(x.cpu(), t.cpu()) for x, t in loader]
    torch.cuda.synchronize()
    return out


def test_loader_matches_the_oracle_and_repeats_per_seed_epoch_rank(npy_tree):
    root, train_txt, _ = npy_tree
    ds = LT_Dataset(root, train_txt, 5)
    ld = lt_device.DeviceLTLoader(ds, 8, train=True, size=32, dset_name="inat18", seed=4, workers=2, device=DEV)
    ld.set_epoch(3)
    a = _collect(ld)
    inline = lt_device.DeviceLTLoader(ds, 8, train=True, size=32, dset_name="inat18", seed=4, workers=0, device=DEV)
    b = _collect(inline)                                             # epoch 0
    inline.set_epoch(3)
    c = _collect(inline)                                             # epoch 3 without worker processes
    ld.set_epoch(3)
    d = _collect(ld)
    assert len(a) == len(ds) // 8
    # the same (seed, epoch, rank) gives the same batches, with 2 workers or none, run after run
    for other in (c, d):
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, other))
    assert not torch.equal(a[0][0], b[0][0])
    idx = ld.indices(3)
    items = []
    for p in range(8):
        i = int(idx[p])
        img = lt_device.to_hwc3(ds.loader(ds.img_path[i]))
        u = lt_device.uniforms(4, 3, 0, p)
        region, words, _ = lt_device.train_sample(img, 32, u, ld.jitter)
        _, _, order, f = lt_device.draw(img.shape[0], img.shape[1], u, ld.jitter)
        items.append(oracle(region, words, (order, *f), *INAT, 32))
        assert int(a[0][1][p]) == ds.targets[i], p
    _check(a[0][0], torch.stack(items), TOL_HUE, INAT)


def test_eval_loader_covers_everything_in_order(npy_tree):
    root, train_txt, eval_txt = npy_tree
    from iif_amd.imbalanced_dataset import LT_Dataset_Eval
    ds = LT_Dataset(root, train_txt, 5)
    ev = LT_Dataset_Eval(root, eval_txt, ds.class_map, 5)
    ld = lt_device.DeviceLTLoader(ev, 4, train=False, size=32, workers=0, device=DEV)
    got = _collect(ld)
    assert [len(t) for _, t in got] == [4, 4, 3]
    assert torch.cat([t for _, t in got]).tolist() == ev.targets
    items = []
    for i in range(len(ev)):
        region, words, _ = lt_device.eval_sample(ev.loader(ev.img_path[i]), 32)
        items.append(oracle(region, words, None, *IMNET, 32))
    _check(torch.cat([x for x, _ in got]), torch.stack(items), TOL)


# ------------------------------------------------------------------------------------------------ two ranks, CLI
def _run(cmd, env=None, timeout=900):
    r = subprocess.run(cmd, env=env or dict(os.environ), capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_see_disjoint_shards(npy_tree, tmp_path):
    root, train_txt, _ = npy_tree
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), os.path.join(HERE, "lt_ddp_worker.py"), root, train_txt, str(tmp_path)], env=env)
    r = [torch.load(tmp_path / ("rank%d.pt" % k)) for k in (0, 1)]
    a, b = r[0]["index"], r[1]["index"]
    assert len(a) == len(b) == 19                          # 37 samples: DistributedSampler pads with one repeat
    assert set(a.tolist()) | set(b.tolist()) == set(range(37)) and len(set(a.tolist()) & set(b.tolist())) <= 1
    targets = torch.tensor(r[0]["targets_all"])
    for k in (0, 1):
        n = len(r[k]["targets"])
        assert torch.equal(r[k]["targets"], targets[r[k]["index"][:n]])
    assert not torch.equal(r[0]["images"], r[1]["images"])


def test_train_cli_places_lt_device_augment(tmp_path):
    rng = np.random.RandomState(1)
    shapes = [(int(rng.randint(60, 140)), int(rng.randint(60, 140)), 3) for _ in range(48)]
    train_txt, eval_txt = write_npy_tree(str(tmp_path), shapes, [i % 6 for i in range(48)], eval_count=16)
    out = _run([sys.executable, "-m", "iif_amd.train", "--dset_name", "places_lt", "--data-path", str(tmp_path),
                "--train-txt", train_txt, "--eval-txt", eval_txt, "--device-augment", "--model", "resnet18",
                "--image-size", "64", "-b", "8", "-j", "2", "--epochs", "1", "--max-iters", "3"], timeout=600)
    assert re.search(r"\* Acc@1 \S+ Acc@5", out)
