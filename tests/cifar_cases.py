"""Shared cases of the CIFAR tests: fake CIFAR trees in torchvision's layout, the test images, and the host oracle of
``iif_cifar_augment``: each image rebuilt from the kernel's dumped draws with torch ops (F.pad, slicing, flip, ToTensor's
division, augment.apply_op_signed, the reference's Cutout mask product, Normalize's sub / div)."""
import os
import pickle

import numpy as np
import torch

from iif_amd import augment
from iif_amd.cifar import CROP_FLIP, CUTOUT, MEAN, POLICY, STD

LAYOUTS = {
    "cifar10": ("cifar-10-batches-py", ["data_batch_%d" % i for i in range(1, 6)], ["test_batch"], "labels", 10),
    "cifar100": ("cifar-100-python", ["train"], ["test"], "fine_labels", 100),
}


def fake_rows(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, 3072)).astype(np.uint8)


def write_fake_cifar(root, name, train_per_class, test_per_class, seed=0):
    """A CIFAR tree with random images and shuffled balanced labels; returns (train data, train labels, test data, test
    labels) as the reader must return them (train batches concatenated in file order)."""
    folder, train_files, test_files, key, C = LAYOUTS[name]
    os.makedirs(os.path.join(root, folder), exist_ok=True)
    rng = np.random.RandomState(seed)
    out = []
    for files, per in ((train_files, train_per_class), (test_files, test_per_class)):
        labels = rng.permutation(np.repeat(np.arange(C), per))
        data = fake_rows(len(labels), seed + len(files))
        for f, d, t in zip(files, np.array_split(data, len(files)), np.array_split(labels, len(files))):
            with open(os.path.join(root, folder, f), "wb") as fh:
                pickle.dump({"data": d, key: t.tolist(), "batch_label": f}, fh, protocol=2)
        out += [data, labels.astype(np.int64)]
    return tuple(out)


def case_images(n=64, seed=7):
    """uint8 [n, 3072]: random images plus the corner cases of the ops - constant (AutoContrast's h == l, Equalize's
    step 0), black, white, narrow-range, two-level and nearly-constant images."""
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 256, size=(n, 3072)).astype(np.uint8)
    x[0] = 128
    x[1] = 0
    x[2] = 255
    x[3] = rng.randint(100, 111, size=3072)
    x[4] = np.where(rng.rand(3072) < 0.5, 40, 210)
    x[5] = 200
    x[5, rng.randint(0, 3072, size=40)] = rng.randint(0, 256, size=40)
    x[6] = np.tile(np.arange(32, dtype=np.uint8) * 8, 96)
    x[7] = rng.randint(0, 16, size=3072) * 17
    return x


def one_sub_policy(name, mag, prob=1.0):
    """25 identical sub-policies: ``name`` at magnitude index ``mag`` applied with ``prob``, its second op never."""
    return [(name, prob, mag, "Invert", 0.0, 0)] * 25


def oracle(rows, params, flags, subs=None):
    """fp32 [B, 3, 32, 32]: the reference's transform of each row (uint8 [3072]) with the draws of ``params`` [B, 10]."""
    subs = augment._P["cifar10"] if subs is None else subs
    mean = torch.tensor(MEAN, dtype=torch.float32)[:, None, None]
    std = torch.tensor(STD, dtype=torch.float32)[:, None, None]
    out = torch.empty(len(rows), 3, 32, 32)
    for i, (row, p) in enumerate(zip(rows, params)):
        img = torch.from_numpy(np.ascontiguousarray(row)).view(3, 32, 32)
        if flags & CROP_FLIP:                               # RandomCrop(32, padding=4), RandomHorizontalFlip
            img = torch.nn.functional.pad(img, (4, 4, 4, 4))[:, p[0]:p[0] + 32, p[1]:p[1] + 32]
            if p[2]:
                img = img.flip(-1)
        x = img.float().div(255)                            # ToTensor
        if flags & POLICY:
            sub = subs[p[3]]
            for j in range(2):
                if p[4 + 2 * j]:
                    x = augment.apply_op_signed(x, sub[3 * j], sub[3 * j + 2], 1.0 if p[5 + 2 * j] else -1.0)
        if flags & CUTOUT:                                  # presets.Cutout(1, 16)
            mask = np.ones((32, 32), np.float32)
            y1, y2 = np.clip(p[8] - 8, 0, 32), np.clip(p[8] + 8, 0, 32)
            x1, x2 = np.clip(p[9] - 8, 0, 32), np.clip(p[9] + 8, 0, 32)
            mask[y1:y2, x1:x2] = 0.0
            x = x * torch.from_numpy(mask).expand_as(x)
        out[i] = (x - mean) / std                           # Normalize
    return out
