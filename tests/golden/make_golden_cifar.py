#!/usr/bin/env python3
"""Generate tests/golden/g21_cifar_imb.npz by RUNNING THE REFERENCE's ``IMBALANCECIFAR10`` / ``IMBALANCECIFAR100``
(classification/imbalanced_dataset.py:12-70) on CPU.

The file is imported as-is.  In this process only, placeholder modules stand in for torchvision, PIL, catalyst and
randaugment (image IO and samplers; as make_golden.py does); here ``torchvision.datasets.CIFAR10`` is a stub whose
``__init__`` sets ``targets`` to a seeded permutation of 5000 (CIFAR-10) / 500 (CIFAR-100) labels per class and ``data``
to rows holding their own source index, so the reference's selection comes out as source indices.  Only data is
written: the fake labels, the selected source indices, the targets and get_cls_num_list().

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cifar.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/classification"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

CONFIGS = [("exp", 0.01), ("exp", 0.02), ("exp", 0.1), ("step", 0.1)]
RAND_NUMBERS = (0, 1)
LABEL_SEED = 2021


def fake_labels(cls_num):
    per = 5000 if cls_num == 10 else 500
    return np.random.RandomState(LABEL_SEED + cls_num).permutation(np.repeat(np.arange(cls_num), per))


def _placeholder_modules():
    class _CIFAR10:
        def __init__(self, root, train=True, transform=None, target_transform=None, download=False):
            t = fake_labels(self.cls_num)
            self.targets = t.tolist()
            self.data = np.arange(len(t), dtype=np.int64).reshape(-1, 1)
    tv = types.ModuleType("torchvision")
    tv.datasets = types.ModuleType("torchvision.datasets"); tv.datasets.CIFAR10 = _CIFAR10
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.update({"torchvision": tv, "torchvision.datasets": tv.datasets, "torchvision.transforms": tv.transforms})
    pil = types.ModuleType("PIL"); pil.Image = types.ModuleType("PIL.Image")
    sys.modules.update({"PIL": pil, "PIL.Image": pil.Image})
    cat = types.ModuleType("catalyst"); cat.data = types.ModuleType("catalyst.data")
    cat.data.BalanceClassSampler = cat.data.DistributedSamplerWrapper = object
    sys.modules.update({"catalyst": cat, "catalyst.data": cat.data})
    ra = types.ModuleType("randaugment")
    ra.CIFAR10Policy = ra.ImageNetPolicy = ra.RandAugment = object
    sys.modules["randaugment"] = ra


_placeholder_modules()
import imbalanced_dataset     # noqa: E402  (reference)


def key(C, imb_type, imb, r):
    return "c%d_%s_%g_r%d" % (C, imb_type, imb, r)


def main():
    out = {}
    for C, klass in ((10, imbalanced_dataset.IMBALANCECIFAR10), (100, imbalanced_dataset.IMBALANCECIFAR100)):
        out["c%d_labels" % C] = fake_labels(C).astype(np.uint8)
        for imb_type, imb in CONFIGS:
            for r in RAND_NUMBERS:
                ds = klass(root="", imb_type=imb_type, imb_factor=imb, rand_number=r, train=True)
                k = key(C, imb_type, imb, r)
                out[k + "_index"] = ds.data[:, 0].astype(np.uint16)
                out[k + "_targets"] = np.asarray(ds.targets, dtype=np.uint8)
                out[k + "_cls_num_list"] = np.asarray(ds.get_cls_num_list(), dtype=np.int64)
    path = os.path.join(HERE, "g21_cifar_imb.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
