"""Shared pieces of the list-dataset device-input tests: a torch oracle of one iif_lt_augment image built from the same
descriptor, and a fake .npy list-file tree."""
import os

import numpy as np
import torch

from iif_amd import augment


def oracle(region, words, jitter=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), size=224):
    """One output image from a region (uint8 HWC) and its descriptor words (h, w, rh, rw, oy, ox, flip), with
    ``jitter`` = (order, fb, fc, fs, fh) or None: interpolate(antialias=True), window, flip, ColorJitter.apply on the clamped
    image, Normalize - TensorTransform's torch ops, in its order."""
    h, w, rh, rw, oy, ox, flip = [int(v) for v in words]
    t = torch.from_numpy(np.ascontiguousarray(region)).permute(2, 0, 1).float() / 255.0
    t = torch.nn.functional.interpolate(t[None], size=(rh, rw), mode="bilinear", align_corners=False, antialias=True)[0]
    t = t[:, oy:oy + size, ox:ox + size]
    if flip:
        t = t.flip(-1)
    if jitter is not None:
        order, fb, fc, fs, fh = jitter
        t = augment.ColorJitter.apply(t.clamp(0.0, 1.0), order, fb, fc, fs, fh)
    return (t - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)


def smooth_image(h, w, seed, channels=3):
    """A uint8 image with structure at several scales (gradients plus noise), so that resampling errors show."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = [128 + 100 * np.sin(x / (3 + 7 * c) + y / (5 + 3 * c) + c) for c in range(channels)]
    img = np.stack(base, -1) + rng.normal(0, 25, size=(h, w, channels))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def write_npy_tree(root, shapes, labels, seed=0, eval_count=None):
    """root/img/<i>.npy for every shape and root/train.txt, root/eval.txt (the first ``eval_count`` lines) listing them."""
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    lines = []
    for i, (shape, lab) in enumerate(zip(shapes, labels)):
        rng = np.random.RandomState(seed * 100003 + i)
        np.save(os.path.join(root, "img", "%d.npy" % i), rng.randint(0, 256, size=shape, dtype=np.uint8))
        lines.append("img/%d.npy %d" % (i, lab))
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(root, "eval.txt"), "w") as f:
        f.write("\n".join(lines[:eval_count or len(lines)]) + "\n")
    return os.path.join(root, "train.txt"), os.path.join(root, "eval.txt")
