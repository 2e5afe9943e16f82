"""ImageNet-LT / Places-LT / iNaturalist-18 batches built on the device (``--device-augment``).

    ds = LT_Dataset(root, "train.txt", 365)                  # transform=None: the loader only decodes
    loader = DeviceLTLoader(ds, 256, train=True, dset_name="places_lt", workers=16)
    for image, target in loader:          # fp32 [256, 3, 224, 224] and int64 [256], both on the device
        ...

DataLoader workers decode each image with the dataset's own ``loader`` (``.npy`` HWC uint8, or PIL), make it HWC with 3
channels and, for training, cut out only the RandomResizedCrop box.  A batch is collated into ONE uint8 buffer (pinned by the
DataLoader): the descriptors, the jitter records, the targets and the regions packed back to back.  The main process uploads
it in one non-blocking copy and ``iif_lt_augment`` (include/iif_amd.h) builds the batch in one launch: antialiased resize,
flip, ColorJitter, Normalize, in TensorTransform's order.

Draws: every random number comes from the counter-based hash of iif_amd/cifar.py keyed on (seed, epoch, rank, position in
this rank's epoch list) with a fixed slot per draw, so the same (seed, epoch, rank) gives the same batches, whatever the
worker count, and a resumed epoch sees the same inputs.  Slots 0..39: the RandomResizedCrop tries (imbalanced_dataset.rrc_box
consumes them in order), 40: the flip, 41..43: the jitter order (Fisher-Yates), 44..47: the jitter factors
(augment.ColorJitter.factors).  The index lists are cifar.epoch_indices': RandomSampler, BalanceClassSampler, their DDP shards.
Evaluation is TensorTransform's geometry (imbalanced_dataset.eval_geometry) without draws.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, augment
from .cifar import _mix64, epoch_indices, sample_keys
from .imbalanced_dataset import eval_geometry, mean_std_hue, rrc_box

JITTER = 1                                                 # IIF_LT_JITTER of include/iif_amd.h
DESC = ("offset", "h", "w", "rh", "rw", "oy", "ox", "flip")        # int64 words per image
JITTER_WORDS = ("order", "fb", "gb", "fc", "gc", "fs", "gs", "fh")  # uint32 words per image (g = 1 - f, fp32 bits)
RRC_SLOTS, FLIP_SLOT, ORDER_SLOT, FACTOR_SLOT, N_SLOTS = 40, 40, 41, 44, 48
JITTER_AMOUNTS = (0.4, 0.4, 0.4)                           # imbalanced_dataset.py:197,205 ColorJitter(0.4, 0.4, 0.4, hue)


def uniforms(seed, epoch, rank, pos):
    """The N_SLOTS uniforms in [0, 1) of one sample: the top 53 bits of mix(key ^ slot), as doubles."""
    key = sample_keys(seed, epoch, rank, [pos])[0]
    u = _mix64(key ^ np.arange(N_SLOTS, dtype=np.uint64)) >> np.uint64(11)
    return u.astype(np.float64) * (1.0 / (1 << 53))


def _stream(u, first, last):
    it = iter(range(first, last))
    return lambda: float(u[next(it)])


def draw(h, w, u, jitter=None):
    """The draws of one training sample of an h x w image from its uniforms ``u``: ((top, left, ch, cw), flip, order,
    factors); order / factors are None without ``jitter`` (an augment.ColorJitter)."""
    box = rrc_box(h, w, _stream(u, 0, RRC_SLOTS))
    flip = bool(u[FLIP_SLOT] < 0.5)
    if jitter is None:
        return box, flip, None, None
    order = [0, 1, 2, 3]
    for k, i in enumerate((3, 2, 1)):
        j = int(u[ORDER_SLOT + k] * (i + 1))
        order[i], order[j] = order[j], order[i]
    return box, flip, order, jitter.factors(_stream(u, FACTOR_SLOT, N_SLOTS))


def jitter_record(order, fb, fc, fs, fh):
    """The uint32 [8] record of iif_lt_augment: the order word, then (f, 1 - f) per blend (rounded from double, as torch rounds
    the python scalars; None -> (1, 0), which leaves the op out) and the hue shift (None -> 0)."""
    word = sum(int(k) << (2 * i) for i, k in enumerate(order))
    vals = []
    for f in (fb, fc, fs):
        f = 1.0 if f is None else float(f)
        vals += [f, 1.0 - f]
    vals.append(0.0 if fh is None else float(fh))
    rec = np.zeros(len(JITTER_WORDS), dtype=np.uint32)
    rec[0] = word
    rec[1:] = np.asarray(vals, dtype=np.float32).view(np.uint32)
    return rec


def to_hwc3(img):
    """A decoded image as a contiguous uint8 HWC array with 3 channels: grey is repeated, alpha dropped."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError("the device path takes uint8 images, got %s" % (a.dtype,))
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 2, 3, 4) or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("an HxW or HxWxC image expected, got shape %s" % (a.shape,))
    if a.shape[2] < 3:                                     # grey (+ alpha): the grey channel three times
        a = np.repeat(a[:, :, :1], 3, axis=2)
    return np.ascontiguousarray(a[:, :, :3])


def train_sample(img, size, u, jitter=None):
    """(region, desc words without the offset, jitter record or None) of one training image."""
    a = to_hwc3(img)
    (top, left, ch, cw), flip, order, factors = draw(a.shape[0], a.shape[1], u, jitter)
    region = np.ascontiguousarray(a[top:top + ch, left:left + cw])
    rec = None if jitter is None else jitter_record(order, *factors)
    return region, (ch, cw, size, size, 0, 0, int(flip)), rec


def eval_sample(img, size):
    a = to_hwc3(img)
    h, w = a.shape[:2]
    nh, nw, top, left = eval_geometry(h, w, size)
    return a, (h, w, nh, nw, top, left, 0), None


def _align(n, a=16):
    return (n + a - 1) // a * a


def pack(samples):
    """Collate [(region, desc words, jitter record or None, target)] into one uint8 tensor: desc int64 [B][8], jitter uint32
    [B][8], targets int64 [B], then the regions at 16-byte aligned offsets (desc[:, 0] counts from the pool's start)."""
    B = len(samples)
    head = B * (8 * 8 + 4 * 8 + 8)
    offs, o = [], 0
    for s in samples:
        offs.append(o)
        o = _align(o + s[0].nbytes)
    buf = np.zeros(_align(head) + o, dtype=np.uint8)
    desc = buf[:B * 64].view(np.int64).reshape(B, 8)
    jit = buf[B * 64:B * 96].view(np.uint32).reshape(B, 8)
    tgt = buf[B * 96:B * 104].view(np.int64)
    pool = buf[_align(head):]
    for i, (region, words, rec, target) in enumerate(samples):
        desc[i, 0] = offs[i]
        desc[i, 1:] = words
        if rec is not None:
            jit[i] = rec
        tgt[i] = target
        pool[offs[i]:offs[i] + region.nbytes] = region.reshape(-1)
    return torch.from_numpy(buf)


def _collate(samples):
    return pack(samples), len(samples)


def unpack(buf, B):
    """(pool, desc, jitter, targets) views of a packed batch (on any device)."""
    head = _align(B * 104)
    return (buf[head:], buf[:B * 64].view(torch.int64).view(B, 8), buf[B * 64:B * 96].view(torch.int32).view(B, 8),
            buf[B * 96:B * 104].view(torch.int64))


def lt_augment(pool, desc, jitter, size, mean, std, flags, out=None):
    """One ``iif_lt_augment`` launch: pool uint8, desc int64 [B, 8], jitter int32 / uint32 words [B, 8] (None without
    JITTER), all on the device; mean / std three floats each.  Returns fp32 [B, 3, size, size]."""
    _lib.require_gpu(pool, desc, jitter)
    if pool.dtype != torch.uint8 or desc.dtype != torch.int64 or (jitter is not None and jitter.dtype != torch.int32):
        raise TypeError("pool uint8, desc int64 and jitter int32 expected")
    B = desc.shape[0]
    if not (pool.is_contiguous() and desc.is_contiguous()) or desc.dim() != 2 or desc.shape[1] != len(DESC):
        raise ValueError("contiguous pool and desc [B, %d] expected" % len(DESC))
    if jitter is not None and (not jitter.is_contiguous() or tuple(jitter.shape) != (B, len(JITTER_WORDS))):
        raise ValueError("contiguous jitter [B, %d] expected" % len(JITTER_WORDS))
    if out is None:
        out = torch.empty(B, 3, size, size, dtype=torch.float32, device=desc.device)
    ms = (ctypes.c_float * 6)(*[float(v) for v in mean], *[float(v) for v in std])
    rc = _lib.lib().iif_lt_augment(_lib.ptr(pool), pool.numel(), _lib.ptr(desc), _lib.ptr(jitter), B, int(size),
                                   ctypes.addressof(ms), int(flags), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "iif_lt_augment")
    return out


class _Samples(torch.utils.data.Dataset):
    """Position p of one rank's epoch list -> (region, desc words, jitter record, target); runs in the DataLoader workers."""

    def __init__(self, dataset, index, train, size, seed, epoch, rank, jitter):
        self.dataset, self.index, self.train, self.size = dataset, index, train, size
        self.seed, self.epoch, self.rank, self.jitter = seed, epoch, rank, jitter

    def __len__(self):
        return len(self.index)

    def __getitem__(self, p):
        i = int(self.index[p])
        img = self.dataset.loader(self.dataset.img_path[i])
        if self.train:
            u = uniforms(self.seed, self.epoch, self.rank, p)
            region, words, rec = train_sample(img, self.size, u, self.jitter)
        else:
            region, words, rec = eval_sample(img, self.size)
        return region, words, rec, int(self.dataset.targets[i])


class DeviceLTLoader(object):
    """Yields device (image, target) batches of a list dataset (LT_Dataset / LT_Dataset_Eval): ``drop_last`` for training,
    every sample for evaluation.  ``dset_name`` picks mean / std and the jitter's hue (imbalanced_dataset.mean_std_hue);
    ``jitter=False`` trains with crop and flip only.  ``mode`` = --sampler.  ``set_epoch`` as DistributedSampler; without it
    each pass over the loader advances the epoch by one."""

    def __init__(self, dataset, batch_size, train=True, size=224, dset_name="imagenet_lt", jitter=True, seed=0, mode="random",
                 distributed=False, rank=None, world=None, workers=4, device="cuda"):
        if mode not in ("random", "upsampling", "downsampling"):
            raise ValueError("unknown sampler %r (random, upsampling, downsampling)" % (mode,))
        self.dataset = dataset
        self.batch_size, self.train, self.size, self.seed, self.mode = int(batch_size), train, int(size), int(seed), mode
        self.mean, self.std, hue = mean_std_hue(dset_name)
        self.jitter = augment.ColorJitter(*JITTER_AMOUNTS, hue) if (train and jitter) else None
        self.flags = JITTER if self.jitter is not None else 0
        if distributed:
            import torch.distributed as dist
            rank = dist.get_rank() if rank is None else rank
            world = dist.get_world_size() if world is None else world
        self.rank, self.world = int(rank or 0), int(world or 1)
        self.workers = int(workers)
        self.epoch = 0
        self.device = torch.device(device)
        n = len(dataset)
        if train and mode != "random":
            from .samplers import BalanceClassSampler
            n = len(BalanceClassSampler(dataset.targets, mode=mode))
        self.list_len = n if self.world == 1 else int(math.ceil(n / self.world))

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self, epoch=None):
        return epoch_indices(len(self.dataset), self.epoch if epoch is None else epoch, self.seed, self.train,
                             self.mode, self.dataset.targets, self.rank, self.world)

    def __len__(self):
        L, B = self.list_len, self.batch_size
        return L // B if self.train else (L + B - 1) // B

    def batches(self, epoch):
        """The packed host batches of one epoch: (uint8 tensor, pinned when a GPU is present; sample count)."""
        samples = _Samples(self.dataset, self.indices(epoch), self.train, self.size, self.seed, epoch, self.rank, self.jitter)
        return torch.utils.data.DataLoader(samples, batch_size=self.batch_size, shuffle=False, drop_last=self.train,
                                           num_workers=self.workers, collate_fn=_collate, pin_memory=torch.cuda.is_available())

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        for buf, B in self.batches(epoch):
            yield self.build(buf.to(self.device, non_blocking=True), B)

    def build(self, dev, B):
        """(image, target) of one packed batch of B samples already on the device."""
        pool, desc, jit, tgt = unpack(dev, B)
        img = lt_augment(pool, desc, jit if self.flags & JITTER else None, self.size, self.mean, self.std, self.flags)
        return img, tgt
