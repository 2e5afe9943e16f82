"""CIFAR-10 / CIFAR-100 from their files, the long-tailed subset of the reference's ``IMBALANCECIFAR10/100``
(classification/imbalanced_dataset.py:12-60) and a loader that builds every augmented batch on the device.

    ds = cifar_lt(root, "cifar100", imb_type="exp", imb_factor=0.01, rand_number=0)
    loader = DeviceCIFARLoader(ds, batch_size=128, train=True, flags=CROP_FLIP | POLICY | CUTOUT)
    for image, target in loader:          # fp32 [128, 3, 32, 32] and int64 [128], both on the device
        ...

Files: torchvision's on-disk layout under ``root`` (``cifar-10-batches-py/data_batch_1..5, test_batch`` or
``cifar-100-python/train, test``; pickles of ``data`` [N, 3072] uint8 rows, planar R, G, B, and ``labels`` /
``fine_labels``).  Nothing is downloaded.  The rows stay in that planar order: row i is torchvision's ``self.data[i]``.

The loader uploads the images and labels once.  Every epoch it materialises the sampler's index list on the host
(RandomSampler, catalyst's BalanceClassSampler for ``--sampler upsampling|downsampling``, DistributedSampler /
DistributedSamplerWrapper under DDP, all from (seed, epoch)), uploads it in one copy and then issues one
``iif_cifar_augment`` launch per batch.  The augmentation draws come from a counter-based hash of (seed, epoch, rank,
position in the epoch's list, draw slot), so the same (seed, epoch) gives the same batches; ``draw_params`` restates
the hash in numpy.
"""
import math
import os
import pickle

import numpy as np
import torch
from torch.utils.data.distributed import DistributedSampler

from . import _lib, augment
from .imbalanced_dataset import img_num_per_cls

CROP_FLIP, POLICY, CUTOUT = 1, 2, 4                       # IIF_CIFAR_* of include/iif_amd.h
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
# the kernel's op codes
OPS = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Color", "Posterize", "Solarize", "Contrast", "Sharpness",
       "Brightness", "AutoContrast", "Equalize", "Invert")
BLEND = ("Color", "Contrast", "Brightness", "Sharpness")
# the columns of the kernel's params output (also its draw slots)
PARAMS = ("crop_y", "crop_x", "flip", "sub_policy", "apply0", "sign0", "apply1", "sign1", "cut_y", "cut_x")
SIDE = 32

_LAYOUT = {
    "cifar10": ("cifar-10-batches-py", ["data_batch_%d" % i for i in range(1, 6)], ["test_batch"], "labels", 10),
    "cifar100": ("cifar-100-python", ["train"], ["test"], "fine_labels", 100),
}


# ------------------------------------------------------------------------------------------------------------- files
def read_cifar(root, name, train=True):
    """(data uint8 [N, 3072], targets int64 [N]) of one split; the train batches concatenated in file order."""
    if name not in _LAYOUT:
        raise KeyError("unknown CIFAR set %r (cifar10, cifar100)" % (name,))
    folder, train_files, test_files, key, _ = _LAYOUT[name]
    paths = [os.path.join(root, folder, f) for f in (train_files if train else test_files)]
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError("%s files not found (nothing is downloaded): %s" % (name, ", ".join(missing)))
    data, targets = [], []
    for p in paths:
        with open(p, "rb") as f:
            entry = pickle.load(f, encoding="latin1")
        data.append(np.asarray(entry["data"], dtype=np.uint8).reshape(-1, 3 * SIDE * SIDE))
        targets.extend(entry[key])
    return np.ascontiguousarray(np.vstack(data)), np.asarray(targets, dtype=np.int64)


def gen_imbalanced_indices(targets, img_num_list, rand_number):
    """Source rows of ``IMBALANCECIFAR10.gen_imbalanced_data`` (imbalanced_dataset.py:39-55), bit for bit: class by class in
    ``np.unique`` order, ``np.where``, shuffle, the first n.  ``RandomState(rand_number)`` gives the MT19937 stream of the
    reference's ``np.random.seed(rand_number)`` and leaves numpy's global state alone."""
    rng = np.random.RandomState(rand_number)
    t = np.asarray(targets, dtype=np.int64)
    sel, num_per_cls = [], {}
    for the_class, n in zip(np.unique(t), img_num_list):
        num_per_cls[int(the_class)] = int(n)
        idx = np.where(t == the_class)[0]
        rng.shuffle(idx)
        sel.append(idx[:n])
    return np.concatenate(sel).astype(np.int64), num_per_cls


class CIFARData(object):
    """Host copy of one CIFAR split: ``data`` uint8 [N, 3072], ``targets`` (list), ``num_per_cls_dict``; the surface of the
    reference's IMBALANCECIFAR10 that the trainer uses."""

    def __init__(self, data, targets, cls_num, num_per_cls_dict=None, source_index=None):
        self.data = data
        self.targets = [int(v) for v in targets]
        self.cls_num = self.num_classes = cls_num
        if num_per_cls_dict is None:
            num_per_cls_dict = {c: int(n) for c, n in enumerate(np.bincount(np.asarray(targets, np.int64), minlength=cls_num))}
        self.num_per_cls_dict = num_per_cls_dict
        self.source_index = source_index

    def __len__(self):
        return len(self.targets)

    def get_cls_num_list(self):
        return [self.num_per_cls_dict[i] for i in range(self.cls_num)]


def cifar_lt(root, name, imb_type="exp", imb_factor=0.01, rand_number=0):
    """The training set of IMBALANCECIFAR10 / IMBALANCECIFAR100: class-sorted rows of the long-tailed subset."""
    data, targets = read_cifar(root, name, train=True)
    C = _LAYOUT[name][4]
    counts = img_num_per_cls(C, len(data), imb_type, imb_factor)
    sel, num_per_cls = gen_imbalanced_indices(targets, counts, rand_number)
    return CIFARData(np.ascontiguousarray(data[sel]), targets[sel], C, num_per_cls, source_index=sel)


def cifar_test(root, name):
    """The full balanced test file (the reference evaluates on datasets.CIFAR10/100(train=False))."""
    data, targets = read_cifar(root, name, train=False)
    return CIFARData(data, targets, _LAYOUT[name][4])


# ------------------------------------------------------------------------------------------------------ index lists
def balanced_indices(labels, mode, rng):
    """One epoch of catalyst's BalanceClassSampler (iif_amd/samplers.py) drawn from ``rng`` instead of numpy's global state:
    with ``RandomState(s)`` it is the list BalanceClassSampler yields after ``np.random.seed(s)``."""
    from .samplers import BalanceClassSampler
    s = BalanceClassSampler(labels, mode=mode)
    indices = []
    for key in sorted(s.lbl2idx):
        replace_flag = s.samples_per_class > len(s.lbl2idx[key])
        indices += rng.choice(s.lbl2idx[key], s.samples_per_class, replace=replace_flag).tolist()
    rng.shuffle(indices)
    return indices


def epoch_indices(n, epoch, seed=0, train=True, mode="random", labels=None, rank=0, world=1):
    """This rank's index list of one epoch, int64.
    train, mode 'random': RandomSampler with a generator seeded seed + epoch (one rank), DistributedSampler(seed=seed) after
    set_epoch(epoch) (several); 'upsampling' / 'downsampling': BalanceClassSampler from RandomState(seed + epoch), sharded as
    DistributedSamplerWrapper does.  Evaluation: 0..n-1, or DistributedSampler(shuffle=False)'s shard."""
    if not train:
        if world == 1:
            return np.arange(n, dtype=np.int64)
        s = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=False)
        return np.asarray(list(s), dtype=np.int64)
    if mode == "random":
        if world == 1:
            g = torch.Generator().manual_seed(seed + epoch)
            return np.asarray(list(torch.utils.data.RandomSampler(range(n), generator=g)), dtype=np.int64)
        s = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=True, seed=seed)
        s.set_epoch(epoch)
        return np.asarray(list(s), dtype=np.int64)
    inner = balanced_indices(labels, mode, np.random.RandomState(seed + epoch))
    if world == 1:
        return np.asarray(inner, dtype=np.int64)
    s = DistributedSampler(range(len(inner)), num_replicas=world, rank=rank, shuffle=True, seed=seed)
    s.set_epoch(epoch)
    return np.asarray([inner[i] for i in s], dtype=np.int64)


# --------------------------------------------------------------------------------------------------- the policy table
def op_constants(name, mag, sign, h=SIDE, w=SIDE):
    """The six constant words p0 .. p5 of one operation at magnitude index ``mag`` and sign -1.0 / +1.0 on an h x w image,
    uint32 [6]: the fp32 affine coefficients (a, b, c, d, e, f) of a geometric op, (f, 1 - f) of a blend op, the posterize
    mask or the solarize threshold (integers); zeros for the rest.  Built in double from augment.py's own tables (_ranges(),
    affine_coefficients) and rounded to fp32 once."""
    m = augment._ranges()[name][mag]
    words = np.zeros(6, dtype=np.uint32)
    if name in augment.GEOMETRIC:
        words[:] = np.asarray(augment.affine_coefficients(name, m, sign, h, w), np.float32).view(np.uint32)
    elif name in BLEND:
        f = 1.0 + m * sign
        words[:2] = np.asarray([f, 1.0 - f], np.float32).view(np.uint32)
    elif name == "Posterize":
        words[0] = (0xFF << (8 - int(m))) & 0xFF
    elif name == "Solarize":
        words[0] = int(math.ceil(m))
    return words


def policy_table(subs=None, h=SIDE, w=SIDE):
    """The kernel's constants for the 25 sub-policies ``subs`` (default: augment._P["cifar10"], CIFAR10Policy), uint32
    [25][2][2][8]: per (sub-policy, op, sign negative / positive) the words [op code, round(prob * 2^24), p0 .. p5] with
    p = op_constants(op, magnitude, sign, h, w)."""
    subs = augment._P["cifar10"] if subs is None else subs
    if len(subs) != 25:
        raise ValueError("the kernel draws one of 25 sub-policies, got %d" % len(subs))
    tab = np.zeros((len(subs), 2, 2, 8), dtype=np.uint32)
    for s, sub in enumerate(subs):
        for j in range(2):
            name, prob, mag = sub[3 * j:3 * j + 3]
            for k, sign in enumerate((-1.0, 1.0)):
                words = tab[s, j, k]
                words[0] = OPS.index(name)
                words[1] = int(round(prob * 2 ** 24))
                words[2:8] = op_constants(name, mag, sign, h, w)
    return tab


# ------------------------------------------------------------------------------------------------------------ the hash
_M64 = (1 << 64) - 1


def _mix64(z):
    """The splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample_keys(seed, epoch, rank, positions):
    """The per-sample hash keys mix(mix(mix(mix(seed) ^ epoch) ^ rank) ^ position), uint64 [len(positions)]; draw slot s of a
    sample is then mix(key ^ s)."""
    k = _mix64(np.uint64(seed & _M64))
    k = _mix64(k ^ np.uint64(epoch & _M64))
    k = _mix64(k ^ np.uint64(rank & _M64))
    return _mix64(k ^ np.asarray(positions, dtype=np.int64).reshape(-1).astype(np.uint64))


def draw_params(seed, epoch, rank, positions, policy=None):
    """numpy restatement of the kernel's draws: int32 [len(positions), 10] in the order of PARAMS.  ``policy`` (the
    policy_table) supplies the application thresholds; without it the two 'applied' columns are 0, as in a launch without
    POLICY."""
    key = sample_keys(seed, epoch, rank, positions)
    u = np.stack([_mix64(key ^ np.uint64(s)) >> np.uint64(32) for s in range(len(PARAMS))], axis=1)
    below = lambda v, n: ((v * np.uint64(n)) >> np.uint64(32)).astype(np.int32)     # noqa: E731
    top = lambda v: (v >> np.uint64(31)).astype(np.int32)                             # noqa: E731
    p = np.zeros((len(key), len(PARAMS)), dtype=np.int32)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = below(u[:, 0], 9), below(u[:, 1], 9), top(u[:, 2]), below(u[:, 3], 25)
    for j in range(2):
        if policy is not None:
            thr = policy[p[:, 3], j, 0, 1].astype(np.uint64)
            p[:, 4 + 2 * j] = (u[:, 4 + 2 * j] >> np.uint64(8)) < thr
        p[:, 5 + 2 * j] = 1 - top(u[:, 5 + 2 * j])
    p[:, 8], p[:, 9] = below(u[:, 8], SIDE), below(u[:, 9], SIDE)
    return p


# ---------------------------------------------------------------------------------------------------------- the kernel
def device_policy(subs=None, device="cuda"):
    """policy_table(subs) on the device, as iif_cifar_augment takes it."""
    return torch.from_numpy(policy_table(subs).reshape(-1).view(np.int32)).to(device)


def augment_batch(data, labels, index, flags, seed=0, epoch=0, rank=0, pos0=0, policy=None, params=False):
    """One ``iif_cifar_augment`` launch over ``index`` (int64 [B], device).  ``data`` uint8 [N, 3072] and ``labels`` int64 [N]
    on the device; ``policy`` the device copy of policy_table() (needed with POLICY).  Returns (image fp32 [B, 3, 32, 32],
    target int64 [B]) and, with ``params=True``, the int32 [B, 10] draws."""
    _lib.require_gpu(data, labels, index, policy)
    if data.dtype != torch.uint8 or labels.dtype != torch.int64 or index.dtype != torch.int64:
        raise TypeError("data uint8, labels int64 and index int64 expected, got %s / %s / %s" % (data.dtype, labels.dtype,
                                                                                                index.dtype))
    if not (data.is_contiguous() and labels.is_contiguous() and index.is_contiguous()) or data[0].numel() != 3 * SIDE * SIDE:
        raise ValueError("contiguous data [N, 3072], labels [N] and index [B] expected")
    B = index.numel()
    out = torch.empty(B, 3, SIDE, SIDE, dtype=torch.float32, device=index.device)
    tgt = torch.empty(B, dtype=torch.int64, device=index.device)
    prm = torch.empty(B, len(PARAMS), dtype=torch.int32, device=index.device) if params else None
    rc = _lib.lib().iif_cifar_augment(_lib.ptr(data), data.shape[0], _lib.ptr(labels), _lib.ptr(index), B, int(pos0),
                                      int(seed) & _M64, int(epoch), int(rank), int(flags), _lib.ptr(policy), _lib.ptr(out),
                                      _lib.ptr(tgt), _lib.ptr(prm), _lib.stream_ptr())
    _lib.check(rc, "iif_cifar_augment")
    return (out, tgt, prm) if params else (out, tgt)


class DeviceCIFARLoader(object):
    """Yields device (image, target) batches of ``dataset`` (a CIFARData): ``drop_last`` for training, every sample for
    evaluation.  ``flags`` = the IIF_CIFAR_* stages (evaluation: 0, normalisation only).  ``mode`` = --sampler.
    ``set_epoch`` as DistributedSampler; without it each pass over the loader advances the epoch by one."""

    def __init__(self, dataset, batch_size, train=True, flags=CROP_FLIP, seed=0, mode="random", distributed=False,
                 rank=None, world=None, device="cuda"):
        if mode not in ("random", "upsampling", "downsampling"):
            raise ValueError("unknown sampler %r (random, upsampling, downsampling)" % (mode,))
        self.dataset = dataset
        self.batch_size, self.train, self.flags, self.seed, self.mode = int(batch_size), train, int(flags), int(seed), mode
        if distributed:
            import torch.distributed as dist
            rank = dist.get_rank() if rank is None else rank
            world = dist.get_world_size() if world is None else world
        self.rank, self.world = int(rank or 0), int(world or 1)
        self.epoch = 0
        self.device = torch.device(device)
        self.data = torch.from_numpy(np.ascontiguousarray(dataset.data)).to(self.device)
        self.labels = torch.tensor(dataset.targets, dtype=torch.int64).to(self.device)
        self.policy = device_policy(device=self.device) if flags & POLICY else None
        n = len(dataset)
        if train and mode != "random":
            from .samplers import BalanceClassSampler
            n = len(BalanceClassSampler(dataset.targets, mode=mode))
        self.list_len = n if self.world == 1 else int(math.ceil(n / self.world))

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self, epoch=None):
        return epoch_indices(len(self.dataset), self.epoch if epoch is None else epoch, self.seed, self.train, self.mode,
                             self.dataset.targets, self.rank, self.world)

    def __len__(self):
        L, B = self.list_len, self.batch_size
        return L // B if self.train else (L + B - 1) // B

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        idx = torch.from_numpy(self.indices(epoch)).to(self.device)
        B = self.batch_size
        for i in range(len(self)):
            yield augment_batch(self.data, self.labels, idx[i * B:(i + 1) * B], self.flags, self.seed, epoch, self.rank,
                                i * B, self.policy)
