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
(augment.ColorJitter.factors), 48..55: the auto-augment policy (draw_policy); a policy run therefore crops and flips exactly
the images a jitter run does.  The index lists are cifar.epoch_indices': RandomSampler, BalanceClassSampler, their DDP shards.
Evaluation is TensorTransform's geometry (imbalanced_dataset.eval_geometry) without draws.

With ``policy`` ("imagenet", "randaugment", "cifar") the policy replaces ColorJitter, as in the reference
(imbalanced_dataset.py:210-225): the workers draw each image's ops and turn them into op records (policy_record), packed as a
section of their own, and ``iif_lt_augment_policy`` runs them on the device between the flip and Normalize.

With ``decode="device"`` (--device-decode) the workers only read baseline JPEG files and parse their headers (iif_amd/jpeg.py);
``iif_jpeg_decode`` decodes each box on the device before the augment launch, and every other file (progressive, CMYK, PNG,
.npy, ...) is decoded by the dataset's loader in the worker, in the same batch (pack_decode).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, augment, jpeg
from .cifar import OPS, _mix64, epoch_indices, op_constants, sample_keys
from .imbalanced_dataset import _default_loader, eval_geometry, mean_std_hue, rrc_box

JITTER = 1                                                 # IIF_LT_JITTER of include/iif_amd.h
DESC = ("offset", "h", "w", "rh", "rw", "oy", "ox", "flip")        # int64 words per image
JITTER_WORDS = ("order", "fb", "gb", "fc", "gc", "fs", "gs", "fh")  # uint32 words per image (g = 1 - f, fp32 bits)
RRC_SLOTS, FLIP_SLOT, ORDER_SLOT, FACTOR_SLOT, N_SLOTS = 40, 40, 41, 44, 48
JITTER_AMOUNTS = (0.4, 0.4, 0.4)                           # imbalanced_dataset.py:197,205 ColorJitter(0.4, 0.4, 0.4, hue)
POLICY_SLOT, N_POLICY_SLOTS = 48, 8                        # slots 48..55 of the same key: the policy draws
OP_NONE = 0xFF                                             # IIF_LT_OP_NONE: an op slot that does nothing
RECORD_WORDS = 8                                           # uint32 per op slot: op code, p0 .. p5 (cifar.op_constants), unused
# --auto-augment value -> augment._P table (None: RandAugment), as TensorTransform maps them
POLICIES = {"imagenet": "imagenet", "cifar": "cifar10", "cifar10": "cifar10", "randaugment": None}
RAND_N, RAND_M = 2, 9                                      # augment.RandAugment(): n = 2 ops at magnitude index 9
# the ops that cost the kernel a sweep of their own: whole-image reductions and gathers (lt_policy.hip)
SWEEP_OPS = augment.GEOMETRIC + ("Sharpness", "Contrast", "AutoContrast", "Equalize")


def uniforms(seed, epoch, rank, pos):
    """The N_SLOTS uniforms in [0, 1) of one sample: the top 53 bits of mix(key ^ slot), as doubles."""
    key = sample_keys(seed, epoch, rank, [pos])[0]
    u = _mix64(key ^ np.arange(N_SLOTS, dtype=np.uint64)) >> np.uint64(11)
    return u.astype(np.float64) * (1.0 / (1 << 53))


def policy_uniforms(seed, epoch, rank, pos):
    """The N_POLICY_SLOTS uniforms of slots POLICY_SLOT.. of one sample, as ``uniforms`` computes its slots."""
    key = sample_keys(seed, epoch, rank, [pos])[0]
    u = _mix64(key ^ np.arange(POLICY_SLOT, POLICY_SLOT + N_POLICY_SLOTS, dtype=np.uint64)) >> np.uint64(11)
    return u.astype(np.float64) * (1.0 / (1 << 53))


def draw_policy(policy, u):
    """The two op slots of one sample from its policy uniforms ``u``: [(name, magnitude index, sign +-1.0) or None] * 2.
    AutoAugment (imagenet, cifar): sub-policy floor(u0 * 25), op j applied when u(1 + 2j) < its probability, sign +1 when
    u(2 + 2j) < 0.5.  RandAugment: op j = RandAugment.OPS[floor(u(2j) * 14)] at magnitude RAND_M, sign +1 when u(1 + 2j) < 0.5."""
    if policy not in POLICIES:
        raise ValueError("unknown policy %r (%s)" % (policy, ", ".join(POLICIES)))
    if POLICIES[policy] is None:
        ops = augment.RandAugment.OPS
        return [(ops[int(u[2 * j] * len(ops))], RAND_M, 1.0 if u[2 * j + 1] < 0.5 else -1.0) for j in range(RAND_N)]
    subs = augment._P[POLICIES[policy]]
    sub = subs[int(u[0] * len(subs))]
    out = []
    for j in range(2):
        name, prob, mag = sub[3 * j:3 * j + 3]
        out.append((name, mag, 1.0 if u[2 + 2 * j] < 0.5 else -1.0) if u[1 + 2 * j] < prob else None)
    return out


def policy_record(ops, size):
    """The uint32 [2][8] op records of iif_lt_augment_policy for the slots ``ops`` (draw_policy) at S = ``size``: the op code
    (the index in cifar.OPS) and op_constants(name, magnitude, sign, size, size); OP_NONE for a slot not applied."""
    rec = np.zeros((2, RECORD_WORDS), dtype=np.uint32)
    rec[:, 0] = OP_NONE
    for j, op in enumerate(ops):
        if op is not None:
            name, mag, sign = op
            rec[j, 0] = OPS.index(name)
            rec[j, 1:7] = op_constants(name, mag, sign, size, size)
    return rec


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


def train_job(data, hd, size, u, jitter=None):
    """train_sample of a stream the device decodes (data: its bytes, hd: jpeg.parse's Header): the same draws on the frame's
    size, which is the decoded image's size; the region is a jpeg.Job for iif_jpeg_decode."""
    (top, left, ch, cw), flip, order, factors = draw(hd.h, hd.w, u, jitter)
    rec = None if jitter is None else jitter_record(order, *factors)
    return jpeg.Job(data, hd, (top, left, ch, cw)), (ch, cw, size, size, 0, 0, int(flip)), rec


def eval_job(data, hd, size):
    """eval_sample of a stream the device decodes: the whole image."""
    nh, nw, top, left = eval_geometry(hd.h, hd.w, size)
    return jpeg.Job(data, hd, (0, 0, hd.h, hd.w)), (hd.h, hd.w, nh, nw, top, left, 0), None


def _align(n, a=16):
    return (n + a - 1) // a * a


def pack(samples):
    """Collate [(region, desc words, jitter record or None, target)] into one uint8 tensor: desc int64 [B][8], jitter uint32
    [B][8], targets int64 [B], then the regions at 16-byte aligned offsets (desc[:, 0] counts from the pool's start).
    Samples of a policy loader carry a fifth item, their op records (policy_record): they go into a section of their own,
    uint32 [B][2][8], after the targets."""
    B = len(samples)
    policy = B > 0 and len(samples[0]) > 4
    if any((len(s) > 4) != policy for s in samples):
        raise ValueError("either every sample carries op records or none does")
    head = B * (8 * 8 + 4 * 8 + 8) + (B * 2 * RECORD_WORDS * 4 if policy else 0)
    offs, o = [], 0
    for s in samples:
        offs.append(o)
        o = _align(o + s[0].nbytes)
    buf = np.zeros(_align(head) + o, dtype=np.uint8)
    desc = buf[:B * 64].view(np.int64).reshape(B, 8)
    jit = buf[B * 64:B * 96].view(np.uint32).reshape(B, 8)
    tgt = buf[B * 96:B * 104].view(np.int64)
    pool = buf[_align(head):]
    if policy:
        ops = buf[B * 104:B * 168].view(np.uint32).reshape(B, 2, RECORD_WORDS)
        for i, sample in enumerate(samples):
            ops[i] = sample[4]
    for i, (region, words, rec, target) in enumerate(s[:4] for s in samples):
        desc[i, 0] = offs[i]
        desc[i, 1:] = words
        if rec is not None:
            jit[i] = rec
        tgt[i] = target
        pool[offs[i]:offs[i] + region.nbytes] = region.reshape(-1)
    return torch.from_numpy(buf)


def _collate(samples):
    return pack(samples), len(samples)


TRAILER = ("jobs", "section", "upload", "out_bytes", "scratch_bytes", "subseq_bits", "unused", "unused")   # int64 words


def pack_decode(samples, subseq_bits=jpeg.SUBSEQ_BITS):
    """``pack`` for a loader that decodes on the device: a sample's region may be a jpeg.Job instead of an array.  The head
    and the host regions are laid out exactly as ``pack`` lays them out (``unpack`` reads them); the JPEG section follows
    the regions (jpeg.layout: records, tables, scans), then a trailer of 8 int64 words (TRAILER).  On the device the upload
    is followed by the regions iif_jpeg_decode writes (out_bytes): the descriptors of the Job samples point there, past the
    upload, so that iif_lt_augment reads both kinds from the one pool."""
    B = len(samples)
    policy = B > 0 and len(samples[0]) > 4
    if any((len(s) > 4) != policy for s in samples):
        raise ValueError("either every sample carries op records or none does")
    head = B * (8 * 8 + 4 * 8 + 8) + (B * 2 * RECORD_WORDS * 4 if policy else 0)
    pool0 = _align(head)
    offs, o = [], 0
    for s in samples:
        if isinstance(s[0], jpeg.Job):
            offs.append(None)
        else:
            offs.append(o)
            o = _align(o + s[0].nbytes)
    jobs = [s[0] for s in samples if isinstance(s[0], jpeg.Job)]
    sec, _, outs, out_bytes, scr_bytes = jpeg.layout(jobs, pool0 + o, subseq_bits)
    up = pool0 + o + len(sec) + 8 * len(TRAILER)
    buf = np.zeros(up, dtype=np.uint8)
    desc = buf[:B * 64].view(np.int64).reshape(B, 8)
    jit = buf[B * 64:B * 96].view(np.uint32).reshape(B, 8)
    tgt = buf[B * 96:B * 104].view(np.int64)
    pool = buf[pool0:]
    if policy:
        ops = buf[B * 104:B * 168].view(np.uint32).reshape(B, 2, RECORD_WORDS)
        for i, sample in enumerate(samples):
            ops[i] = sample[4]
    k = 0
    for i, (region, words, rec, target) in enumerate(s[:4] for s in samples):
        if offs[i] is None:
            desc[i, 0] = up - pool0 + outs[k]
            k += 1
        else:
            desc[i, 0] = offs[i]
            pool[offs[i]:offs[i] + region.nbytes] = region.reshape(-1)
        desc[i, 1:] = words
        if rec is not None:
            jit[i] = rec
        tgt[i] = target
    buf[pool0 + o:pool0 + o + len(sec)] = sec
    buf[up - 8 * len(TRAILER):].view(np.int64)[:] = (len(jobs), pool0 + o, up, out_bytes, scr_bytes, subseq_bits, 0, 0)
    return torch.from_numpy(buf)


def trailer(buf):
    """{TRAILER name: value} of a pack_decode batch (a host tensor)."""
    return dict(zip(TRAILER, buf[-8 * len(TRAILER):].view(torch.int64).tolist()))


class _DecodeCollate(object):
    def __init__(self, subseq_bits):
        self.subseq_bits = subseq_bits

    def __call__(self, samples):
        return pack_decode(samples, self.subseq_bits), len(samples)


def unpack(buf, B, policy=False):
    """(pool, desc, jitter, targets) views of a packed batch (on any device); with ``policy`` (a batch of a policy loader)
    (pool, desc, jitter, targets, op records int32 [B, 2, 8])."""
    if policy:
        head = _align(B * 168)
        return (buf[head:], buf[:B * 64].view(torch.int64).view(B, 8), buf[B * 64:B * 96].view(torch.int32).view(B, 8),
                buf[B * 96:B * 104].view(torch.int64), buf[B * 104:B * 168].view(torch.int32).view(B, 2, RECORD_WORDS))
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


def lt_augment_policy(pool, desc, ops, size, mean, std, work=None, out=None):
    """One ``iif_lt_augment_policy`` launch: pool uint8, desc int64 [B, 8], ops int32 / uint32 words [B, 2, 8]
    (policy_record), all on the device; mean / std three floats each; ``work`` the kernel's scratch image, fp32
    [B, 3, size, size] (allocated when None).  Returns fp32 [B, 3, size, size]."""
    _lib.require_gpu(pool, desc, ops, work, out)
    if pool.dtype != torch.uint8 or desc.dtype != torch.int64 or ops.dtype != torch.int32:
        raise TypeError("pool uint8, desc int64 and ops int32 expected")
    B = desc.shape[0]
    if not (pool.is_contiguous() and desc.is_contiguous()) or desc.dim() != 2 or desc.shape[1] != len(DESC):
        raise ValueError("contiguous pool and desc [B, %d] expected" % len(DESC))
    if not ops.is_contiguous() or tuple(ops.shape) != (B, 2, RECORD_WORDS):
        raise ValueError("contiguous ops [B, 2, %d] expected" % RECORD_WORDS)
    shape = (B, 3, int(size), int(size))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=desc.device)
    if work is None:
        work = torch.empty(shape, dtype=torch.float32, device=desc.device)
    for name, t in (("work", work), ("out", out)):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("%s must be a contiguous fp32 %s tensor" % (name, list(shape)))
    if work.data_ptr() == out.data_ptr():
        raise ValueError("work and out must be distinct buffers")
    ms = (ctypes.c_float * 6)(*[float(v) for v in mean], *[float(v) for v in std])
    rc = _lib.lib().iif_lt_augment_policy(_lib.ptr(pool), pool.numel(), _lib.ptr(desc), _lib.ptr(ops), B, int(size),
                                          ctypes.addressof(ms), _lib.ptr(work), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "iif_lt_augment_policy")
    return out


class _Samples(torch.utils.data.Dataset):
    """Position p of one rank's epoch list -> (region, desc words, jitter record, target[, op records]); runs in the
    DataLoader workers."""

    def __init__(self, dataset, index, train, size, seed, epoch, rank, jitter, policy=None, decode=False):
        self.dataset, self.index, self.train, self.size = dataset, index, train, size
        self.seed, self.epoch, self.rank, self.jitter, self.policy = seed, epoch, rank, jitter, policy
        self.decode = decode

    def __len__(self):
        return len(self.index)

    def _image(self, i):
        """(decoded image, None) or, for a stream the device decodes, (None, (bytes, Header)).  A routed file is decoded
        from the bytes already read, as the default loader decodes it."""
        path = self.dataset.img_path[i]
        if self.decode and not path.endswith(".npy"):
            with open(path, "rb") as f:
                data = f.read()
            hd = jpeg.parse(data)
            if not isinstance(hd, str):
                return None, (data, hd)
            import io
            from PIL import Image
            return Image.open(io.BytesIO(data)).convert("RGB"), None
        return self.dataset.loader(path), None

    def __getitem__(self, p):
        i = int(self.index[p])
        img, job = self._image(i)
        if self.train and self.policy is not None:
            u = uniforms(self.seed, self.epoch, self.rank, p)
            region, words, _ = train_sample(img, self.size, u) if job is None else train_job(*job, self.size, u)
            ops = draw_policy(self.policy, policy_uniforms(self.seed, self.epoch, self.rank, p))
            return region, words, None, int(self.dataset.targets[i]), policy_record(ops, self.size)
        if self.train:
            u = uniforms(self.seed, self.epoch, self.rank, p)
            if job is None:
                region, words, rec = train_sample(img, self.size, u, self.jitter)
            else:
                region, words, rec = train_job(*job, self.size, u, self.jitter)
        else:
            region, words, rec = eval_sample(img, self.size) if job is None else eval_job(*job, self.size)
        return region, words, rec, int(self.dataset.targets[i])


class DeviceLTLoader(object):
    """Yields device (image, target) batches of a list dataset (LT_Dataset / LT_Dataset_Eval): ``drop_last`` for training,
    every sample for evaluation.  ``dset_name`` picks mean / std and the jitter's hue (imbalanced_dataset.mean_std_hue);
    ``jitter=False`` trains with crop and flip only.  ``policy`` ("imagenet", "randaugment", "cifar"; training only) runs
    that auto-augment policy on the device instead of the jitter.  ``mode`` = --sampler.  ``set_epoch`` as
    DistributedSampler; without it each pass over the loader advances the epoch by one.  ``decode="device"``
    (--device-decode) decodes the baseline JPEG files on the device (iif_jpeg_decode, ``subseq_bits`` its subsequence
    length) instead of in the workers; it replaces the default loader only.  ``decode_failures()`` counts the images whose
    scan the device found malformed (their regions are jpeg.FILL)."""

    def __init__(self, dataset, batch_size, train=True, size=224, dset_name="imagenet_lt", jitter=True, seed=0, mode="random",
                 distributed=False, rank=None, world=None, workers=4, device="cuda", policy=None, decode="host",
                 subseq_bits=jpeg.SUBSEQ_BITS):
        if mode not in ("random", "upsampling", "downsampling"):
            raise ValueError("unknown sampler %r (random, upsampling, downsampling)" % (mode,))
        if policy is not None and policy not in POLICIES:
            raise ValueError("unknown policy %r (%s)" % (policy, ", ".join(POLICIES)))
        if decode not in ("host", "device"):
            raise ValueError("unknown decode %r (host, device)" % (decode,))
        if decode == "device" and getattr(dataset, "loader", None) is not _default_loader:
            raise ValueError("decode='device' replaces the default loader only; this dataset has a custom loader=")
        if not jpeg.MIN_SUBSEQ_BITS <= int(subseq_bits) <= 1 << 24:
            raise ValueError("subseq_bits must be in [%d, 2^24]" % jpeg.MIN_SUBSEQ_BITS)
        self.decode, self.subseq_bits = decode, int(subseq_bits)
        self._scratch, self._failures = None, None
        self.dataset = dataset
        self.batch_size, self.train, self.size, self.seed, self.mode = int(batch_size), train, int(size), int(seed), mode
        self.mean, self.std, hue = mean_std_hue(dset_name)
        self.policy = policy if train else None
        self.jitter = augment.ColorJitter(*JITTER_AMOUNTS, hue) if (train and jitter and self.policy is None) else None
        self._work = None                                  # iif_lt_augment_policy's scratch image, reused while (B, S) stays
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
        device = self.decode == "device"
        samples = _Samples(self.dataset, self.indices(epoch), self.train, self.size, self.seed, epoch, self.rank, self.jitter,
                           self.policy, decode=device)
        return torch.utils.data.DataLoader(samples, batch_size=self.batch_size, shuffle=False, drop_last=self.train,
                                           num_workers=self.workers, collate_fn=_DecodeCollate(self.subseq_bits) if device
                                           else _collate, pin_memory=torch.cuda.is_available())

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        for buf, B in self.batches(epoch):
            dev = self.upload(buf) if self.decode == "device" else buf.to(self.device, non_blocking=True)
            yield self.build(dev, B)

    def upload(self, buf):
        """The device buffer of a pack_decode batch: the upload (one copy), then the regions iif_jpeg_decode writes there
        (launched here, on the current stream)."""
        t = trailer(buf)
        up, n = t["upload"], t["jobs"]
        dev = torch.empty(up + t["out_bytes"], dtype=torch.uint8, device=self.device)
        dev[:up].copy_(buf, non_blocking=True)
        if n:
            if self._scratch is None or self._scratch.numel() < t["scratch_bytes"] or self._scratch.device != dev.device:
                self._scratch = torch.empty(t["scratch_bytes"] * 5 // 4 + 16, dtype=torch.uint8, device=dev.device)
            sec = t["section"]
            rec = dev[sec:sec + n * jpeg.REC_WORDS * 8].view(torch.int64).view(n, jpeg.REC_WORDS)
            status = torch.empty(n, dtype=torch.int32, device=dev.device)
            jpeg.launch(dev[:up], rec, n, self._scratch, dev[up:], status, t["subseq_bits"])
            fails = (status != 0).sum()
            self._failures = fails if self._failures is None else self._failures + fails
        return dev

    def decode_failures(self, reset=False):
        """Images of this loader's batches since the last reset whose scan the device could not decode (``reset``: start
        counting again).  Synchronises with the device: ask where the caller waits anyway (train.py: at the end of an
        epoch)."""
        n = 0 if self._failures is None else int(self._failures)
        if reset:
            self._failures = None
        return n

    def build(self, dev, B):
        """(image, target) of one packed batch of B samples already on the device."""
        if self.policy is not None:
            pool, desc, _, tgt, ops = unpack(dev, B, policy=True)
            shape = (B, 3, self.size, self.size)
            if self._work is None or tuple(self._work.shape) != shape or self._work.device != dev.device:
                self._work = torch.empty(shape, dtype=torch.float32, device=dev.device)
            return lt_augment_policy(pool, desc, ops, self.size, self.mean, self.std, work=self._work), tgt
        pool, desc, jit, tgt = unpack(dev, B)
        img = lt_augment(pool, desc, jit if self.flags & JITTER else None, self.size, self.mean, self.std, self.flags)
        return img, tgt
