"""COCO run-length encoding restated in numpy / plain Python from pycocotools' rleEncode, rleToString and rleFrString
(common/maskApi.c): the reference of tests/test_mask_rle_host.py and tests/test_mask_rle_gpu.py.  pycocotools itself is not a
dependency of the project.

A mask [H, W] is read in column-major order, pixel j = x * H + y.  ``counts`` alternates run lengths starting with a run of
zeros, which may be 0 long; the string writes count i as the signed difference to count i - 2 (from i = 3 on), five bits at a
time from the low end with a continuation bit, offset by 48."""
import numpy as np


def encode_loop(mask):
    """rleEncode as it is written, one pixel at a time (small masks: ``encode`` is checked against it)."""
    m = np.asarray(mask)
    flat = (m != 0).T.reshape(-1).tolist()                     # column-major
    counts, p, c = [], False, 0
    for v in flat:
        if v != p:
            counts.append(c)
            c, p = 0, v
        c += 1
    counts.append(c)
    return counts


def encode(mask):
    """[H, W] (anything that compares to 0) -> list of counts."""
    m = np.asarray(mask)
    assert m.ndim == 2
    flat = (m != 0).T.reshape(-1)                              # column-major
    before = np.concatenate([[False], flat[:-1]])
    edges = np.concatenate([[0], np.flatnonzero(flat != before), [flat.size]])
    return [int(c) for c in np.diff(edges)]


def to_string(counts):
    """list of counts -> bytes."""
    out = bytearray()
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        while True:
            c = x & 0x1f
            x >>= 5                                             # Python's >> is arithmetic
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(c + 48)
            if not more:
                break
    return bytes(out)


def from_string(s):
    """bytes -> list of counts (rleFrString)."""
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def decode(counts, H, W):
    """list of counts -> bool [H, W]."""
    assert sum(counts) == H * W, (sum(counts), H, W)
    values = np.arange(len(counts)) % 2 == 1
    return np.repeat(values, counts).reshape(W, H).T.copy()


def encode_rle(mask):
    """What ``pycocotools.mask.encode(np.asfortranarray(mask))`` returns."""
    m = np.asarray(mask)
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": to_string(encode(m))}
