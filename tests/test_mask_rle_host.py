"""COCO run-length encoding of masks (iif_amd.mmdet_mask_loss: paste_masks_rle, encode_masks, get_seg_masks_rle; csrc/mask_rle.hip,
iif_rle_to_string in csrc/iif_host.cpp), the part that needs no device: the restatement tests/rle_ref.py against known answers,
the host string encoder against the restatement, the entry points in header, library and ctypes table with their argument checks
(by status code), and the Python side's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from . import rle_ref as R
from iif_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("iif_paste_rle_count", "iif_paste_rle_fill", "iif_mask_rle_count", "iif_mask_rle_fill", "iif_rle_to_string",
           "iif_rle_workspace_bytes")


def _mask(H, W, *boxes):
    """bool [H, W] with the (y0, y1, x0, x1) ranges (ends included) set."""
    m = np.zeros((H, W), dtype=bool)
    for y0, y1, x0, x1 in boxes:
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def crossing_mask():
    """61 x 93 with a run of 71 ones that crosses from the bottom of column 40 into the top of column 41."""
    return _mask(61, 93, (10, 49, 5, 5), (0, 2, 6, 6), (20, 60, 40, 40), (0, 29, 41, 41))


def big_rectangle():
    return _mask(800, 1333, (100, 699, 200, 1199))


yy, xx = np.mgrid[0:5, 0:7]
# (mask, counts, string): answers of an independent restatement of rleEncode / rleToString, each round-tripped through a decoder
KNOWN = [
    (_mask(3, 4), [12], b"<"),
    (~_mask(3, 4), [0, 12], b"0<"),
    (_mask(3, 4, (0, 0, 0, 0)), [0, 1, 11], b"01;"),
    (_mask(3, 4, (2, 2, 3, 3)), [11, 1], b";1"),
    (_mask(4, 5, (1, 2, 1, 3)), [5, 2, 2, 2, 2, 2, 5], b"5220003"),
    ((yy + xx) % 2 == 1, [1] * 35, b"111" + 32 * b"0"),
    (_mask(800, 1333), [1066400], b"P]aP1"),
    (~_mask(800, 1333), [0, 1066400], b"0P]aP1"),
    (crossing_mask(), [315, 40, 11, 3, 2091, 71, 3142], b"k9X1;kNPQ2T2kP1"),
]


def native_string(counts, cap=None):
    """(status, bytes written, *len) of iif_rle_to_string; the buffer is 8 bytes longer than ``cap`` and pre-filled with '#'."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    cap = 7 * len(c) if cap is None else cap
    buf = ctypes.create_string_buffer(b"#" * (cap + 8), cap + 8)
    n = ctypes.c_int64(-1)
    rc = _lib.lib().iif_rle_to_string(c.ctypes.data if len(c) else None, len(c), buf, cap, ctypes.byref(n))
    assert buf.raw[cap:] == b"#" * 8                            # nothing past the capacity, whatever the status
    return rc, buf.raw[:cap], n.value


@pytest.mark.parametrize("k", range(len(KNOWN)))
def test_restatement_gives_the_known_answers(k):
    mask, counts, string = KNOWN[k]
    assert R.encode(mask) == counts
    if mask.size <= 10000:
        assert R.encode_loop(mask) == counts
    assert R.to_string(counts) == string
    assert R.from_string(string) == counts
    assert np.array_equal(R.decode(R.from_string(string), *mask.shape), mask)
    assert R.encode_rle(mask) == {"size": list(mask.shape), "counts": string}


def test_restatement_on_the_large_rectangle():
    m = big_rectangle()
    counts = R.encode(m)
    s = R.to_string(counts)
    assert len(counts) == 2001 and counts[:4] == [160100, 600, 200, 600]
    assert len(s) == 2010 and s.startswith(b"T[l4hb0X6000")
    assert R.from_string(s) == counts and np.array_equal(R.decode(counts, 800, 1333), m)


def test_vectorised_encode_equals_the_loop_on_random_masks():
    rng = np.random.RandomState(4100)
    for H, W, p in ((1, 1, 0.5), (1, 17, 0.5), (17, 1, 0.5), (9, 11, 0.1), (9, 11, 0.9), (33, 20, 0.5)):
        for _ in range(4):
            m = rng.rand(H, W) < p
            assert R.encode(m) == R.encode_loop(m)
            assert np.array_equal(R.decode(R.from_string(R.to_string(R.encode(m))), H, W), m)


@pytest.mark.parametrize("k", range(len(KNOWN)))
def test_native_string_on_the_known_answers(k):
    _, counts, string = KNOWN[k]
    rc, out, n = native_string(counts)
    assert rc == 0 and n == len(string) and out[:n] == string


def test_native_string_equals_the_restatement():
    rng = np.random.RandomState(4101)
    cases = [[1, 1, 1000000, 1, 1, 1], [0, 5], [0], [5, 0, 0, 7], [1 << 15, 1, 1 << 15, 1 << 20, 1, (1 << 20) + 3, 2, 1],
             [(1 << 31) - 1, 1, 1, (1 << 31) - 1, 1], [(1 << 32) - 1, 0, 0, (1 << 32) - 1, 0], [15, 16, 31, 32, 15, 16, 0, 1023, 1024],
             R.encode(big_rectangle())]
    for hi in (2, 40, 1 << 10, 1 << 15, 1 << 16, 1 << 20, 1 << 21, 1 << 31):
        for m in (1, 2, 3, 4, 7, 64):
            cases.append(rng.randint(0, hi, size=m, dtype=np.int64).tolist())
    mixed = rng.randint(0, 1 << 21, size=500, dtype=np.int64)
    mixed[rng.rand(500) < 0.3] = 0
    mixed[rng.rand(500) < 0.2] = 1
    cases.append(mixed.tolist())
    for counts in cases:
        want = R.to_string(counts)
        rc, out, n = native_string(counts)
        assert rc == 0 and n == len(want) and out[:n] == want, counts[:8]
        assert R.from_string(want) == counts
    rc, out, n = native_string([])
    assert rc == 0 and n == 0


def test_native_string_with_too_little_room():
    counts = R.encode(crossing_mask())
    want = R.to_string(counts)
    rc, out, n = native_string(counts, cap=len(want))
    assert rc == 0 and out == want
    for cap in (len(want) - 1, 3, 0):
        rc, out, n = native_string(counts, cap=cap)             # (native_string checks the bytes past the capacity)
        assert rc == -1 and n == len(want) and out == want[:cap]
    L = _lib.lib()
    c = np.array(counts, dtype=np.uint32)
    buf = ctypes.create_string_buffer(32)
    assert L.iif_rle_to_string(None, 3, buf, 32, None) == -1 and L.iif_rle_to_string(c.ctypes.data, -1, buf, 32, None) == -1
    assert L.iif_rle_to_string(c.ctypes.data, 3, None, 32, None) == -1 and L.iif_rle_to_string(c.ctypes.data, 3, buf, -1, None) == -1
    assert L.iif_rle_to_string(c.ctypes.data, len(c), buf, 32, None) == 0 and buf.raw[:len(want)] == want      # len is optional


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_entry_points_in_header_library_and_table():
    text = open(os.path.join(ROOT, "include", "iif_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        proto = re.search(r"int(?:64_t)?\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.lib().iif_rle_workspace_bytes.restype is ctypes.c_int64
    # the paste entries take iif_paste_masks' arguments (its output aside) in its order
    paste = _lib.SIGNATURES["iif_paste_masks"][:-2]
    assert _lib.SIGNATURES["iif_paste_rle_count"][:len(paste)] == paste and _lib.SIGNATURES["iif_paste_rle_fill"][:len(paste)] == paste


def test_workspace_size():
    L = _lib.lib()
    assert L.iif_rle_workspace_bytes(-1, 8, 8) == 0 and L.iif_rle_workspace_bytes(1, 0, 8) == 0
    assert L.iif_rle_workspace_bytes(1, 1, 1) == 8 + 2 * 8                   # one item, rounded up to 8 bytes; two offsets
    assert L.iif_rle_workspace_bytes(4, 512, 640) == 4 * 640 * 4 * 4 + 5 * 8
    assert L.iif_rle_workspace_bytes(4, 512, 640) < 100 * 1024
    assert L.iif_rle_workspace_bytes(3, 129, 7) == (3 * 7 * 2 * 4 + 7) // 8 * 8 + 4 * 8


def test_paste_rle_checks_arguments_before_launching():
    L = _lib.lib()
    one = 64            # a non-null, aligned stand-in: the checks fail before any pointer is used
    need = L.iif_rle_workspace_bytes(3, 61, 93)

    def lead(kw):
        return (kw.get("pred", one), kw.get("dtype", 0), 0, kw.get("labels", one), kw.get("boxes", one), kw.get("ld", 5),
                kw.get("N", 3), kw.get("C", 5), kw.get("h", 28), kw.get("w", 28), kw.get("img_h", 61), kw.get("img_w", 93),
                kw.get("thr", 0.5), kw.get("ws", one), kw.get("ws_bytes", need), kw.get("totals", one))

    def count(**kw):
        return L.iif_paste_rle_count(*lead(kw), None)

    def fill(**kw):
        return L.iif_paste_rle_fill(*lead(kw), kw.get("total", 3), kw.get("pos", one), kw.get("runs", one), None)
    for call in (count, fill):                                  # iif_paste_masks' checks, with its codes
        assert call(pred=None) == -1 and call(boxes=None) == -1
        assert call(pred=66) == -1 and call(boxes=66) == -1 and call(labels=68) == -1 and call(pred=65, dtype=1) == -1
        assert call(dtype=2) == -1 and call(N=-1) == -1 and call(N=65536) == -1 and call(C=0) == -1 and call(ld=3) == -1
        assert call(h=0) == -1 and call(w=0) == -1 and call(img_h=0) == -1 and call(img_w=-1) == -1
        assert call(thr=-0.5) == -1 and call(thr=float("nan")) == -1
        assert call(h=65) == -2 and call(w=65) == -2 and call(img_h=65536, img_w=32768) == -2
        assert call(N=0, pred=None, boxes=None, labels=None, ws=None, totals=None, pos=None, runs=None) == 0
        assert call(ws=None) == -1 and call(ws=68) == -1 and call(totals=None) == -1 and call(totals=66) == -1
        assert call(ws_bytes=need - 1) == -1
    assert fill(pos=None) == -1 and fill(runs=None) == -1 and fill(pos=66) == -1 and fill(runs=66) == -1
    assert fill(total=2) == -1                                  # every mask has at least one count


def test_mask_rle_checks_arguments_before_launching():
    L = _lib.lib()
    one = 64
    need = L.iif_rle_workspace_bytes(3, 61, 93)

    def lead(kw):
        H, W = kw.get("H", 61), kw.get("W", 93)
        ld_row = kw.get("ld_row", W)
        return (kw.get("masks", one), ld_row, kw.get("ld_mask", H * ld_row), kw.get("N", 3), H, W, kw.get("ws", one),
                kw.get("ws_bytes", need), kw.get("totals", one))

    def count(**kw):
        return L.iif_mask_rle_count(*lead(kw), None)

    def fill(**kw):
        return L.iif_mask_rle_fill(*lead(kw), kw.get("total", 3), kw.get("pos", one), kw.get("runs", one), None)
    for call in (count, fill):
        assert call(masks=None) == -1 and call(N=-1) == -1 and call(N=65536) == -1 and call(H=0) == -1 and call(W=-3) == -1
        assert call(ld_row=92) == -1                            # a pitch below the width
        assert call(ld_mask=60 * 93 + 92) == -1                 # masks that overlap
        assert call(H=65536, W=32768, ws_bytes=1 << 40) == -2
        assert call(N=0, masks=None, ws=None, totals=None, pos=None, runs=None) == 0
        assert call(ws=None) == -1 and call(ws=68) == -1 and call(totals=None) == -1 and call(totals=66) == -1
        assert call(ws_bytes=need - 1) == -1
    assert fill(pos=None) == -1 and fill(runs=None) == -1 and fill(pos=66) == -1 and fill(runs=66) == -1 and fill(total=2) == -1


# ------------------------------------------------------------------------------------------------------------ Python surface
def test_python_side_refusals():
    from iif_amd import mmdet_mask_loss as ML
    from iif_amd.mmdet_mask_target import DeviceBitmapMasks
    pred, boxes, labels = torch.zeros(2, 3, 28, 28), torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64)
    for fn in (ML.paste_masks, ML.paste_masks_rle):             # the same checks, the same exceptions
        with pytest.raises(NotImplementedError):
            fn(pred, boxes, labels, 20, 30, -1)                 # the uint8 visualisation branch
        with pytest.raises(NotImplementedError):
            fn(pred.half(), boxes, labels, 20, 30, 0.5)
        with pytest.raises(NotImplementedError):
            fn(pred, boxes.double(), labels, 20, 30, 0.5)
        with pytest.raises(NotImplementedError):
            fn(torch.zeros(2, 3, 65, 28), boxes, labels, 20, 30, 0.5)
        with pytest.raises(NotImplementedError):
            fn(pred, boxes, labels, 65536, 32768, 0.5)
        with pytest.raises(ValueError):
            fn(pred, boxes[:, :3], labels, 20, 30, 0.5)
        with pytest.raises(ValueError):
            fn(pred[0], boxes, labels, 20, 30, 0.5)
        with pytest.raises(ValueError):
            fn(pred, boxes, labels[:1], 20, 30, 0.5)
        with pytest.raises(_lib.IIFNativeError):                # CPU tensors are rejected, not emulated
            fn(pred, boxes, labels, 20, 30, 0.5)
    with pytest.raises(_lib.IIFNativeError):
        ML.get_seg_masks_rle(pred, boxes, labels, dict(mask_thr_binary=0.5), (20, 30, 3), np.ones(4), True, 3)
    with pytest.raises(NotImplementedError):
        ML.get_seg_masks_rle(pred, boxes, labels, dict(mask_thr_binary=-1), (20, 30, 3), np.ones(4), True, 3)
    assert "pin_memory" not in ML.get_seg_masks_rle.__code__.co_varnames
    with pytest.raises(_lib.IIFNativeError):
        ML.encode_masks(torch.zeros(2, 8, 8, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        ML.encode_masks(torch.zeros(2, 8, 8))                   # a float mask tensor
    with pytest.raises(NotImplementedError):
        ML.encode_masks(np.zeros((2, 8, 8), dtype=np.uint8))    # host masks: pycocotools' own ground
    with pytest.raises(ValueError):
        ML.encode_masks(torch.zeros(2, 2, 8, 8, dtype=torch.uint8))
    with pytest.raises(_lib.IIFNativeError):                    # host masks inside the class are uploaded: no device here
        ML.encode_masks(DeviceBitmapMasks(np.ones((3, 8, 8), dtype=bool), 8, 8))
    for word in ("encode_mask_results", "mask_util.encode", "area", "polygons"):
        assert word in ML.__doc__, word
