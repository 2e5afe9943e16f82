"""Baseline JPEG decoding on the device (``--device-decode``): the workers parse the marker segments, the device decodes.

    imgs = jpeg.decode([open(p, "rb").read() for p in paths])             # uint8 HWC device tensors, as PIL decodes them
    imgs = jpeg.decode(datas, boxes=[(top, left, h, w), ...])              # only those boxes

The host side (this module) reads the markers up to SOS and never touches the entropy-coded bytes: ``parse`` returns a
``Header`` (the frame, de-zigzagged quantisation tables, Huffman tables as device lookup tables, the restart interval) or
the reason the stream stays on the host.  ``iif_jpeg_decode`` (include/iif_amd.h) does the rest in two launches: per image
one workgroup destuffs the scan, decodes it (restart intervals in parallel; without them, fixed-length bit subsequences
decoded speculatively and re-decoded until each starts where its predecessor ends), dequantises and runs the ISLOW IDCT on
the blocks the box needs; then upsampling (libjpeg's fancy h2v1 / h2v2 filters), YCbCr -> RGB and the HWC uint8 store.

What the device decodes: sequential Huffman (SOF0 / SOF1), 8-bit, one component or three in one interleaved scan that
libjpeg reads as YCbCr (JFIF, Adobe transform != 0, or ids 1, 2, 3), sampling 4:4:4, 4:2:2 or 4:2:0, with or without
restart intervals.  Everything else is routed (``parse`` returns a string naming why) and decoded by the dataset's loader.
"""
import numpy as np
import torch

from . import _lib

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                   46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)   # zigzag position k -> natural index
REC_WORDS = 32                       # int64 words per record, IIF_JPEG_REC_WORDS
(R_SCAN, R_SCAN_LEN, R_TABLES, R_H, R_W, R_NCOMP, R_HMAX, R_VMAX, R_DRI, R_TOP, R_LEFT, R_BH, R_BW, R_OUT, R_SCRATCH,
 R_SCRATCH_LEN, R_COMP0) = range(17)
HUFF_BYTES = 1424                    # look uint16[512], maxcode int32[18], valoff int32[18], vals uint8[256]
HUFF_SLOTS = 6
TABLE_BYTES = 3 * 64 * 2 + HUFF_SLOTS * HUFF_BYTES   # quantisation int16 [3][64] (natural order), then the Huffman slots
SUB_WORDS = 20                       # int32 per bit subsequence in the scratch (start state, two end states)
SUBSEQ_BITS = 1024                   # default subsequence length of the entropy decoder
MIN_SUBSEQ_BITS = 32
FILL = 128                           # IIF_JPEG_FILL: every byte of a region the device could not decode
STATUS = {0: "ok", 1: "bad record", 2: "invalid Huffman code", 3: "coefficient overflow", 4: "truncated scan",
          5: "missing restart marker"}


def _align(n, a=16):
    return (n + a - 1) // a * a


class Header(object):
    """What the device needs of one baseline stream (``parse``).  ``comps``: (DC slot, AC slot) per component in scan order,
    slots into ``huff`` (device lookup tables); ``qt`` int16 [3][64] in natural order."""
    __slots__ = ("h", "w", "ncomp", "hmax", "vmax", "comps", "dri", "scan_off", "qt", "huff", "ids")

    def mcu(self):
        return (8 * self.vmax, 8 * self.hmax) if self.ncomp == 3 else (8, 8)


def huff_table(bits, vals):
    """The device lookup table of one DHT table (16 code-length counts, the symbols): HUFF_BYTES bytes, or None when the
    counts do not form a prefix code (libjpeg refuses such a table, so the stream is routed)."""
    look = np.zeros(512, dtype=np.uint16)
    maxcode = np.full(18, -1, dtype=np.int32)
    valoff = np.zeros(18, dtype=np.int32)
    code, k = 0, 0
    for l in range(1, 17):
        n = int(bits[l - 1])
        if n:
            valoff[l] = k - code
            if l <= 9:
                for j in range(n):
                    lo = (code + j) << (9 - l)
                    look[lo:lo + (1 << (9 - l))] = (l << 8) | int(vals[k + j])
            code += n
            k += n
            maxcode[l] = code - 1
            if code >= (1 << l):         # jdhuff.c: no code may be all ones
                return None
        code <<= 1
    maxcode[17] = 0x7FFFFFFF
    out = np.zeros(HUFF_BYTES, dtype=np.uint8)
    out[:1024] = look.view(np.uint8)
    out[1024:1096] = maxcode.view(np.uint8)
    out[1096:1168] = valoff.view(np.uint8)
    out[1168:1168 + len(vals)] = vals
    return out


_HUFF_CACHE = {}


def _huff_cached(raw):
    """huff_table of a raw DHT entry (counts + symbols), cached per process: most files of a dataset share their tables."""
    t = _HUFF_CACHE.get(raw)
    if t is None:
        if len(_HUFF_CACHE) > 256:
            _HUFF_CACHE.clear()
        t = huff_table(np.frombuffer(raw, dtype=np.uint8, count=16), np.frombuffer(raw, dtype=np.uint8, offset=16))
        _HUFF_CACHE[raw] = t if t is not None else False
    return t if t is not False else None


_ROUTED_SOF = {0xC2: "progressive", 0xC6: "progressive", 0xCA: "progressive", 0xCE: "progressive", 0xC3: "lossless",
               0xC7: "lossless", 0xCB: "lossless", 0xCF: "lossless", 0xC5: "hierarchical", 0xC9: "arithmetic",
               0xCD: "arithmetic", 0xCC: "arithmetic", 0xDC: "DNL height", 0xDE: "hierarchical", 0xDF: "hierarchical"}


def parse(data):
    """Read the markers of ``data`` (bytes) up to the first SOS.  Returns a Header, or a string: why the stream is routed
    to the host decoder."""
    mv = memoryview(data)
    n = len(mv)
    if n < 4 or mv[0] != 0xFF or mv[1] != 0xD8:
        return "not a JPEG stream"
    i = 2
    frame = None
    qt, huff = {}, {}                # DQT id -> int16 [64]; (class 0 DC / 1 AC, id) -> raw counts + symbols
    dri, jfif, adobe = 0, False, None
    while True:
        if i >= n or mv[i] != 0xFF:
            return "truncated header" if i >= n else "bad marker"
        while i < n and mv[i] == 0xFF:
            i += 1
        if i >= n:
            return "truncated header"
        m = mv[i]
        i += 1
        if m == 0xD9:
            return "no scan"
        if 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        if m in _ROUTED_SOF:
            return _ROUTED_SOF[m]
        if i + 2 > n:
            return "truncated header"
        seg = (mv[i] << 8) | mv[i + 1]
        if seg < 2 or i + seg > n:
            return "truncated header"
        s = mv[i + 2:i + seg]
        i += seg
        if m in (0xC0, 0xC1):
            if frame is not None:
                return "two frames"
            if len(s) < 6:
                return "truncated header"
            if s[0] != 8:
                return "%d-bit samples" % s[0]
            h, w, nf = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if len(s) < 6 + 3 * nf:
                return "truncated header"
            if h == 0:
                return "DNL height"
            if w == 0:
                return "zero width"
            if nf not in (1, 3):
                return "%d components" % nf
            frame = (h, w, [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(nf)])
        elif m == 0xC4:
            k = 0
            while k < len(s):
                if k + 17 > len(s):
                    return "truncated header"
                tc, th = s[k] >> 4, s[k] & 15
                cnt = sum(s[k + 1:k + 17])
                if tc > 1 or th > 3 or cnt > 256 or k + 17 + cnt > len(s):
                    return "bad Huffman table"
                if tc == 0 and any(v > 15 for v in s[k + 17:k + 17 + cnt]):
                    return "bad Huffman table"
                huff[(tc, th)] = bytes(s[k + 1:k + 17 + cnt])
                k += 17 + cnt
        elif m == 0xDB:
            k = 0
            while k < len(s):
                pq, tq = s[k] >> 4, s[k] & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or k + 1 + size > len(s):
                    return "bad quantisation table"
                raw = np.frombuffer(bytes(s[k + 1:k + 1 + size]), dtype=">u2" if pq else np.uint8).astype(np.int64)
                nat = np.zeros(64, dtype=np.int64)
                nat[ZIGZAG] = raw
                qt[tq] = nat.astype(np.uint16).view(np.int16)      # libjpeg's ISLOW multiplier table is a short
                k += 1 + size
        elif m == 0xDD:
            if len(s) < 2:
                return "truncated header"
            dri = (s[0] << 8) | s[1]
        elif m == 0xE0:
            if len(s) >= 14 and bytes(s[:5]) == b"JFIF\x00":       # jdmarker.c examine_app0: APP0_DATA_LEN
                jfif = True
        elif m == 0xEE:
            if len(s) >= 12 and bytes(s[:5]) == b"Adobe":
                adobe = s[11]
        elif m == 0xDA:
            if frame is None:
                return "scan before frame"
            if len(s) < 1 or len(s) < 4 + 2 * s[0]:
                return "truncated header"
            ns = s[0]
            h, w, comps = frame
            if ns != len(comps):
                return "multi-scan"
            sc = [(s[1 + 2 * j], s[2 + 2 * j] >> 4, s[2 + 2 * j] & 15) for j in range(ns)]
            if s[1 + 2 * ns] != 0 or s[2 + 2 * ns] != 63 or s[3 + 2 * ns] != 0:
                return "bad spectral selection"
            if [c[0] for c in sc] != [c[0] for c in comps]:
                return "scan order"
            return _header(h, w, comps, sc, qt, huff, dri, jfif, adobe, i)


def _header(h, w, comps, sc, qt, huff, dri, jfif, adobe, scan_off):
    nf = len(comps)
    ids = tuple(c[0] for c in comps)
    if nf == 3:
        # jdapimin.c default_decompress_parms, restricted to what certainly means YCbCr
        ycc = jfif or (adobe is not None and adobe != 0) or (adobe is None and ids == (1, 2, 3))
        if not ycc:
            return "RGB colour space"
        (h0, v0), (h1, v1), (h2, v2) = [(c[1], c[2]) for c in comps]
        if (h1, v1, h2, v2) != (1, 1, 1, 1) or (h0, v0) not in ((1, 1), (2, 1), (2, 2)):
            return "sampling %dx%d,%dx%d,%dx%d" % (h0, v0, h1, v1, h2, v2)
        hmax, vmax = h0, v0
    else:
        hmax = vmax = 1              # one component: a non-interleaved scan of 8 x 8 blocks whatever its factors
    hd = Header()
    hd.h, hd.w, hd.ncomp, hd.hmax, hd.vmax, hd.dri, hd.scan_off, hd.ids = h, w, nf, hmax, vmax, dri, scan_off, ids
    hd.qt = np.zeros((3, 64), dtype=np.int16)
    hd.huff, hd.comps, keys = [], [], []
    for c, ((_, _, _, tq), (_, td, ta)) in enumerate(zip(comps, sc)):
        if tq not in qt:
            return "missing quantisation table"
        hd.qt[c] = qt[tq]
        slots = []
        for key in ((0, td), (1, ta)):
            if key not in huff:
                return "missing Huffman table"
            if key not in keys:
                t = _huff_cached(huff[key])
                if t is None:
                    return "bad Huffman table"
                keys.append(key)
                hd.huff.append(t)
            slots.append(keys.index(key))
        hd.comps.append((slots[0], slots[1]))
    return hd


def tables(hd):
    """The TABLE_BYTES table block of a Header."""
    out = np.zeros(TABLE_BYTES, dtype=np.uint8)
    out[:384] = hd.qt.reshape(-1).view(np.uint8)
    for k, t in enumerate(hd.huff):
        out[384 + k * HUFF_BYTES:384 + (k + 1) * HUFF_BYTES] = t
    return out


def window(hd, top, left, bh, bw):
    """MCU rows [my0, my1) and columns [mx0, mx1) the box (top, left, bh, bw) needs, with the chroma rows / columns that
    fancy upsampling reads next to it (the device computes the same)."""
    mh, mw = hd.mcu()
    y0, y1, x0, x1 = top, top + bh - 1, left, left + bw - 1
    my0, my1, mx0, mx1 = y0 // mh, y1 // mh, x0 // mw, x1 // mw
    if hd.ncomp == 3 and hd.vmax == 2:
        dh = (hd.h + 1) // 2
        my0, my1 = min(my0, max(0, y0 // 2 - 1) // 8), max(my1, min(dh - 1, y1 // 2 + 1) // 8)
    if hd.ncomp == 3 and hd.hmax == 2:
        dw = (hd.w + 1) // 2
        mx0, mx1 = min(mx0, max(0, x0 // 2 - 1) // 8), max(mx1, min(dw - 1, x1 // 2 + 1) // 8)
    return my0, my1 + 1, mx0, mx1 + 1


def scratch_bytes(hd, scan_len, top, left, bh, bw, subseq_bits=SUBSEQ_BITS):
    """Device scratch of one image (the kernel checks the record's figure against the same sum): the destuffed scan, the
    restart segment starts, the subsequence states, the coefficients int16 [blocks][64], one uint8 plane per component."""
    my0, my1, mx0, mx1 = window(hd, top, left, bh, bw)
    mcux = -(-hd.w // hd.mcu()[1])
    need = (my1 - 1) * mcux + mx1
    nint = -(-need // hd.dri) if hd.dri else 0
    nsub = 0 if hd.dri else max(1, -(-scan_len * 8 // subseq_bits))
    blocks = [(my1 - my0) * (mx1 - mx0) * (hd.hmax * hd.vmax if c == 0 else 1) for c in range(hd.ncomp)]
    return (_align(scan_len + 16) + _align(4 * (nint + 1)) + _align(4 * SUB_WORDS * nsub) + _align(128 * sum(blocks))
            + sum(_align(64 * b) for b in blocks))


class Job(object):
    """One device-decodable stream of a batch: its bytes, Header and box (top, left, bh, bw)."""
    __slots__ = ("data", "hd", "box")

    def __init__(self, data, hd, box):
        self.data, self.hd, self.box = data, hd, tuple(int(v) for v in box)

    @property
    def nbytes(self):
        return self.box[2] * self.box[3] * 3


def layout(jobs, base, subseq_bits=SUBSEQ_BITS):
    """Place the records, tables and scans of ``jobs`` in an upload section that starts at byte ``base`` (16-aligned) of the
    upload buffer.  Returns (section uint8 array, records int64 [n][REC_WORDS] (a view of it), region offsets in the output
    part, output bytes, scratch bytes); the records' table and scan offsets count from the upload buffer's start."""
    n = len(jobs)
    o = _align(n * REC_WORDS * 8)
    tab_off, scan_off = [], []
    for j in jobs:
        tab_off.append(o)
        o += TABLE_BYTES
        scan_off.append(o)
        o = _align(o + len(j.data) - j.hd.scan_off)
    sec = np.zeros(o, dtype=np.uint8)
    rec = sec[:n * REC_WORDS * 8].view(np.int64).reshape(n, REC_WORDS)
    outs, out_o, scr_o = [], 0, 0
    for k, j in enumerate(jobs):
        hd, (top, left, bh, bw) = j.hd, j.box
        scan = np.frombuffer(j.data, dtype=np.uint8, offset=hd.scan_off)
        sec[tab_off[k]:tab_off[k] + TABLE_BYTES] = tables(hd)
        sec[scan_off[k]:scan_off[k] + len(scan)] = scan
        scr = scratch_bytes(hd, len(scan), top, left, bh, bw, subseq_bits)
        r = rec[k]
        r[R_SCAN], r[R_SCAN_LEN], r[R_TABLES] = base + scan_off[k], len(scan), base + tab_off[k]
        r[R_H], r[R_W], r[R_NCOMP], r[R_HMAX], r[R_VMAX], r[R_DRI] = hd.h, hd.w, hd.ncomp, hd.hmax, hd.vmax, hd.dri
        r[R_TOP], r[R_LEFT], r[R_BH], r[R_BW] = top, left, bh, bw
        r[R_OUT], r[R_SCRATCH], r[R_SCRATCH_LEN] = out_o, scr_o, scr
        for c, (dc, ac) in enumerate(hd.comps):
            r[R_COMP0 + c] = dc | (ac << 4)
        outs.append(out_o)
        out_o = _align(out_o + j.nbytes)
        scr_o = _align(scr_o + scr)
    return sec, rec, outs, out_o, scr_o


def launch(data, rec, n, scratch, out, status, subseq_bits=SUBSEQ_BITS):
    """One ``iif_jpeg_decode`` call: data uint8 (the upload buffer: records, tables and scans), rec int64 [n][REC_WORDS]
    (a view of it), scratch and out uint8, status int32 [n]; all on the device."""
    _lib.require_gpu(data, rec, scratch, out, status)
    for name, t, dt in (("data", data, torch.uint8), ("rec", rec, torch.int64), ("scratch", scratch, torch.uint8),
                        ("out", out, torch.uint8), ("status", status, torch.int32)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor" % (name, dt))
    if tuple(rec.shape) != (n, REC_WORDS) or status.numel() < n:
        raise ValueError("rec [%d, %d] and status [>= %d] expected" % (n, REC_WORDS, n))
    rc = _lib.lib().iif_jpeg_decode(_lib.ptr(data), data.numel(), _lib.ptr(rec), int(n), _lib.ptr(scratch), scratch.numel(),
                                    _lib.ptr(out), out.numel(), int(subseq_bits), _lib.ptr(status), _lib.stream_ptr())
    _lib.check(rc, "iif_jpeg_decode")


def decode(datas, boxes=None, subseq_bits=SUBSEQ_BITS, device="cuda", return_status=False):
    """Decode the baseline JPEG byte strings ``datas`` on the device: a list of uint8 HWC [h, w, 3] device tensors equal to
    ``np.asarray(Image.open(f).convert("RGB"))`` (cropped to ``boxes[i]`` = (top, left, h, w) when given).  A stream the
    device does not decode raises ValueError with parse's reason; a malformed scan gives a region of FILL and, with
    ``return_status``, a non-zero word in the returned int32 status tensor (STATUS names the codes)."""
    if not MIN_SUBSEQ_BITS <= int(subseq_bits) <= 1 << 24:
        raise ValueError("subseq_bits must be in [%d, 2^24]" % MIN_SUBSEQ_BITS)
    jobs = []
    for k, d in enumerate(datas):
        hd = parse(d)
        if isinstance(hd, str):
            raise ValueError("stream %d is not decoded on the device: %s" % (k, hd))
        box = (0, 0, hd.h, hd.w) if boxes is None or boxes[k] is None else boxes[k]
        top, left, bh, bw = (int(v) for v in box)
        if bh < 1 or bw < 1 or top < 0 or left < 0 or top + bh > hd.h or left + bw > hd.w:
            raise ValueError("box %s outside the %d x %d image" % (tuple(box), hd.h, hd.w))
        jobs.append(Job(d, hd, (top, left, bh, bw)))
    dev = torch.device(device)
    status = torch.zeros(len(jobs), dtype=torch.int32, device=dev)
    if not jobs:
        return ([], status) if return_status else []
    sec, _, outs, out_bytes, scr_bytes = layout(jobs, 0, subseq_bits)
    data = torch.from_numpy(sec).to(dev)
    rec = data[:len(jobs) * REC_WORDS * 8].view(torch.int64).view(len(jobs), REC_WORDS)
    out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=dev)
    scratch = torch.empty(max(scr_bytes, 16), dtype=torch.uint8, device=dev)
    launch(data, rec, len(jobs), scratch, out, status, subseq_bits)
    imgs = [out[o:o + j.nbytes].view(j.box[2], j.box[3], 3) for o, j in zip(outs, jobs)]
    return (imgs, status) if return_status else imgs
