"""A numpy restatement of the device JPEG pipeline (iif_amd/jpeg.py, iif_amd/csrc/jpeg_decode.hip) in libjpeg's default
arithmetic, stage by stage: destuffing, Huffman decoding to coefficients through the device lookup tables, the ISLOW IDCT
with its range limit, fancy upsampling and jdcolor's YCbCr -> RGB.  Test infrastructure: serial, slow, and the oracle the
kernel's stages are held to."""
import numpy as np

from iif_amd import jpeg


def photo(h, w, seed, grey=False):
    """A seeded photo-like uint8 HWC (or HW with ``grey``) image: low-frequency shading per channel, a few discs and
    rectangles, mild noise; not uniform noise, which is the worst case of entropy coding."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        a, b, ph = rng.uniform(0.005, 0.05), rng.uniform(0.005, 0.05), rng.uniform(0, 6)
        img[..., c] = 120 + 70 * np.sin(a * x + ph) * np.cos(b * y)
    for _ in range(4):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.1, 0.4) * max(h, w)
        col = rng.uniform(0, 255, 3)
        m = ((y - cy) ** 2 + (x - cx) ** 2 < r * r) if rng.rand() < 0.5 else ((abs(y - cy) < r / 2) & (abs(x - cx) < r))
        img[m] = 0.3 * img[m] + 0.7 * col
    img += rng.normal(0, 6, img.shape)
    a = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return a[..., 0] if grey else a


def encode(img, **opts):
    """JPEG bytes of a uint8 image through Pillow (``subsampling`` 0 / 1 / 2, ``quality``, ``optimize``, restart options)."""
    import io
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", **opts)
    return f.getvalue()


def pil_decode(data):
    """The reference decode: np.asarray(Image.open(f).convert("RGB"))."""
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def destuff(scan):
    """(entropy-coded bytes with stuffing and markers removed, start of each restart segment in them)."""
    out, segs, i, n = bytearray(), [0], 0, len(scan)
    while i < n:
        b = scan[i]
        if b == 0xFF:
            nx = scan[i + 1] if i + 1 < n else -1
            if nx == 0:
                out.append(0xFF)
                i += 2
                continue
            if nx == 0xFF:
                i += 1
                continue
            if 0xD0 <= nx <= 0xD7:
                segs.append(len(out))
                i += 2
                continue
            break
        out.append(b)
        i += 1
    return bytes(out), segs


def _factors(hd):
    return [(hd.hmax, hd.vmax) if c == 0 else (1, 1) for c in range(hd.ncomp)]


def coefficients(data, hd):
    """int64 coefficient planes [block rows][blocks per row][64] (natural order, DC resolved) of every component."""
    d, segs = destuff(bytes(memoryview(data)[hd.scan_off:]))
    d += b"\0" * 8
    mh, mw = hd.mcu()
    mcux, mcuy = -(-hd.w // mw), -(-hd.h // mh)
    fac = _factors(hd)
    planes = [np.zeros((mcuy * v, mcux * h, 64), np.int64) for h, v in fac]
    tabs = []
    for t in hd.huff:
        tabs.append((t[:1024].view(np.uint16), t[1024:1096].view(np.int32), t[1096:1168].view(np.int32), t[1168:]))
    st = {"p": 0}

    def peek():
        p = st["p"]
        return (int.from_bytes(d[p >> 3:(p >> 3) + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF

    def symbol(t):
        look, maxcode, valoff, vals = t
        w = peek()
        e = int(look[w >> 23])
        if e:
            ln, s = e >> 8, e & 255
        else:
            ln = 10
            while ln <= 16 and (w >> (32 - ln)) > maxcode[ln]:
                ln += 1
            if ln > 16:
                raise ValueError("invalid Huffman code at bit %d" % st["p"])
            s = int(vals[(int(valoff[ln]) + (w >> (32 - ln))) & 255])
        st["p"] += ln
        return s

    def extend(s):
        v = peek() >> (32 - s)
        st["p"] += s
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v

    pred, seg = [0, 0, 0], 0
    for m in range(mcux * mcuy):
        if hd.dri and m and m % hd.dri == 0:
            seg += 1
            st["p"], pred = segs[seg] * 8, [0, 0, 0]
        my, mx = divmod(m, mcux)
        for c, (h, v) in enumerate(fac):
            dct, act = tabs[hd.comps[c][0]], tabs[hd.comps[c][1]]
            for by in range(v):
                for bx in range(h):
                    blk = planes[c][my * v + by, mx * h + bx]
                    s = symbol(dct)
                    pred[c] += extend(s) if s else 0
                    blk[0] = ((pred[c] + 32768) & 0xFFFF) - 32768
                    k = 1
                    while k < 64:
                        rs = symbol(act)
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > 63:
                                raise ValueError("coefficient index past 63")
                            blk[jpeg.ZIGZAG[k]] = extend(s)
                            k += 1
                        elif r == 15:
                            k += 16
                        else:
                            break
    return planes


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _range_limit(x):
    """libjpeg's post-IDCT range limit table, indexed by the centred value masked to 10 bits."""
    x = x & 1023
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896))).astype(np.uint8)


def _butterfly(x):
    """jidctint.c's 1-D pass on eight arrays, before the descale."""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (x[0] + x[4]) * 8192
    tmp1 = (x[0] - x[4]) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]


def idct_islow(coef, q):
    """coef int64 [..., 64] (natural order), q int16 [64] -> uint8 [..., 8, 8]: jpeg_idct_islow."""
    d = (coef.astype(np.int64) * q.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    ws = np.stack([_descale(o, 11) for o in _butterfly([d[..., k, :] for k in range(8)])], axis=-2)
    return np.stack([_range_limit(_descale(o, 18)) for o in _butterfly([ws[..., :, k] for k in range(8)])], axis=-1)


def planes(data, hd):
    """uint8 sample planes of every component (whole MCUs)."""
    out = []
    for c, cp in enumerate(coefficients(data, hd)):
        px = idct_islow(cp, hd.qt[c])
        R, C = cp.shape[:2]
        out.append(px.transpose(0, 2, 1, 3).reshape(R * 8, C * 8))
    return out


def upsample(plane, hd):
    """A chroma plane brought to the image size as libjpeg's defaults do (jdsample.c): h2v1 / h2v2 fancy upsampling (the
    triangle filters, edge samples replicated), plain replication when the plane is at most 2 samples wide."""
    H, W = hd.h, hd.w
    if hd.hmax == 1:
        return plane[:H, :W]
    dw, dh = (W + 1) // 2, (H + 1) // 2 if hd.vmax == 2 else H
    c = plane[:dh, :dw].astype(np.int64)
    if dw <= 2:
        up = np.repeat(c, 2, axis=1)
        return (np.repeat(up, 2, axis=0) if hd.vmax == 2 else up)[:H, :W]
    j = np.arange(dw)
    jl, jr = np.maximum(j - 1, 0), np.minimum(j + 1, dw - 1)
    if hd.vmax == 1:
        even, odd = (3 * c + c[:, jl] + 1) >> 2, (3 * c + c[:, jr] + 2) >> 2
        return np.stack([even, odd], -1).reshape(dh, 2 * dw)[:H, :W]
    i = np.arange(dh)
    rows = []
    for nb in (np.maximum(i - 1, 0), np.minimum(i + 1, dh - 1)):     # output rows 2i (row above), 2i + 1 (row below)
        cs = 3 * c + c[nb]
        rows.append(np.stack([(3 * cs + cs[:, jl] + 8) >> 4, (3 * cs + cs[:, jr] + 7) >> 4], -1).reshape(dh, 2 * dw))
    return np.stack(rows, 1).reshape(2 * dh, 2 * dw)[:H, :W]


def ycc_to_rgb(y, cb, cr):
    """jdcolor.c ycc_rgb_convert (16-bit fixed point, FIX(1.402) = 91881, FIX(0.34414) = 22554, FIX(0.71414) = 46802,
    FIX(1.772) = 116130)."""
    y = y.astype(np.int64)
    cb, cr = cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    """uint8 HWC [h, w, 3] of a stream jpeg.parse accepts."""
    hd = jpeg.parse(data)
    assert not isinstance(hd, str), hd
    p = planes(data, hd)
    y = p[0][:hd.h, :hd.w]
    if hd.ncomp == 1:
        return np.repeat(y[:, :, None], 3, axis=2)
    return ycc_to_rgb(y, upsample(p[1], hd), upsample(p[2], hd))
