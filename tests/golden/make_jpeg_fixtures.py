"""Writes tests/golden/jpeg/: the device JPEG decoder's fixtures, made with Pillow (libjpeg-turbo).

    python tests/golden/make_jpeg_fixtures.py

<name>.jpg for every case below (tests/jpeg_ref.photo sources: smooth shading, hard-edged shapes, mild texture), the
routing cases (progressive, CMYK, PNG bytes under a .jpg name, a header cut short), and expected.json: per file its size,
Pillow's sampling, the routing reason the parser must give (None: decoded on the device), the restart interval, the SHA-256 and shape of
np.asarray(Image.open(f).convert("RGB")); <name>.npy holds that array for the images of at most 33 x 47 pixels.  Nothing
in expected.json comes from the parser under test: the routing reasons follow from how each routed file is made, the
components and restart interval (in MCUs) from the save options, the rest from Pillow."""
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image, JpegImagePlugin

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SMALL = 33 * 47
SUB = {"grey": None, "s444": 0, "s422": 1, "s420": 2}


def cases():
    """(name, sampling key, h, w, save options)."""
    out = []
    for (h, w) in [(1, 1), (2, 2), (3, 5), (1, 17), (17, 1), (15, 15)]:
        for s in SUB:
            out.append(("%s_q75_%dx%d" % (s, h, w), s, h, w, dict(quality=75)))
    for s in SUB:
        out.append(("%s_q90_33x47" % s, s, 33, 47, dict(quality=90)))
    for q in (5, 50, 75, 95, 100):
        out.append(("s420_q%d_33x47" % q, "s420", 33, 47, dict(quality=q)))
    out.append(("s420_q75_opt_33x47", "s420", 33, 47, dict(quality=75, optimize=True)))
    out.append(("s444_q75_opt_47x33", "s444", 47, 33, dict(quality=75, optimize=True)))
    out.append(("s420_q75_rstblocks_33x47", "s420", 33, 47, dict(quality=75, restart_marker_blocks=3)))
    out.append(("s422_q75_rstrows_47x33", "s422", 47, 33, dict(quality=75, restart_marker_rows=1)))
    out.append(("grey_q75_rstblocks_33x47", "grey", 33, 47, dict(quality=75, restart_marker_blocks=5)))
    out.append(("s420_q90_375x500", "s420", 375, 500, dict(quality=90)))
    out.append(("s420_q90_500x375", "s420", 500, 375, dict(quality=90)))
    out.append(("s422_q75_rstrows_375x500", "s422", 375, 500, dict(quality=75, restart_marker_rows=2)))
    out.append(("grey_q90_500x375", "grey", 500, 375, dict(quality=90)))
    return out


def _dri(s, w, opts):
    """The restart interval in MCUs libjpeg writes for these save options (jcparam.c: restart_in_rows * MCUs per row)."""
    if "restart_marker_blocks" in opts:
        return opts["restart_marker_blocks"]
    if "restart_marker_rows" in opts:
        return opts["restart_marker_rows"] * -(-w // (16 if s in ("s422", "s420") else 8))
    return 0


def main():
    sys.path.insert(0, ROOT)
    from tests.jpeg_ref import encode, photo
    items = []
    for k, (name, s, h, w, opts) in enumerate(cases()):
        kw = dict(opts) if SUB[s] is None else dict(opts, subsampling=SUB[s])
        items.append((name, encode(photo(h, w, k, grey=s == "grey"), **kw),
                      dict(route=None, ncomp=1 if s == "grey" else 3, dri=_dri(s, w, opts))))
    items.append(("route_progressive_33x47", encode(photo(33, 47, 900), quality=75, progressive=True),
                  dict(route="progressive")))
    f = io.BytesIO()
    Image.fromarray(photo(33, 47, 901)).convert("CMYK").save(f, "JPEG", quality=75)
    items.append(("route_cmyk_33x47", f.getvalue(), dict(route="4 components")))
    f = io.BytesIO()
    Image.fromarray(photo(33, 47, 902)).save(f, "PNG")
    items.append(("route_png_33x47", f.getvalue(), dict(route="not a JPEG stream")))
    items.append(("route_truncated", encode(photo(33, 47, 903), quality=75)[:150], dict(route="truncated header")))
    os.makedirs(OUT, exist_ok=True)
    expected = {}
    for name, data, known in items:
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        e = dict(known, bytes=len(data))
        try:
            im = Image.open(io.BytesIO(data))
            a = np.asarray(im.convert("RGB"))
            e.update(h=im.size[1], w=im.size[0], mode=im.mode, shape=list(a.shape),
                     sha256=hashlib.sha256(a.tobytes()).hexdigest())
            if im.format == "JPEG":
                e["sampling"] = JpegImagePlugin.get_sampling(im)
            if a.shape[0] * a.shape[1] <= SMALL:
                np.save(os.path.join(OUT, name + ".npy"), a)
        except Exception as ex:              # the header cut short: PIL cannot decode it either
            e["pil_error"] = type(ex).__name__
        expected[name] = e
    with open(os.path.join(OUT, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1, sort_keys=True)
    print("%d files, %d bytes" % (len(items), sum(os.path.getsize(os.path.join(OUT, p)) for p in os.listdir(OUT))))


if __name__ == "__main__":
    main()
