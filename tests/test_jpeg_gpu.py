"""iif_jpeg_decode on the MI355X: every fixture of tests/golden/jpeg decoded whole and in boxes against PIL's decode (the
committed SHA-256 / arrays, and PIL itself on further seeded images where it imports), the shortest and the default
subsequence length, malformed scans, and the device-decode DeviceLTLoader against the host-decode one on a mixed tree
(jitter, policy and evaluation batches, two ranks, determinism) and through the training CLI."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from iif_amd import jpeg, lt_device
from iif_amd.imbalanced_dataset import LT_Dataset, LT_Dataset_Eval

from .jpeg_ref import encode, photo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "jpeg")
with open(os.path.join(FIX, "expected.json")) as _f:
    EXPECTED = json.load(_f)
DEVICE = sorted(k for k, e in EXPECTED.items() if e["route"] is None)


def _read(name):
    with open(os.path.join(FIX, name + ".jpg"), "rb") as f:
        return f.read()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def full():
    """{fixture: its device decode}, each checked against PIL's committed SHA-256 (and array, for the small ones)."""
    imgs, status = jpeg.decode([_read(n) for n in DEVICE], device=DEV, return_status=True)
    assert status.cpu().tolist() == [0] * len(DEVICE)
    out = {}
    for n, im in zip(DEVICE, imgs):
        a = im.cpu().numpy()
        assert list(a.shape) == EXPECTED[n]["shape"], n
        assert _sha(a) == EXPECTED[n]["sha256"], n
        p = os.path.join(FIX, n + ".npy")
        if os.path.exists(p):
            assert np.array_equal(a, np.load(p)), n
        out[n] = a
    return out


def test_full_decode_of_every_fixture_equals_pil(full):
    assert len(full) == len(DEVICE) >= 40


def _boxes(h, w, rng):
    out = [(0, 0, 1, 1), (h - 1, w - 1, 1, 1), (0, w - 1, h, 1), (h - 1, 0, 1, w), (0, 0, h, w), (h // 2, w // 2, 1, 1)]
    if h > 20 and w > 20:
        out += [(7, 15, 10, 3), (15, 7, 2, 11), (16, 16, h - 16, w - 16), (h - 9, w - 17, 9, 17)]     # across MCU edges
    for _ in range(6):
        bh, bw = rng.randint(1, h + 1), rng.randint(1, w + 1)
        out.append((rng.randint(0, h - bh + 1), rng.randint(0, w - bw + 1), bh, bw))
    return out


def test_boxes_equal_the_crops(full):
    rng = np.random.RandomState(0)
    datas, boxes, names = [], [], []
    for n in DEVICE:
        for b in _boxes(EXPECTED[n]["h"], EXPECTED[n]["w"], rng):
            datas.append(_read(n))
            boxes.append(b)
            names.append(n)
    imgs, status = jpeg.decode(datas, boxes, device=DEV, return_status=True)
    assert int(status.abs().sum()) == 0
    for n, (t, l, bh, bw), im in zip(names, boxes, imgs):
        assert np.array_equal(im.cpu().numpy(), full[n][t:t + bh, l:l + bw]), (n, (t, l, bh, bw))


def test_shortest_and_default_subsequences_agree(full):
    datas = [_read(n) for n in DEVICE]
    for bits in (jpeg.MIN_SUBSEQ_BITS, 4096):
        imgs = jpeg.decode(datas, device=DEV, subseq_bits=bits)
        for n, im in zip(DEVICE, imgs):
            assert np.array_equal(im.cpu().numpy(), full[n]), (n, bits)


def test_seeded_images_against_pil():
    pytest.importorskip("PIL")
    from .jpeg_ref import pil_decode
    rng = np.random.RandomState(7)
    datas = []
    for k in range(24):
        h, w = int(rng.randint(1, 300)), int(rng.randint(1, 300))
        opts = dict(quality=int(rng.choice([10, 60, 85, 92, 98])), optimize=bool(k % 3 == 0))
        grey = k % 5 == 4
        if not grey:
            opts["subsampling"] = int(k % 3)
        if k % 4 == 1:
            opts["restart_marker_blocks"] = int(rng.randint(1, 7))
        datas.append(encode(photo(h, w, 500 + k, grey=grey), **opts))
    imgs = jpeg.decode(datas, device=DEV, subseq_bits=64)
    for k, (d, im) in enumerate(zip(datas, imgs)):
        assert np.array_equal(im.cpu().numpy(), pil_decode(d)), k


def test_malformed_scans_set_status_and_leave_the_others_exact(full):
    good = ["s420_q90_33x47", "s444_q90_33x47", "grey_q90_33x47", "s422_q75_rstrows_47x33", "s420_q90_375x500"]
    d0 = _read("s420_q90_33x47")
    hd = jpeg.parse(d0)
    truncated = d0[:hd.scan_off + 20]
    ones = d0[:hd.scan_off] + b"\xff\x00" * 64 + b"\xff\xd9"            # all-ones bits: no Huffman code
    rst = _read("s422_q75_rstrows_47x33")
    hr = jpeg.parse(rst)
    scan = rst[hr.scan_off:]
    for m in range(8):
        scan = scan.replace(bytes([0xFF, 0xD0 + m]), b"")
    no_rst = rst[:hr.scan_off] + scan
    bad = [truncated, ones, no_rst]
    datas = [_read(good[0]), bad[0], _read(good[1]), bad[1], _read(good[2]), bad[2], _read(good[3]), _read(good[4])]
    imgs, status = jpeg.decode(datas, device=DEV, return_status=True)
    st = status.cpu().tolist()
    assert [s != 0 for s in st] == [False, True, False, True, False, True, False, False], st
    assert st[1] == 4 and st[3] == 2, st
    for k in (1, 3, 5):
        assert bool((imgs[k] == jpeg.FILL).all()), k
    for k, n in zip((0, 2, 4, 6, 7), good):
        assert np.array_equal(imgs[k].cpu().numpy(), full[n]), n


def _code(t, sym):
    """(length, code) of symbol ``sym`` in the device lookup table t (jpeg.huff_table)."""
    look, maxcode, valoff, vals = t[:1024].view(np.uint16), t[1024:1096].view(np.int32), t[1096:1168].view(np.int32), t[1168:]
    for i, e in enumerate(look.tolist()):
        if e and (e & 255) == sym:
            return e >> 8, i >> (9 - (e >> 8))
    for ln in range(10, 17):
        for code in range(int(maxcode[ln]), -1, -1):
            idx = int(valoff[ln]) + code
            if idx < 0 or (code >> (ln - 9)) < 512 and look[code >> (ln - 9)]:
                break
            if vals[idx] == sym:
                return ln, code
    raise KeyError(sym)


def _scan(bits):
    """Entropy-coded bytes of a '0'/'1' string: padded with ones, 0xFF stuffed, then EOI."""
    bits += "1" * (-len(bits) % 8)
    out = bytearray()
    for k in range(0, len(bits), 8):
        out.append(int(bits[k:k + 8], 2))
        if out[-1] == 0xFF:
            out.append(0)
    return bytes(out) + b"\xff\xd9"


def test_coefficient_overflow_and_bad_records_next_to_good_images(full):
    """A scan whose first block runs past coefficient 63 (DC 0, then four ZRL-like runs of 15 zeros + 1) gets status 3 and
    a filled region; records that point outside the data, the scratch or the output, or carry an impossible geometry, get
    status 1 without a fault, and a filled region where the region itself lies in bounds; the good images stay exact."""
    grey = _read("grey_q90_33x47")
    hd = jpeg.parse(grey)
    dl, dc = _code(hd.huff[hd.comps[0][0]], 0)
    al, ac = _code(hd.huff[hd.comps[0][1]], 0xF1)
    bits = format(dc, "0%db" % dl) + (format(ac, "0%db" % al) + "1") * 4
    overflow = grey[:hd.scan_off] + _scan(bits)
    names = ["s420_q90_33x47", "grey_q90_33x47", "s444_q90_33x47", "s422_q75_rstrows_47x33"]
    datas = [_read(names[0]), overflow, _read(names[1]), _read(names[2]), _read(names[3]), _read(names[0]),
             _read(names[1]), _read(names[2])]
    jobs = [jpeg.Job(d, jpeg.parse(d), (0, 0, jpeg.parse(d).h, jpeg.parse(d).w)) for d in datas]
    sec, rec, outs, out_bytes, scr_bytes = jpeg.layout(jobs, 0)
    rec[5, jpeg.R_SCAN] = len(sec) + 4096               # scan past the data
    rec[6, jpeg.R_SCRATCH_LEN] = 16                     # scratch smaller than the image needs
    rec[7, jpeg.R_H] = -3                               # impossible geometry
    rec[3, jpeg.R_OUT] = out_bytes                      # region past the output: nothing may be written
    data = torch.from_numpy(sec).to(DEV)
    r = data[:len(jobs) * jpeg.REC_WORDS * 8].view(torch.int64).view(len(jobs), jpeg.REC_WORDS)
    out = torch.full((out_bytes + 64,), 7, dtype=torch.uint8, device=DEV)
    scratch = torch.empty(scr_bytes, dtype=torch.uint8, device=DEV)
    status = torch.full((len(jobs),), -1, dtype=torch.int32, device=DEV)
    jpeg.launch(data, r, len(jobs), scratch, out, status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 3, 0, 1, 0, 1, 1, 1]
    o = out.cpu().numpy()
    region = lambda k: o[outs[k]:outs[k] + jobs[k].nbytes]                          # noqa: E731
    for k in (1, 5, 6, 7):
        assert (region(k) == jpeg.FILL).all(), k
    assert (region(3) == 7).all() and (o[out_bytes:] == 7).all()                    # its own slot and the tail untouched
    for k, n in ((0, names[0]), (2, names[1]), (4, names[3])):
        assert np.array_equal(region(k).reshape(full[n].shape), full[n]), n


# ------------------------------------------------------------------------------------------------------------ loader
@pytest.fixture(scope="module")
def mixed_tree(tmp_path_factory):
    """A list-file tree of device-decodable JPEGs (every sampling, restart intervals, grey), routed files (progressive,
    CMYK, PNG bytes named .jpg) and .npy arrays."""
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    root = tmp_path_factory.mktemp("jpeg_lt")
    os.makedirs(os.path.join(str(root), "img"))
    rng = np.random.RandomState(3)
    lines = []
    for i in range(45):
        h, w = int(rng.randint(40, 140)), int(rng.randint(40, 140))
        kind = i % 9
        img = photo(h, w, 1000 + i, grey=kind == 3)
        name = "img/%d.jpg" % i
        if kind in (0, 1, 2):
            data = encode(img, quality=int(rng.choice([50, 75, 90, 95])), subsampling=kind)
        elif kind == 3:
            data = encode(img, quality=85)
        elif kind == 4:
            data = encode(img, quality=80, subsampling=2, restart_marker_blocks=2)
        elif kind == 5:
            data = encode(img, quality=80, progressive=True)
        elif kind == 6:
            f = io.BytesIO()
            Image.fromarray(img).convert("CMYK").save(f, "JPEG", quality=80)
            data = f.getvalue()
        elif kind == 7:
            f = io.BytesIO()
            Image.fromarray(img).save(f, "PNG")
            data = f.getvalue()
        else:
            data, name = None, "img/%d.npy" % i
            np.save(os.path.join(str(root), name), img)
        if data is not None:
            with open(os.path.join(str(root), name), "wb") as f:
                f.write(data)
        lines.append("%s %d" % (name, i % 5))
    for fn, ls in (("train.txt", lines), ("eval.txt", lines[:19])):
        with open(os.path.join(str(root), fn), "w") as f:
            f.write("\n".join(ls) + "\n")
    return str(root), os.path.join(str(root), "train.txt"), os.path.join(str(root), "eval.txt")


def _batches(loader, epoch):
    loader.set_epoch(epoch)
    out = [(x.cpu(), t.cpu()) for x, t in loader]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("policy", [None, "imagenet", "randaugment"])
def test_device_decode_loader_equals_host_decode(mixed_tree, policy):
    root, train_txt, _ = mixed_tree
    ds = LT_Dataset(root, train_txt, 5)
    kw = dict(train=True, size=48, dset_name="places_lt", seed=11, workers=2, device=DEV, policy=policy)
    host = lt_device.DeviceLTLoader(ds, 8, **kw)
    dev = lt_device.DeviceLTLoader(ds, 8, decode="device", **kw)
    a, b = _batches(host, 2), _batches(dev, 2)
    assert len(a) == len(ds) // 8 and _same(a, b)
    assert dev.decode_failures() == 0
    assert _same(b, _batches(dev, 2))                                  # the same (seed, epoch, rank), again
    assert not torch.equal(b[0][0], _batches(dev, 3)[0][0])


def test_device_decode_eval_and_two_ranks(mixed_tree):
    root, train_txt, eval_txt = mixed_tree
    ds = LT_Dataset(root, train_txt, 5)
    ev = LT_Dataset_Eval(root, eval_txt, ds.class_map, 5)
    kw = dict(train=False, size=40, workers=0, device=DEV)
    assert _same(_batches(lt_device.DeviceLTLoader(ev, 6, **kw), 0),
                 _batches(lt_device.DeviceLTLoader(ev, 6, decode="device", **kw), 0))
    for rank in (0, 1):
        kw = dict(train=True, size=40, seed=5, rank=rank, world=2, workers=1, device=DEV)
        assert _same(_batches(lt_device.DeviceLTLoader(ds, 4, **kw), 1),
                     _batches(lt_device.DeviceLTLoader(ds, 4, decode="device", **kw), 1))


def _first_loss(extra, root, train_txt, eval_txt):
    """The first logged training loss of one CLI run in a fresh process whose global RNG (the model's initialisation) is
    seeded, so that two runs differ only by their input path."""
    args = ["--dset_name", "places_lt", "--data-path", root, "--train-txt", train_txt, "--eval-txt", eval_txt,
            "--device-augment", "--model", "resnet18", "--image-size", "64", "-b", "8", "-j", "2", "--epochs", "1",
            "--max-iters", "2", "--print-freq", "1"] + extra
    boot = ("import runpy, sys, torch; torch.manual_seed(0); sys.argv = ['iif_amd.train'] + sys.argv[1:]; "
            "runpy.run_module('iif_amd.train', run_name='__main__')")
    cmd = [sys.executable, "-c", boot] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    out = r.stdout + r.stderr
    m = re.search(r"loss: ([-0-9.e+]+)", out)
    assert m, out[-3000:]
    return m.group(1), out


def test_train_cli_device_decode_first_loss_equals_host_decode(mixed_tree):
    root, train_txt, eval_txt = mixed_tree
    host, _ = _first_loss([], root, train_txt, eval_txt)
    dev, out = _first_loss(["--device-decode"], root, train_txt, eval_txt)
    assert host == dev
    assert re.search(r"epoch 0: device JPEG decode failures: train 0, eval 0", out)
