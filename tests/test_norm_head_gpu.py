"""The row kernels of iif_amd/csrc/norm_head.hip, called directly, against the float64 closed forms of tests/head_cases.py.

Every (rows, cols) of ``head_cases.ROWS`` x ``head_cases.COLS`` (last blocks with 1, 3 and 4 live waves; one lane chunk, its two
neighbours, ten and 32 chunks), every operand with leading dimension cols, cols + 1 and cols + 7 independently, every dtype
combination the entries accept.  Inputs live in buffers whose padding is NaN (a read outside the window poisons the result),
outputs in buffers pre-filled with a sentinel (nothing outside the window may change).  Bounds: head_cases' docstring; every
element of every row is compared, no tolerance is fitted to the kernels.

Measured on the MI355X, worst |error| / bound over all shapes, leading dimensions and dtypes (each test prints its own table):
  rowmap forward   fp32 out 0.13 (2.4e-7), norms 0.06;  backward fp32 out 0.19 (mode 0), 0.16 (mode 1)
  rownorm          forward 0.19, norms 0.07, backward 0.31 (power 0.5 with a row scale)
  bf16 outputs     0.996 in every combination: a single round-to-nearest of bf16 (8 significand bits) is up to 2^-8 of a value
                   just above a power of two, which is the whole of the bound's bf16 term; the fp32 part stays as above
  dot_window       0.93 (2.8e-8: the final fp32 rounding of a one-element window);  transpose: bit-exact
The mode-1 row of norm 1e-13 (eps 1e-12) was 1e-3 of g / eps away before the kernel dropped the projection term there.
"""
import itertools

import pytest
import torch

from tests import head_cases as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
NAN = float("nan")
SENT = -7.0                                     # exact in bf16 and fp32
SHAPES = [(r, c) for r in H.ROWS for c in H.COLS]
FWD_DTYPES = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)]
BWD_DTYPES = [(F32, F32, F32), (BF16, BF16, BF16), (BF16, F32, BF16), (F32, BF16, F32)]     # (x, g, dx)
WORST = {}


def _note(key, ratio, err):
    if ratio > WORST.get(key, (0.0, 0.0))[0]:
        WORST[key] = (ratio, err)


def _report(prefix):
    for k in sorted(k for k in WORST if k.startswith(prefix)):
        print("  worst %-28s ratio %.3f  err %.3e" % (k, WORST[k][0], WORST[k][1]))


def _check(key, got, ref_d, bound_d):
    ratio, err = H.worst_ratio(got, ref_d, bound_d)
    _note(key, ratio, err)
    return ratio


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_rowmap_forward(rows, cols):
    """Measured (MI355X, worst |error| / bound over the 30 shapes): fp32 out 0.13 (mode 0), 0.12 (mode 1); norms 0.06; bf16 out
    0.996 (one bf16 rounding, see the module docstring)."""
    from iif_amd import ops
    bad = []
    for (xdt, odt), (mode, scale, eps) in itertools.product(FWD_DTYPES, [(0, 2.5, 1e-12), (1, 1.0, 1e-12), (1, 1.0, 0.0)]):
        x = H.rows_matrix(rows, cols, 100 + cols, xdt, tiny=eps > 0)
        out, b_out, n, b_n = H.rowmap_forward_bounds(x, mode, scale, eps)
        out_d, b_out_d = out.to(DEV), H.stored(b_out, out, odt).to(DEV)
        n_d, b_n_d = n.to(DEV), b_n.to(DEV)
        for px, po in itertools.product(H.PADS, H.PADS):
            _, xw = H.padded(x, px, xdt, NAN, DEV)
            obuf, ow = H.padded((rows, cols), po, odt, SENT, DEV)
            nbuf = torch.full((rows + 2,), SENT, dtype=F32, device=DEV)
            ops.rowmap_forward(xw, mode, scale, ow, nbuf[1:rows + 1], eps=eps)
            key = "fwd m%d %s->%s" % (mode, str(xdt)[6:], str(odt)[6:])
            r1 = _check(key, ow, out_d, b_out_d)
            r2 = _check("fwd norms m%d" % mode, nbuf[1:rows + 1], n_d, b_n_d)
            ok = H.outside_untouched(obuf, rows, cols, SENT) and nbuf[0].item() == SENT and nbuf[-1].item() == SENT
            if not (r1 <= 1 and r2 <= 1 and ok):
                bad.append((key, eps, px, po, r1, r2, ok))
        # norms=None: the same output, nothing else written
        _, xw = H.padded(x, 0, xdt, NAN, DEV)
        obuf, ow = H.padded((rows, cols), 1, odt, SENT, DEV)
        ops.rowmap_forward(xw, mode, scale, ow, None, eps=eps)
        if not (_check("fwd m%d nonorms" % mode, ow, out_d, b_out_d) <= 1 and H.outside_untouched(obuf, rows, cols, SENT)):
            bad.append(("norms=None", mode, xdt, odt))
        if rows >= 3:                                                  # the row of zeros comes out as zeros, exactly
            assert (ow[1] == 0).all()
    _report("fwd")
    assert not bad, bad


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_rowmap_backward(rows, cols):
    """Measured (MI355X, worst |error| / bound over the 30 shapes): fp32 dx 0.19 (mode 0), 0.16 (mode 1); bf16 dx 0.996."""
    from iif_amd import ops
    bad = []
    for (xdt, gdt, ddt), (mode, scale, eps) in itertools.product(BWD_DTYPES, [(0, 2.5, 1e-12), (1, 1.0, 1e-12), (1, 1.0, 0.0)]):
        x = H.rows_matrix(rows, cols, 200 + cols, xdt, tiny=eps > 0)
        g = H.rows_matrix(rows, cols, 300 + cols, gdt, special=False)
        n32 = (x * x).sum(-1).sqrt().float()                           # the stored norm the kernel is handed
        dx, b_dx = H.rowmap_backward_bounds(x, n32.to(F64), g, mode, scale, eps)
        dx_d, b_d = dx.to(DEV), H.stored(b_dx, dx, ddt).to(DEV)
        n_d = n32.to(DEV)
        key = "bwd m%d %s,%s->%s" % (mode, str(xdt)[6:], str(gdt)[6:], str(ddt)[6:])
        for px, pg, pd in itertools.product(H.PADS, H.PADS, H.PADS):
            _, xw = H.padded(x, px, xdt, NAN, DEV)
            _, gw = H.padded(g, pg, gdt, NAN, DEV)
            dbuf, dw = H.padded((rows, cols), pd, ddt, SENT, DEV)
            ops.rowmap_backward(xw, n_d, gw, mode, scale, dw, eps=eps)
            r1 = _check(key, dw, dx_d, b_d)
            ok = H.outside_untouched(dbuf, rows, cols, SENT)
            if not (r1 <= 1 and ok):
                bad.append((key, eps, px, pg, pd, r1, ok))
        if rows >= 3:                 # a row of zeros: mode 0 passes scale * g (one fp32 product), mode 1 leaves it at zero
            if mode == 0:
                want = (g[1].float() * torch.tensor(scale, dtype=F32)).to(ddt)
                assert torch.equal(dw[1].cpu(), want), key
            else:
                assert (dw[1] == 0).all(), key
        if rows >= 5 and mode == 1 and eps > 0:
            # norm 1e-13 < eps: the map is x / eps there, so the gradient is g / eps with no projection term
            r3 = H.worst_ratio(dw[3], (g[3] / eps).to(DEV), H.stored(16 * H.U24 * (g[3] / eps).abs(), g[3] / eps, ddt).to(DEV))[0]
            assert r3 <= 1, (key, r3)
    _report("bwd")
    assert not bad, bad


def test_rowmap_refuses_other_dtype_combinations():
    """The four (x, g, dx) triples the backward entry does not instantiate, and dtype codes outside {fp32, bf16} in either
    entry, return IIF_EINVAL before anything is launched: the output keeps its sentinel."""
    from iif_amd import _lib, ops
    rows, cols = 5, 65
    x = H.rows_matrix(rows, cols, 1)
    n_d = x.norm(dim=1).float().to(DEV)
    for xdt, gdt, ddt in itertools.product((F32, BF16), repeat=3):
        if (xdt, gdt, ddt) in BWD_DTYPES:
            continue
        xw, gw = x.to(DEV).to(xdt), x.to(DEV).to(gdt)
        dx = torch.full((rows, cols), SENT, dtype=ddt, device=DEV)
        with pytest.raises(_lib.IIFNativeError, match="IIF_EINVAL"):
            ops.rowmap_backward(xw, n_d, gw, 1, 1.0, dx)
        assert (dx == SENT).all()
    L = _lib.lib()
    xw = x.to(DEV).float()
    out = torch.full((rows, cols), SENT, dtype=F32, device=DEV)
    for xc, oc in ((2, 0), (0, 2), (-1, 1)):
        assert L.iif_rowmap_forward(_lib.ptr(xw), xc, rows, cols, cols, 1, 1.0, 1e-12, _lib.ptr(out), oc, cols, 0,
                                    _lib.stream_ptr()) == -1
        assert L.iif_rowmap_backward(_lib.ptr(xw), xc, _lib.ptr(n_d), _lib.ptr(xw), 0, rows, cols, cols, cols, 1, 1.0, 1e-12,
                                     _lib.ptr(out), oc, cols, _lib.stream_ptr()) == -1
    assert (out == SENT).all()


ROWNORM_COLS = H.COLS + (2304,)                 # 2304: a 3 x 3 NormedConv2d row over 256 channels


def _row_scale(rows, seed):
    r = torch.randn(rows, generator=torch.Generator().manual_seed(seed), dtype=F64).float().to(F64) * 2
    if rows >= 3:
        r[0] = 0.0
    if rows >= 4:
        r[2] = -1.75
    return r


@pytest.mark.parametrize("rows,cols", [(r, c) for r in H.ROWS for c in ROWNORM_COLS])
def test_rownorm_forward_backward(rows, cols):
    """Measured (MI355X, worst |error| / bound over the 35 shapes): forward 0.19, norms 0.07, backward 0.31."""
    from iif_amd import ops
    bad = []
    scale, eps = 20.0, 1e-6
    x = H.rows_matrix(rows, cols, 400 + cols, F32, special=False)
    if rows >= 3:
        x[1] = 0
    g = H.rows_matrix(rows, cols, 500 + cols, F32, special=False)
    for power, with_r in itertools.product((1.0, 2.0, 0.5), (False, True)):
        r = _row_scale(rows, rows) if with_r else None
        r_d = None if r is None else r.float().to(DEV)
        out, b_out, n, b_n = H.rownorm_forward_bounds(x, r, power, scale, eps)
        v = x if r is None else x * r[:, None]
        n32 = (v * v).sum(-1).sqrt().float()
        dx, b_dx = H.rownorm_backward_bounds(x, r, n32.to(F64), g, power, scale, eps)
        out_d, b_out_d, n_d, b_n_d, dx_d, b_dx_d = (t.to(DEV) for t in (out, b_out, n, b_n, dx, b_dx))
        n32_d = n32.to(DEV)
        key = "rownorm p%g%s" % (power, " r" if with_r else "")
        for px, pg, po in itertools.product(H.PADS, H.PADS, H.PADS):
            _, xw = H.padded(x, px, F32, NAN, DEV)
            _, gw = H.padded(g, pg, F32, NAN, DEV)
            obuf, ow = H.padded((rows, cols), po, F32, SENT, DEV)
            dbuf, dw = H.padded((rows, cols), po, F32, SENT, DEV)
            nbuf = torch.full((rows + 2,), SENT, dtype=F32, device=DEV)
            ops.rownorm_forward(xw, power, scale, eps, ow, nbuf[1:rows + 1], row_scale=r_d)
            ops.rownorm_backward(xw, n32_d, gw, power, scale, eps, dw, row_scale=r_d)
            r1 = _check(key + " fwd", ow, out_d, b_out_d)
            r2 = _check(key + " norms", nbuf[1:rows + 1], n_d, b_n_d)
            r3 = _check(key + " bwd", dw, dx_d, b_dx_d)
            ok = (H.outside_untouched(obuf, rows, cols, SENT) and H.outside_untouched(dbuf, rows, cols, SENT)
                  and nbuf[0].item() == SENT and nbuf[-1].item() == SENT)
            if not (r1 <= 1 and r2 <= 1 and r3 <= 1 and ok):
                bad.append((key, px, pg, po, r1, r2, r3, ok))
        if rows >= 3:                                                  # the row of zeros: forward 0, backward r g scale / eps
            assert (ow[1] == 0).all()
            rr = 1.0 if r is None else r[1]
            want = rr * g[1] * scale / eps
            assert H.worst_ratio(dw[1], want.to(DEV), (16 * H.U24 * want.abs()).to(DEV))[0] <= 1, key
            if with_r:
                assert (ow[0] == 0).all() and (dw[0] == 0).all()       # row scale 0
    _report("rownorm")
    assert not bad, bad


def test_rownorm_zero_rows_touch_nothing():
    from iif_amd import ops
    x = torch.empty((0, 64), dtype=F32, device=DEV)
    out = torch.full((4, 64), SENT, dtype=F32, device=DEV)
    norms = torch.full((4,), SENT, dtype=F32, device=DEV)
    ops.rownorm_forward(x, 1.0, 20.0, 1e-6, out[:0], norms[:0])
    ops.rownorm_backward(x, norms[:0], x, 1.0, 20.0, 1e-6, out[:0])
    ops.rowmap_forward(x, 1, 1.0, out[:0], norms[:0])
    ops.rowmap_backward(x, norms[:0], x, 1, 1.0, out[:0])
    torch.cuda.synchronize()
    assert (out == SENT).all() and (norms == SENT).all()


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 100])
@pytest.mark.parametrize("cols", [1, 31, 32, 33, 100])
def test_transpose_is_bit_exact(rows, cols):
    from iif_amd import ops
    src = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows * 101 + cols))
    for pi, po in itertools.product(H.PADS, H.PADS):
        _, sw = H.padded(src, pi, F32, NAN, DEV)
        dbuf, dw = H.padded((cols, rows), po, F32, SENT, DEV)
        ops.transpose_f32(sw, dw)
        assert torch.equal(dw.cpu(), src.t()), (pi, po)
        assert H.outside_untouched(dbuf, cols, rows, SENT), (pi, po)


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 255), (3, 85), (1, 256), (16, 16), (1, 257), (257, 1), (10, 1000)])
def test_dot_window(rows, cols):
    """rows * cols in {1, 255, 256, 257, 10 000}: below, at and above one pass of the 256 threads.  Measured (MI355X): worst
    |error| / bound 0.93, 2.8e-8 absolute (the final fp32 rounding)."""
    from iif_amd import ops
    a = H.rows_matrix(rows, cols, 600 + cols, special=False)
    b = H.rows_matrix(rows, cols, 700 + cols, special=False)
    div = torch.tensor([5.0], dtype=F32, device=DEV)
    for pa, pb, (alpha, use_div) in itertools.product(H.PADS, H.PADS, [(1.0, False), (2.0, True), (-0.375, False)]):
        _, aw = H.padded(a, pa, F32, NAN, DEV)
        _, bw = H.padded(b, pb, F32, NAN, DEV)
        out = torch.full((3,), SENT, dtype=F32, device=DEV)
        ops.dot_window_f32(aw, bw, rows, cols, alpha, out[1:2], alpha_div=div if use_div else None)
        ref, bound = H.dot_window(a, b, alpha, 5.0 if use_div else None)
        got = out.cpu().to(F64)
        err = abs(got[1].item() - ref.item())
        _note("dot_window", err / bound.item() if err else 0.0, err)
        assert err <= bound.item(), (pa, pb, alpha, use_div, err, bound.item())
        assert got[0] == SENT and got[2] == SENT
    _report("dot_window")
