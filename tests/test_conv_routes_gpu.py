"""The 256 x 128 tile of the convolution entry (conv_igemm_dma_utap256_kernel: conv_igemm_dma_body with eight waves) against
float64, at sizes whose route is pinned through the launch-free query, and the smallest cases for the kernel / operand-set pairs
of the route census that no other test reaches (tests/conv_route_cases.py).

Every case first asserts the route (ops.conv_route), then runs the public ops wrapper and compares every element with a float64
evaluation of the same bf16 operands made of plain tensor operations: per tap a shifted, zero-padded slice of the source times
that tap's weight slab, accumulated (the data gradient as the transpose: the products scattered to the source positions; stride
2 by strided slices).  No convolution routine is called.

Bound per element, from where staged_drain / conv_epilogue_staged round (conv_igemm.hip):
  1. the fp32 accumulator (plus the fp32 source bias of a two-source launch, which joins it BEFORE the rounding) is rounded to
     bf16 once, when the tile is parked in LDS:                       2^-8 |acc + bias|
  2. with a residual, the parked bf16 value and the bf16 residual (gated by its ReLU bit) are added in fp32 and the sum is
     rounded to bf16 again:                                            2^-8 (|acc + bias + residual| + the terms 1 and 4: the
     value rounded here is the parked one, that far from the reference's)
  3. the gated store zeroes elements by the upstream bits and rounds nothing;
  4. the accumulation itself, K = taps x Cs (+ Cs2) products in fp32:  2 K 2^-24 S,  S = float64 sum of |a| |b| (the same
     reference over absolute values).
2^-8 is the largest relative error of one rounding to bf16's 8 significant bits (half an ulp of a value just above a power of
two), so over millions of elements the largest error / bound ratio comes close to 1 without ever passing it: the bound has no
slack for a wrong element to hide in.  The gates of these operand sets are INPUTS (random bits), not decisions the kernel
takes, so gated elements are compared exactly (zero where the bit is clear) and nothing is excluded near zero: the excluded
share is 0 <= 1e-3.

Partial rows: forward statistics are (sum, sum of squares) of the STORED bf16 values; the upstream sums are (sum g, sum g xhat)
of the stored values gated by the upstream bits, xhat = (x - mean) invstd; the gated store leaves (sum of the stored, 0).  The
references are float64 sums of exactly those, tolerances as in the sibling tests of test_conv_gpu.py (forward statistics 1e-5,
upstream and two-source sums 2e-6, gated store 8 x 2e-6, each times max(1, largest reference sum))."""
import pytest
import torch

from tests import conv_route_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
CANARY = 4096                       # bf16 elements behind dst
SPARE_ROWS = 8
CHUNK = 8192                        # rows of a float64 product at a time


@pytest.fixture(scope="module")
def ops256():
    from iif_amd import _lib, ops
    L = _lib.lib()
    L.iif_set_cu_budget(0)
    if L.iif_get_cu_budget() != 256:
        pytest.skip("the routes of this module are pinned for 256 compute units")
    return ops


def _mm(a, b64):
    """a [m, k] (any float dtype) @ b64 [k, n] in float64, CHUNK rows at a time."""
    out = torch.empty(a.shape[0], b64.shape[1], dtype=torch.float64, device=a.device)
    for i in range(0, a.shape[0], CHUNK):
        out[i:i + CHUNK] = a[i:i + CHUNK].double() @ b64
    return out


def _pad64(t, pad_h, pad_w, absolute):
    n, h, w, c = t.shape
    out = torch.zeros(n, h + 2 * pad_h, w + 2 * pad_w, c, dtype=torch.float64, device=t.device)
    out[:, pad_h:pad_h + h, pad_w:pad_w + w] = t.double().abs() if absolute else t.double()
    return out


def ref_forward(x, w, k, stride, pad, ho, wo, absolute=False):
    """[n * ho * wo, cout] float64: sum over taps of (shifted slice of the padded source) @ (that tap's weight slab)^T."""
    n, h, wd, cin = x.shape
    w64 = w.double().abs() if absolute else w.double()
    if k == 1 and stride == 1:
        return _mm((x.abs() if absolute else x).reshape(-1, cin), w64[:, :cin].t())
    xp = _pad64(x, pad, pad, absolute)
    out = torch.zeros(n * ho * wo, w.shape[0], dtype=torch.float64, device=x.device)
    for r in range(k):
        for s in range(k):
            sl = xp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride]
            out += _mm(sl.reshape(-1, cin), w64[:, (r * k + s) * cin:(r * k + s + 1) * cin].t())
    return out


def ref_dgrad(dy, wt, k, stride, pad, h, wd, absolute=False):
    """[n * h * wd, cin] float64, the transpose of ref_forward: the products of every tap scattered to the source positions."""
    n, ho, wo, cout = dy.shape
    w64 = wt.double().abs() if absolute else wt.double()
    src = dy.abs() if absolute else dy
    if k == 1 and stride == 1:
        return _mm(src.reshape(-1, cout), w64[:, :cout].t())
    hp, wp = max(h + 2 * pad, stride * (ho - 1) + k), max(wd + 2 * pad, stride * (wo - 1) + k)
    dxp = torch.zeros(n, hp, wp, wt.shape[0], dtype=torch.float64, device=dy.device)
    for r in range(k):
        for s in range(k):
            t = _mm(src.reshape(-1, cout), w64[:, (r * k + s) * cout:(r * k + s + 1) * cout].t())
            dxp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride] += t.view(n, ho, wo, -1)
    return dxp[:, pad:pad + h, pad:pad + wd].reshape(n * h * wd, -1)


def last_row_term(case, src, wgt, pixel, channels=32):
    """What the last `channels` source channels of the last tap that reads inside the image contribute to destination pixel
    (n, y, x), float64 [cd]; None if no tap does."""
    n_, h, w, cin, cout, k, stride = case.layer
    pad = k // 2
    b, y, x = pixel
    cs = src.shape[3]
    channels = min(channels, cs)
    term = None
    for r in range(k):
        for s in range(k):
            if case.direction == "fwd":
                ys, xs = y * stride + r - pad, x * stride + s - pad
            else:
                if (y + pad - r) % stride or (x + pad - s) % stride:
                    continue
                ys, xs = (y + pad - r) // stride, (x + pad - s) // stride
            if 0 <= ys < src.shape[1] and 0 <= xs < src.shape[2]:
                lo = (r * k + s) * cs + cs - channels
                term = wgt[:, lo:lo + channels].double() @ src[b, ys, xs, cs - channels:].double()
    return term


def _bits(gen, count):
    return torch.randint(0, 256, (count // 8,), dtype=torch.uint8, device=DEV, generator=gen)


def _mask(bits, m, c):
    return ((bits.view(-1, 1).int() >> torch.arange(8, device=bits.device).view(1, 8)) & 1).view(m, c).bool()


def run_case(ops, case):
    """Runs the case twice; returns everything the checks need."""
    n, h, w, cin, cout, k, stride = case.layer
    pad = k // 2
    ho, wo = ops.conv_out_hw(h, w, k, k, stride, pad)
    operands = C.operands_of(case.direction, case.opset)
    gen = torch.Generator(device=DEV).manual_seed(1000 + sum(case.layer))
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)           # noqa: E731
    if case.direction == "fwd":
        src, (dn, dh, dw, cd), kk = rnd(n, h, w, cin).to(BF), (n, ho, wo, cout), k * k * cin
    elif case.direction == "dgrad":
        src, (dn, dh, dw, cd), kk = rnd(n, ho, wo, cout).to(BF), (n, h, w, cin), k * k * cout
    else:
        src, (dn, dh, dw, cd), kk = rnd(n, h, w, cin).to(BF), (n, h, w, cout), cin + case.cs2
    m = dn * dh * dw
    wgt = (rnd(cd, kk) / kk ** 0.5).to(BF)
    src2 = torch.relu(rnd(n, h, w, case.cs2)).to(BF) if "src2" in operands else None
    sbias = rnd(cd) * 0.5 if "src_bias" in operands else None
    res = rnd(dn, dh, dw, cd).to(BF) if "res" in operands else None
    acc_into = "res_is_dst" in operands               # dst += ...: the residual IS the destination, filled anew for each call
    rbits = _bits(gen, m * cd) if "res_bits" in operands else None
    ubits = _bits(gen, m * cd) if "up_bits" in operands else None
    upx = rnd(dn, dh, dw, cd).to(BF) if "up_x" in operands else None
    stats = None
    if "up_stats" in operands:
        stats = torch.zeros(4, cd, device=DEV)
        stats[0] = rnd(cd) * 0.1
        stats[1] = torch.rand(cd, device=DEV, generator=gen) + 0.5
    rows = case.rows
    outs = []
    for _ in range(2):
        buf = torch.full((m * cd + CANARY,), float("nan"), dtype=BF, device=DEV)
        buf[m * cd:].view(torch.int16).copy_(torch.arange(CANARY, device=DEV, dtype=torch.int16))
        out = buf[:m * cd].view(dn, dh, dw, cd)
        if acc_into:
            out.copy_(res)
        partial = torch.full((rows + SPARE_ROWS, 2, cd), float("nan"), device=DEV) if "partial" in operands else None
        nt = None
        if case.direction == "fwd":
            if partial is not None:
                nt = ops.conv_forward_bnstats(src, wgt, k, k, stride, pad, out, partial.view(-1))
            else:
                ops.conv_forward(src, wgt, k, k, stride, pad, out=out, res=res)
        elif case.direction == "dgrad":
            if "gated_store" in operands:
                nt = ops.conv_dgrad_masksum(src, wgt, (h, w), out, ubits, partial.view(-1), res=res, res_bits=rbits)
            elif partial is not None:
                nt = ops.conv_dgrad_bnbwd(src, wgt, k, k, stride, pad, (h, w), out, upx, ubits, stats, partial.view(-1), res=res,
                                          res_bits=rbits)
            else:
                ops.conv_dgrad(src, wgt, k, k, stride, pad, (h, w), out=out, res=out if acc_into else res, res_bits=rbits)
        else:
            nt = ops.conv_dgrad2_bnbwd(src, src2, wgt, sbias, out, upx, ubits, stats, None if partial is None else partial.view(-1))
            nt = nt if partial is not None else None
        outs.append((buf, partial, nt))
    torch.cuda.synchronize()
    return dict(src=src, wgt=wgt, src2=src2, sbias=sbias, res=res, rbits=rbits, ubits=ubits, upx=upx, stats=stats, outs=outs,
                m=m, cd=cd, kk=kk, dims=(dn, dh, dw), ho=ho, wo=wo, operands=operands)


def reference(case, r):
    """(float64 reference of the stored tensor [m, cd], per-element bound, gate mask or None)."""
    n, h, w, cin, cout, k, stride = case.layer
    pad = k // 2
    m, cd = r["m"], r["cd"]
    both = []
    for absolute in (False, True):
        if case.direction == "fwd":
            v = ref_forward(r["src"], r["wgt"], k, stride, pad, r["ho"], r["wo"], absolute)
        elif case.direction == "dgrad":
            v = ref_dgrad(r["src"], r["wgt"], k, stride, pad, h, w, absolute)
        else:
            w64 = r["wgt"].double().abs() if absolute else r["wgt"].double()
            a, b = (r["src"].abs(), r["src2"].abs()) if absolute else (r["src"], r["src2"])
            v = _mm(a.reshape(m, cin), w64[:, :cin].t()) + _mm(b.reshape(m, case.cs2), w64[:, cin:cin + case.cs2].t())
        both.append(v)
    acc, S = both
    if r["sbias"] is not None:
        acc = acc + r["sbias"].double()
    bound = 2.0 ** -8 * acc.abs() + 2.0 * r["kk"] * 2.0 ** -24 * S                  # roundings 1 and 4
    if r["res"] is not None:
        rr = r["res"].reshape(m, cd).double()
        if r["rbits"] is not None:
            rr = rr * _mask(r["rbits"], m, cd)
        acc = acc + rr
        bound = bound + 2.0 ** -8 * (acc.abs() + bound)                             # rounding 2, of a value within `bound` of acc
    gate = _mask(r["ubits"], m, cd) if "gated_store" in r["operands"] else None
    return acc, bound, gate


def compare(got, ref, bound, gate):
    """Largest |got - ref| / bound over the elements the gate lets through, and whether the gated-off ones are exactly zero."""
    err = (got.double() - ref).abs()
    if gate is not None:
        zero_ok = bool((got.view(torch.int16)[~gate] == 0).all())
        err = err * gate
    else:
        zero_ok = True
    return (err / bound.clamp_min(1e-300)).max().item(), zero_ok


def sums_reference(case, r, got, rows_mask=None):
    """float64 [2, cd]: what the partial rows add up to, from the STORED tensor (rows_mask: only these rows of it)."""
    m, cd = r["m"], r["cd"]
    g = got.double()
    if r["ubits"] is not None and "gated_store" not in r["operands"]:
        g = g * _mask(r["ubits"], m, cd)
    if rows_mask is not None:
        g = g * rows_mask.view(m, 1)
    if r["upx"] is not None:
        xhat = (r["upx"].reshape(m, cd).double() - r["stats"][0].double()) * r["stats"][1].double()
        return torch.stack([g.sum(0), (g * xhat).sum(0)])
    if "gated_store" in r["operands"]:
        return torch.stack([g.sum(0), torch.zeros(cd, dtype=torch.float64, device=g.device)])
    return torch.stack([g.sum(0), (g * g).sum(0)])


def sums_tolerance(case):
    if "gated_store" in C.operands_of(case.direction, case.opset):
        return 2e-6 * 8
    return 1e-5 if case.direction == "fwd" else 2e-6


def sums_close(ps, ref, tol):
    return all((ps[i] - ref[i]).abs().max().item() <= tol * max(1.0, ref[i].abs().max().item()) for i in range(2))


def last_tile_rows(case, r):
    """Mask [m] of the destination pixels in the last pixel tile of the last launch, and the last valid pixel of that launch."""
    dn, dh, dw = r["dims"]
    m = r["m"]
    tile = 256 if case.launches[-1][0] == "tile256" else 128
    if len(case.launches) == 1:
        mask = torch.zeros(m, dtype=torch.bool, device=DEV)
        mask[(m - 1) // tile * tile:] = True
        return mask, (dn - 1, dh - 1, dw - 1)
    # class by class: the last launch is parity class 3, pixels (2 yy + 1, 2 xx + 1) in (n, yy, xx) order
    hd, wd = dh // 2, dw // 2
    idx = torch.arange(dn * hd * wd, device=DEV)
    b, rem = idx // (hd * wd), idx % (hd * wd)
    pix = (b * dh + 2 * (rem // wd) + 1) * dw + 2 * (rem % wd) + 1
    mask = torch.zeros(m, dtype=torch.bool, device=DEV)
    mask[pix[(len(idx) - 1) // tile * tile:]] = True
    return mask, (dn - 1, 2 * (hd - 1) + 1, 2 * (wd - 1) + 1)


RATIOS = {}


@pytest.mark.parametrize("case", C.GPU_CASES + C.CENSUS_CASES, ids=lambda c: c.id)
def test_route_case(case, ops256):
    ops = ops256
    operands = C.operands_of(case.direction, case.opset)
    ans = C.route(C.case_desc(case), operands, case.cs2)
    assert isinstance(ans, list) and tuple((f, i) for f, i, _ in ans) == case.launches, (case.id, ans)
    assert sum(x[2] for x in ans) == case.rows, (case.id, ans)
    r = run_case(ops, case)
    m, cd = r["m"], r["cd"]
    (buf, partial, nt), (buf2, partial2, nt2) = r["outs"]
    # the second call is bit-identical, nothing behind dst is touched
    assert torch.equal(buf.view(torch.int16), buf2.view(torch.int16))
    assert torch.equal(buf[m * cd:].view(torch.int16), torch.arange(CANARY, device=DEV, dtype=torch.int16))
    got = buf[:m * cd].view(m, cd)
    assert not torch.isnan(got).any()                       # every row written, the ragged last tile's included
    ref, bound, gate = reference(case, r)
    ratio, zero_ok = compare(got, ref, bound, gate)
    RATIOS[case.id] = ratio
    print("%s: largest error / bound %.3f" % (case.id, ratio))
    assert zero_ok, case.id
    assert ratio <= 1.0, (case.id, ratio)
    mask, (b, y, x) = last_tile_rows(case, r)
    # control 1: the reference without the last 32 source channels of the last tap, for the last valid row only, must FAIL
    dn, dh, dw = r["dims"]
    row = (b * dh + y) * dw + x
    if case.direction == "dgrad2":
        term = r["wgt"][:, case.layer[3] + case.cs2 - 32:case.layer[3] + case.cs2].double() @ r["src2"].reshape(m, -1)[row, -32:].double()
    else:
        term = last_row_term(case, r["src"], r["wgt"], (b, y, x))
    assert term is not None
    wrong = ref[row] - term
    g_row = None if gate is None else gate[row:row + 1]
    assert compare(got[row:row + 1], ref[row:row + 1], bound[row:row + 1], g_row)[0] <= 1.0
    assert compare(got[row:row + 1], wrong[None], bound[row:row + 1], g_row)[0] > 1.0, case.id
    if partial is None:
        assert nt is None
        return
    # partial rows: the query's count, canaries behind it, float64 sums of what the kernel sums
    assert nt == nt2 == case.rows
    assert torch.isnan(partial[nt:]).all() and not torch.isnan(partial[:nt]).any()
    assert torch.equal(partial[:nt], partial2[:nt])
    ps = partial[:nt].double().sum(0)
    tol = sums_tolerance(case)
    sref = sums_reference(case, r, got)
    if "gated_store" in operands:
        assert not partial[:nt, 1].any()
    assert sums_close(ps, sref, tol), (case.id, [(ps[i] - sref[i]).abs().max().item() for i in range(2)])
    # control 2: the reference without the partial row of the last (ragged) tile must FAIL (the 256-row tile: one row per tile)
    if case.launches[-1][0] == "tile256":
        assert not sums_close(ps, sums_reference(case, r, got, ~mask), tol), case.id


def test_reference_is_a_convolution():
    """The float64 reference itself, on the host: against the definition written out as loops over a tiny case, forward and
    data gradient, stride 1 and 2."""
    g = torch.Generator().manual_seed(5)
    for k, stride, h, w in ((3, 1, 5, 4), (3, 2, 7, 5), (1, 2, 5, 5), (1, 1, 3, 3)):
        n, cin, cout, pad = 2, 3, 4, k // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        x = torch.randn(n, h, w, cin, generator=g)
        wt = torch.randn(cout, k * k * cin, generator=g)
        exp = torch.zeros(n, ho, wo, cout, dtype=torch.float64)
        dy = torch.randn(n, ho, wo, cout, generator=g)
        wtt = wt.view(cout, k, k, cin).permute(3, 1, 2, 0).reshape(cin, k * k * cout)
        dexp = torch.zeros(n, h, w, cin, dtype=torch.float64)
        for yo in range(ho):
            for xo in range(wo):
                for r in range(k):
                    for s in range(k):
                        ys, xs = yo * stride + r - pad, xo * stride + s - pad
                        if 0 <= ys < h and 0 <= xs < w:
                            slab = wt[:, (r * k + s) * cin:(r * k + s + 1) * cin].double()
                            exp[:, yo, xo] += x[:, ys, xs].double() @ slab.t()
                            dexp[:, ys, xs] += dy[:, yo, xo].double() @ slab
        assert (ref_forward(x, wt, k, stride, pad, ho, wo).view_as(exp) - exp).abs().max() < 1e-12
        assert (ref_dgrad(dy, wtt, k, stride, pad, h, w).view_as(dexp) - dexp).abs().max() < 1e-12
