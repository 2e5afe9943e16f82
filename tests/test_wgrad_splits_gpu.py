"""The weight gradient's split-K rounds and slab reduction, bit-exactly (conv_wgrad.hip: every kernel family, the padded grid,
the ragged last split, the one-pass and two-stage slab sums, the rounds a small workspace shrinks).

Exact by construction: the operands are integers from {-2, ..., 2} - exact in bf16 and fp32, every product exact, every
partial sum bounded by 4 M < 2^24 - so EVERY fp32 summation order gives the same bits, and the reference is the float64
weight gradient of the same integers (torch.nn.grad.conv2d_weight on the CPU).  Comparisons are torch.equal.  Before every
launch the output (pad columns included) and the whole workspace are filled with NaN: afterwards the logical columns equal the
reference, the pad columns and everything behind (splits + chunks) slabs are still NaN, and the slabs hold no NaN in their
logical columns.  Which kernel and how many splits a call got is the planning query's answer (iif_conv_wgrad_plan);
tests/test_wgrad_plan_host.py checks on the host that every case realises the counts its id names."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ARENA_FLOATS = (112 << 20) // 4             # the 4-group nine-tap case at 155 splits: 169 slabs of 584 KiB
IDS = [c.name for c in W.CASES]


@pytest.fixture(scope="module")
def arena():
    return torch.empty(ARENA_FLOATS, dtype=torch.float32, device=DEV)


@pytest.fixture
def family_env(monkeypatch):
    def set_(case):
        if case.family == "regstage":
            monkeypatch.setenv("IIF_CONV_REGSTAGE", "1")          # read per call by the launch and by the query
        else:
            monkeypatch.delenv("IIF_CONV_REGSTAGE", raising=False)
    return set_


def _tdt(c):
    return torch.bfloat16 if c.dtype == W.BF16 else torch.float32


def _reference(c, x, dy, dy2):
    """float64 weight gradient of NHWC float64 operands as [rows, K] KRSC rows."""
    xn, dyn = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    if dy2 is not None:
        dyn = torch.cat([dyn, dy2.permute(0, 3, 1, 2)], 1)
    if c.kind == "stem":                                             # 4 x 4, two rows / columns of padding on the top / left, one behind
        xn, pad = F.pad(xn, (2, 1, 2, 1)), 0
    else:
        pad = c.pad
    rows = dyn.shape[1]
    ref = torch.nn.grad.conv2d_weight(xn, (rows, c.cin // c.groups, c.r, c.r), dyn, c.stride, pad, 1, c.groups)
    return ref.permute(0, 2, 3, 1).reshape(rows, -1)


_OPERANDS = {}


def _operands(c):
    """(x, dy, dy2 on the device in the case's type, exact reference [rows, K] float32), computed once per case."""
    if c.name not in _OPERANDS:
        g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
        hd, wd = W.out_hw(c)
        assert 4 * c.n * hd * wd < 2 ** 24                           # every partial sum is an exactly representable integer
        x = torch.randint(-2, 3, (c.n, c.h, c.w, c.cin), generator=g).double()
        dy = x if c.kind == "gram" else torch.randint(-2, 3, (c.n, hd, wd, c.cout), generator=g).double()
        dy2 = torch.randint(-2, 3, (c.n, hd, wd, c.cd2), generator=g).double() if c.kind == "stacked" else None
        ref = _reference(c, x, dy, dy2)
        assert torch.equal(ref, ref.round()) and ref.abs().max().item() <= 4 * c.n * hd * wd
        xd = x.to(_tdt(c)).to(DEV)
        dyd = xd if c.kind == "gram" else dy.to(_tdt(c)).to(DEV)
        _OPERANDS[c.name] = (xd, dyd, None if dy2 is None else dy2.to(_tdt(c)).to(DEV), ref.float())
    return _OPERANDS[c.name]


def _plan(c, workspace_bytes, request):
    from iif_amd import ops
    row = W.row_of(c)
    return ops.conv_wgrad_plan(*row[:12], _tdt(c), row[12], workspace_bytes, request, c.cd2)


def _launch(c, operands, out, ws, request):
    from iif_amd import ops
    x, dy, dy2 = operands
    if c.kind == "stacked":
        ops.wgrad1x1_stacked(x.view(-1, c.cin), dy.view(-1, c.cout), dy2.view(-1, c.cd2), out, ws, request)
    else:
        ops.conv_wgrad(x, dy, c.r, c.r, c.stride, c.pad, ldw=out.shape[1], out=out, workspace=ws, splits=request, groups=c.groups)


def _run(c, arena, request, ws_floats="ample", operands=None, ref=None):
    """One poisoned launch, checked; returns (the query's plan, the padded output).  ws_floats: "ample" (room for the stage
    area and four slabs more), None (no workspace) or a number of floats."""
    if operands is None:
        *operands, ref = _operands(c)
    ldw = W.pad_ldw(c)
    rows, k = c.cout + max(c.cd2, 0), ldw - 8
    slab = rows * ldw
    assert slab == W.slab_floats(W.row_of(c), c.cd2)
    if ws_floats == "ample":
        want = _plan(c, 1 << 40, request)
        ws_floats = (want.splits + W.cdiv(want.splits, 16) + 4) * slab
    ws = None
    if ws_floats is not None:
        assert ws_floats <= ARENA_FLOATS
        ws = arena[:ws_floats]
        ws.fill_(NAN)
    p = _plan(c, 0 if ws is None else ws_floats * 4, request)
    assert p.family == c.family, (c.name, p)
    out = torch.full((rows, ldw), NAN, device=DEV)
    _launch(c, operands, out, ws, request)
    if ref is not None:
        assert torch.equal(out[:, :k].cpu(), ref), (c.name, request, p)
    assert out[:, k:].isnan().all(), (c.name, request, p, "pad columns written")
    if ws is not None:
        used = (p.splits + p.chunks) * slab if p.splits > 1 else 0
        if p.splits > 1:
            assert not ws[:p.splits * slab].view(p.splits, rows, ldw)[:, :, :k].isnan().any(), (c.name, request, p)
        if p.stages == 2:
            assert not ws[p.splits * slab:used].view(p.chunks, rows, ldw)[:, :, :k].isnan().any(), (c.name, request, p)
        assert ws[used:].isnan().all(), (c.name, request, p, "workspace written behind the slabs")
    return p, out


REALISED = [(c, t, q) for c in W.CASES for t, q in sorted(W.requests(c).items())]


@pytest.mark.parametrize("case,target,q", REALISED, ids=["%s-%s-splits%d" % (c.family, c.name, t) for c, t, _ in REALISED])
def test_requested_split_counts_give_the_exact_gradient(case, target, q, arena, family_env):
    """Every split count the case realises (1, 2, both sides of 16 / 32 / 48, >= 97, >= 512 for the `full` cases; the id names
    the family and the count, the query confirms both); counts above 32 in the two-stage form AND forced into one pass by a
    workspace of exactly that many slabs - or, on a slab of 1 MiB and more, in the one pass chosen by size."""
    family_env(case)
    slab = W.slab_floats(W.row_of(case), case.cd2)
    p, _ = _run(case, arena, q)
    assert p.splits == target, (case.name, target, q, p)
    assert p.blocks >= p.tiles * p.splits
    if target > 32:
        small = W.cdiv(slab, 1024) < 256
        assert small != ("1mib" in case.name or "2mib" in case.name)
        assert p.stages == (2 if small else 1) and p.chunks == (W.cdiv(target, 16) if small else 0), (case.name, p)
        if small:
            p1, _ = _run(case, arena, q, ws_floats=target * slab)
            assert (p1.splits, p1.stages, p1.chunks) == (target, 1, 0), (case.name, p1)
    else:
        assert p.stages == (1 if target > 1 else 0)


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_shrunk_and_automatic_rounds_give_the_exact_gradient(case, arena, family_env):
    """The paths that shrink a round: no workspace (one split straight into the padded-pitch output), a workspace of 5 slabs
    under a request of 33, a workspace with a slab and a half of room; and the automatic rounds for the whole, a half and a
    quarter of the device."""
    family_env(case)
    slab = W.slab_floats(W.row_of(case), case.cd2)
    p, _ = _run(case, arena, 33, ws_floats=None)
    assert (p.splits, p.stages, p.blocks) == (1, 0, p.tiles * (1 if case.family == "regstage" else 8) * (case.groups if case.family == "dma" else 1))
    p, _ = _run(case, arena, 0, ws_floats=None)
    assert p.splits == 1
    p, _ = _run(case, arena, 33, ws_floats=5 * slab)
    assert 1 < p.splits <= 5 and p.stages == 1, p
    p, _ = _run(case, arena, 33, ws_floats=slab + slab // 2)
    assert p.splits == 1
    p, _ = _run(case, arena, 3, ws_floats=2 * slab + 4)
    assert p.splits == 2
    auto = [_run(case, arena, r)[0] for r in (0, -2, -4)]
    assert auto[0].splits >= auto[1].splits >= auto[2].splits >= 1
    if case.name == "nt_64_auto":
        assert auto[0].splits > 32 and auto[0].stages == 2, auto[0]


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 32, 33, 48, 49, 256])
@pytest.mark.parametrize("room", [False, True], ids=["no_stage_room", "stage_room"])
def test_slab_sum_is_the_exact_sum_and_keeps_to_its_columns(n, room, arena):
    """iif_slab_sum on integer slabs [40, 136] of which 128 columns count (6 blocks of the sum kernel): the int64 sum, the
    columns behind `cols` of the poisoned output untouched, nothing written behind the stage area."""
    from iif_amd import ops
    rows, ld, cols = 40, 136, 128
    slab = rows * ld
    nch = W.cdiv(n, 16)
    g = torch.Generator().manual_seed(n)
    vals = torch.randint(-2, 3, (n, rows, ld), generator=g)
    total = (n + nch + 2) * slab if room else n * slab
    buf = arena[:total]
    buf.fill_(NAN)
    buf[:n * slab].copy_(vals.float().view(-1).to(DEV))
    out = torch.full((rows, ld), NAN, device=DEV)
    ops.slab_sum(buf, n, rows, ld, cols, out)
    assert torch.equal(out[:, :cols].cpu().long(), vals.sum(0)[:, :cols])
    assert out[:, cols:].isnan().all()
    assert torch.equal(buf[:n * slab].cpu().view(n, rows, ld).long(), vals)                  # the slabs themselves are only read
    two_stage = room and n > 32
    if room:
        stage = buf[n * slab:(n + nch) * slab].view(nch, rows, ld)
        assert stage[:, :, cols:].isnan().all()
        assert stage[:, :, :cols].isnan().all() != two_stage
        assert buf[(n + nch) * slab:].isnan().all()
    if two_stage:
        chunks = torch.stack([vals[i * 16:(i + 1) * 16].sum(0) for i in range(nch)])
        assert torch.equal(stage[:, :, :cols].cpu().long(), chunks[:, :, :cols])


@pytest.mark.parametrize("name,req,form", [("nt_128_w31", 49, "two_stage"), ("nt_128_w31", 49, "one_pass"), ("t_1mib", 33, "by_size"),
                                                 ("stem_98", 49, "two_stage"), ("dma_3x3s2_bf16", 48, "one_pass")])
def test_random_operands_within_the_fp32_accumulation_bound(name, req, form, arena):
    """Non-integer operands, once per form of the reduction: random bf16 values against the float64 products of the same bf16
    values.  fp32 accumulation of M exact products in ANY order errs by at most (M - 1) u sum|x||dy| (1 + O(M u)), u = 2^-24
    [Higham, Accuracy and Stability of Numerical Algorithms, section 4.2]: the bound is M 2^-24 sum_m |x||dy| per element.
    Two calls with the same req give the same bits."""
    c = W.CASE[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) + 1)
    hd, wd = W.out_hw(c)
    x = torch.randn(c.n, c.h, c.w, c.cin, generator=g).bfloat16()
    dy = torch.randn(c.n, hd, wd, c.cout, generator=g).bfloat16()
    ref = _reference(c, x.double(), dy.double(), None)
    bound = c.n * hd * wd * 2.0 ** -24 * _reference(c, x.double().abs(), dy.double().abs(), None)
    slab = W.slab_floats(W.row_of(c), 0)
    ws_floats = req * slab if form == "one_pass" else "ample"
    operands = (x.to(DEV), dy.to(DEV), None)
    p, a = _run(c, arena, req, ws_floats, operands, None)
    assert p.splits == req and (p.stages, p.chunks) == ((2, W.cdiv(req, 16)) if form == "two_stage" else (1, 0)), p
    _, b = _run(c, arena, req, ws_floats, operands, None)
    k = ref.shape[1]
    assert torch.equal(a[:, :k], b[:, :k])
    err = (a[:, :k].double().cpu() - ref).abs()
    assert (err <= bound).all(), (name, form, (err / bound.clamp_min(1e-300)).max().item())
