"""The persistent kernels under a compute-unit budget (iif_set_cu_budget): gemm1x1_regw_kernel, gemm1x1_stream_kernel,
conv3x3_regw64_kernel, stem4x4_kernel and what they leave behind (BN partial rows, prologue column sums, P / Gram slabs).

A rank that overlaps its gradient all-reduce with backward runs these kernels at 240 of 256 CUs; the parity tests of
tests/test_conv_gpu.py all run at budget 0, where the grid of a small shape is bounded by its tile count.  Every test here runs
the same operands at budget 0 and at 64 (the minimum), 72 (ragged) and 240 (the multi-rank default) and asserts
  * stored tensors: no NaN left, bit-identical to the budget-0 run (the K order of an element does not depend on the grid) and
    within 2^-7 of the tensor's maximum of a float64 evaluation of the same bf16 operands;
  * row and slab counts: the value of the documented rule (include/iif_amd.h, iif_persistent_grid_blocks; restated below in
    Python), never more than ceil(M / 128), rows below the count without NaN, rows at and above it untouched (NaN canaries,
    eight spare rows at least), and - for the budgets listed as binding - a count that differs from the budget-0 count;
  * sums of the rows against float64 sums of the stored tensor, P / Gram against the float64 products, each at the tolerance the
    corresponding test of tests/test_conv_gpu.py uses.
Shapes: the smallest at which a budget binds on 256 CUs, next to a ragged one per family."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
BUDGETS = (64, 72, 240)
NAN = float("nan")


# ---------------------------------------------------------------------------------------------- the documented counts
def grid_blocks(unit, budget, n=256):
    """iif_persistent_grid_blocks: the largest whole number of units within the budget, unless that gives up more CUs than the
    reservation asked for - then the device's whole-unit grid."""
    b = budget if 0 < budget < n else n
    if unit <= 0:
        return b
    g = b // unit * unit
    return n // unit * unit if b - g > n - b else g


def regw_rows(m, mt, s, budget):
    """gemm1x1_regw_kernel with partial rows: tile sequences in eights, S blocks each; never more sequences than groups of eight
    tiles need, never more rows than ceil(M / 128)."""
    unit = 8 * s
    grid = min(grid_blocks(unit, budget), (m // mt + 7) // 8 * unit)
    rows128 = (m + 127) // 128
    if grid // s > rows128:
        grid = rows128 // 8 * unit
    return grid // s


def stream_rows(m, s, budget):
    """gemm1x1_stream_kernel: one row per tile sequence that has a tile."""
    mtiles = (m + 127) // 128
    grid = min(grid_blocks(8 * s, budget), (mtiles + 7) // 8 * 8 * s)
    return min(grid // s, mtiles)


def two_per_cu_rows(ntiles, m, budget):
    """conv3x3_regw64_kernel and stem4x4_kernel: two blocks per CU in whole groups of 8, one row per block."""
    b = budget if 0 < budget < 256 else 256
    grid = min(2 * b // 8 * 8, (ntiles + 7) // 8 * 8)
    rows128 = (m + 127) // 128
    if grid > rows128:
        grid = rows128 // 8 * 8
    return grid


def test_the_restated_rule_is_the_librarys():
    """The Python restatement above against iif_persistent_grid_blocks, and one literal per family (256 CUs)."""
    from iif_amd import _lib
    L = _lib.lib()
    try:
        L.iif_set_cu_budget(0)
        if L.iif_get_cu_budget() != 256:
            pytest.skip("the counts of this module are for 256 compute units")
        for b in (0,) + BUDGETS + (120, 200):
            L.iif_set_cu_budget(b)
            for unit in (8, 16, 32, 64, 128):
                assert L.iif_persistent_grid_blocks(unit) == grid_blocks(unit, b), (b, unit)
    finally:
        L.iif_set_cu_budget(0)
    assert regw_rows(8192, 64, 4, 240) == 56 and regw_rows(8192, 64, 4, 0) == 64      # 256 -> 1024 at 32 x 16 x 16: 224 blocks
    assert regw_rows(32768, 64, 1, 240) == 240 and regw_rows(4096, 32, 8, 64) == 8
    assert stream_rows(7056, 8, 64) == 8 and stream_rows(7840, 4, 240) == 56 and stream_rows(31360, 1, 0) == 245
    assert two_per_cu_rows(512, 32768, 64) == 128 and two_per_cu_rows(45, 2880, 0) == 16
    assert two_per_cu_rows(256, 32768, 72) == 144 and two_per_cu_rows(294, 37632, 240) == 288


# ---------------------------------------------------------------------------------------------- fixtures and helpers
@pytest.fixture
def cu_budget():
    """at(cus) sets the budget; budget 0 is restored whatever happens.  The module's counts are for 256 CUs."""
    from iif_amd import _lib
    L = _lib.lib()
    L.iif_set_cu_budget(0)
    if L.iif_get_cu_budget() != 256:
        pytest.skip("the counts of this module are for 256 compute units")

    def at(cus):
        _lib.check(L.iif_set_cu_budget(cus), "iif_set_cu_budget")
        assert L.iif_get_cu_budget() == (cus if cus else 256)
    try:
        yield at
    finally:
        L.iif_set_cu_budget(0)
        assert L.iif_get_cu_budget() == 256


@pytest.fixture
def conv_env(monkeypatch):
    """Set / unset convolution switches and make the library read them again (it caches them when it is loaded)."""
    from iif_amd import _lib

    def set_(**kv):
        for k, v in kv.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
        _lib.check(_lib.lib().iif_conv_reload_env(), "iif_conv_reload_env")
    yield set_
    monkeypatch.undo()
    _lib.lib().iif_conv_reload_env()


def nan_rows(m, c):
    return torch.full(((m + 127) // 128 + 8, 2, c), NAN, device=DEV)


def nan_like(shape):
    return torch.full(shape, NAN, dtype=BF, device=DEV)


def rows_ok(buf, count, expect, m, what):
    """Count as documented, <= ceil(M / 128); rows below it written, rows at and above it untouched."""
    assert count == expect, (what, count, expect)
    assert 0 < count <= (m + 127) // 128, (what, count)
    assert buf.shape[0] >= count + 8
    assert not torch.isnan(buf[:count]).any(), what
    assert torch.isnan(buf[count:]).all(), what


def stored_ok(t, base, ref, what):
    """No NaN, bit-identical to the budget-0 run, 2^-7 of the maximum from the float64 reference."""
    assert not torch.isnan(t).any(), what
    assert torch.equal(t, base), what
    assert (t.view(ref.shape).to(F64) - ref).abs().max().item() <= 2.0 ** -7 * ref.abs().max().item(), what


def unpack(bits, m, c):
    return ((bits.view(-1, 1).int() >> torch.arange(8, device=bits.device).view(1, 8)) & 1).view(m, c).to(F64)


def guard(counts, binds, what):
    """The budget was not ignored: where it binds, the count differs from the budget-0 count."""
    print("\n[%s] rows at budget 0 / 64 / 72 / 240: %s" % (what, " / ".join(str(counts[b]) for b in (0,) + BUDGETS)))
    for b in binds:
        assert counts[b] != counts[0], (what, b, counts)


def conv_f64(xp, w):
    """Stride-1 convolution in float64 as one GEMM over unfolded patches: xp [n, c, h, w] (already padded), w [o, c, kh, kw];
    returns NHWC."""
    n, c, h, wd = xp.shape
    o, _, kh, kw = w.shape
    cols = F.unfold(xp, (kh, kw))                                     # [n, c kh kw, L]
    return (w.reshape(o, -1) @ cols).view(n, o, h - kh + 1, wd - kw + 1).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------- gemm1x1_regw_kernel: forward + sums
# (n, hw, K, N, S, rows per tile, budgets that bind).  The plain forward has no 64 -> 256 instance (that shape runs with
# epilogue operands or in the never-stored passes, below), so its two 64 -> 256 shapes run as 128 -> 512 here; (32, 16, 128 -> 512)
# takes 64 columns per wave, one slice, and ceil(M / 128) bounds it at every budget; (32, 16, 256 -> 512) and
# (32, 16, 256 -> 1024) are the shapes at which units of 16 and 32 bind - the latter gets 224 blocks of 256 at budget 240.
REGW_FWD = [(32, 32, 128, 512, 1, 64, (64, 72, 240)), (5, 24, 128, 512, 1, 64, ()), (32, 16, 128, 512, 1, 64, ()),
            (32, 16, 256, 512, 2, 64, (64, 72)), (32, 16, 256, 1024, 4, 64, (64, 72, 240)), (64, 8, 256, 1024, 4, 64, (64, 72)),
            (64, 8, 512, 2048, 8, 32, (64, 72))]


@pytest.mark.parametrize("case", REGW_FWD, ids=lambda c: "%dx%dx%d_%d_%d" % (c[0], c[1], c[1], c[2], c[3]))
def test_regw1x1_forward_with_sums_under_a_budget(case, cu_budget):
    """conv_forward_bnstats on the register-weight kernel: stored output, row count and canaries, sums of the rows against the
    float64 sums of the stored output at 1e-6 (test_forward_1x1_weights_in_registers_equals_the_tile_kernel)."""
    from iif_amd import ops
    n, hw, k, c, s, mt, binds = case
    m = n * hw * hw
    g = torch.Generator().manual_seed(k + c + n)
    x = torch.randn(n, hw, hw, k, generator=g).bfloat16().to(DEV)
    wt = (torch.randn(c, k, generator=g) / k ** 0.5).bfloat16().to(DEV)
    ref = x.view(m, k).to(F64) @ wt.to(F64).t()
    runs, counts = {}, {}
    for b in (0,) + BUDGETS:
        cu_budget(b)
        out, partial = nan_like((n, hw, hw, c)), nan_rows(m, c)
        counts[b] = ops.conv_forward_bnstats(x, wt, 1, 1, 1, 0, out, partial.view(-1))
        runs[b] = (out, partial)
    cu_budget(0)
    guard(counts, binds, "regw forward %s" % (case[:4],))
    for b in (0,) + BUDGETS:
        out, partial = runs[b]
        rows_ok(partial, counts[b], regw_rows(m, mt, s, b), m, (case, b))
        stored_ok(out, runs[0][0], ref, (case, b))
        flat = out.view(m, c).to(F64)
        sums = torch.stack([flat.sum(0), (flat * flat).sum(0)])
        ps = partial[:counts[b]].to(F64).sum(0)
        assert (ps - sums).abs().max().item() <= 1e-6 * sums.abs().max().item(), (case, b)


# ------------------------------------------------------------------------- the never-stored forward
@pytest.mark.parametrize("case", [(32, 32, 64, 256, 1, (64, 72, 240)), (32, 16, 128, 512, 2, (64, 72))],
                         ids=lambda c: "%dx%dx%d_%d_%d" % (c[0], c[1], c[1], c[2], c[3]))
def test_never_stored_forward_under_a_budget(case, cu_budget):
    """conv_forward_stats_acc (rows of the unrounded accumulators: 1e-5 of sum |y| / sum y^2 against the float64 product, as
    test_never_stored_forward_on_the_register_weight_kernel) and conv_forward_bn_relu2, bit-identical under every budget to
    the convolution followed by bn_apply (plain residual, normalised residual, none) - whose own values are checked against
    float64."""
    from iif_amd import ops
    n, hw, k, c, s, binds = case
    m = n * hw * hw
    assert ops.conv_fwdbn_ok(n, hw, hw, k, c, BF)
    g = torch.Generator().manual_seed(13 * k + hw)
    x = torch.relu(torch.randn(n, hw, hw, k, generator=g)).to(BF).to(DEV)
    w = (torch.randn(c, k, generator=g) / k ** 0.5).to(BF).to(DEV)
    res = torch.randn(n, hw, hw, c, generator=g).to(BF).to(DEV)
    yd = x.view(m, k).to(F64) @ w.to(F64).t()
    s_ref, q_ref, a_ref_sum = yd.sum(0), (yd * yd).sum(0), yd.abs().sum(0)
    stats2 = torch.zeros(4, c, device=DEV)
    stats2[2] = torch.rand(c, generator=g).to(DEV) + 0.5
    stats2[3] = torch.randn(c, generator=g).to(DEV) * 0.2
    gamma, beta = torch.rand(c, generator=g).to(DEV) + 0.5, torch.randn(c, generator=g).to(DEV) * 0.1
    stats = torch.zeros(4, c, device=DEV)
    counts, base = {}, {}
    for b in (0,) + BUDGETS:
        cu_budget(b)
        p = nan_rows(m, c)
        counts[b] = ops.conv_forward_stats_acc(x, w, p.view(-1))
        rows_ok(p, counts[b], regw_rows(m, 64, s, b), m, (case, b))
        ps = p[:counts[b]].to(F64).sum(0)
        assert ((ps[0] - s_ref).abs() <= 1e-5 * a_ref_sum + 1e-6).all(), (case, b)
        assert ((ps[1] - q_ref).abs() <= 1e-5 * q_ref + 1e-6).all(), (case, b)
        if b == 0:
            ops.bn_finalize_stats(p.view(-1), counts[0], m, c, gamma, beta, torch.zeros(c, device=DEV), torch.ones(c, device=DEV),
                                  stats, 1e-5, 0.1)
        y = ops.conv_forward(x, w, 1, 1, 1, 0)
        assert (y.view(m, c).to(F64) - yd).abs().max().item() <= 2.0 ** -7 * yd.abs().max().item()
        a_ref = torch.empty_like(y)
        bits_ref = torch.zeros(m * c // 8, dtype=torch.uint8, device=DEV)
        for i, (r_, rs_) in enumerate(((res, None), (res, stats2), (None, None))):
            ops.bn_apply(y.view(m, c), stats, a_ref.view(m, c), relu=True, residual=None if r_ is None else r_.view(m, c),
                         residual_stats=rs_, relu_bits=bits_ref)
            a_two = nan_like(tuple(y.shape))
            bits_two = torch.full_like(bits_ref, 0xAA)
            ops.conv_forward_bn_relu2(x, w, a_two, stats, bits_two, res=r_, res_stats=rs_)
            assert torch.equal(a_two, a_ref) and torch.equal(bits_two, bits_ref), (case, b, i)
            if b == 0:
                base[i] = (a_two, bits_two)
            assert torch.equal(a_two, base[i][0]) and torch.equal(bits_two, base[i][1]), (case, b, i)
    cu_budget(0)
    guard(counts, binds, "never-stored %s" % (case[:4],))


# ------------------------------------------------------------------------- the BN + ReLU prologue
@pytest.mark.parametrize("stats_only", [False, True], ids=["stored", "stats_only"])
def test_prologue_under_a_budget(stats_only, cu_budget):
    """conv_forward_bnstats_pro at 32 x 16 x 16, 256 -> 1024 (four slices, units of 32: 64 / 16 / 16 / 56 sequences): the
    activation and its bits equal bn_apply's, the output the budget-0 run's and float64's, the partial rows AND the act_csum
    rows counted and canaried; act_csum sums at 1e-5 of sum |a| (test_bn_relu_prologue_in_the_convolution_operand_path)."""
    from iif_amd import ops
    n, hw, c, C = 32, 16, 256, 1024
    m = n * hw * hw
    assert ops.conv_pro_ok(n, hw, hw, c, C, BF, stats_only)
    g = torch.Generator().manual_seed(17 * c + hw)
    x_raw = torch.randn(n, hw, hw, c, generator=g).to(BF).to(DEV)
    w = (torch.randn(C, c, generator=g) / c ** 0.5).to(BF).to(DEV)
    st = torch.zeros(4, c)
    st[2] = torch.rand(c, generator=g) + 0.5
    st[3] = torch.randn(c, generator=g) * 0.3
    st = st.to(DEV)
    a_ref = torch.empty_like(x_raw)
    bits_ref = torch.zeros(m * c // 8, dtype=torch.uint8, device=DEV)
    ops.bn_apply(x_raw.view(m, c), st, a_ref.view(m, c), relu=True, relu_bits=bits_ref)
    ad = a_ref.view(m, c).to(F64)
    yd = ad @ w.to(F64).t()
    counts, base = {}, None
    for b in (0,) + BUDGETS:
        cu_budget(b)
        p, csum = nan_rows(m, C), nan_rows(m, c)
        act, bits = nan_like(tuple(x_raw.shape)), torch.full_like(bits_ref, 0x55)
        y = None if stats_only else nan_like((n, hw, hw, C))
        counts[b] = nt = ops.conv_forward_bnstats_pro(x_raw, st, act, bits, w, y, p.view(-1), act_csum=csum)
        expect = regw_rows(m, 64, 4, b)
        rows_ok(p, nt, expect, m, ("rows", b))
        rows_ok(csum, nt, expect, m, ("act_csum", b))
        assert torch.equal(act, a_ref) and torch.equal(bits, bits_ref), b
        ps = p[:nt].to(F64).sum(0)
        if stats_only:
            assert ((ps[0] - yd.sum(0)).abs() <= 1e-5 * yd.abs().sum(0) + 1e-6).all(), b
            assert ((ps[1] - (yd * yd).sum(0)).abs() <= 1e-5 * (yd * yd).sum(0) + 1e-6).all(), b
        else:
            base = y if b == 0 else base
            stored_ok(y, base, yd, b)
            flat = y.view(m, C).to(F64)
            sums = torch.stack([flat.sum(0), (flat * flat).sum(0)])
            assert (ps - sums).abs().max().item() <= 1e-6 * sums.abs().max().item(), b
        assert (csum[:nt, 1] == 0).all()
        assert ((csum[:nt, 0].to(F64).sum(0) - ad.sum(0)).abs() <= 1e-5 * ad.abs().sum(0) + 1e-6).all(), b
    cu_budget(0)
    guard(counts, BUDGETS, "prologue stats_only=%s" % stats_only)
    assert counts[240] == 56 and counts[0] == 64


# ------------------------------------------------------------------------- data gradient with masked store + sums
# (8, 32, k128, ..): 128 tiles, but ceil(M / 128) = 64 rows bound the grid at every budget: its counts do not move
@pytest.mark.parametrize("case", [(32, 32, 64, 256, 64, (64, 72, 240)), (8, 32, 128, 256, 64, ())],
                         ids=lambda c: "%dx%dx%d_k%d_n%d_c%d" % (c[0], c[1], c[1], c[2], c[3], c[4]))
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
def test_dgrad_masksum_family_under_a_budget(case, with_res, cu_budget):
    """conv_dgrad_masksum (upstream output read), conv_dgrad_masksum_rx (recomputed) and conv_dgrad_masksum_rx_pg (P / Gram slabs):
    one stored tensor, one set of rows (bit-identical among the three at one budget), ns slabs = the sequence count and the
    slabs behind them untouched.  Sums of the rows against float64 of the stored tensor at 1e-5 of the column's absolute sum
    (test_conv3x3_64_channels_weights_in_registers); iif_slab_sum of the slabs against the float64 products at 2e-5
    (test_recomputing_producer_leaves_the_algebra_matrices_behind)."""
    from iif_amd import ops
    n, hw, k, C, c2, binds = case
    m = n * hw * hw
    assert ops.conv_dgrad_rx_pg_ok(n, hw, hw, k, C, c2, BF)
    g = torch.Generator().manual_seed(11 * k + c2 + hw)
    a2 = torch.relu(torch.randn(n, hw, hw, c2, generator=g)).to(BF).to(DEV)
    w3 = (torch.randn(C, c2, generator=g) / c2 ** 0.5).to(BF).to(DEV)
    dy = torch.randn(n, hw, hw, k, generator=g).to(BF).to(DEV)
    wt = (torch.randn(C, k, generator=g) / k ** 0.5).to(BF).to(DEV)
    ubits = torch.randint(0, 256, (m * C // 8,), dtype=torch.uint8, generator=g).to(DEV)
    res = torch.randn(n, hw, hw, C, generator=g).to(BF).to(DEV) if with_res else None
    rbits = torch.randint(0, 256, (m * C // 8,), dtype=torch.uint8, generator=g).to(DEV) if with_res else None
    stats = torch.zeros(4, C)
    stats[0] = torch.randn(C, generator=g) * 0.1
    stats[1] = torch.rand(C, generator=g) + 0.5
    stats = stats.to(DEV)
    y3 = ops.conv_forward(a2, w3, 1, 1, 1, 0)                          # what the forward pass would have stored
    ref = dy.view(m, k).to(F64) @ wt.to(F64).t()
    if with_res:
        ref = ref + res.view(m, C).to(F64) * unpack(rbits, m, C)
    ref = ref * unpack(ubits, m, C)
    xhat = (y3.view(m, C).to(F64) - stats[0].to(F64)) * stats[1].to(F64)
    a2d = a2.view(m, c2).to(F64)
    ref_g = a2d.t() @ a2d
    ld = c2
    counts, base = {}, None
    for b in (0,) + BUDGETS:
        cu_budget(b)
        expect = regw_rows(m, 64, 1, b)
        o1, o2, o3 = (nan_like((n, hw, hw, C)) for _ in range(3))
        p1, p2, p3 = (nan_rows(m, C) for _ in range(3))
        slabs = torch.full(((m + 127) // 128 + 8, C + c2, ld), NAN, device=DEV)
        nt1 = ops.conv_dgrad_masksum(dy, wt, (hw, hw), o1, ubits, p1.view(-1), res=res, res_bits=rbits, up_x=y3, up_stats=stats)
        nt2 = ops.conv_dgrad_masksum_rx(dy, wt, (hw, hw), o2, ubits, p2.view(-1), a2, w3, stats, res=res, res_bits=rbits)
        nt3, ns = ops.conv_dgrad_masksum_rx_pg(dy, wt, (hw, hw), o3, ubits, p3.view(-1), a2, w3, stats, slabs.view(-1), ld,
                                               res=res, res_bits=rbits)
        counts[b] = nt1
        for p_, nt_, what in ((p1, nt1, "masksum"), (p2, nt2, "rx"), (p3, nt3, "rx_pg")):
            rows_ok(p_, nt_, expect, m, (what, case, b))
        rows_ok(slabs, ns, expect, m, ("slabs", case, b))
        assert torch.equal(p1[:nt1], p2[:nt2]) and torch.equal(p1[:nt1], p3[:nt3]), (case, b)
        base = o1 if b == 0 else base
        for o_ in (o1, o2, o3):
            stored_ok(o_, base, ref, (case, b))
        gs = o1.view(m, C).to(F64)
        ps = p1[:nt1].to(F64).sum(0)
        assert (ps[0] - gs.sum(0)).abs().max().item() <= 1e-5 * gs.abs().sum(0).max().item(), (case, b)
        assert (ps[1] - (gs * xhat).sum(0)).abs().max().item() <= 1e-5 * (gs * xhat).abs().sum(0).max().item(), (case, b)
        ext = torch.full((C + c2, ld), NAN, device=DEV)
        ops.slab_sum(slabs.view(-1), ns, C + c2, ld, c2, ext)
        got = ext.to(F64)
        assert (got[:C] - gs.t() @ a2d).abs().max().item() <= 2e-5 * (gs.abs().t() @ a2d).max().item(), (case, b)
        assert (got[C:] - ref_g).abs().max().item() <= 2e-5 * ref_g.max().item(), (case, b)
    cu_budget(0)
    guard(counts, binds, "dgrad masksum %s" % (case[:5],))


# ------------------------------------------------------------------------- conv3x3_regw64_kernel
@pytest.mark.parametrize("n,hw,binds", [(32, 32, (64, 72)), (5, 24, ()), (65, 8, ())], ids=["32x32x32", "5x24x24", "65x8x8"])
def test_regw3x3_under_a_budget(n, hw, binds, cu_budget):
    """3 x 3 over 64 -> 64 channels, two blocks per CU: forward + sums (1e-6), data gradient + upstream BN-backward sums (1e-5) as
    test_conv3x3_64_channels_weights_in_registers, and the affine epilogue of the inference forward (routed to this kernel:
    iif_conv_affine_route), bit-identical to the convolution followed by bn_apply under every budget.  (32, 32): 512 tiles, 256
    rows at budget 0 and 240 (ceil(M / 128) bounds them), 128 at 64, 144 at 72; (5, 24): 45 tiles over 16 blocks; (65, 8): 65
    tiles in per-XCD ranges of nine over 32 blocks, four per XCD - the last XCD has two tiles, so two of its blocks are idle and
    must still write a zero row (the stem's (3, 112, 112) has one such block at budget 0 and 240)."""
    from iif_amd import ops
    c = 64
    m = n * hw * hw
    g = torch.Generator().manual_seed(n * 100 + hw)
    x = torch.randn(n, hw, hw, c, generator=g).bfloat16().to(DEV)
    w = (torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5).bfloat16()
    wk = w.permute(0, 2, 3, 1).reshape(c, 9 * c).contiguous().to(DEV)                   # [cout][r][s][cin]
    wt = w.permute(1, 2, 3, 0).reshape(c, 9 * c).contiguous().to(DEV)                   # [cin][r][s][cout]: the data gradient's operand
    upx = torch.randn(n, hw, hw, c, generator=g).bfloat16().to(DEV)
    bits = torch.randint(0, 256, (m * c // 8,), dtype=torch.uint8, generator=g).to(DEV)
    res = torch.randn(n, hw, hw, c, generator=g).bfloat16().to(DEV)
    stats = torch.zeros(4, c)
    stats[0] = torch.randn(c, generator=g) * 0.1
    stats[1] = torch.rand(c, generator=g) + 0.5
    stats[2] = torch.rand(c, generator=g) + 0.5
    stats[3] = torch.randn(c, generator=g) * 0.2
    stats = stats.to(DEV)
    assert ops.conv_affine_route(n, hw, hw, c, hw, hw, c, 3, 3, 1, 1, 9 * c, has_res=True, has_relu_bits=True) == "regw3x3"
    xp = F.pad(x.to(F64).permute(0, 3, 1, 2), (1, 1, 1, 1))
    wd = w.to(DEV).to(F64)
    ref = conv_f64(xp, wd)
    refd = conv_f64(xp, wd.transpose(0, 1).flip(2, 3))                  # conv_transpose2d(x, w, padding=1)
    mask = unpack(bits, m, c)
    xhat = (upx.view(m, c).to(F64) - stats[0].to(F64)) * stats[1].to(F64)
    counts, base = {}, None
    for b in (0,) + BUDGETS:
        cu_budget(b)
        expect = two_per_cu_rows(n * (hw // 8) ** 2, m, b)
        out, dx, aff = (nan_like((n, hw, hw, c)) for _ in range(3))
        p1, p2 = nan_rows(m, c), nan_rows(m, c)
        counts[b] = nt = ops.conv_forward_bnstats(x, wk, 3, 3, 1, 1, out, p1.view(-1))
        nt2 = ops.conv_dgrad_bnbwd(x, wt, 3, 3, 1, 1, (hw, hw), dx, upx, bits, stats, p2.view(-1))
        abits = torch.full((m * c // 8,), 0xAA, dtype=torch.uint8, device=DEV)
        ops.conv_forward_affine(x, wk, 3, 3, 1, 1, aff, stats, res=res, relu_bits=abits)
        rows_ok(p1, nt, expect, m, ("forward", n, hw, b))
        rows_ok(p2, nt2, expect, m, ("dgrad", n, hw, b))
        base = (out, dx, aff, abits) if b == 0 else base
        stored_ok(out, base[0], ref, ("forward", n, hw, b))
        stored_ok(dx, base[1], refd, ("dgrad", n, hw, b))
        a_ref = torch.empty_like(out)
        bits_ref = torch.zeros_like(abits)
        ops.bn_apply(out.view(m, c), stats, a_ref.view(m, c), relu=True, residual=res.view(m, c), relu_bits=bits_ref)
        assert not torch.isnan(aff).any()
        assert torch.equal(aff, a_ref) and torch.equal(abits, bits_ref), (n, hw, b)
        assert torch.equal(aff, base[2]) and torch.equal(abits, base[3]), (n, hw, b)
        flat = out.view(m, c).to(F64)
        ps = p1[:nt].to(F64).sum(0)
        assert (ps[0] - flat.sum(0)).abs().max().item() <= 1e-6 * flat.abs().sum(0).max().item(), (n, hw, b)
        assert (ps[1] - (flat * flat).sum(0)).abs().max().item() <= 1e-6 * (flat * flat).sum(0).max().item(), (n, hw, b)
        gq = dx.view(m, c).to(F64) * mask
        ps2 = p2[:nt2].to(F64).sum(0)
        assert (ps2[0] - gq.sum(0)).abs().max().item() <= 1e-5 * gq.abs().sum(0).max().item(), (n, hw, b)
        assert (ps2[1] - (gq * xhat).sum(0)).abs().max().item() <= 1e-5 * (gq * xhat).abs().sum(0).max().item(), (n, hw, b)
    cu_budget(0)
    guard(counts, binds, "regw3x3 %dx%dx%d" % (n, hw, hw))


# ------------------------------------------------------------------------- stem4x4_kernel
# (3, 16, 16) has six tiles: with statistics the stem kernel needs eight rows' worth and leaves it to the general kernel, so the
# ragged case is (3, 112, 112): 294 tiles over 288 / 128 / 144 / 288 blocks
@pytest.mark.parametrize("n,h,w,binds", [(8, 64, 64, (64, 72)), (3, 112, 112, (64, 72))], ids=["8x64x64", "3x112x112"])
def test_stem4x4_under_a_budget(n, h, w, binds, cu_budget):
    """The space-to-depth stem (4 x 4, 16 -> 64 channels) with statistics: stored output, rows, sums at the bounds of
    test_stem_s2d_forward_window_kernel."""
    from iif_amd import ops
    m = n * h * w
    g = torch.Generator().manual_seed(n * 1000 + w)
    x = torch.randn(n, h, w, 16, generator=g).bfloat16().to(DEV)
    wt = (torch.randn(64, 256, generator=g) * 0.1).bfloat16().to(DEV)
    xp = F.pad(x.to(F64).permute(0, 3, 1, 2), (2, 1, 2, 1))
    ref = conv_f64(xp, wt.to(F64).view(64, 4, 4, 16).permute(0, 3, 1, 2))
    counts, base = {}, None
    for b in (0,) + BUDGETS:
        cu_budget(b)
        out, partial = nan_like((n, h, w, 64)), nan_rows(m, 64)
        counts[b] = nt = ops.conv_forward_bnstats(x, wt, 4, 4, 1, 2, out, partial)
        rows_ok(partial, nt, two_per_cu_rows(m // 128, m, b), m, (n, h, w, b))
        base = out if b == 0 else base
        stored_ok(out, base, ref, (n, h, w, b))
        flat = out.view(m, 64).to(F64)
        s1, s2 = flat.sum(0), (flat * flat).sum(0)
        ps = partial[:nt].to(F64).sum(0)
        assert (ps[0] - s1).abs().max().item() <= 1e-5 * max(1.0, flat.abs().sum(0).max().item()), (n, h, w, b)
        assert (ps[1] - s2).abs().max().item() <= 1e-5 * s2.max().item(), (n, h, w, b)
    cu_budget(0)
    guard(counts, binds, "stem %dx%dx%d" % (n, h, w))


# ------------------------------------------------------------------------- gemm1x1_stream_kernel
# (n, hw, cin, cout, slices of the forward's plan, slices of the data gradient's plan, binding budgets); None: the direction has
# no resident plan (K = 128, K > 256) and is not run.  (9, 28, 256 -> 1024) stands in for (9, 28, 128 -> 512), which has no plan:
# eight slices, and budget 64 is a grid of exactly one unit; (10, 28, 512 -> 256) is the data gradient with four slices,
# units of 32: 62 / 16 / 16 / 56 rows.
STREAM = [(40, 28, 64, 256, 1, 1, (64, 72, 240)), (9, 28, 256, 1024, 8, None, (64, 72)), (37, 28, 256, 64, 1, 1, (64, 72)),
          (10, 28, 512, 256, None, 4, (64, 72, 240))]


@pytest.mark.parametrize("case", STREAM, ids=lambda c: "%dx%dx%d_%d_to_%d" % (c[0], c[1], c[1], c[2], c[3]))
def test_stream1x1_under_a_budget(case, cu_budget, conv_env):
    """The streaming 1x1 kernel forced onto every shape it has a plan for, register-weight kernels off: forward + sums, data
    gradient with a masked residual, with the upstream sums, with both.  min(sequences, tiles) rows; the sums at the bounds
    of test_stream1x1_forward_stats_and_dgrad_epilogues."""
    from iif_amd import ops
    n, hw, cin, cout, s_fwd, s_dg, binds = case
    m = n * hw * hw
    conv_env(IIF_CONV_STREAM1X1_FORCE="1", IIF_CONV_NO_STREAM1X1=None, IIF_CONV_NO_REGW="1")
    g = torch.Generator().manual_seed(n * 1000 + cin + cout)
    x = torch.randn(n, hw, hw, cin, generator=g).to(BF).to(DEV)
    wt = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(BF).to(DEV)
    wd = wt.to(F64)
    if s_fwd is not None:
        ref = x.view(m, cin).to(F64) @ wd.t()
        counts, base = {}, None
        for b in (0,) + BUDGETS:
            cu_budget(b)
            out, partial = nan_like((n, hw, hw, cout)), nan_rows(m, cout)
            counts[b] = nt = ops.conv_forward_bnstats(x, wt, 1, 1, 1, 0, out, partial.view(-1))
            rows_ok(partial, nt, stream_rows(m, s_fwd, b), m, ("forward", case, b))
            base = out if b == 0 else base
            stored_ok(out, base, ref, ("forward", case, b))
            flat = out.view(m, cout).to(F64)
            s1, s2 = flat.sum(0), (flat * flat).sum(0)
            ps = partial[:nt].to(F64).sum(0)
            assert (ps[0] - s1).abs().max().item() <= 2e-6 * max(1.0, s1.abs().max().item()) * 8, (case, b)
            assert (ps[1] - s2).abs().max().item() <= 2e-5 * s2.abs().max().item(), (case, b)
        cu_budget(0)
        guard(counts, binds, "stream forward %s" % (case[:4],))
    if s_dg is None:
        return
    dy = torch.randn(n, hw, hw, cout, generator=g).to(BF).to(DEV)
    res = torch.randn(n, hw, hw, cin, generator=g).to(BF).to(DEV)
    upx = torch.randn(n, hw, hw, cin, generator=g).to(BF).to(DEV)
    rbits = torch.randint(0, 256, (m * cin // 8,), dtype=torch.uint8, generator=g).to(DEV)
    bits, bits2 = (torch.randint(0, 256, (m * cin // 8,), dtype=torch.uint8, generator=g).to(DEV) for _ in range(2))
    stats = torch.zeros(4, cin)
    stats[0] = torch.randn(cin, generator=g) * 0.1
    stats[1] = torch.rand(cin, generator=g) + 0.5
    stats = stats.to(DEV)
    wtt = torch.zeros(cin, (cout + 15) // 16 * 16, dtype=BF, device=DEV)
    ops.weight_transpose(wt.float(), cout, cin, 1, wtt)
    ref_plain = dy.view(m, cout).to(F64) @ wd
    ref_res = ref_plain + res.view(m, cin).to(F64) * unpack(rbits, m, cin)
    xhat = (upx.view(m, cin).to(F64) - stats[0].to(F64)) * stats[1].to(F64)
    counts, base = {}, None
    for b in (0,) + BUDGETS:
        cu_budget(b)
        expect = stream_rows(m, s_dg, b)
        dx = ops.conv_dgrad(dy, wtt, 1, 1, 1, 0, (hw, hw), res=res, res_bits=rbits)
        out2, out3 = nan_like((n, hw, hw, cin)), nan_like((n, hw, hw, cin))
        p2, p3 = nan_rows(m, cin), nan_rows(m, cin)
        counts[b] = nt2 = ops.conv_dgrad_bnbwd(dy, wtt, 1, 1, 1, 0, (hw, hw), out2, upx, bits, stats, p2.view(-1))
        nt3 = ops.conv_dgrad_bnbwd(dy, wtt, 1, 1, 1, 0, (hw, hw), out3, upx, bits2, stats, p3.view(-1), res=res, res_bits=rbits)
        rows_ok(p2, nt2, expect, m, ("dgrad + sums", case, b))
        rows_ok(p3, nt3, expect, m, ("dgrad + residual + sums", case, b))
        base = (dx, out2, out3) if b == 0 else base
        stored_ok(dx, base[0], ref_res, ("dgrad + residual", case, b))
        stored_ok(out2, base[1], ref_plain, ("dgrad + sums", case, b))
        stored_ok(out3, base[2], ref_res, ("dgrad + residual + sums", case, b))
        for o_, p_, nt_, bt in ((out2, p2, nt2, bits), (out3, p3, nt3, bits2)):
            gq = o_.view(m, cin).to(F64) * unpack(bt, m, cin)
            t1, t2 = gq.sum(0), (gq * xhat).sum(0)
            ps = p_[:nt_].to(F64).sum(0)
            assert (ps[0] - t1).abs().max().item() <= 2e-6 * max(1.0, t1.abs().max().item()) * 8, (case, b)
            assert (ps[1] - t2).abs().max().item() <= 2e-6 * max(1.0, t2.abs().max().item()) * 8, (case, b)
    cu_budget(0)
    guard(counts, binds, "stream dgrad %s" % (case[:4],))
