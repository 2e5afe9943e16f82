"""The weight gradient's split-K decision as a value, on the host alone (iif_conv_wgrad_plan launches nothing).

  * the query equals the plain-Python restatement of the rule (tests/wgrad_cases.py, written from the documentation) over every
    convolution of the supported networks and each with one field broken, the stem, the stacked 1x1 and the Gram matrix, over
    requests {0, -2, -4, 1, 3, 33, 600} and workspaces {none, ample, k slabs, exactly the splits with no stage room};
  * the invariants of a round hold on every row;
  * the GPU cases of tests/test_wgrad_splits_gpu.py run the family they name and realise the split counts they claim, and
    every family covers every boundary of the slab sum;
  * the argument checks of the query and of iif_slab_sum."""
import ctypes

import pytest

from iif_amd import _lib
from tests import wgrad_cases as W
from tests.test_conv_select_host import _rows

SPLITS = (0, -2, -4, 1, 3, 33, 600)
AMPLE = 64 << 20


def query(row, cd2=0, workspace_bytes=0, splits=0):
    """The library's answer as wgrad_cases.Plan, or the status where it refuses."""
    n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, ldw, g, dt = row
    d = _lib.ConvDesc(n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, 0, ldw, dt, _lib.IIF_F32, g, None, 0)
    out = (ctypes.c_int32 * 10)()
    rc = _lib.lib().iif_conv_wgrad_plan(ctypes.byref(d), cd2, workspace_bytes, splits, ctypes.addressof(out))
    return W.Plan(W.FAMILIES[out[0]], *out[1:]) if rc == 0 else rc


def _grid_rows():
    """(row, cd2): the networks' convolutions as the weight gradient sees them (ldw >= r s cs holds for all of them), the stems
    at three sizes (the last does not fit the stem kernel's ring), stacked 1x1 launches and Gram matrices."""
    rows = [(row, 0) for row in _rows() if row[11] >= row[7] * row[8] * row[3] and row[11] % 4 == 0]
    for n, hw in ((256, 112), (3, 17), (1, 130)):
        rows.append(((n, hw, hw, 16, hw, hw, 64, 4, 4, 1, 2, 256, 1, W.BF16), 0))
    for n, hw, cs, cd1, cd2 in ((256, 56, 64, 256, 64), (64, 28, 128, 512, 128), (3, 55, 64, 128, 72), (2, 7, 64, 256, 8)):
        rows.append(((n, hw, hw, cs, hw, hw, cd1, 1, 1, 1, 0, cs, 1, W.BF16), cd2))
    for n, hw, c in ((256, 56, 64), (64, 28, 128), (3, 13, 256)):
        rows.append(((n, hw, hw, c, hw, hw, c, 1, 1, 1, 0, c, 1, W.BF16), -1))
    return rows


def _workspaces(row, cd2, splits):
    slab4 = W.slab_floats(row, cd2) * 4
    want = W.plan(row, cd2, 1 << 50, splits, regstage=False)
    want = want.splits if want else 1
    return (0, AMPLE, 5 * slab4, 2 * slab4 + 12, want * slab4, want * slab4 + slab4 - 4)


def test_query_equals_the_restated_rule_and_keeps_its_invariants(monkeypatch):
    monkeypatch.delenv("IIF_CONV_REGSTAGE", raising=False)
    rows = _grid_rows()
    assert len(rows) > 150
    checked, two_stage, cut = 0, 0, 0
    for row, cd2 in rows:
        slab4 = W.slab_floats(row, cd2) * 4
        auto = {}
        for splits in SPLITS:
            for wsb in _workspaces(row, cd2, splits):
                want, got = W.plan(row, cd2, wsb, splits, regstage=False), query(row, cd2, wsb, splits)
                assert want is not None and got == want, (row, cd2, wsb, splits, got, want)
                assert 1 <= got.splits <= got.nsteps
                assert (got.splits - 1) * got.steps_per_split < got.nsteps <= got.splits * got.steps_per_split
                if got.splits > 1:
                    assert got.splits * slab4 <= wsb and got.stages in (1, 2)
                else:
                    assert got.stages == 0
                if got.stages == 2:
                    assert got.splits > 32 and got.chunks == W.cdiv(got.splits, 16) and (got.splits + got.chunks) * slab4 <= wsb
                    two_stage += 1
                else:
                    assert got.chunks == 0
                if splits > 0:
                    assert got.splits <= splits
                cut += got.splits == wsb // slab4 and wsb > 0
                checked += 1
            auto[splits] = query(row, cd2, 1 << 50, splits).splits
        assert auto[-2] <= auto[0] and auto[-4] <= auto[-2], (row, auto)        # a share of the device never gets more splits
    assert checked > 6000 and two_stage > 100 and cut > 500, (checked, two_stage, cut)


def test_full_round_of_the_56x56_nine_tap_layer():
    """ResNet-50 at 256 x 224: the 56 x 56 nine-tap layer gets the full round, 2 blocks on each of 256 CUs = a grid of 512.
    Its 26 912 steps are dealt 53 to a split, which 508 splits exhaust: the other 4 blocks of the round are padding."""
    row = (256, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1, 576, 1, W.BF16)
    got = query(row, 0, 128 << 20, 0)
    assert got.family == "ninetap" and got.tiles == 1 and got.blocks == 512, got
    assert got.nsteps == 26912 and got.steps_per_split == W.cdiv(26912, 512) == 53 and got.splits == W.cdiv(26912, 53) == 508, got
    assert (got.stages, got.chunks) == (2, 32)
    half = query(row, 0, 128 << 20, -2)
    assert half.blocks == 256 and half.steps_per_split == W.cdiv(26912, 256), half


def test_register_staged_switch_is_read_per_call(monkeypatch):
    rows = [rc for rc in _grid_rows() if rc[1] == 0][::7]
    monkeypatch.setenv("IIF_CONV_REGSTAGE", "1")
    seen = set()
    for row, cd2 in rows:
        for splits in (0, 3, 33):
            want, got = W.plan(row, cd2, AMPLE, splits, regstage=True), query(row, cd2, AMPLE, splits)
            assert got == (want if want is not None else -2), (row, splits, got, want)
            seen.add(got.family if want else "refused")
    assert seen == {"regstage", "refused"}
    monkeypatch.delenv("IIF_CONV_REGSTAGE")
    assert query(rows[0][0], 0, AMPLE, 0).family != "regstage"


def test_operands_beyond_the_32_bit_offsets_take_the_register_staged_kernel():
    row = (4096, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1, 576, 1, W.F32)               # 3.3 GB of fp32 per operand
    assert query(row, 0, AMPLE, 0) == W.plan(row, 0, AMPLE, 0, regstage=False) and query(row, 0, AMPLE, 0).family == "regstage"
    row = (4096, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1, 576, 1, W.BF16)              # 1.6 GB of bf16: still the nine-tap kernel
    assert query(row, 0, AMPLE, 0).family == "ninetap"


# ---- the GPU cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_gpu_case_runs_its_family_and_realises_its_counts(case, monkeypatch):
    if case.family == "regstage":
        monkeypatch.setenv("IIF_CONV_REGSTAGE", "1")
    else:
        monkeypatch.delenv("IIF_CONV_REGSTAGE", raising=False)
    row = W.row_of(case)
    hd, wd = W.out_hw(case)
    assert 4 * case.n * hd * wd < 2 ** 24                           # every partial sum of {-2..2} products is an exact fp32
    reqs = W.requests(case)
    assert reqs
    for target, q in reqs.items():
        got = query(row, case.cd2, 1 << 40, q)
        assert got.family == case.family and got.splits == target, (case.name, target, q, got)
    pixels = {"ninetap": case.n * (hd + 2) * (wd + 2), "stem": case.n * (hd + 3) * (wd + 3)}.get(case.family, case.n * hd * wd)
    assert pixels % 32 != 0 or case.name == "nt_64_auto"            # a ragged last step (3 x 56 x 56 padded pixels are whole steps)


def test_every_family_covers_every_boundary_of_the_slab_sum(monkeypatch):
    for fam in W.FAMILIES:
        if fam == "regstage":
            monkeypatch.setenv("IIF_CONV_REGSTAGE", "1")
        else:
            monkeypatch.delenv("IIF_CONV_REGSTAGE", raising=False)
        seen, ragged, tiles = set(), False, set()
        for c in W.CASES:
            if c.family != fam:
                continue
            for target, q in W.requests(c).items():
                got = query(W.row_of(c), c.cd2, 1 << 40, q)
                seen.add(got.splits)
                ragged |= got.nsteps % got.steps_per_split != 0
                tiles.add((got.bc, got.bnw))
        assert set(W.TARGETS) <= seen and max(seen) >= W.MANY, (fam, sorted(seen))
        assert ragged, fam
        if fam in ("ninetap", "stem"):
            assert max(seen) >= W.FULL, (fam, max(seen))
        if fam == "1x1":
            assert tiles >= {(256, 128), (128, 128), (64, 128), (64, 64), (64, 256)}, tiles
        if fam == "dma":
            assert {t[0] for t in tiles} == {64, 128, 256}, tiles


# ---- argument checks ----------------------------------------------------------------------------------------------------
def test_plan_query_rejects_what_the_launch_rejects():
    L = _lib.lib()
    out = (ctypes.c_int32 * 10)()
    addr = ctypes.addressof(out)
    good = dict(n=2, hs=8, ws=8, cs=64, hd=8, wd=8, cd=64, r=3, s=3, stride=1, pad=1, transposed=0, ldw=576, dtype=W.BF16,
                dst_dtype=W.F32, groups=1)

    def rc(cd2=0, wsb=0, **kw):
        f = dict(good, **kw)
        d = _lib.ConvDesc(*[f[k] for k in ("n", "hs", "ws", "cs", "hd", "wd", "cd", "r", "s", "stride", "pad", "transposed", "ldw",
                                           "dtype", "dst_dtype", "groups")], None, 0)
        return L.iif_conv_wgrad_plan(ctypes.byref(d), cd2, wsb, 0, addr)
    assert rc() == 0
    assert L.iif_conv_wgrad_plan(None, 0, 0, 0, addr) == -1                       # no descriptor
    d = _lib.ConvDesc(*[good[k] for k in ("n", "hs", "ws", "cs", "hd", "wd", "cd", "r", "s", "stride", "pad", "transposed", "ldw",
                                          "dtype", "dst_dtype", "groups")], None, 0)
    assert L.iif_conv_wgrad_plan(ctypes.byref(d), 0, 0, 0, None) == -1            # nowhere to answer
    assert rc(dtype=7) == -1                                                      # neither fp32 nor bf16
    assert rc(ldw=578) == -2 and rc(ldw=572) == -2                                # pitch not in 4s; shorter than a row
    assert rc(n=0) == -1 and rc(wsb=-1) == -1 and rc(transposed=1) == -1
    assert rc(stride=3) == -2 and rc(cs=60) == -2 and rc(cd=60) == -2
    assert rc(cd2=-2) == -1
    assert rc(cd2=-1, cd=128) == -1                                               # x and dy of a Gram matrix are one tensor
    assert rc(cd2=8) == -2                                                        # stacked: 1x1 only
    one = dict(r=1, s=1, pad=0, ldw=64)
    assert rc(cd2=8, **dict(one, cd=128)) == 0
    assert rc(cd2=8, **one) == -2 and rc(cd2=4, **dict(one, cd=128)) == -2        # cd1 in 128s, cd2 in 8s
    assert rc(cd2=8, **dict(one, cd=128, dtype=W.F32)) == -2


def test_slab_sum_rejects_a_width_that_is_no_multiple_of_four():
    """The slab sum moves 4-float vectors and tests the first column of each against `cols`: with cols % 4 != 0 it would write
    up to three columns past it, so the entry refuses (include/iif_amd.h).  Host buffers stand in for device memory: the
    checks return before anything is launched."""
    L = _lib.lib()
    raw = (ctypes.c_float * 200)()
    addr = (ctypes.addressof(raw) + 15) // 16 * 16
    for cols in (1, 2, 3, 5, 6, 7):
        assert L.iif_slab_sum(addr, 64, 1, 4, 8, cols, addr + 512, None) == -1, cols
    assert L.iif_slab_sum(addr, 64, 1, 4, 8, 12, addr + 512, None) == -1          # wider than the pitch, as before
