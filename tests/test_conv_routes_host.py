"""Which kernel every launch of the convolution entry takes, asked of the launch-free query iif_conv_route (ops.conv_route): no
test here needs a device; without one the library sizes persistent grids for 256 compute units, the MI355X's count.

  * every GPU case of test_conv_routes_gpu.py takes the launches it is pinned to (family, columns per tile, partial rows), and
    the sizes next to the 256-row tile's conditions leave it;
  * the census - every layer of the networks of test_conv_select_host.NETS, forward and as data gradient, with every operand
    set of conv_route_cases - answers as recorded (CENSUS);
  * every kernel / direction / operand-set triple of that census names an existing test that checks it against a reference
    (COVERAGE);
  * the 256-row tile carries the launches of ResNet50 at batch 256 that the GPU cases stand for, and none at batch 64."""
import ctypes

import pytest
import torch

from iif_amd import _lib, ops
from tests import conv_route_cases as C


@pytest.fixture(scope="module")
def census():
    return C.census_rows()


@pytest.mark.parametrize("case", C.GPU_CASES + C.CENSUS_CASES, ids=lambda c: c.id)
def test_gpu_cases_take_the_launches_they_are_pinned_to(case):
    ans = C.route(C.case_desc(case), C.operands_of(case.direction, case.opset), case.cs2)
    assert isinstance(ans, list), (case.id, ans)
    assert tuple((f, i) for f, i, _ in ans) == case.launches, (case.id, ans)
    assert sum(r for _, _, r in ans) == case.rows, (case.id, ans)


def test_tile256_launch_geometry():
    """The pinned launches in full: 512 threads, one block per tile in whole groups of 8 pixel tiles, one partial row per 256
    pixels - ceil(M / 256), not ceil(M / 128)."""
    for case in C.GPU_CASES:
        desc = C.case_desc(case)
        for l in ops.conv_route(*desc, operands=C.operands_of(case.direction, case.opset), cs2=case.cs2):
            if l.family != "tile256":
                continue
            assert (l.inst, l.block, l.grid_y) == (128, 512, 1), case.id
            assert l.ntiles == (desc[6] + 127) // 128 and l.grid == (l.mtiles + 7) // 8 * 8 * l.ntiles, (case.id, l)
            assert l.mtiles * l.ntiles >= 384, (case.id, l)
            if l.cls < 0:
                assert l.mtiles == (desc[0] * desc[4] * desc[5] + 255) // 256, (case.id, l)
            assert l.rows in (0, l.mtiles), (case.id, l)
    # the class-by-class stride-2 data gradient: parity classes 0 .. 3 in order, 98 + 49 + 49 + 48 rows
    case = next(c for c in C.GPU_CASES if len(c.launches) == 4)
    ls = ops.conv_route(*C.case_desc(case), operands=C.operands_of(case.direction, case.opset))
    assert [l.cls for l in ls] == [0, 1, 2, 3] and [l.rows for l in ls] == [98, 49, 49, 48]


@pytest.mark.parametrize("why,direction,opset,layer,family", C.NOT_TILE256, ids=[c[0] for c in C.NOT_TILE256])
def test_sizes_next_to_the_pins_leave_the_256_row_tile(why, direction, opset, layer, family):
    case = C.Case(why, direction, opset, layer, 0, (), 0)
    ans = C.route(C.case_desc(case), C.operands_of(direction, opset))
    assert isinstance(ans, list) and [f for f, _, _ in ans] == [family], (why, ans)


def test_query_arguments_and_refusals():
    L = _lib.lib()
    d = _lib.ConvDesc(1, 1, 5889, 1024, 1, 5889, 2048, 1, 1, 1, 0, 0, 1024, _lib.IIF_BF16, _lib.IIF_BF16, 1, None, 0)
    out = (ctypes.c_int32 * 9)()
    assert L.iif_conv_route(None, 0, 0, ctypes.addressof(out), 9) == -1
    assert L.iif_conv_route(ctypes.byref(d), 0, 0, None, 9) == -1
    assert L.iif_conv_route(ctypes.byref(d), 0, 0, None, 0) == 1                       # only the count
    assert L.iif_conv_route(ctypes.byref(d), 0, 0, ctypes.addressof(out), 9) == 1 and out[0] == ops.CONV_ROUTES.index("tile256")
    assert L.iif_conv_route(ctypes.byref(d), ops.CONV_OPERANDS["src2"], 0, ctypes.addressof(out), 9) == -1       # no cs2
    # what the entry refuses, the query refuses with the same code: a gated store on a forward, a second source on a 3x3,
    # the residual's ReLU bits on a stride-2 data gradient, fp32 partial rows
    assert C.route((1, 1, 5889, 1024, 1, 5889, 2048, 1, 1, 1, 0, 0, 1024), ("partial", "gated_store")) == -1
    assert C.route((2, 14, 14, 128, 14, 14, 128, 3, 3, 1, 1, 1, 1152 + 64), ("src2",), 64) == -2
    assert C.route((2, 7, 7, 128, 14, 14, 128, 3, 3, 2, 1, 1, 1152), ("res", "res_bits")) == -2
    with pytest.raises(_lib.IIFNativeError):
        ops.conv_route(2, 14, 14, 128, 14, 14, 128, 1, 1, 1, 0, 0, 128, operands=("partial",), dtype=torch.float32)
    # the register-weight forms behind their own entries: never-stored statistics, the prologue, the recomputed upstream x
    fam = lambda desc, o, cs2=0: [f for f, _, _ in C.route(desc, o, cs2)]              # noqa: E731
    assert fam((4, 16, 16, 64, 16, 16, 256, 1, 1, 1, 0, 0, 64), ("partial", "no_store_acc")) == ["regw1x1"]
    assert fam((4, 16, 16, 64, 16, 16, 256, 1, 1, 1, 0, 0, 64), ("partial", "prologue", "no_store_acc")) == ["regw1x1"]
    assert C.route((4, 16, 16, 64, 16, 16, 256, 1, 1, 1, 0, 0, 64), ("partial", "prologue")) == -2      # (no storing form at K = 64)
    assert fam((4, 16, 16, 64, 16, 16, 256, 1, 1, 1, 0, 1, 64), ("partial", "up_bits", "up_stats", "gated_store", "rx"), 64) == ["regw1x1"]
    assert ops.conv_dgrad_rx_ok(4, 16, 16, 64, 256, 64, torch.bfloat16) and ops.conv_pro_ok(4, 16, 16, 64, 256, torch.bfloat16, True)
    assert not ops.conv_pro_ok(4, 16, 16, 64, 256, torch.bfloat16, False)


def test_census_answers_as_recorded(census):
    table = C.census_table(census)
    assert list(table) == list(C.CENSUS) and len(table) > 60, (len(table), len(C.CENSUS))
    wrong = [(k, table[k], C.CENSUS[k]) for k in table if table[k] != C.CENSUS[k]]
    assert not wrong, wrong[:5]


def test_every_census_key_names_a_test_that_checks_it(census):
    keys = C.census_keys(census)
    assert len(keys) > 90
    missing = [k for k in keys if k not in C.COVERAGE]
    assert not missing, missing
    unresolved = [(k, C.COVERAGE[k]) for k in keys if C.resolve(C.COVERAGE[k]) is None]
    assert not unresolved, unresolved
    # (and the map names nothing the census does not have: a stale entry would claim a kernel that no layer takes)
    assert sorted(C.COVERAGE) == keys


def test_tile256_reach(census):
    """The fact the 256-row cases rest on: at batch 256 ResNet50 runs these launches on the 256-row tile, at batch 64 none."""
    at = lambda geo, d, o: census[(geo, 1, d, o)]                                        # noqa: E731
    s2_128, s2_256 = (256, 56, 56, 128, 28, 28, 128, 3, 3, 2, 1, 1152), (256, 28, 28, 256, 14, 14, 256, 3, 3, 2, 1, 2304)
    shortcut = (256, 14, 14, 1024, 7, 7, 2048, 1, 1, 2, 0, 1024)
    conv3 = (256, 14, 14, 256, 14, 14, 1024, 1, 1, 1, 0, 256)
    for geo in (s2_128, s2_256, shortcut):
        assert at(geo, "fwd", "stats") == "tile256:128", geo
    for o in ("dst_acc", "masked_res", "up_sums", "up_sums_masked_res", "gated"):         # the conv3 data gradient from 1024 channels
        assert at(conv3, "dgrad", o) == "tile256:128", o
    for o in C.DGRAD2_SETS:                                                                # ... and on the BN3-algebra route
        assert at(conv3, "dgrad2", o) == "tile256:128", o
    # the affine 1x1 1024 -> 256 of the fused evaluation forward
    assert ops.conv_affine_route(256, 14, 14, 1024, 14, 14, 256, 1, 1, 1, 0, 1024) == "tile256"
    assert ops.conv_affine_route(64, 14, 14, 1024, 14, 14, 256, 1, 1, 1, 0, 1024) == "tile_2stage"
    b64 = [(k, v) for k, v in census.items() if k[0][0] == 64 and "tile256" in v]
    assert not b64, b64
