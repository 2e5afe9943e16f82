"""The compute-unit budget of the persistent grids on the host: how iif_set_cu_budget rounds, how many blocks a whole-unit grid
gets under a budget (iif_persistent_grid_blocks) and that the planning queries do not depend on it.  No device: the library
assumes 256 CUs without one, and every table here is for 256.  Every test leaves budget 0 behind."""
import pytest

from iif_amd import _lib
from tests.test_conv_select_host import RECORDED, _answers

IIF_EINVAL = -1


@pytest.fixture
def budget():
    """Set a budget through the C ABI; budget 0 (the whole device) is restored whatever the test does."""
    L = _lib.lib()
    if L.iif_get_cu_budget() != 256:
        L.iif_set_cu_budget(0)
    assert L.iif_get_cu_budget() == 256, "these tables are for 256 compute units"

    def set_(cus):
        return L.iif_set_cu_budget(cus)
    try:
        yield set_
    finally:
        L.iif_set_cu_budget(0)
        assert L.iif_get_cu_budget() == 256


def test_set_cu_budget_rounds_as_the_header_states(budget):
    """Rounded down to a multiple of 8, at least 64, at most the device; 0 = the whole device; a negative value is refused and
    changes nothing."""
    L = _lib.lib()
    asked = [0, 1, 7, 64, 71, 72, 100, 240, 255, 256, 300]
    expect = [256, 64, 64, 64, 64, 72, 96, 240, 248, 256, 256]
    got = []
    for cus in asked:
        assert budget(cus) == 0, cus
        got.append(L.iif_get_cu_budget())
    assert got == expect
    for before in (0, 72, 240):
        assert budget(before) == 0
        was = L.iif_get_cu_budget()
        assert budget(-1) == IIF_EINVAL and budget(-240) == IIF_EINVAL
        assert L.iif_get_cu_budget() == was


# budget -> {unit: blocks}, by hand from the rule in include/iif_amd.h (n = 256): g = b / unit * unit, kept unless b - g > n - b
GRID_BLOCKS = {
    0:   {8: 256, 16: 256, 32: 256, 64: 256, 128: 256},
    64:  {8: 64,  16: 64,  32: 64,  64: 64,  128: 0},        # 128: gives up 64 <= 192
    72:  {8: 72,  16: 64,  32: 64,  64: 64,  128: 0},        # 128: gives up 72 <= 184
    120: {8: 120, 16: 112, 32: 96,  64: 64,  128: 0},        # 64: 56 <= 136; 128: 120 <= 136
    128: {8: 128, 16: 128, 32: 128, 64: 128, 128: 128},
    200: {8: 200, 16: 192, 32: 192, 64: 192, 128: 256},      # 128: g = 128 gives up 72 > 56
    240: {8: 240, 16: 240, 32: 224, 64: 256, 128: 256},      # 32: 16 <= 16; 64: 48 > 16; 128: 112 > 16
}


def test_persistent_grid_blocks_follow_the_documented_rule(budget):
    """iif_persistent_grid_blocks(unit) over units 8 .. 128 and seven budgets against GRID_BLOCKS.  Before the rule was
    corrected (it compared what the DEVICE's whole-unit grid loses, full - g, with the reservation, which for 256 CUs ignores
    every budget that is not a whole number of units) the entries (240, 32), (72, 16), (120, 16) and (200, 32) failed: 256
    blocks each instead of 224, 64, 112 and 192 - and with them every other entry whose budget is not a multiple of its unit,
    (64, 128) -> 0 included."""
    L = _lib.lib()
    wrong = []
    for b, row in GRID_BLOCKS.items():
        assert budget(b) == 0
        for unit, blocks in row.items():
            got = L.iif_persistent_grid_blocks(unit)
            if got != blocks:
                wrong.append(((b, unit), got, blocks))
    assert not wrong, wrong
    assert budget(240) == 0
    assert L.iif_persistent_grid_blocks(0) == 240 and L.iif_persistent_grid_blocks(-8) == 240      # unit <= 0: the budget itself


# one 56 x 56, one 28 x 28 and one 14 x 14 row of the recorded table: the expanding 1x1 layers, which say yes to the never-stored
# forward, the prologue and (as data gradients) to the recomputing producer and its P / Gram form
QUERY_ROWS = [(256, 56, 56, 64, 56, 56, 256, 1, 1, 1, 0, 64, 1, 1), (256, 28, 28, 128, 28, 28, 512, 1, 1, 1, 0, 128, 1, 1),
              (256, 14, 14, 256, 14, 14, 1024, 1, 1, 1, 0, 256, 1, 1)]


@pytest.mark.parametrize("cus", [64, 240])
def test_planning_queries_do_not_depend_on_the_budget(cus, budget):
    """iif_conv_fwdbn_ok, iif_conv_pro_ok, iif_conv_dgrad_rx_ok and iif_conv_dgrad_rx_pg_ok (and the other queries of the recorded
    table) answer under a budget what they answer without one: the engine plans its routes once, at budget 0, and launches them
    under the reducer's budget."""
    L = _lib.lib()
    free = {row: _answers(row) for row in QUERY_ROWS}
    assert budget(cus) == 0 and L.iif_get_cu_budget() == cus
    for row in QUERY_ROWS:
        got = _answers(row)
        assert got == free[row] == RECORDED[row], (row, got, free[row], RECORDED[row])
        assert "1" in got[:3] and "1" in got[8:], (row, got)            # not a row of refusals
