"""The conv3 route of every block of a training step, decided on the host alone (resnet_engine._train_routes).

The table below was recorded from the commit BEFORE the routes became one record per block, where they were spread over eight
containers of _Plan (alg3_units, twopass_units, rx_units, nostore_units, pro_units, pg_units, ds_alg, _alg_rows) and two
run-time predicates.  How: for every case and switch set a _Plan of that commit was constructed (no step run) and, per block,
the route its step would take was read off the containers exactly as its forward / backward did:
    backward  standard unless the closing unit was in alg3_units; then rx if in rx_units, else pure if its "is pure" predicate said so, else producer
    forward   nostore if in nostore_units and alg3_units, else twopass if in twopass_units, else stored
    prologue  an entry in pro_units whose instance kind matched the forward route (and the fused backward on); csum_rows: with rows
    gram      producer if in pg_units, else stacked if its "Gram stacked" predicate said so, else ahead (None outside alg3_units)
    ds_algebra  the block's shortcut unit had an entry in ds_alg
STREAMS_OFF: plans built without a device (CPU tensors; the two largest shapes on the meta device), which have no side streams.
STREAMS_ON: the same plans built on an MI355X with IIF_SIDE_STREAMS=1 (weight-gradient stream everywhere, shortcut stream where the
network has convolutional shortcuts and computes in bf16); the function is asked with wg_stream=True, ds_stream=True.
The byte counts of bench.streaming_pass_bytes are that commit's too."""
import functools
import os

import pytest
import torch

from iif_amd import _lib, resnet_engine
from iif_amd.resnet_engine import _Route, _train_routes
from tests.test_fused_eval_host import _net

BF, F32 = torch.bfloat16, torch.float32
# the four networks of test_conv_select_host.NETS, ResNet-50 at the shapes of the GPU tests, and once with fp32 compute
CASES = [("resnet50", 256, 224, BF), ("resnet50", 64, 224, BF), ("resnext101_32x4d", 128, 224, BF), ("resnet32", 128, 32, BF),
         ("resnet50", 32, 64, BF), ("resnet50", 32, 128, BF), ("resnet50", 32, 224, BF), ("resnet50", 32, 64, F32)]
P0 = {"IIF_BN3_ALGEBRA_PURE_MIN_ELEMS": "0"}
SWITCHES = [{}, {"IIF_NO_RX": "1"}, P0, dict(P0, IIF_NO_RX="1"), {"IIF_NO_NOSTORE": "1"}, {"IIF_NO_NOSTORE": "1", "IIF_NO_RX": "1"},
            dict(P0, IIF_TWOPASS="1"), dict(P0, IIF_TWOPASS="1", IIF_NO_RX="1"), {"IIF_NO_PROLOGUE": "1"}, {"IIF_PRO_MAX_K": "512"},
            {"IIF_NO_PG": "1"}, {"IIF_NO_GRAM_STACKED": "1"}, {"IIF_NO_DS_ALGEBRA": "1"}, {"IIF_NO_BN3_ALGEBRA": "1"},
            {"IIF_NO_BWD_FUSE": "1"}]
ALL_SWITCHES = sorted({k for s in SWITCHES for k in s})

# One block per token, in forward order ("*k": k blocks alike); five letters: backward (S standard, P pure, D producer, X rx),
# forward (s stored, t twopass, n nostore), prologue (- none, p prologue, c prologue that leaves the column sums),
# Gram matrix (- no algebra, a ahead, k stacked, g producer), shortcut algebra (- / d).
BACKWARD = {"S": "standard", "P": "pure", "D": "producer", "X": "rx"}
FORWARD = {"s": "stored", "t": "twopass", "n": "nostore"}
GRAM = {"-": None, "a": "ahead", "k": "stacked", "g": "producer"}
TABLES = [
    "Xnca-*7 Dsca-*6 Ss---*3",
    "Pnca-*7 Dsca-*6 Ss---*3",
    "Xnca-*7 Pnca-*6 Ss---*3",
    "Pnca-*13 Ss---*3",
    "Xs-a-*7 Dsca-*6 Ss---*3",
    "Ps-a-*7 Dsca-*6 Ss---*3",
    "Xnca- Xt-a-*2 Xnca- Xt-a-*3 Pnca- Pt-a-*5 Ss---*3",
    "Pnca- Pt-a-*2 Pnca- Pt-a-*3 Pnca- Pt-a-*5 Ss---*3",
    "Xn-a-*7 Ds-a-*6 Ss---*3",
    "Xnca-*7 Dsca-*6 Ssp--*3",
    "Ss---*7 Ssp--*6 Ss---*3",
    "Ss---*16",
    "Ds-a-*7 Dsca-*6 Ss---*3",
    "Xnca-*2 Pnca- Dsca-*4 Ss---*26",
    "Pnca-*3 Dsca-*4 Ss---*26",
    "Xnca-*2 Pnca-*5 Ss---*26",
    "Pnca-*7 Ss---*26",
    "Xs-a-*2 Ps-a- Dsca-*4 Ss---*26",
    "Ps-a-*3 Dsca-*4 Ss---*26",
    "Xnca- Xt-a- Pt-a- Pnca- Pt-a-*3 Ss---*26",
    "Pnca- Pt-a-*2 Pnca- Pt-a-*3 Ss---*26",
    "Xn-a-*2 Pn-a- Ds-a-*4 Ss---*26",
    "Xnca-*2 Pnca- Dsca-*4 Ssp--*23 Ss---*3",
    "Ss---*3 Ssp--*4 Ss---*26",
    "Ss---*33",
    "Ss---*15",
    "Xnca-*7 Ds-a-*6 Ss---*3",
    "Ds-a-*13 Ss---*3",
    "Xnca-*7 Ps-a-*6 Ss---*3",
    "Pnca-*7 Ps-a-*6 Ss---*3",
    "Xs-a-*7 Ds-a-*6 Ss---*3",
    "Xnca- Xt-a-*2 Xnca- Xt-a-*3 Ps-a- Pt-a-*5 Ss---*3",
    "Pnca- Pt-a-*2 Pnca- Pt-a-*3 Ps-a- Pt-a-*5 Ss---*3",
    "Xncgd Xncg-*2 Xnck-*4 Dsck-*6 Ss---*3",
    "Pncad Pnca-*6 Dsck-*6 Ss---*3",
    "Xncgd Xncg-*2 Xnck-*4 Pnca-*6 Ss---*3",
    "Pncad Pnca-*12 Ss---*3",
    "Xs-gd Xs-g-*2 Xs-k-*4 Dsck-*6 Ss---*3",
    "Ps-ad Ps-a-*6 Dsck-*6 Ss---*3",
    "Xncgd Xt-g-*2 Xnck- Xt-k-*3 Pnca- Pt-a-*5 Ss---*3",
    "Pncad Pt-a-*2 Pnca- Pt-a-*3 Pnca- Pt-a-*5 Ss---*3",
    "Xn-gd Xn-g-*2 Xn-k-*4 Ds-k-*6 Ss---*3",
    "Xncgd Xncg-*2 Xnck-*4 Dsck-*6 Ssp--*3",
    "Xnckd Xnck-*6 Dsck-*6 Ss---*3",
    "Xncad Xnca-*6 Dsca-*6 Ss---*3",
    "Xncg-*3 Xnck-*4 Dsck-*6 Ss---*3",
    "Ds-kd Ds-k-*6 Dsck-*6 Ss---*3",
    "Xnckd Xnck- Pnca- Dsck-*4 Ss---*26",
    "Pncad Pnca-*2 Dsck-*4 Ss---*26",
    "Xnckd Xnck- Pnca-*5 Ss---*26",
    "Pncad Pnca-*6 Ss---*26",
    "Xs-kd Xs-k- Ps-a- Dsck-*4 Ss---*26",
    "Ps-ad Ps-a-*2 Dsck-*4 Ss---*26",
    "Xnckd Xt-k- Pt-a- Pnca- Pt-a-*3 Ss---*26",
    "Pncad Pt-a-*2 Pnca- Pt-a-*3 Ss---*26",
    "Xn-kd Xn-k- Pn-a- Ds-k-*4 Ss---*26",
    "Xnckd Xnck- Pnca- Dsck-*4 Ssp--*23 Ss---*3",
    "Xncad Xnca- Pnca- Dsca-*4 Ss---*26",
    "Xnck-*2 Pnca- Dsck-*4 Ss---*26",
    "Xncgd Xncg-*2 Xnck-*4 Ds-k-*6 Ss---*3",
    "Ds-kd Ds-k-*12 Ss---*3",
    "Xncgd Xncg-*2 Xnck-*4 Ps-a-*6 Ss---*3",
    "Pncad Pnca-*6 Ps-a-*6 Ss---*3",
    "Xs-gd Xs-g-*2 Xs-k-*4 Ds-k-*6 Ss---*3",
    "Xncgd Xt-g-*2 Xnck- Xt-k-*3 Ps-a- Pt-a-*5 Ss---*3",
    "Pncad Pt-a-*2 Pnca- Pt-a-*3 Ps-a- Pt-a-*5 Ss---*3",
    "Xnckd Xnck-*6 Ds-k-*6 Ss---*3",
    "Xncad Xnca-*6 Ds-a-*6 Ss---*3",
    "Xncg-*3 Xnck-*4 Ds-k-*6 Ss---*3",
]
STREAMS_OFF = [
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 0, 0, 10, 11],
    [0, 12, 2, 3, 4, 12, 6, 7, 8, 9, 0, 0, 0, 10, 11],
    [13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 13, 13, 13, 23, 24],
    [25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25],
    [26, 27, 28, 29, 30, 27, 31, 32, 8, 26, 26, 26, 26, 11, 11],
    [0, 12, 2, 3, 4, 12, 6, 7, 8, 0, 0, 0, 0, 10, 11],
    [0, 12, 2, 3, 4, 12, 6, 7, 8, 9, 0, 0, 0, 10, 11],
    [11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11],
]
STREAMS_ON = [
    [33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 10, 11],
    [33, 46, 35, 36, 37, 46, 39, 40, 41, 42, 43, 44, 45, 10, 11],
    [47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 47, 57, 58, 23, 24],
    [25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25],
    [59, 60, 61, 62, 63, 60, 64, 65, 41, 59, 66, 67, 68, 11, 11],
    [33, 46, 35, 36, 37, 46, 39, 40, 41, 33, 43, 44, 45, 10, 11],
    [33, 46, 35, 36, 37, 46, 39, 40, 41, 42, 43, 44, 45, 10, 11],
    [11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11],
]
# STREAMS_OFF / STREAMS_ON [case][switch set] -> index into TABLES
BENCH_BYTES = {(256, 224): 16574331588.0, (32, 64): 680008644.0}        # bench.streaming_pass_bytes of ResNet-50, 1000 classes


def _decode(table):
    rows = []
    for tok in table.split(" "):
        code, _, k = tok.partition("*")
        b, f, p, g, d = code
        rows += [_Route(BACKWARD[b], FORWARD[f], p != "-", p == "c", GRAM[g], d == "d")] * int(k or 1)
    return rows


@functools.lru_cache(maxsize=None)
def _case_net(arch, dt):
    return _net(arch, dt)


def _block_names(net):
    names = {id(m): n for n, m in net.named_modules()}
    return [names[id(blk)] for st in net._stages for blk in st]


@pytest.fixture
def switches(monkeypatch):
    """Set exactly one switch set (whatever the caller's environment holds) and make the library read its own again."""
    def set_(sw):
        for k in ALL_SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in sw.items():
            monkeypatch.setenv(k, v)
        _lib.check(_lib.lib().iif_conv_reload_env(), "iif_conv_reload_env")
    set_({})
    yield set_
    monkeypatch.undo()
    _lib.lib().iif_conv_reload_env()


def _table(net, n, hw, dt, streams):
    return [(name,) + tuple(r) for name, r in _train_routes(net, n, hw, hw, dt, streams, streams)]


@pytest.mark.parametrize("streams", [False, True], ids=["streams_off", "streams_on"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=["%s-%dx%d-%s" % (a, n, hw, str(dt)[6:]) for a, n, hw, dt in CASES])
def test_routes_are_those_of_the_parent_commit(ci, streams, switches):
    arch, n, hw, dt = CASES[ci]
    net = _case_net(arch, dt)
    names = _block_names(net)
    for si, sw in enumerate(SWITCHES):
        switches(sw)
        want = [(name,) + tuple(r) for name, r in zip(names, _decode(TABLES[(STREAMS_ON if streams else STREAMS_OFF)[ci][si]]))]
        got = _table(net, n, hw, dt, streams)
        assert len(got) == len(names) and got == want, (sw, [(g, e) for g, e in zip(got, want) if g != e])


# Recorded from the parent in the same way: ResNet-50 at 32 x 224 x 224 with the DMA range lowered (bytes; no streams), default
# switches / IIF_BN3_ALGEBRA_PURE_MIN_ELEMS=0:
# the operand-size conditions, which the parent asked of the plan's tensors and the function asks of element counts
DMA_LIMITED = {40000000: ("Ss---*3 Xnca-*4 Dsca-*6 Ss---*3", "Ss---*3 Xnca-*4 Pnca-*6 Ss---*3"),
               20000000: ("Ss---*7 Dsca-*6 Ss---*3", "Ss---*7 Pnca-*6 Ss---*3"),
               10000000: ("Ss---*7 Ssp--*6 Ss---*3", "Ss---*7 Ssp--*6 Ss---*3"),
               3000000: ("Ss---*16", "Ss---*16")}


@pytest.mark.parametrize("limit", sorted(DMA_LIMITED))
def test_routes_inside_a_lowered_dma_range(limit, switches, monkeypatch):
    monkeypatch.setattr(resnet_engine, "_DMA_LIMIT", limit)
    net = _case_net("resnet50", BF)
    for sw, table in zip(({}, P0), DMA_LIMITED[limit]):
        switches(sw)
        assert [r for _, r in _train_routes(net, 32, 224, 224, BF, False, False)] == _decode(table), sw


def test_the_table_walks_every_route():
    """Not a table of one answer: every value of every field is recorded somewhere, the two-pass forward in front of a recomputing
    producer included (decided on the size alone: the order-dependent case of the eight containers, now said in the open)."""
    rows = [r for t in TABLES for r in _decode(t)]
    assert {r.backward for r in rows} == set(BACKWARD.values()) and {r.forward for r in rows} == set(FORWARD.values())
    assert {r.gram for r in rows} == set(GRAM.values()) and {r.ds_algebra for r in rows} == {False, True}
    assert {(r.prologue, r.csum_rows) for r in rows} == {(False, False), (True, False), (True, True)}
    assert any(r.backward == "rx" and r.forward == "twopass" for r in rows)
    assert all((r.backward == "standard") == (r.gram is None) for r in rows)
    assert all(r.forward == "stored" or r.backward != "standard" for r in rows)      # a never-stored output is never read by a BN backward


def test_the_route_function_is_pure(switches):
    arch, n, hw, dt = CASES[4]
    net = _case_net(arch, dt)
    env = dict(os.environ)
    first = _table(net, n, hw, dt, True)
    assert _table(net, n, hw, dt, True) == first
    other = resnet_engine._Plan(net, 8, 96, 96)                        # a plan of another shape in between (CPU tensors)
    assert [r for _, r in _train_routes(net, 8, 96, 96, dt, False, False)] == [other._route(b["units"][-1]) for b in other.blocks]
    assert _table(net, n, hw, dt, True) == first and dict(os.environ) == env
    assert "fused" in other._eval_routing().values()                  # (the inference routing of the plan is a table of its own)
    switches({"IIF_NO_BN3_ALGEBRA": "1"})                              # and it reads the switches when it is called
    assert _table(net, n, hw, dt, True) != first


@pytest.mark.parametrize("n,hw,ci", [(256, 224, 0), (32, 64, 4)])
def test_views_and_byte_model_as_on_the_parent(n, hw, ci, switches):
    """What bench.py reads of a plan - alg3_units, nostore_units, pro_units[u3] = (conv2 unit, rows or None) - are views of the
    records, equal to the parent's sets at the two benchmark shapes; its byte count is the parent's number."""
    import bench
    from iif_amd import resnet_pytorch
    net = resnet_pytorch.resnet50(num_classes=1000, device="cpu", compute_dtype=BF, pretrained="None")
    if n * hw * hw > 64 * 128 * 128:
        net._device = torch.device("meta")                             # (nothing is computed: the plan's tensors need no memory)
    assert bench.streaming_pass_bytes(net, n, hw)[0] == BENCH_BYTES[(n, hw)]
    plan = net._plan(n, hw, hw)
    want = dict(zip(_block_names(net), _decode(TABLES[STREAMS_OFF[ci][0]])))
    names = {id(m): k for k, m in net.named_modules()}
    block = lambda u: names[id(u.conv)].rsplit(".", 1)[0]              # noqa: E731
    assert all(names[id(u.conv)].endswith(".conv3") for u in plan.alg3_units)
    assert sorted(block(u) for u in plan.alg3_units) == sorted(k for k, r in want.items() if r.backward != "standard")
    assert sorted(block(u) for u in plan.rx_units) == sorted(k for k, r in want.items() if r.backward == "rx")
    assert sorted(block(u) for u in plan.nostore_units) == sorted(k for k, r in want.items() if r.forward == "nostore")
    assert not plan.twopass_units and not plan.pg_units
    pro = plan.pro_units
    assert [block(u) for u in pro] == [k for k, r in want.items() if r.prologue]
    for u3, (u2, rows) in pro.items():
        assert names[id(u2.conv)] == block(u3) + ".conv2" and (rows is not None) == want[block(u3)].csum_rows
    # 13 algebra units, 7 of them on the never-stored forward behind the recomputing producer: the benchmark's mix
    assert (len(plan.alg3_units), len(plan.rx_units), len(plan.nostore_units)) == (13, 7, 7)
    for view in ("alg3_units", "rx_units", "twopass_units", "nostore_units", "pg_units", "pro_units"):
        with pytest.raises(AttributeError):
            setattr(plan, view, set())
    # the one supported way to the standard routes on a live plan: the prologue stays where its instance stores conv3's output
    plan.standard_routes = True
    for b in plan.blocks:
        u = b["units"][-1]
        r = want[block(u)]
        keep = r.prologue and r.forward != "nostore"
        assert plan._route(u) == _Route(prologue=keep, csum_rows=keep and r.csum_rows)
    plan.standard_routes = False
    assert [plan._route(b["units"][-1]) for b in plan.blocks] == list(want.values())
