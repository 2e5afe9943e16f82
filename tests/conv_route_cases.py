"""Cases of the convolution route tests (test_conv_routes_host.py asks the launch-free query iif_conv_route, test_conv_routes_gpu.py
runs the kernels): the launches pinned to the 256 x 128 tile, the census of which kernel every layer of the supported networks
takes with every operand set, and the map from each kernel / operand-set pair of that census to the test that checks it against a
reference.  Nothing here needs a device."""
import collections

from iif_amd import ops

# ---- operand sets (names of ops.CONV_OPERANDS), by direction -----------------------------------------------------------------
UP = ("partial", "up_x", "up_bits", "up_stats")
FWD_SETS = collections.OrderedDict([("plain", ()), ("stats", ("partial",))])
DGRAD_SETS = collections.OrderedDict([
    ("plain", ()), ("dst_acc", ("res", "res_is_dst")), ("masked_res", ("res", "res_bits")), ("up_sums", UP),
    ("up_sums_masked_res", UP + ("res", "res_bits")), ("gated", ("partial", "up_bits", "gated_store"))])
# the data gradient of a bottleneck's conv3 on the BN3-algebra route: K runs over [g~ | a2], with and without the upstream sums
DGRAD2_SETS = collections.OrderedDict([("two_source", ("src2", "src_bias")), ("two_source_sums", ("src2", "src_bias") + UP)])
# (GPU cases only)
EXTRA_SETS = {"residual": ("res",)}


def operands_of(direction, opset):
    return {"fwd": FWD_SETS, "dgrad": DGRAD_SETS, "dgrad2": DGRAD2_SETS}[direction].get(opset) or EXTRA_SETS.get(opset, ())


def route(desc, operands, cs2=0, groups=1):
    """[(family, inst, rows)] per launch of descriptor tuple (n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, transposed, ldw), or the
    status code of the refusal."""
    try:
        return [(l.family, l.inst, l.rows) for l in ops.conv_route(*desc, operands=operands, cs2=cs2, groups=groups)]
    except ops._lib.IIFNativeError as e:
        return -2 if "EUNSUPPORTED" in str(e) else -1


# ---- GPU cases ---------------------------------------------------------------------------------------------------------------
# id, direction, operand set, (n, h_in, w_in, c_in, c_out, k, stride) of the LAYER (forward: x [n, h_in, w_in, c_in] ->
# [n, h_out, w_out, c_out]; dgrad: dy on the output grid -> dx on the input grid; dgrad2: 1x1, c_in = channels of g~ (first
# source), cs2 those of a2, c_out the destination's), cs2, then what the query must answer: family and columns per tile of each
# launch, and the partial rows of the call (0: the operand set has none).
Case = collections.namedtuple("Case", "id direction opset layer cs2 launches rows")
T256, T2S = ("tile256", 128), ("tile_2stage", 128)


def _c(id_, direction, opset, layer, rows, cs2=0, launches=(T256,)):
    return Case(id_, direction, opset, layer, cs2, tuple(launches), rows)


W1 = (1, 1, 5889, 1024, 2048, 1, 1)                 # 24 x 16 tiles = 384, the last tile ONE row
GPU_CASES = [
    _c("fwd1x1-plain", "fwd", "plain", W1, 0),
    _c("fwd1x1-residual", "fwd", "residual", W1, 0),
    _c("fwd1x1-stats", "fwd", "stats", W1, 24),
    _c("fwd1x1s2-stats-in_shift", "fwd", "stats", (2, 109, 109, 1024, 2048, 1, 2), 24),         # M = 2 x 55 x 55 = 6050
    _c("fwd3x3s2-stats", "fwd", "stats", (3, 129, 129, 128, 1024, 3, 2), 50),                   # M = 3 x 65 x 65 = 12675, 50 x 8
    _c("fwd3x3-plain", "fwd", "plain", (2, 113, 113, 128, 512, 3, 1), 0),                       # M = 25538, 100 x 4 (no halo: W = 113)
    _c("dgrad3x3-up_sums", "dgrad", "up_sums", (2, 113, 113, 512, 128, 3, 1), 100),             # dy 128 -> dx 512
    _c("dgrad1x1-plain", "dgrad", "plain", (1, 1, 5889, 2048, 1024, 1, 1), 0),                  # dy 1024 -> dx 2048
    _c("dgrad1x1-dst_acc", "dgrad", "dst_acc", (1, 1, 5889, 2048, 1024, 1, 1), 0),
    _c("dgrad1x1-masked_res", "dgrad", "masked_res", (1, 1, 5889, 2048, 1024, 1, 1), 0),
    _c("dgrad1x1-up_sums", "dgrad", "up_sums", (1, 1, 5889, 2048, 1024, 1, 1), 24),
    _c("dgrad1x1-gated", "dgrad", "gated", (1, 1, 5889, 2048, 1024, 1, 1), 24),
    _c("dgrad2-sums", "dgrad2", "two_source_sums", (1, 1, 12033, 512, 1024, 1, 1), 48, cs2=512),          # 48 x 8
    _c("dgrad2-production", "dgrad2", "two_source", (1, 1, 48897, 1024, 256, 1, 1), 0, cs2=256),        # 192 x 2
    # stride-2 data gradient, class by class: class 0 (one tap, K = 512) on the two-stage tile, classes 1 - 3 here; the rows of
    # the four launches follow each other in one buffer (98 + 49 + 49 + 48)
    _c("dgrad3x3s2-up_sums-scatter", "dgrad", "up_sums", (2, 157, 157, 1024, 512, 3, 2), 244, launches=(T2S, T256, T256, T256)),
    # edges
    _c("fwd1x1-stats-tail255", "fwd", "stats", (1, 1, 6143, 1024, 2048, 1, 1), 24),
    _c("dgrad1x1-up_sums_masked_res-tail33", "dgrad", "up_sums_masked_res", (1, 1, 23 * 256 + 33, 2048, 1024, 1, 1), 24),
    _c("fwd1x1-stats-cd2056", "fwd", "stats", (1, 1, 5633, 1024, 2056, 1, 1), 23),              # 17 column tiles, the last 8 wide
    _c("fwd1x1-stats-cs1056", "fwd", "stats", (1, 1, 5889, 1056, 2048, 1, 1), 24),              # 33 K steps: not in threes
]


def case_desc(case):
    """Descriptor tuple of a GPU case, as ops.conv_route takes it."""
    n, h, w, cin, cout, k, stride = case.layer
    pad = k // 2
    ho, wo = ops.conv_out_hw(h, w, k, k, stride, pad)
    if case.direction == "fwd":
        return (n, h, w, cin, ho, wo, cout, k, k, stride, pad, 0, k * k * cin)
    if case.direction == "dgrad":
        return (n, ho, wo, cout, h, w, cin, k, k, stride, pad, 1, k * k * cout)
    return (n, h, w, cin, h, w, cout, 1, 1, 1, 0, 1, cin + case.cs2)


# Sizes next to the pinned ones that leave the 256-row tile: what the pins rest on (use_bm256 and the kernels tried before it)
NOT_TILE256 = [
    ("M % 32 == 0: register weights", "fwd", "plain", (1, 1, 5888, 1024, 2048, 1, 1), "regw1x1"),
    ("23 x 16 = 368 tiles", "fwd", "plain", (1, 1, 5889 - 256, 1024, 2048, 1, 1), "tile_2stage"),
    ("K = 992", "fwd", "plain", (1, 1, 5889, 992, 2048, 1, 1), "tile_2stage"),
    ("64 columns", "fwd", "plain", (1, 1, 384 * 256 - 1, 1024, 64, 1, 1), "tile_2stage"),
    ("3x3 / stride 1 at W = 28: the halo kernel", "fwd", "plain", (16, 28, 28, 128, 512, 3, 1), "halo"),
]


# ---- census ------------------------------------------------------------------------------------------------------------------
def census_layers():
    """(net index, layer name, forward geometry (n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, ldw), groups, is conv3 of a
    bottleneck) of every convolution after the stem of NETS (test_conv_select_host), the convolutional shortcuts included."""
    from tests.test_conv_select_host import NETS
    from tests.test_fused_eval_host import _conv_descs, _net
    out = []
    for ni, (arch, n, hw) in enumerate(NETS):
        net = _net(arch)
        descs = _conv_descs(net, n, hw, hw)
        bottleneck = any(name.endswith("conv3") for name, *_ in descs)
        by_block = collections.OrderedDict()
        for name, geo, g, _, _ in descs:
            out.append((ni, name, geo, g, bottleneck and name.endswith("conv3")))
            by_block.setdefault(name.rsplit(".", 1)[0], []).append(geo)
        for si, st in enumerate(net._stages):
            for bi, blk in enumerate(st):
                if blk.downsample is not None:
                    first, last = by_block["layer%d.%d" % (si + 1, bi)][0], by_block["layer%d.%d" % (si + 1, bi)][-1]
                    dcv = blk.downsample[0]
                    out.append((ni, "layer%d.%d.downsample" % (si + 1, bi),
                                (first[0], first[1], first[2], dcv.cin, last[4], last[5], dcv.cout, 1, 1, dcv.stride, 0, dcv.cin), 1, False))
    return out


def census_rows(layers=None):
    """{(geometry, groups, direction, operand set): "family:inst|..." or the refusal's code} - one launch per "|"."""
    rows = collections.OrderedDict()
    for _, _, geo, g, conv3 in layers or census_layers():
        n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, ldw = geo
        todo = [("fwd", k, v, (n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, 0, ldw), 0) for k, v in FWD_SETS.items()]
        todo += [("dgrad", k, v, (n, hd, wd, cd, hs, ws, cs, r, s, stride, pad, 1, r * s * cd), 0) for k, v in DGRAD_SETS.items()]
        if conv3:
            todo += [("dgrad2", k, v, (n, hd, wd, cd, hs, ws, cs, 1, 1, 1, 0, 1, cd + cs), cs) for k, v in DGRAD2_SETS.items()]
        for direction, opset, operands, desc, cs2 in todo:
            key = (geo, g, direction, opset)
            if key not in rows:
                ans = route(desc, operands, cs2, g)
                rows[key] = str(ans) if isinstance(ans, int) else "|".join("%s:%d" % (f, i) for f, i, _ in ans)
    return rows


def census_table(rows):
    """census_rows() in the form of CENSUS: {geometry + (groups,): (forward answers, data-gradient answers, two-source answers)},
    each a blank-separated string in the order of FWD_SETS / DGRAD_SETS / DGRAD2_SETS ("" where the layer is no conv3)."""
    tab = collections.OrderedDict()
    for (geo, g, direction, opset), v in rows.items():
        tab.setdefault(geo + (g,), {})[(direction, opset)] = v
    return collections.OrderedDict(
        (k, tuple(" ".join(a[(d, o)] for o in sets if (d, o) in a) for d, sets in (("fwd", FWD_SETS), ("dgrad", DGRAD_SETS), ("dgrad2", DGRAD2_SETS))))
        for k, a in tab.items())


def census_keys(rows):
    """The distinct "family:inst/direction/operand set" of the launches in census_rows() (refusals aside), sorted."""
    return sorted({"%s/%s/%s" % (part, d, o) for (_, _, d, o), v in rows.items() if not v.startswith("-") for part in v.split("|")})


# Smallest cases for the kernel / operand-set pairs of the census that no test outside test_conv_routes_gpu.py checks against a
# reference (COVERAGE below names them): a layer of the census at the smallest batch that keeps the kernel.
def _k(key, layer, rows=0, cs2=0):
    kern, direction, opset = key.split("/")
    family, inst = kern.split(":")
    return Case("census-" + key.replace("/", "-").replace(":", ""), direction, opset, layer, cs2, ((family, int(inst)),), rows)


H128, H256 = (63, 28, 28, 128, 128, 3, 1), (246, 7, 7, 512, 512, 3, 1)             # the halo kernel needs >= 192 tiles
T7, G16 = (1, 7, 7, 512, 512, 3, 1), (1, 32, 32, 16, 16, 3, 1)                     # K = 4608: three-stage tile; 16 channels: general taps
CENSUS_CASES = [
    _k("tile_2stage:64/dgrad/gated", (1, 56, 56, 64, 64, 1, 1), 25),
    _k("tile_2stage:64/dgrad2/two_source_sums", (1, 56, 56, 256, 64, 1, 1), 25, cs2=64),
    _k("tile_2stage:128/dgrad2/two_source_sums", (1, 14, 14, 1024, 256, 1, 1), 2, cs2=256),
    _k("tile:128/fwd/stats", T7, 1),
    _k("tile:128/dgrad/masked_res", T7),
    _k("tile:128/dgrad/up_sums", T7, 1),
    _k("tile:128/dgrad/up_sums_masked_res", T7, 1),
    _k("tile:128/dgrad2/two_source", (1, 7, 7, 2048, 512, 1, 1), cs2=512),
    _k("tile:128/dgrad2/two_source_sums", (1, 7, 7, 2048, 512, 1, 1), 1, cs2=512),
    _k("tile_general:64/dgrad/masked_res", G16),
    _k("tile_general:64/dgrad/up_sums", G16, 8),
    _k("tile_general:64/dgrad/up_sums_masked_res", G16, 8),
    _k("tile_mc:128/dgrad/dst_acc", (1, 28, 28, 256, 256, 3, 2)),
    _k("regw3x3:0/fwd/plain", (1, 8, 8, 64, 64, 3, 1)),
    _k("regw3x3:0/dgrad/plain", (1, 8, 8, 64, 64, 3, 1)),
    _k("stream1x1:256/fwd/plain", (42, 56, 56, 64, 256, 1, 1)),                     # >= 1024 tiles: 4 per persistent block
    _k("stream1x1:64/fwd/plain", (42, 56, 56, 256, 64, 1, 1)),
    _k("stream1x1:128/fwd/plain", (42, 56, 56, 256, 128, 1, 1)),
    _k("regw1x1:6/dgrad/up_sums_masked_res", (1, 56, 56, 256, 64, 1, 1), 24),
    _k("regw1x1:14/dgrad/plain", (1, 56, 56, 256, 128, 1, 1)),
    _k("regw1x1:7/dgrad/up_sums_masked_res", (1, 56, 56, 256, 128, 1, 1), 24),
    _k("regw1x1:17/dgrad/plain", (4, 28, 28, 128, 512, 1, 1)),
    _k("regw1x1:13/dgrad/plain", (4, 28, 28, 512, 128, 1, 1)),
    _k("regw1x1:15/dgrad/plain", (4, 28, 28, 512, 256, 1, 1)),
    _k("regw1x1:8/dgrad/up_sums_masked_res", (4, 28, 28, 512, 256, 1, 1), 24),
    _k("regw1x1:18/dgrad/plain", (8, 14, 14, 256, 1024, 1, 1)),
    _k("regw1x1:16/dgrad/plain", (8, 14, 14, 1024, 512, 1, 1)),
    _k("regw1x1:9/dgrad/up_sums", (8, 14, 14, 1024, 512, 1, 1), 8),
    _k("regw1x1:9/dgrad/up_sums_masked_res", (8, 14, 14, 1024, 512, 1, 1), 8),
    _k("halo:128/fwd/plain", H128),
    _k("halo:128/dgrad/plain", H128),
    _k("halo:128/dgrad/dst_acc", H128),
    _k("halo:128/dgrad/masked_res", H128),
    _k("halo:128/dgrad/up_sums", H128, 386),
    _k("halo:128/dgrad/up_sums_masked_res", H128, 386),
    _k("halo:256/fwd/plain", H256),
    _k("halo:256/dgrad/plain", H256),
    _k("halo:256/dgrad/dst_acc", H256),
    _k("halo:256/dgrad/masked_res", H256),
    _k("halo:256/dgrad/up_sums", H256, 48),
    _k("halo:256/dgrad/up_sums_masked_res", H256, 48),
]


# ---- coverage: census key -> the test that checks that kernel with that operand set against a reference -----------------------
_OWN, _CONV = "tests.test_conv_routes_gpu::test_route_case[%s]", "tests.test_conv_gpu::"
COVERAGE = {"%s/%s/%s" % (c.launches[-1][0] + ":%d" % c.launches[-1][1], c.direction, c.opset): _OWN % c.id for c in CENSUS_CASES}
COVERAGE.update({
    "tile256:128/fwd/plain": _OWN % "fwd1x1-plain", "tile256:128/fwd/stats": _OWN % "fwd1x1-stats",
    "tile256:128/dgrad/plain": _OWN % "dgrad1x1-plain", "tile256:128/dgrad/dst_acc": _OWN % "dgrad1x1-dst_acc",
    "tile256:128/dgrad/masked_res": _OWN % "dgrad1x1-masked_res", "tile256:128/dgrad/up_sums": _OWN % "dgrad1x1-up_sums",
    "tile256:128/dgrad/up_sums_masked_res": _OWN % "dgrad1x1-up_sums_masked_res-tail33",
    "tile256:128/dgrad/gated": _OWN % "dgrad1x1-gated", "tile256:128/dgrad2/two_source": _OWN % "dgrad2-production",
    "tile256:128/dgrad2/two_source_sums": _OWN % "dgrad2-sums"})
for _test, _keys in {
    # against torch's convolution in fp32 (every case list of these tests was walked through the query)
    "test_conv_forward_and_dgrad": "tile:128/dgrad/dst_acc tile:128/dgrad/plain tile:128/fwd/plain tile_2stage:128/dgrad/dst_acc "
                                   "tile_2stage:128/dgrad/plain tile_2stage:128/fwd/plain tile_2stage:64/dgrad/dst_acc "
                                   "tile_2stage:64/dgrad/plain tile_2stage:64/fwd/plain tile_general:64/dgrad/dst_acc "
                                   "tile_general:64/dgrad/plain tile_general:64/fwd/plain tile_mc:128/dgrad/plain tile_mc:64/dgrad/dst_acc "
                                   "tile_mc:64/dgrad/plain",
    "test_conv_fused_bn_statistics": "tile_2stage:128/fwd/stats tile_2stage:64/fwd/stats tile_general:64/fwd/stats",
    "test_dgrad_with_relu_masked_residual": "tile_2stage:64/dgrad/masked_res",
    # float64 textbook gradient
    "test_dgrad_emits_upstream_bn_backward_sums": "regw1x1:6/dgrad/up_sums regw1x1:7/dgrad/up_sums regw1x1:8/dgrad/up_sums "
                                                  "tile_2stage:128/dgrad/up_sums tile_2stage:64/dgrad/up_sums tile_mc:128/dgrad/up_sums "
                                                  "tile_mc:64/dgrad/up_sums",
    "test_conv3x3_64_channels_weights_in_registers": "regw3x3:0/fwd/stats regw3x3:1/dgrad/up_sums",
    "test_bn3_backward_by_algebra": "tile_2stage:128/dgrad2/two_source tile_2stage:64/dgrad2/two_source",
    "test_conv3x3_halo_kernel": "halo:128/fwd/stats halo:256/fwd/stats",
    # against torch, the tile-kernel side of the comparison included (stored tensors bit-identical)
    "test_stream1x1_forward_stats_and_dgrad_epilogues": "stream1x1:128/fwd/stats stream1x1:256/fwd/stats stream1x1:64/fwd/stats "
                                                        "tile_2stage:128/dgrad/masked_res tile_2stage:128/dgrad/up_sums_masked_res "
                                                        "tile_2stage:64/dgrad/up_sums_masked_res",
    # bit-identical to the plain data gradient followed by the gate (the row above), sums against those of the stored tensor
    "test_dgrad_masked_store_and_column_sums": "regw1x1:6/dgrad/gated regw1x1:7/dgrad/gated regw1x1:8/dgrad/gated regw1x1:9/dgrad/gated "
                                               "tile_2stage:128/dgrad/gated",
    # bit-identical to the tile kernels of test_conv_forward_and_dgrad (same K order), sums against those of the stored tensor
    "test_forward_1x1_weights_in_registers_equals_the_tile_kernel": " ".join(
        "regw1x1:%d/fwd/%s" % (i, o) for i in (13, 14, 15, 16, 17, 18) for o in ("plain", "stats")),
}.items():
    COVERAGE.update({k: _CONV + _test for k in _keys.split()})


def resolve(node):
    """The test function a node id of COVERAGE names (and, for a case of this module's lists, that the case exists)."""
    import importlib
    module, _, name = node.partition("::")
    name, _, param = name.partition("[")
    fn = getattr(importlib.import_module(module), name, None)
    if param and param.rstrip("]") not in {c.id for c in GPU_CASES + CENSUS_CASES}:
        return None
    return fn if callable(fn) else None


# ---- the census as recorded: geometry (n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, ldw) + (groups,) -> answers --------------
_MC4 = "|".join(["tile_2stage:128"] * 4)
_MC4N = "|".join(["tile_2stage:64"] * 4)
_T2, _T2N = "tile_2stage:128", "tile_2stage:64"
CENSUS = {
    # ResNet50, batch 256
    (256, 56, 56, 64, 56, 56, 64, 1, 1, 1, 0, 64, 1): (" ".join([_T2N] * 2), " ".join([_T2N] * 6), ""),
    (256, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1, 576, 1): ("regw3x3:0 regw3x3:0", "regw3x3:0 %s %s regw3x3:1 %s -2" % (_T2N, _T2N, _T2N), ""),
    (256, 56, 56, 64, 56, 56, 256, 1, 1, 1, 0, 64, 1): ("stream1x1:256 stream1x1:256", " ".join([_T2N] * 6), " ".join([_T2N] * 2)),
    (256, 56, 56, 256, 56, 56, 64, 1, 1, 1, 0, 256, 1): ("stream1x1:64 stream1x1:64", "%s %s %s regw1x1:6 regw1x1:6 regw1x1:6" % (_T2, _T2, _T2), ""),
    (256, 56, 56, 256, 56, 56, 128, 1, 1, 1, 0, 256, 1): ("stream1x1:128 stream1x1:128", "regw1x1:14 %s %s regw1x1:7 regw1x1:7 regw1x1:7" % (_T2, _T2), ""),
    (256, 56, 56, 128, 28, 28, 128, 3, 3, 2, 1, 1152, 1): ("tile256:128 tile256:128", "tile_mc:128 tile_mc:128 -2 tile_mc:128 -2 -2", ""),
    (256, 28, 28, 128, 28, 28, 512, 1, 1, 1, 0, 128, 1): ("regw1x1:13 regw1x1:13", "regw1x1:17 " + " ".join([_T2] * 5), "tile256:128 tile256:128"),
    (256, 28, 28, 512, 28, 28, 128, 1, 1, 1, 0, 512, 1): ("regw1x1:17 regw1x1:17", "regw1x1:13 %s %s regw1x1:7 regw1x1:7 regw1x1:7" % (_T2, _T2), ""),
    (256, 28, 28, 128, 28, 28, 128, 3, 3, 1, 1, 1152, 1): ("halo:128 halo:128", "halo:128 halo:128 halo:128 halo:128 halo:128 -2", ""),
    (256, 28, 28, 512, 28, 28, 256, 1, 1, 1, 0, 512, 1): (" ".join([_T2] * 2), "regw1x1:15 %s %s regw1x1:8 regw1x1:8 regw1x1:8" % (_T2, _T2), ""),
    (256, 28, 28, 256, 14, 14, 256, 3, 3, 2, 1, 2304, 1): ("tile256:128 tile256:128", "tile_mc:128 tile_mc:128 -2 tile_mc:128 -2 -2", ""),
    (256, 14, 14, 256, 14, 14, 1024, 1, 1, 1, 0, 256, 1): ("regw1x1:15 regw1x1:15", "regw1x1:18 " + " ".join(["tile256:128"] * 5), "tile256:128 tile256:128"),
    (256, 14, 14, 1024, 14, 14, 256, 1, 1, 1, 0, 1024, 1): ("regw1x1:18 regw1x1:18", "regw1x1:15 %s %s regw1x1:8 regw1x1:8 regw1x1:8" % (_T2, _T2), ""),
    (256, 14, 14, 256, 14, 14, 256, 3, 3, 1, 1, 2304, 1): ("halo:256 halo:256", "halo:256 halo:256 halo:256 halo:256 halo:256 -2", ""),
    (256, 14, 14, 1024, 14, 14, 512, 1, 1, 1, 0, 1024, 1): ("tile256:128 tile256:128", "regw1x1:16 %s %s regw1x1:9 regw1x1:9 regw1x1:9" % (_T2, _T2), ""),
    (256, 14, 14, 512, 7, 7, 512, 3, 3, 2, 1, 4608, 1): ("tile:128 tile:128", "%s %s -2 %s -2 -2" % (_MC4, _MC4, _MC4), ""),
    (256, 7, 7, 512, 7, 7, 2048, 1, 1, 1, 0, 512, 1): ("regw1x1:16 regw1x1:16", " ".join([_T2] * 6), "tile:128 tile:128"),
    (256, 7, 7, 2048, 7, 7, 512, 1, 1, 1, 0, 2048, 1): (" ".join([_T2] * 2), "regw1x1:16 " + " ".join([_T2] * 5), ""),
    (256, 7, 7, 512, 7, 7, 512, 3, 3, 1, 1, 4608, 1): ("halo:256 halo:256", "halo:256 halo:256 halo:256 halo:256 halo:256 -2", ""),
    (256, 56, 56, 256, 28, 28, 512, 1, 1, 2, 0, 256, 1): (" ".join([_T2] * 2), "tile_mc:128 %s -2 tile_mc:128 -2 -2" % _T2, ""),
    (256, 28, 28, 512, 14, 14, 1024, 1, 1, 2, 0, 512, 1): (" ".join([_T2] * 2), "tile_mc:128 tile256:128 -2 tile_mc:128 -2 -2", ""),
    (256, 14, 14, 1024, 7, 7, 2048, 1, 1, 2, 0, 1024, 1): ("tile256:128 tile256:128", "tile_mc:128 tile256:128 -2 tile_mc:128 -2 -2", ""),
    # ResNet50, batch 64
    (64, 56, 56, 64, 56, 56, 64, 1, 1, 1, 0, 64, 1): (" ".join([_T2N] * 2), " ".join([_T2N] * 6), ""),
    (64, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1, 576, 1): ("regw3x3:0 regw3x3:0", "regw3x3:0 %s %s regw3x3:1 %s -2" % (_T2N, _T2N, _T2N), ""),
    (64, 56, 56, 64, 56, 56, 256, 1, 1, 1, 0, 64, 1): ("stream1x1:256 stream1x1:256", " ".join([_T2N] * 6), " ".join([_T2N] * 2)),
    (64, 56, 56, 256, 56, 56, 64, 1, 1, 1, 0, 256, 1): ("stream1x1:64 stream1x1:64", "%s %s %s regw1x1:6 regw1x1:6 regw1x1:6" % (_T2, _T2, _T2), ""),
    (64, 56, 56, 256, 56, 56, 128, 1, 1, 1, 0, 256, 1): ("stream1x1:128 stream1x1:128", "regw1x1:14 %s %s regw1x1:7 regw1x1:7 regw1x1:7" % (_T2, _T2), ""),
    (64, 56, 56, 128, 28, 28, 128, 3, 3, 2, 1, 1152, 1): (" ".join([_T2] * 2), "tile_mc:128 tile_mc:128 -2 tile_mc:128 -2 -2", ""),
    (64, 28, 28, 128, 28, 28, 512, 1, 1, 1, 0, 128, 1): ("regw1x1:13 regw1x1:13", "regw1x1:17 " + " ".join([_T2] * 5), " ".join([_T2] * 2)),
    (64, 28, 28, 512, 28, 28, 128, 1, 1, 1, 0, 512, 1): ("regw1x1:17 regw1x1:17", "regw1x1:13 %s %s regw1x1:7 regw1x1:7 regw1x1:7" % (_T2, _T2), ""),
    (64, 28, 28, 128, 28, 28, 128, 3, 3, 1, 1, 1152, 1): ("halo:128 halo:128", "halo:128 halo:128 halo:128 halo:128 halo:128 -2", ""),
    (64, 28, 28, 512, 28, 28, 256, 1, 1, 1, 0, 512, 1): (" ".join([_T2] * 2), "regw1x1:15 %s %s regw1x1:8 regw1x1:8 regw1x1:8" % (_T2, _T2), ""),
    (64, 28, 28, 256, 14, 14, 256, 3, 3, 2, 1, 2304, 1): (" ".join([_T2] * 2), "tile_mc:128 tile_mc:128 -2 tile_mc:128 -2 -2", ""),
    (64, 14, 14, 256, 14, 14, 1024, 1, 1, 1, 0, 256, 1): ("regw1x1:15 regw1x1:15", "regw1x1:18 " + " ".join([_T2] * 5), " ".join([_T2] * 2)),
    (64, 14, 14, 1024, 14, 14, 256, 1, 1, 1, 0, 1024, 1): ("regw1x1:18 regw1x1:18", "regw1x1:15 %s %s regw1x1:8 regw1x1:8 regw1x1:8" % (_T2, _T2), ""),
    (64, 14, 14, 256, 14, 14, 256, 3, 3, 1, 1, 2304, 1): (" ".join([_T2] * 2), " ".join([_T2] * 5) + " -2", ""),
    (64, 14, 14, 1024, 14, 14, 512, 1, 1, 1, 0, 1024, 1): (" ".join([_T2] * 2), "regw1x1:16 %s %s regw1x1:9 regw1x1:9 regw1x1:9" % (_T2, _T2), ""),
    (64, 14, 14, 512, 7, 7, 512, 3, 3, 2, 1, 4608, 1): ("tile:128 tile:128", "%s %s -2 %s -2 -2" % (_MC4, _MC4, _MC4), ""),
    (64, 7, 7, 512, 7, 7, 2048, 1, 1, 1, 0, 512, 1): ("regw1x1:16 regw1x1:16", " ".join([_T2] * 6), "tile:128 tile:128"),
    (64, 7, 7, 2048, 7, 7, 512, 1, 1, 1, 0, 2048, 1): (" ".join([_T2] * 2), "regw1x1:16 " + " ".join([_T2] * 5), ""),
    (64, 7, 7, 512, 7, 7, 512, 3, 3, 1, 1, 4608, 1): ("tile:128 tile:128", "tile:128 tile:128 tile:128 tile:128 tile:128 -2", ""),
    (64, 56, 56, 256, 28, 28, 512, 1, 1, 2, 0, 256, 1): (" ".join([_T2] * 2), "tile_mc:128 %s -2 tile_mc:128 -2 -2" % _T2, ""),
    (64, 28, 28, 512, 14, 14, 1024, 1, 1, 2, 0, 512, 1): (" ".join([_T2] * 2), "tile_mc:128 %s -2 tile_mc:128 -2 -2" % _T2, ""),
    (64, 14, 14, 1024, 7, 7, 2048, 1, 1, 2, 0, 1024, 1): (" ".join([_T2] * 2), "tile_mc:128 %s -2 tile_mc:128 -2 -2" % _T2, ""),
    # ResNeXt-101 32x4d, batch 128 (grouped 3x3 layers: 64-channel chunks)
    (128, 56, 56, 64, 56, 56, 128, 1, 1, 1, 0, 64, 1): (" ".join([_T2] * 2), " ".join([_T2N] * 6), ""),
    (128, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1, 576, 2): (" ".join([_T2N] * 2), " ".join([_T2N] * 5) + " -2", ""),
    (128, 56, 56, 128, 56, 56, 256, 1, 1, 1, 0, 128, 1): ("regw1x1:14 regw1x1:14", " ".join([_T2] * 6), " ".join([_T2] * 2)),
    (128, 56, 56, 256, 56, 56, 128, 1, 1, 1, 0, 256, 1): ("stream1x1:128 stream1x1:128", "regw1x1:14 %s %s regw1x1:7 regw1x1:7 regw1x1:7" % (_T2, _T2), ""),
    (128, 56, 56, 256, 56, 56, 256, 1, 1, 1, 0, 256, 1): (" ".join([_T2] * 2), " ".join([_T2] * 6), ""),
    (128, 56, 56, 64, 28, 28, 64, 3, 3, 2, 1, 576, 4): (" ".join([_T2N] * 2), "%s %s -2 %s -2 -2" % (_MC4N, _MC4N, _MC4N), ""),
    (128, 28, 28, 256, 28, 28, 512, 1, 1, 1, 0, 256, 1): ("regw1x1:15 regw1x1:15", " ".join([_T2] * 6), "tile256:128 tile256:128"),
    (128, 28, 28, 512, 28, 28, 256, 1, 1, 1, 0, 512, 1): (" ".join([_T2] * 2), "regw1x1:15 %s %s regw1x1:8 regw1x1:8 regw1x1:8" % (_T2, _T2), ""),
    (128, 28, 28, 64, 28, 28, 64, 3, 3, 1, 1, 576, 4): (" ".join([_T2N] * 2), " ".join([_T2N] * 5) + " -2", ""),
    (128, 28, 28, 512, 28, 28, 512, 1, 1, 1, 0, 512, 1): (" ".join([_T2] * 2), " ".join([_T2] * 6), ""),
    (128, 28, 28, 64, 14, 14, 64, 3, 3, 2, 1, 576, 8): (" ".join([_T2N] * 2), "%s %s -2 %s -2 -2" % (_MC4N, _MC4N, _MC4N), ""),
    (128, 14, 14, 512, 14, 14, 1024, 1, 1, 1, 0, 512, 1): ("regw1x1:16 regw1x1:16", " ".join(["tile256:128"] * 6), "tile256:128 tile256:128"),
    (128, 14, 14, 1024, 14, 14, 512, 1, 1, 1, 0, 1024, 1): ("tile256:128 tile256:128", "regw1x1:16 %s %s regw1x1:9 regw1x1:9 regw1x1:9" % (_T2, _T2), ""),
    (128, 14, 14, 64, 14, 14, 64, 3, 3, 1, 1, 576, 8): (" ".join([_T2N] * 2), " ".join([_T2N] * 5) + " -2", ""),
    (128, 14, 14, 1024, 14, 14, 1024, 1, 1, 1, 0, 1024, 1): ("tile256:128 tile256:128", " ".join(["tile256:128"] * 6), ""),
    (128, 14, 14, 64, 7, 7, 64, 3, 3, 2, 1, 576, 16): (" ".join([_T2N] * 2), "%s %s -2 %s -2 -2" % (_MC4N, _MC4N, _MC4N), ""),
    (128, 7, 7, 1024, 7, 7, 2048, 1, 1, 1, 0, 1024, 1): ("regw1x1:18 regw1x1:18", " ".join([_T2] * 6), "tile:128 tile:128"),
    (128, 7, 7, 2048, 7, 7, 1024, 1, 1, 1, 0, 2048, 1): (" ".join([_T2] * 2), "regw1x1:18 " + " ".join(["tile256:128"] * 5), ""),
    (128, 7, 7, 64, 7, 7, 64, 3, 3, 1, 1, 576, 16): (" ".join([_T2N] * 2), " ".join([_T2N] * 5) + " -2", ""),
    (128, 56, 56, 64, 56, 56, 256, 1, 1, 1, 0, 64, 1): ("stream1x1:256 stream1x1:256", " ".join([_T2N] * 6), ""),
    (128, 56, 56, 256, 28, 28, 512, 1, 1, 2, 0, 256, 1): (" ".join([_T2] * 2), "tile_mc:128 %s -2 tile_mc:128 -2 -2" % _T2, ""),
    (128, 28, 28, 512, 14, 14, 1024, 1, 1, 2, 0, 512, 1): (" ".join([_T2] * 2), "tile_mc:128 tile256:128 -2 tile_mc:128 -2 -2", ""),
    (128, 14, 14, 1024, 7, 7, 2048, 1, 1, 2, 0, 1024, 1): ("tile256:128 tile256:128", "tile_mc:128 %s -2 tile_mc:128 -2 -2" % _T2, ""),
    # ResNet32 (CIFAR), batch 128
    (128, 32, 32, 16, 32, 32, 16, 3, 3, 1, 1, 144, 1): ("tile_general:64 tile_general:64", " ".join(["tile_general:64"] * 5) + " -2", ""),
    (128, 32, 32, 16, 16, 16, 32, 3, 3, 2, 1, 144, 1): ("tile_general:64 tile_general:64", "tile_mc:64 tile_mc:64 -2 tile_mc:64 -2 -2", ""),
    (128, 16, 16, 32, 16, 16, 32, 3, 3, 1, 1, 288, 1): (" ".join([_T2N] * 2), " ".join([_T2N] * 5) + " -2", ""),
    (128, 16, 16, 32, 8, 8, 64, 3, 3, 2, 1, 288, 1): (" ".join([_T2N] * 2), "tile_mc:64 tile_mc:64 -2 tile_mc:64 -2 -2", ""),
    (128, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 576, 1): ("regw3x3:0 regw3x3:0", "regw3x3:0 %s %s regw3x3:1 %s -2" % (_T2N, _T2N, _T2N), ""),
}
