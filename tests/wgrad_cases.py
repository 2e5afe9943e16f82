"""The weight gradient's split-K rule restated in plain Python, and the case tables that tests/test_wgrad_plan_host.py (no
device) and tests/test_wgrad_splits_gpu.py share.

`plan` is written from the description of iif_conv_wgrad_plan in include/iif_amd.h and DESIGN.md section 4h, with the
default values of the IIF_WGRAD_* switches; the host test compares it with the library's answer.  Nothing here needs the
library or a device."""
import collections
import os

F32, BF16 = 0, 1                                            # iif_amd._lib.IIF_F32 / IIF_BF16
FAMILIES = ("regstage", "dma", "1x1", "ninetap", "stem")    # IIF_WGRAD_* of include/iif_amd.h
Plan = collections.namedtuple("Plan", "family bc bnw tiles nsteps splits steps_per_split blocks stages chunks")
MIB = 1 << 20


def cdiv(a, b):
    return -(-a // b)


def slab_floats(row, cd2=0):
    n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, ldw, g, dt = row
    return max(g, 1) * (cd + max(cd2, 0)) * ldw


def plan(row, cd2=0, workspace_bytes=0, splits=0, regstage=None):
    """row = (n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, ldw, groups, dtype), channels per group.  cd2 as the query's.
    Returns a Plan, or None where the launch is refused (the register-staged kernel has no grouped form)."""
    n, hs, ws, cs, hd, wd, cd, r, s, stride, pad, ldw, g, dt = row
    if regstage is None:
        regstage = "IIF_CONV_REGSTAGE" in os.environ
    g = max(g, 1)
    esz = 2 if dt == BF16 else 4
    m, k = n * hd * wd, r * s * cs
    cd_total = cd + max(cd2, 0)
    stacked, gram = cd2 > 0, cd2 == -1
    big = n * hs * ws * g * cs * esz >= 0x7ffffff0 or m * g * cd * esz >= 0x7ffffff0
    dma = stacked or not (regstage or big)
    same, dense = (hs, ws) == (hd, wd), g == 1
    family = None
    if dt == BF16 and dma and not stacked:
        chans = (cs % 64 == 0 and cd % 64 == 0) if dense else (cs == 64 and cd == 64 and ldw >= 576)
        if (r, s, stride, pad) == (3, 3, 1, 1) and same and wd <= 61 and chans and n * (hd + 2) * (wd + 2) <= 0x7fff0000:
            family = "ninetap"
        elif ((r, s, stride, pad) == (4, 4, 1, 2) and same and dense and (cs, cd) == (16, 64)
              and cdiv(2 * (wd + 3) + 2, 32) + (wd + 35) // 32 <= 12 and n * (hd + 3) * (wd + 3) <= 0x7fff0000):
            family = "stem"
    if stacked or (family is None and dt == BF16 and dma and (r, s, stride, pad) == (1, 1, 1, 0) and same and dense):
        family = "1x1"
    if family is None:
        family = "dma" if dma else "regstage"
        if g > 1 and not dma:
            return None

    if family == "ninetap":
        bc, bnw = 64, 64
        tiles = g if not dense else (cs // 64) * (cd // 64)
        round_tiles = tiles                                  # the tile count already counts the groups
        nsteps, per_cu = cdiv(n * (hd + 2) * (wd + 2), 32), 2
    elif family == "stem":
        bc, bnw, tiles, round_tiles = 64, 256, 1, 1
        nsteps, per_cu = cdiv(n * (hd + 3) * (wd + 3), 32), 2
    elif family == "1x1":
        if stacked:
            bc = 256 if cd % 256 == 0 else 128
        else:
            bc = 256 if cd % 256 == 0 else (64 if cd <= 64 else 128)
        bnw = 64 if (bc == 64 and cs <= 64) else (256 if (bc == 64 and cs % 256 == 0) else 128)
        tiles = cdiv(cd_total, bc) * cdiv(cs, bnw)
        round_tiles = tiles
        nsteps = cdiv(m, 32)
        per_cu = {256: 1, 128: 3}.get(bc, 2 if bnw == 256 else 4)
    else:
        bc = 256 if (family == "dma" and dt == BF16 and dense and cd % 256 == 0) else (64 if cd <= 64 else 128)
        bnw = 128
        tiles = cdiv(cd, bc) * cdiv(k, 128)
        round_tiles = tiles * g
        nsteps = cdiv(m, 32 if dt == BF16 else 16)
        per_cu = {256: 1, 128: 3, 64: 4}[bc]

    slab = g * cd_total * ldw
    sp = splits
    if sp <= 0:
        share = max(1, -splits)
        sp = 256 * per_cu // share // round_tiles
        if family == "ninetap" and not dense:
            sp //= 4
        sp = min(max(sp, 1), max(1, nsteps // 8))
        if family == "1x1" and sp > 8:
            div = 8 if gram else (2 if slab * 4 <= 4 * MIB else 1)       # (up to 256 KiB: 2; up to 4 MiB: 2)
            sp = max(sp // div, 8) if div > 1 else sp
    sp = min(sp, workspace_bytes // (slab * 4))
    sp = min(max(sp, 1), nsteps, 65535)
    sps = cdiv(nsteps, sp)
    sp = cdiv(nsteps, sps)
    blocks = tiles * sp if family == "regstage" else tiles * (g if family == "dma" else 1) * cdiv(sp, 8) * 8
    stages, chunks = (0, 0) if sp == 1 else (1, 0)
    if sp > 32 and cdiv(slab, 1024) < 256 and (sp + cdiv(sp, 16)) * slab * 4 <= workspace_bytes:
        stages, chunks = 2, cdiv(sp, 16)
    return Plan(family, bc, bnw, tiles, nsteps, sp, sps, blocks, stages, chunks)


def realised(nsteps, request):
    """Splits realised for a positive request when the workspace holds them all."""
    sp = min(max(request, 1), nsteps, 65535)
    return cdiv(nsteps, cdiv(nsteps, sp))


def request_for(nsteps, target):
    """The smallest request that realises exactly `target` splits over `nsteps` steps, or None."""
    for q in range(1, nsteps + 1):
        if realised(nsteps, q) == target:
            return q
    return None


# ---- the GPU cases ------------------------------------------------------------------------------------------------------
# Realised split counts every family must cover across its cases: both sides of the 16-slab groups of the slab sum (15 / 16 / 17,
# 31 / 32 / 33, 48 / 49), the trivial ends, and one of at least 97; ninetap and stem also one of at least 512 at one step each.
TARGETS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49)
MANY, FULL = 97, 512

Case = collections.namedtuple("Case", "name family n h w cin cout r stride pad groups dtype kind cd2")


def _c(name, family, n, h, w, cin, cout, r, stride, pad, groups=1, dtype=BF16, kind="conv", cd2=0):
    return Case(name, family, n, h, w, cin, cout, r, stride, pad, groups, dtype, kind, cd2)


# Step counts 96 (-> 96, 48, 32, 16, 2, 1), 98 (-> 98, 49, 33, 17) and 155 (-> 155, 31, 16, 15) between them realise every target;
# each shape below has one of them (bf16; fp32 steps are 16 pixels: twice as many) and a ragged last step.
CASES = [
    # nine taps per block: steps over N (H + 2) (W + 2) padded pixels; W + 3 <= 32 and > 32 (the two ring leads)
    _c("nt_64_w13", "ninetap", 2, 100, 13, 64, 64, 3, 1, 1),                     # 3 060 padded pixels: 96 steps
    _c("nt_128_w31", "ninetap", 1, 93, 31, 128, 128, 3, 1, 1),                   # 3 135: 98
    _c("nt_g4_w20", "ninetap", 3, 73, 20, 256, 256, 3, 1, 1, groups=4),          # 4 950: 155
    _c("nt_64_auto", "ninetap", 3, 54, 54, 64, 64, 3, 1, 1),                     # 294 steps: the automatic round is 36
    _c("nt_64_full", "ninetap", 5, 56, 56, 64, 64, 3, 1, 1),                     # 526 steps, one per split
    # space-to-depth stem: steps over N (H + 3) (W + 3)
    _c("stem_96", "stem", 1, 48, 57, 16, 64, 4, 1, 2, kind="stem"),
    _c("stem_98", "stem", 1, 52, 54, 16, 64, 4, 1, 2, kind="stem"),
    _c("stem_155", "stem", 1, 63, 72, 16, 64, 4, 1, 2, kind="stem"),
    _c("stem_full", "stem", 2, 90, 90, 16, 64, 4, 1, 2, kind="stem"),            # 541 steps
    # 1x1 as [1, 1, m, C], m % 32 != 0: every tile
    _c("t256x128", "1x1", 1, 1, 3067, 128, 256, 1, 1, 0),
    _c("t128x128", "1x1", 1, 1, 3129, 128, 128, 1, 1, 0),
    _c("t64x128", "1x1", 1, 1, 4951, 128, 64, 1, 1, 0),
    _c("t64x64", "1x1", 1, 1, 3067, 64, 64, 1, 1, 0),
    _c("t64x256", "1x1", 1, 1, 3129, 256, 64, 1, 1, 0),
    _c("stacked_128", "1x1", 1, 1, 4951, 64, 128, 1, 1, 0, kind="stacked", cd2=72),       # last tile of dy2: 72 of 128 rows
    _c("stacked_256", "1x1", 1, 1, 3067, 64, 256, 1, 1, 0, kind="stacked", cd2=72),       # 72 of 256
    _c("gram_64", "1x1", 1, 1, 3129, 64, 64, 1, 1, 0, kind="gram", cd2=-1),
    _c("t_1mib", "1x1", 1, 1, 1053, 512, 512, 1, 1, 0),                          # a 1 MiB slab, 33 steps: one pass by size
]
for _dt, _tag in ((BF16, "bf16"), (F32, "f32")):
    CASES += [
        _c("dma_3x3s2_" + _tag, "dma", 3, 59, 67, 64, 128, 3, 2, 1, dtype=_dt),                # M = 3 060
        _c("dma_1x1s2_" + _tag, "dma", 1, 109, 113, 64, 64, 1, 2, 0, dtype=_dt),               # 3 135
        _c("dma_cin16_" + _tag, "dma", 2, 45, 55, 16, 32, 3, 1, 1, dtype=_dt),                 # 4 950; ragged K tail
        _c("dma_cout24_" + _tag, "dma", 1, 51, 60, 8, 24, 3, 1, 1, dtype=_dt),                 # 3 060
        _c("dma_t256_" + _tag, "dma", 1, 109, 113, 32, 256, 1, 2, 0, dtype=_dt),               # 3 135; the 256-channel tile (bf16)
        _c("dma_g4x8_" + _tag, "dma", 2, 45, 55, 32, 32, 3, 1, 1, groups=4, dtype=_dt),        # 4 950; 8-channel groups
        _c("dma_2mib_" + _tag, "dma", 1, 53, 77, 256, 256, 3, 2, 1, dtype=_dt),                # M = 1 053, a 2.25 MiB slab
        _c("rs_3x3_" + _tag, "regstage", 1, 51, 60, 64, 64, 3, 1, 1, dtype=_dt),               # 3 060
        _c("rs_1x1_" + _tag, "regstage", 1, 55, 57, 32, 72, 1, 1, 0, dtype=_dt),               # 3 135
        _c("rs_s2_" + _tag, "regstage", 2, 89, 109, 16, 24, 3, 2, 1, dtype=_dt),               # 4 950
    ]
CASE = {c.name: c for c in CASES}


def pad_ldw(c):
    """Row pitch of the case's output: 8 pad columns behind the K logical ones."""
    return c.r * c.r * (c.cin // c.groups) + 8


def out_hw(c):
    if c.kind == "stem":
        return c.h, c.w
    return (c.h + 2 * c.pad - c.r) // c.stride + 1, (c.w + 2 * c.pad - c.r) // c.stride + 1


def row_of(c):
    """The case as the descriptor row `plan` and the query take (channels per group, the padded pitch)."""
    hd, wd = out_hw(c)
    return (c.n, c.h, c.w, c.cin // c.groups, hd, wd, c.cout // c.groups, c.r, c.r, c.stride, c.pad, pad_ldw(c), c.groups, c.dtype)


def requests(c):
    """{realised count: positive request} the case runs: every target its step count realises, the largest count (>= MANY), and
    nothing else."""
    p = plan(row_of(c), c.cd2, 1 << 40, 1, regstage=c.family == "regstage")
    assert p is not None and p.family == c.family, (c.name, p)
    out = {}
    for t in TARGETS + (p.nsteps,):
        q = request_for(p.nsteps, t)
        if q is not None and (t in TARGETS or t >= MANY):
            out[t] = q
    return out
