"""The size-selected paths of the BN, pool and SE streaming kernels on the device, against the float64 references of
tests/stream_cases.py: for each host-side launch decision (unroll 1 / 2 / 4 of the BN normalisation passes, the three
IIF_BN_* switches, the block caps of the grid-stride kernels, the row cap of the fused stem pool, the row groups of
iif_bn_backward_pool_fused) the smallest tensor on each side of it, with ragged ends.  tests/test_stream_cases_host.py holds
every case to the side of its threshold through the planning query.

The inputs make the arithmetic exact (see stream_cases), so outputs and decision bytes are compared BIT FOR BIT over every
element; every output starts as NaN (0xAA for bytes) with a guard band behind it that must come back untouched.  Only the routes
that form sums on the device are bounded; those print measured / allowed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import stream_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, BF16, FP32 = torch.float64, torch.bfloat16, torch.float32
DT_IDS = list(S.DTYPES)


def ratio(err, bound):
    """max of measured / allowed (0 / 0 counts as 0)"""
    return (err.double() / bound.double().clamp_min(1e-300)).max().item()


def nan_like(*shape, dt=FP32):
    return torch.full(shape, float("nan"), dtype=dt, device=DEV)


# ------------------------------------------------------------------------------------------------ BN normalisation passes
@pytest.mark.parametrize("key", DT_IDS)
@pytest.mark.parametrize("name", S.BN_TABLE)
def test_bn_apply_unrolled_tails_exact(name, key):
    """iif_bn_apply at U = 1 / 2 / 4 with a ragged last trip, fixed and reloaded coefficients: ReLU on / off x residual none /
    plain / normalised x with / without decision bytes, bit for bit."""
    assert S.check_bn_apply_exact(name, S.DTYPES[key], DEV) == []


@pytest.mark.parametrize("key", DT_IDS)
@pytest.mark.parametrize("name", S.BN_TABLE)
def test_bn_backward_apply_sums_unrolled_tails_exact(name, key):
    """iif_bn_backward_apply_sums (exact coefficients from power-of-two sums): mask none / from y / from bits x with / without
    the masked gradient, and once in place (dx == gy), bit for bit; dgamma / dbeta are bit copies of the local sums."""
    assert S.check_bn_backward_exact(name, S.DTYPES[key], DEV) == []


@pytest.mark.parametrize("key", DT_IDS)
@pytest.mark.parametrize("name", S.BN_SUM_CASES)
def test_bn_backward_routes_that_form_their_sums(name, key):
    """iif_bn_backward (mask from bits) and iif_bn_backward_relu_recompute at U = 2 / 4: the device forms the sums, so
      dbeta, dgamma  within 6 eps l2(terms) + 4e-6 l1(terms) of the float64 sums, per channel (stream_cases.sum_bound: the bound
                     tests/test_layers_gpu.py uses for these sums),
      dx             per element within stream_cases.dx_bound: with k1 = gamma invstd, k2 = s1 / m, k3 = (s2 / m) invstd and
                     dx = k1 (d - k2 - (x - mean) k3), an error b1 of s1 and b2 of s2 moves dx by at most
                     |k1| (b1 / m + |x - mean| invstd b2 / m); the fp32 roundings of the three coefficients and the four
                     operations add at most 8 * 2^-24 |k1| (|d| + |k2| + |x - mean| |k3|); the store adds one rounding to the
                     storage type: at most half a unit of bf16's eighth significant bit, 2^-8 |dx|."""
    from iif_amd import _lib, ops
    dt = S.DTYPES[key]
    m, c = S.bn_shape(name, dt)
    d = S.bn_case_inputs(name, dt, DEV)
    x, gy = S.rnd(d["x"], dt), S.rnd(d["gy"], dt)
    stats, gamma = d["stats"].float().contiguous(), d["gamma"].float()
    _, mask = S.bn_apply_ref(d["x"], d["stats"], True)
    bits = S.pack_bits(mask, S.vec(dt))
    dx_ref, dg_ref, db_ref, (t1, t2) = S.bn_backward_ref(d["gy"], d["x"], mask, d["gamma"], d["stats"][0], d["stats"][1])
    b1, b2 = S.sum_bound(t1, dt), S.sum_bound(t2, dt)
    allowed = S.dx_bound(dx_ref, t1, d["x"], d["gamma"], d["stats"][0], d["stats"][1], b1, b2, dt)
    ws = ops.bn_workspace(m, c, DEV)
    for route in ("bits", "recompute"):
        dxbuf, dx = S.guarded(m * c, dt, DEV)
        dg, db = nan_like(c), nan_like(c)
        if route == "bits":
            ops.bn_backward(gy, None, x, stats, gamma, dg, db, dx.view(m, c), ws, relu_bits=bits)
        else:
            _lib.check(_lib.lib().iif_bn_backward_relu_recompute(_lib.ptr(gy), _lib.ptr(x), _lib.dtype_code(x), m, c, _lib.ptr(stats),
                                                                 _lib.ptr(gamma), _lib.ptr(dg), _lib.ptr(db), _lib.ptr(dx), _lib.ptr(ws),
                                                                 ws.numel(), _lib.stream_ptr()), "iif_bn_backward_relu_recompute")
        r_b = ratio((db.double() - db_ref).abs(), b1)
        r_g = ratio((dg.double() - dg_ref).abs(), b2)
        r_x = ratio((dx.view(m, c).double() - dx_ref).abs(), allowed)
        print("\n[%s %s %s] measured / allowed: dbeta %.3f  dgamma %.3f  dx %.3f" % (name, key, route, r_b, r_g, r_x))
        assert S.guard_intact(dxbuf, m * c)
        assert r_b <= 1.0 and r_g <= 1.0 and r_x <= 1.0, (route, r_b, r_g, r_x)


# name: (environment, expectations of the worker, cases, time limit in seconds)
SWITCHES = {
    "grid_cap_7": ({"IIF_BN_GRID_CAP": "7"}, ["trips=2"], ["cap3000", "u1_top", "u2_b"], 240),
    "nt_stores": ({"IIF_BN_NT_STORES": "1"}, ["nts=1"], ["cap3000", "u2_b", "u4_b"], 240),
    "unroll_2": ({"IIF_BN_UNROLL": "2"}, ["u=2"], ["u4_b"], 180),
}


def test_bn_switch_variants_in_fresh_processes():
    """IIF_BN_GRID_CAP=7 (the outer loop takes many trips), IIF_BN_NT_STORES=1 (the other half of the compiled instances) and
    IIF_BN_UNROLL=2 on a U = 4 tensor: the exact forward and backward comparisons in a fresh child per setting (the switches are
    read once per process), one child at a time, each under its own time limit; the first failure ends the test."""
    for name, (env, expect, cases, limit) in SWITCHES.items():
        e = dict(os.environ)
        for k in ("IIF_BN_GRID_CAP", "IIF_BN_NT_STORES", "IIF_BN_UNROLL"):
            e.pop(k, None)
        e.update(env)
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "tests.stream_env_worker"] + expect + cases,
                           cwd=ROOT, env=e, capture_output=True, text=True)
        print("\n[%s]\n%s" % (name, r.stdout))
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        assert r.stdout.count("bit-identical") == 2 * len(cases), r.stdout


# ------------------------------------------------------------------------------------------------ grid-stride kernels past their cap
@pytest.mark.parametrize("src,dst", [(FP32, BF16), (BF16, FP32), (FP32, FP32)], ids=["f32_bf16", "bf16_f32", "f32_f32"])
def test_cast_past_the_block_cap(src, dst):
    from iif_amd import ops
    n = S.N_CAST
    h = S.hash_t(n, 300, DEV)
    # fp32 sources carry 17 significant bits so that the cast to bf16 really rounds (ties included)
    v = S.act(h, 0) + (S._bits(h, 20, 9) - 256).to(F64) / 2.0 ** 15 if src == FP32 else S.act(h, 0)
    s = v.to(src)
    buf, out = S.guarded(n, dst, DEV)
    ops.cast(s, out)
    assert S.same_bits(out, s.to(dst)) and S.guard_intact(buf, n)


def _opt_inputs(n, salt):
    h = S.hash_t(n, salt, DEV)
    return S.act(h, 0), [S.act(h, 9), S.act(h, 18)]


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_sgd_step_past_the_block_cap(nesterov):
    """Two steps over n = 8 388 608 + 4 099 (second trip of the f32x4 body, a three-element scalar tail) against the float64
    recurrence.  lr, momentum and weight decay are powers of two or short binary fractions, so the only errors are the fp32
    roundings of the six operations of a step (each 2^-24 of an operand no larger than |p| + |buf| + |g|): allowed
    2 steps x 8 x 2^-24 (|p| + |buf| + max |g|) per element, for the parameters and for the momentum buffer."""
    from iif_amd import ops
    n, lr, mom, wd = S.N_OPT, 0.125, 0.875, 2.0 ** -10
    p64, grads = _opt_inputs(n, 310)
    b64 = torch.zeros_like(p64)
    pbuf, p = S.guarded(n, FP32, DEV)
    bbuf, b = S.guarded(n, FP32, DEV)
    p.copy_(p64); b.zero_()
    for g64 in grads:
        S.sgd_ref(p64, g64, b64, lr, mom, wd, nesterov)
        ops.sgd_step(p, g64.float(), b, lr, mom, wd, nesterov)
    allowed = 16 * 2.0 ** -24 * (p64.abs() + b64.abs() + 4.0)
    r_p, r_b = ratio((p.double() - p64).abs(), allowed), ratio((b.double() - b64).abs(), allowed)
    print("\n[sgd nesterov=%s] measured / allowed: p %.3f  buf %.3f" % (nesterov, r_p, r_b))
    assert r_p <= 1.0 and r_b <= 1.0 and S.guard_intact(pbuf, n) and S.guard_intact(bbuf, n)


@pytest.mark.parametrize("centered", [False, True], ids=["plain", "centred"])
@pytest.mark.parametrize("momentum", [0.0, 0.875], ids=["nomom", "mom"])
def test_rmsprop_step_past_the_block_cap(momentum, centered):
    """Two steps over n = 8 388 608 + 4 099 against the float64 recurrence.  Constants exact in fp32; sqrtf and the division
    are correctly rounded, so a step is about twelve roundings of 2^-24 relative.  g / avg is at most 1 / sqrt(1 - alpha) = 2.83
    and the centred difference sq - ga^2 keeps at least 7/8 of sq (ga^2 <= (1 - alpha) sq after the first step), so nothing
    amplifies an error by more than about 1.3: allowed 2 steps x 16 x 2^-24 (|p| + |buf| + 4) per element."""
    from iif_amd import ops
    n, lr, alpha, eps, wd = S.N_OPT, 2.0 ** -7, 0.875, 0.03125, 2.0 ** -10
    p64, grads = _opt_inputs(n, 320)
    sq64 = torch.zeros_like(p64)
    b64 = torch.zeros_like(p64) if momentum else None
    a64 = torch.zeros_like(p64) if centered else None
    bufs = [S.guarded(n, FP32, DEV) for _ in range(4)]
    p, sq, b, a = (v for _, v in bufs)
    p.copy_(p64); sq.zero_(); b.zero_(); a.zero_()
    for g64 in grads:
        S.rmsprop_ref(p64, g64, sq64, b64, a64, lr, alpha, eps, wd, momentum)
        ops.rmsprop_step(p, g64.float(), sq, lr, alpha, eps, wd, momentum, momentum_buf=b if momentum else None,
                         grad_avg=a if centered else None)
    allowed = 32 * 2.0 ** -24 * (p64.abs() + (b64.abs() if momentum else 0.0) + 4.0)
    r_p = ratio((p.double() - p64).abs(), allowed)
    r_s = ratio((sq.double() - sq64).abs(), 32 * 2.0 ** -24 * (sq64.abs() + 1.0))
    print("\n[rmsprop momentum=%s centred=%s] measured / allowed: p %.3f  square_avg %.3f" % (momentum, centered, r_p, r_s))
    assert r_p <= 1.0 and r_s <= 1.0
    if momentum:
        assert ratio((b.double() - b64).abs(), allowed) <= 1.0
    if centered:
        assert ratio((a.double() - a64).abs(), allowed) <= 1.0
    assert all(S.guard_intact(bf, n) for bf, _ in bufs)


def _se_inputs(dt):
    n, hw, c = S.SE_SHAPE
    c = c if dt == BF16 else c // 2
    d = S.bn_inputs(n * hw, c, 330, DEV)
    h = S.hash_t(n * c, 331, DEV).view(n, c)
    d.update(e=S.excite(h, 0), off=S.coef_b(h, 8))
    for k in ("x", "r", "gy"):
        d[k] = d[k].view(n, hw, c)
    return n, hw, c, d


@pytest.mark.parametrize("key", DT_IDS)
def test_se_stream_passes_past_the_block_cap(key):
    """iif_se_apply (residual none / plain / normalised) and iif_se_backward_form at 1 076 480 vectors against the cap of
    4 096 blocks (1 048 576): the sample index n = (i / cv) / hw of the second trip; exact."""
    from iif_amd import ops
    dt = S.DTYPES[key]
    n, hw, c, d = _se_inputs(dt)
    v = S.vec(dt)
    x, r = S.rnd(d["x"], dt).view(n, 58, 58, c), S.rnd(d["r"], dt).view(n, 58, 58, c)
    st, st2, e = d["stats"].float().contiguous(), d["stats2"].float().contiguous(), d["e"].float().contiguous()
    for res in ("none", "plain", "normalised"):
        rr = None if res == "none" else d["r"]
        s2 = d["stats2"] if res == "normalised" else None
        y_ref, mask = S.se_apply_ref(d["x"], d["stats"], d["e"], rr, s2)
        ybuf, y = S.guarded(n * hw * c, dt, DEV)
        bbuf, bits = S.guarded(n * hw * c // v, torch.uint8, DEV)
        ops.se_apply(x, st, e, y.view(n, 58, 58, c), bits, residual=None if rr is None else r, residual_stats=None if s2 is None else st2)
        assert S.same_bits(y.view(n, hw, c), S.rnd(y_ref, dt)), res
        assert S.same_bits(bits, S.pack_bits(mask, v)), res
        assert S.guard_intact(ybuf, n * hw * c) and S.guard_intact(bbuf, n * hw * c // v), res
    obuf, out = S.guarded(n * hw * c, dt, DEV)
    ops.se_backward_form(S.rnd(d["gy"], dt).view(n, 58, 58, c), e, d["off"].float().contiguous(), out.view(n, 58, 58, c))
    assert S.same_bits(out.view(n, hw, c), S.rnd(S.se_form_ref(d["gy"], d["e"], d["off"]), dt)) and S.guard_intact(obuf, n * hw * c)


@pytest.mark.parametrize("key", DT_IDS)
def test_se_sums_at_the_same_shape(key):
    """iif_se_squeeze and iif_se_backward_sums on the shape above: per (sample, channel) sums against float64 under
    6 eps l2 + 4e-6 l1 of the terms; the masked gradient written in place is exact."""
    from iif_amd import ops
    dt = S.DTYPES[key]
    n, hw, c, d = _se_inputs(dt)
    v = S.vec(dt)
    x = S.rnd(d["x"], dt).view(n, 58, 58, c)
    sums = nan_like(n, c)
    ops.se_squeeze(x, sums)
    r0 = ratio((sums.double() - d["x"].sum(1)).abs(), S.sum_bound(d["x"], dt, 1))
    _, mask = S.se_apply_ref(d["x"], d["stats"], d["e"], d["r"])
    bits = S.pack_bits(mask, v)
    gbuf, g = S.guarded(n * hw * c, dt, DEV)
    g.copy_(S.rnd(d["gy"], dt).view(-1))
    s1, s2 = nan_like(n, c), nan_like(n, c)
    ops.se_backward_sums(g.view(n, 58, 58, c), bits, x, s1, s2)
    gm = torch.where(mask, d["gy"], torch.zeros_like(d["gy"]))
    assert S.same_bits(g.view(n, hw, c), S.rnd(gm, dt)) and S.guard_intact(gbuf, n * hw * c)
    r1 = ratio((s1.double() - gm.sum(1)).abs(), S.sum_bound(gm, dt, 1))
    r2 = ratio((s2.double() - (gm * d["x"]).sum(1)).abs(), S.sum_bound(gm * d["x"], dt, 1))
    print("\n[se sums %s] measured / allowed: squeeze %.3f  s1 %.3f  s2 %.3f" % (key, r0, r1, r2))
    assert r0 <= 1.0 and r1 <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("key", DT_IDS)
def test_avgpool_backward_past_the_block_cap(key):
    """dx[n, j, c] = gy[n, c] / hw over 2 152 960 vectors (cap 2 097 152): the sample index of the second trip.  gy / hw is one
    fp32 multiplication by the rounded reciprocal, restated here in fp32 and rounded to the storage type: exact."""
    from iif_amd import ops
    dt = S.DTYPES[key]
    n, hw, c = S.AVG_SHAPE
    c = c if dt == BF16 else c // 2
    gy = S.act(S.hash_t(n * c, 340, DEV), 0).view(n, c)
    buf, dx = S.guarded(n * hw * c, dt, DEV)
    ops.avgpool_backward(S.rnd(gy, dt), hw, out=dx.view(n, hw, c))
    inv = float(np.float32(1.0) / np.float32(hw))              # the correctly rounded fp32 reciprocal
    ref = (gy.float() * inv).to(dt)[:, None, :].expand(n, hw, c)
    assert S.same_bits(dx.view(n, hw, c), ref) and S.guard_intact(buf, n * hw * c)


@pytest.mark.parametrize("key", DT_IDS)
def test_general_maxpool_past_the_block_cap(key):
    """iif_maxpool_forward / iif_maxpool_backward, the general kernel (k = 3, stride 1, pad 1) on a 257 x 257 image: 2 113 568
    output vectors (cap 2 097 152).  ReLU-like inputs with long runs of ties: values exact, arg max by the first-maximum rule,
    backward (up to nine windows per pixel; sums of multiples of 1/64, exact in fp32, rounded once to the storage type) exact."""
    from iif_amd import ops
    dt = S.DTYPES[key]
    n, h, w, c = S.MAXPOOL_SHAPE
    c = c if dt == BF16 else c // 2
    hh = S.hash_t(n * h * w * c, 350, DEV).view(n, h, w, c)
    x = (S.act(hh, 0) * 4).round().clamp_min(0.0) / 4           # 17 distinct values, half of them 0: ties everywhere
    y, idx = ops.maxpool_forward(S.rnd(x, dt), 3, 1, 1)
    y_ref, code = S.maxpool_ref(x, 3, 1, 1)
    assert S.same_bits(y, S.rnd(y_ref, dt)) and torch.equal(idx, code)
    gy = S.act(hh, 9)
    buf, dx = S.guarded(n * h * w * c, dt, DEV)
    ops.maxpool_backward(S.rnd(gy, dt), idx, (n, h, w, c), 3, 1, 1, out=dx.view(n, h, w, c))
    ref = S.maxpool_scatter(gy, code, (h, w), 3, 1, 1)
    assert S.same_bits(dx.view(n, h, w, c), S.rnd(ref, dt)) and S.guard_intact(buf, n * h * w * c)


@pytest.mark.parametrize("key", DT_IDS)
def test_option_a_shortcut_past_the_block_cap(key):
    """iif_shortcut_a_forward (4 384 640 elements: three trips) and iif_shortcut_a_backward_acc (2 121 600: two), odd H and W."""
    from iif_amd import ops
    dt = S.DTYPES[key]
    n, h, w, cin, cout = S.SHORTCUT_SHAPE
    ho, wo, cpad = (h + 1) // 2, (w + 1) // 2, (cout - cin) // 2
    hh = S.hash_t(n * h * w * cin, 360, DEV).view(n, h, w, cin)
    x = S.act(hh, 0)
    ybuf, y = S.guarded(n * ho * wo * cout, dt, DEV)
    ops.shortcut_a_forward(S.rnd(x, dt), cout, out=y.view(n, ho, wo, cout))
    ref = torch.zeros(n, ho, wo, cout, dtype=F64, device=DEV)
    ref[..., cpad:cpad + cin] = x[:, ::2, ::2, :]
    assert S.same_bits(y.view(n, ho, wo, cout), S.rnd(ref, dt)) and S.guard_intact(ybuf, n * ho * wo * cout)
    g = S.act(S.hash_t(n * ho * wo * cout, 361, DEV), 0).view(n, ho, wo, cout)
    dx0 = S.act(hh, 9) / 2                                       # |dx0 + g| < 8 in multiples of 1/128: exact, 11 bits
    dbuf, dx = S.guarded(n * h * w * cin, dt, DEV)
    dx.copy_(S.rnd(dx0, dt).view(-1))
    ops.shortcut_a_backward_acc(S.rnd(g, dt), dx.view(n, h, w, cin))
    ref = S.rnd(dx0, dt).double()
    ref[:, ::2, ::2, :] += g[..., cpad:cpad + cin]
    assert S.same_bits(dx.view(n, h, w, cin), S.rnd(ref, dt)) and S.guard_intact(dbuf, n * h * w * cin)


@pytest.mark.parametrize("key", DT_IDS)
def test_im2col_and_weight_transpose_past_the_block_cap(key):
    from iif_amd import ops
    dt = S.DTYPES[key]
    n, cin, h, w, r, stride, pad, kp = S.IM2COL_SHAPE
    if dt == FP32:
        n = 2 * n                                                # half as many elements per vector
    img = S.act(S.hash_t(n * cin * h * w, 370, DEV), 0).view(n, cin, h, w)
    ref = S.im2col_ref(img, r, r, stride, pad, kp)
    assert ref.numel() // S.vec(dt) > 8192 * 256
    buf, out = S.guarded(ref.numel(), dt, DEV)
    ops.im2col_nchw(img.float(), r, r, stride, pad, kp, dt, out=out.view(ref.shape))
    assert S.same_bits(out.view(ref.shape), S.rnd(ref, dt)) and S.guard_intact(buf, ref.numel())
    cout, ci, rs, ldw, ldwt = S.WT_SHAPE
    wm = S.act(S.hash_t(cout * ldw, 371, DEV), 0).view(cout, ldw)
    wbuf, wt = S.guarded(ci * ldwt, dt, DEV)
    ops.weight_transpose(wm.float(), cout, ci, rs, wt.view(ci, ldwt))
    wref = torch.zeros(ci, ldwt, dtype=F64, device=DEV)
    wref[:, :cout] = wm[:, :ci].t()
    assert S.same_bits(wt.view(ci, ldwt), S.rnd(wref, dt)) and S.guard_intact(wbuf, ci * ldwt)


# ------------------------------------------------------------------------------------------------ the stem pool
def _stem_forward(x, stats, dt):
    from iif_amd import _lib
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    cnt = n * ho * wo * c
    bufs = [S.guarded(cnt, dt, DEV), S.guarded(cnt, torch.uint8, DEV), S.guarded(cnt, dt, DEV)]
    (_, y), (_, idx), (_, px) = bufs
    _lib.check(_lib.lib().iif_maxpool_bn_forward(_lib.ptr(x), _lib.dtype_code(x), _lib.ptr(stats), n, h, w, c, 3, 2, 1, _lib.ptr(y),
                                                 _lib.ptr(idx), _lib.ptr(px), _lib.stream_ptr()), "iif_maxpool_bn_forward")
    assert all(S.guard_intact(b, cnt) for b, _ in bufs)
    return (t.view(n, ho, wo, c) for t in (y, idx, px))


@pytest.mark.parametrize("key", DT_IDS)
def test_fused_stem_pool_past_the_row_cap(key):
    """iif_maxpool_bn_forward with 16 800 pooled rows against the cap of 16 384 blocks: the rows of the second trip; pooled value,
    raw value at the arg max and arg-max code exact against the reference."""
    dt = S.DTYPES[key]
    n, h, w, c = S.STEM_POOL_SHAPE
    c = c if dt == BF16 else c // 2
    x = S.act(S.hash_t(n * h * w * c, 380, DEV), 0).view(n, h, w, c)
    st = S.channel_coefs(c, 380, DEV)["stats"]
    y, idx, px = _stem_forward(S.rnd(x, dt), st.float().contiguous(), dt)
    y_ref, code, px_ref = S.stem_pool_ref(x, st, dt)
    assert S.same_bits(y, S.rnd(y_ref, dt)) and torch.equal(idx, code) and S.same_bits(px, S.rnd(px_ref, dt))


@pytest.mark.parametrize("name", list(S.POOL_FUSED_CASES))
def test_bn_backward_pool_fused_per_answer_of_the_plan(name):
    """iif_bn_backward_pool_fused, one case per answer of the planning query (XCD remap on / off, grown rows per block, a short
    last group, a row wider than 512 vectors, a block of fewer than 256 and of 256 .. 512 vectors, odd H and W, C = 128, fp32).
    Reference: the pooled gradient scattered in float64 through the kernel's own arg max, rounded to the storage type as the
    kernel rounds the gathered sum, gated by a x + b > 0, then the BN backward.  dgamma / dbeta within 6 eps l2 + 4e-6 l1 of
    the float64 sums per channel; dx per element within stream_cases.dx_bound (derivation in
    test_bn_backward_routes_that_form_their_sums).  And the existing identity: fused = pooled sums + iif_maxpool_backward +
    recompute, bit for bit."""
    from iif_amd import _lib, ops
    n, h, w, c, key, _, _ = S.POOL_FUSED_CASES[name]
    dt = S.DTYPES[key]
    salt = 400 + list(S.POOL_FUSED_CASES).index(name)
    x64 = S.act(S.hash_t(n * h * w * c, salt, DEV), 0).view(n, h, w, c)
    cf = S.channel_coefs(c, salt, DEV)
    st64, gamma64 = cf["stats"], cf["gamma"]
    x, stats, gamma = S.rnd(x64, dt), st64.float().contiguous(), gamma64.float().contiguous()
    pooled, idx, pool_x = _stem_forward(x, stats, dt)
    y_ref, code, px_ref = S.stem_pool_ref(x64, st64, dt)
    assert S.same_bits(pooled, S.rnd(y_ref, dt)) and torch.equal(idx, code) and S.same_bits(pool_x, S.rnd(px_ref, dt))
    pooled, idx, pool_x = pooled.contiguous(), idx.contiguous(), pool_x.contiguous()
    ho, wo = idx.shape[1], idx.shape[2]
    gp64 = S.act(S.hash_t(n * ho * wo * c, salt + 50, DEV), 0).view(n, ho, wo, c)
    gp = S.rnd(gp64, dt)
    m = n * h * w
    L = _lib.lib()
    ws = ops.bn_workspace(m, c, DEV)
    dxbuf, dx = S.guarded(m * c, dt, DEV)
    dg, db = nan_like(c), nan_like(c)
    _lib.check(L.iif_bn_backward_pool_fused(_lib.ptr(gp), _lib.ptr(idx), _lib.ptr(pool_x), _lib.ptr(x), _lib.dtype_code(x), n, h, w, c, ho, wo,
                                            _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(dg), _lib.ptr(db), _lib.ptr(dx), _lib.ptr(ws),
                                            ws.numel(), _lib.stream_ptr()), "iif_bn_backward_pool_fused")
    assert S.guard_intact(dxbuf, m * c)
    dx_ref, dg_ref, db_ref, (t1, t2) = S.pool_fused_ref(gp64, idx, x64, st64, gamma64, dt)
    b1, b2 = S.sum_bound(t1, dt), S.sum_bound(t2, dt)
    allowed = S.dx_bound(dx_ref, t1, x64.view(m, c), gamma64, st64[0], st64[1], b1, b2, dt)
    r_b, r_g = ratio((db.double() - db_ref).abs(), b1), ratio((dg.double() - dg_ref).abs(), b2)
    r_x = ratio((dx.view(m, c).double() - dx_ref).abs(), allowed)
    print("\n[pool_fused %s] measured / allowed: dbeta %.3f  dgamma %.3f  dx %.3f" % (name, r_b, r_g, r_x))
    assert r_b <= 1.0 and r_g <= 1.0 and r_x <= 1.0
    # the unfused route on the same tensors
    dy = nan_like(n, h, w, c, dt=dt)
    _lib.check(L.iif_maxpool_backward(_lib.ptr(gp), _lib.ptr(idx), _lib.dtype_code(gp), n, h, w, c, 3, 2, 1, _lib.ptr(dy), _lib.stream_ptr()),
               "iif_maxpool_backward")
    dg2, db2 = nan_like(c), nan_like(c)
    _lib.check(L.iif_bn_backward_relu_recompute_pooled(_lib.ptr(dy), _lib.ptr(x), _lib.dtype_code(x), m, c, _lib.ptr(stats), _lib.ptr(gamma),
                                                       _lib.ptr(dg2), _lib.ptr(db2), _lib.ptr(dy), _lib.ptr(ws), ws.numel(), _lib.ptr(gp),
                                                       _lib.ptr(pool_x), n * ho * wo, _lib.stream_ptr()), "iif_bn_backward_relu_recompute_pooled")
    assert S.same_bits(dx.view(n, h, w, c), dy) and S.same_bits(dg, dg2) and S.same_bits(db, db2)
