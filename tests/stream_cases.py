"""Cases, inputs and float64 references of the size-selected paths of the streaming kernels (bn.hip stream_grid, pool_misc.hip
sblocks, optim.hip rms_blocks, se.hip stream_blocks, the row grid of the fused stem pool, the row groups of
iif_bn_backward_pool_fused).  Shared by tests/test_stream_cases_host.py (no device), tests/test_stream_paths_gpu.py and its
worker tests/stream_env_worker.py.

Inputs come from the fixed integer hash of tests/ce_cases.py (restated on torch integers so that a 17 M element tensor is made
on the device; the host test holds the two to each other) and are chosen so that the arithmetic is EXACT:
  activations, residuals, gradients   k / 64, integer |k| <= 255                  (8 significant bits: exact in bf16)
  a, a2, k1, k3                       non-zero multiples of 1/8 in [-2, 2]
  invstd                              +-2^e, e in -3 .. 1 (a subset of the above: gamma = k1 / invstd and the sums that give
                                      k2, k3 are then exact too)
  b, b2, mean, k2, SE offsets         multiples of 1/64 in [-1, 1]
  excitations                         multiples of 1/16 in (0, 1]
Every intermediate of  fmaf(a, x, b) (+ r | + fmaf(a2, r, b2)),  (a x + b) e + ...,  k1 (d - k2 - (x - mean) k3)  then has
fewer than 24 significant bits: the fp32 result is the exact value whatever the compiler contracts, the bf16 result its
round-to-nearest-even, every ReLU decision is determined, and the device result can be held to the float64 reference bit for
bit with no element left out."""
import numpy as np
import torch

from iif_amd import _lib

F64 = torch.float64
BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = {"bf16": BF16, "f32": FP32}


def vec(dt):
    return 8 if dt == BF16 else 4


# ------------------------------------------------------------------------------------------------ the planning query
FAMILY = {"bn": 0, "grid": 1, "rms": 2, "se": 3, "stem_rows": 4, "pool_fused": 5}


def plan(family, work, w=0, cv=0):
    """iif_stream_plan: (blocks, U, non-temporal stores, trips), or for "pool_fused" (groups, rows per block, remap, rows of
    the last group).  Host only."""
    out = np.zeros(4, dtype=np.int32)
    _lib.check(_lib.lib().iif_stream_plan(FAMILY[family], int(work), int(w), int(cv), out.ctypes.data), "iif_stream_plan")
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------------------------------------ cases
# BN normalisation passes, [M, C]: name -> (M, C in bf16 (fp32: C / 2, the same vectors), U, total % (256 U), channel vectors)
BN_CASES = {
    "cap3000": (375, 64, 1, 184, 8),
    "u1_top": (16383, 512, 1, 192, 64),
    "u2_a": (16387, 512, 2, 192, 64),
    "u2_b": (16389, 512, 2, 320, 64),
    "u4_a": (32771, 512, 4, 192, 64),
    "u4_b": (32779, 512, 4, 704, 64),
    "u2_nf": (174763, 48, 2, 2, 6),
    "u4_nf": (349527, 48, 4, 10, 6),
}
BN_TABLE = [n for n in BN_CASES if n != "cap3000"]            # the cases of the issue's table
BN_SUM_CASES = ("u2_b", "u4_b", "u4_nf")                      # the routes that form their own sums run on these only


def bn_shape(name, dt):
    m, c = BN_CASES[name][:2]
    return m, c if dt == BF16 else c // 2


def bn_vectors(name):
    m, c = BN_CASES[name][:2]
    return m * c // 8


# grid-stride kernels past their cap: name -> (family, work items as the entry counts them, cap in work items)
N_CAST = 2097152 + 1003
N_OPT = 8388608 + 4099
SE_SHAPE = (5, 58 * 58, 512)                 # (n, hw, C in bf16)
AVG_SHAPE = (10, 58 * 58, 512)
MAXPOOL_SHAPE = (4, 257, 257, 64)            # k = 3, stride 1, pad 1: as many output as input vectors
SHORTCUT_SHAPE = (65, 31, 33, 120, 248)      # n, h, w, cin, cout
IM2COL_SHAPE = (9, 3, 225, 223, 7, 2, 3, 160)   # n, cin, h, w, r (= s), stride, pad, kp
WT_SHAPE = (1030, 2047, 1, 2048, 1040)       # cout, cin, rs, ldw, ldwt
STEM_POOL_SHAPE = (300, 112, 4, 8)           # n, h, w, C in bf16: 16 800 pooled rows


def grid_cases():
    n, hw, c = SE_SHAPE
    na, hwa, ca = AVG_SHAPE
    mn, mh, mw, mc = MAXPOOL_SHAPE
    sn, sh, sw, sci, sco = SHORTCUT_SHAPE
    sho, swo = (sh + 1) // 2, (sw + 1) // 2
    i_n, i_c, i_h, i_w, i_r, i_s, i_p, i_kp = IM2COL_SHAPE
    i_ho, i_wo = (i_h + 2 * i_p - i_r) // i_s + 1, (i_w + 2 * i_p - i_r) // i_s + 1
    return {
        "cast": ("grid", N_CAST, 8192 * 256),
        "sgd": ("grid", N_OPT // 4 + 1, 8192 * 256),
        "rmsprop": ("rms", N_OPT // 4 + 1, 8192 * 256),
        "se_stream": ("se", n * hw * c // 8, 4096 * 256),
        "avgpool_bwd": ("grid", na * hwa * ca // 8, 8192 * 256),
        "maxpool": ("grid", mn * mh * mw * mc // 8, 8192 * 256),
        "shortcut_fwd": ("grid", sn * sho * swo * sco, 8192 * 256),
        "shortcut_bwd": ("grid", sn * sho * swo * sci, 8192 * 256),
        "im2col": ("grid", i_n * i_ho * i_wo * i_kp // 8, 8192 * 256),
        "weight_transpose": ("grid", WT_SHAPE[1] * WT_SHAPE[4], 8192 * 256),
        "stem_pool_rows": ("stem_rows", STEM_POOL_SHAPE[0] * (STEM_POOL_SHAPE[1] // 2), 16384),
    }


# iif_bn_backward_pool_fused: name -> (n, h, w, c, dtype, (remap, rows per block grown beyond 8, short last group),
#                                      pipeline class of the LAST block: vectors < 256 / 256 .. 512 / > 512)
POOL_FUSED_CASES = {
    "remap_on": (8, 32, 16, 64, "bf16", (1, True, False), "long"),
    "remap_off_short": (3, 18, 22, 64, "bf16", (0, True, True), "long"),
    "wide_row": (1, 16, 112, 64, "bf16", (0, False, False), "long"),
    "lt256": (1, 9, 3, 64, "bf16", (0, True, True), "lt256"),
    "mid": (1, 17, 3, 64, "bf16", (0, True, True), "mid"),
    "odd_hw": (2, 17, 23, 64, "bf16", (0, True, True), "long"),
    "c128": (2, 8, 8, 128, "bf16", (0, True, False), "long"),
    "f32_short": (3, 18, 22, 64, "f32", (0, False, True), "long"),
    "f32_remap_on": (8, 32, 16, 32, "f32", (1, True, False), "long"),
}


# ------------------------------------------------------------------------------------------------ inputs
_M64 = (1 << 64) - 1


def _s64(v):
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


def _lsr(v, k):
    return (v >> k) & ((1 << (64 - k)) - 1)


def hash_t(n, salt, device="cpu"):
    """ce_cases._hash on torch int64 (two's complement of the same 64 bits), made on ``device``."""
    v = torch.arange(n, dtype=torch.int64, device=device) + _s64(salt << 40)
    v = v + _s64(0x9E3779B97F4A7C15)
    v = (v ^ _lsr(v, 30)) * _s64(0xBF58476D1CE4E5B9)
    v = (v ^ _lsr(v, 27)) * _s64(0x94D049BB133111EB)
    return v ^ _lsr(v, 31)


def _bits(h, shift, n):
    return _lsr(h, shift) & ((1 << n) - 1)


def act(h, shift):
    """k / 64, |k| <= 255, as float64"""
    return (_bits(h, shift, 9) - 256).clamp_min(-255).to(F64) / 64.0


def coef_a(h, shift):
    """non-zero multiples of 1/8 in [-2, 2]"""
    j = _bits(h, shift, 5)
    return (j - 16 + (j >= 16).to(torch.int64)).to(F64) / 8.0


def coef_b(h, shift):
    """multiples of 1/64 in [-1, 1]"""
    return (_bits(h, shift, 8) % 129 - 64).to(F64) / 64.0


def coef_pow2(h, shift):
    """+-2^e, e in -3 .. 1"""
    e = _bits(h, shift, 3) % 5 - 3
    s = 1 - 2 * _bits(h, shift + 3, 1)
    return s.to(F64) * torch.pow(torch.tensor(2.0, dtype=F64, device=h.device), e.to(F64))


def excite(h, shift):
    """multiples of 1/16 in (0, 1]"""
    return (_bits(h, shift, 4) + 1).to(F64) / 16.0


COUNT = float(1 << 20)          # total_count of iif_bn_backward_apply_sums: a power of two


def channel_coefs(c, salt, device):
    """float64 per-channel rows: stats [4, c] (mean, invstd, a, b), stats2 [4, c], k1, k2, k3, gamma = k1 / invstd, and the
    (local, total) sums of iif_bn_backward_apply_sums: total = (k2, k3 / invstd) * COUNT, local arbitrary (it is only copied)."""
    h = hash_t(c, salt + 7000, device)
    g = hash_t(c, salt + 7001, device)
    mean, invstd = coef_b(h, 0), coef_pow2(h, 8)
    stats = torch.stack([mean, invstd, coef_a(h, 12), coef_b(h, 17)])
    stats2 = torch.stack([coef_b(h, 25), coef_pow2(h, 33), coef_a(h, 37), coef_b(h, 42)])
    k1, k2, k3 = coef_a(g, 0), coef_b(g, 5), coef_a(g, 13)
    total = torch.stack([k2 * COUNT, k3 / invstd * COUNT])
    local = torch.stack([act(g, 18) * 3.0 + 0.1, act(g, 27) * 0.7 - 0.3])
    return {"stats": stats, "stats2": stats2, "k1": k1, "k2": k2, "k3": k3, "gamma": k1 / invstd, "total": total, "local": local}


def bn_inputs(m, c, salt, device):
    """float64 [m, c] x, r, gy of one BN case + channel_coefs."""
    h = hash_t(m * c, salt, device).view(m, c)
    d = channel_coefs(c, salt, device)
    d.update(x=act(h, 0), r=act(h, 9), gy=act(h, 18))
    return d


def bn_case_inputs(name, dt, device):
    m, c = bn_shape(name, dt)
    return bn_inputs(m, c, 100 + sorted(BN_CASES).index(name), device)


def rnd(t, dt):
    """float64 -> the storage type (every value here is exact in fp32, so this is ONE rounding)"""
    return t if dt == F64 else t.to(FP32).to(dt)


def pack_bits(mask, v):
    """[.., c] bool -> one byte per v channels, bit k = channel k of the vector"""
    w = 2 ** torch.arange(v, device=mask.device, dtype=torch.int32)
    return (mask.reshape(-1, v).to(torch.int32) * w).sum(1).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ float64 references
def bn_apply_ref(x, stats, relu, r=None, stats2=None):
    """(y, decision mask) of iif_bn_apply; all float64."""
    t = stats[2] * x + stats[3]
    if r is not None:
        t = t + ((stats2[2] * r + stats2[3]) if stats2 is not None else r)
    return (t.clamp_min(0.0) if relu else t), t > 0


def bn_bwd_apply_ref(gy, x, mask, k1, k2, k3, mean):
    """(dx, masked gradient) of the normalisation pass of the BN backward; mask None: no ReLU."""
    d = gy if mask is None else torch.where(mask, gy, torch.zeros_like(gy))
    return k1 * (d - k2 - (x - mean) * k3), d


def bn_backward_ref(gy, x, mask, gamma, mean, invstd):
    """Training-mode BN backward from its definition: (dx, dgamma, dbeta, the per-channel terms of the two sums)."""
    d = gy if mask is None else torch.where(mask, gy, torch.zeros_like(gy))
    xhat = (x - mean) * invstd
    t2 = d * xhat
    s1, s2 = d.sum(0), t2.sum(0)
    m = x.shape[0]
    dx = gamma * invstd * (d - s1 / m - xhat * (s2 / m))
    return dx, s2, s1, (d, t2)


def sum_bound(terms, dt, dim=0):
    """The project's bound of a per-channel fp32 sum against float64 (tests/test_layers_gpu.py): 6 eps l2 + 4e-6 l1."""
    eps = 2.0 ** -24 if dt == FP32 else 2.0 ** -9
    return 6 * eps * terms.pow(2).sum(dim).sqrt() + 4e-6 * terms.abs().sum(dim)


def dx_bound(dx_ref, d, x, gamma, mean, invstd, b1, b2, dt):
    """Per-element bound of dx = k1 (d - k2 - (x - mean) k3), k1 = gamma invstd, k2 = s1 / m, k3 = (s2 / m) invstd, where the
    device's sums are within b1 (s1) and b2 (s2) of the float64 sums:
        |k1| (b1 / m + |x - mean| invstd b2 / m)                  the coefficient errors carried through,
      + 8 * 2^-24 |k1| (|d| + |k2| + |x - mean| |k3|)              the fp32 roundings of k1, k2, k3 and of the four operations,
      + eps_store |dx|                                           one rounding to the storage type: bf16 keeps 8 significant bits,
                                                                 so round-to-nearest moves a value by at most half a unit of the
                                                                 eighth, 2^-8 |dx| (fp32: in the line above)."""
    m = x.shape[0]
    k1 = (gamma * invstd).abs()
    xm = (x - mean).abs()
    s1, s2 = d.sum(0), (d * (x - mean) * invstd).sum(0)
    carried = k1 * (b1 / m + xm * invstd.abs() * b2 / m)
    arith = 8 * 2.0 ** -24 * k1 * (d.abs() + (s1 / m).abs() + xm * (s2 / m * invstd).abs())
    return carried + arith + (2.0 ** -8 if dt == BF16 else 0.0) * dx_ref.abs()


def se_apply_ref(x, stats, e, r=None, stats2=None):
    """x, r [n, hw, c], e [n, c] -> (y, mask) of iif_se_apply (always ReLU)."""
    t = (stats[2] * x + stats[3]) * e[:, None, :]
    if r is not None:
        t = t + ((stats2[2] * r + stats2[3]) if stats2 is not None else r)
    return t.clamp_min(0.0), t > 0


def se_form_ref(g, e, o):
    return g * e[:, None, :] + o[:, None, :]


def maxpool_ref(x, k, stride, pad):
    """x [N, H, W, C] -> (y, code): the first maximum in (kh, kw) scan order, code = kh * k + kw."""
    n, h, w, c = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    z = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad), value=float("-inf"))
    best = torch.full((n, ho, wo, c), float("-inf"), dtype=x.dtype, device=x.device)
    code = torch.zeros((n, ho, wo, c), dtype=torch.uint8, device=x.device)
    for kh in range(k):
        for kw in range(k):
            v = z[:, kh:kh + (ho - 1) * stride + 1:stride, kw:kw + (wo - 1) * stride + 1:stride, :]
            better = v > best
            best = torch.where(better, v, best)
            code = torch.where(better, torch.full_like(code, kh * k + kw), code)
    return best, code


def maxpool_scatter(g, code, in_hw, k, stride, pad):
    """Backward of a max pool through given arg-max codes: g [N, Ho, Wo, C] -> [N, H, W, C]."""
    n, ho, wo, c = g.shape
    h, w = in_hw
    cd = code.long()
    hh = torch.arange(ho, device=g.device).view(1, ho, 1, 1) * stride - pad + cd // k
    ww = torch.arange(wo, device=g.device).view(1, 1, wo, 1) * stride - pad + cd % k
    nn_ = torch.arange(n, device=g.device).view(n, 1, 1, 1)
    cc = torch.arange(c, device=g.device).view(1, 1, 1, c)
    flat = ((nn_ * h + hh) * w + ww) * c + cc
    out = torch.zeros(n * h * w * c, dtype=g.dtype, device=g.device)
    out.index_add_(0, flat.reshape(-1), g.reshape(-1))
    return out.view(n, h, w, c)


def gather_at_code(x, code, k, stride, pad):
    """x [N, H, W, C] at the arg max of every window: [N, Ho, Wo, C]."""
    n, ho, wo, c = code.shape
    cd = code.long()
    hh = torch.arange(ho, device=x.device).view(1, ho, 1, 1) * stride - pad + cd // k
    ww = torch.arange(wo, device=x.device).view(1, 1, wo, 1) * stride - pad + cd % k
    nn_ = torch.arange(n, device=x.device).view(n, 1, 1, 1).expand_as(cd)
    cc = torch.arange(c, device=x.device).view(1, 1, 1, c).expand_as(cd)
    return x[nn_, hh, ww, cc]


def stem_pool_ref(x, stats, dt):
    """iif_maxpool_bn_forward (3 / 2 / 1): the max over relu(a x + b) rounded to the storage type -> (y, code, pool_x)."""
    t = rnd((stats[2] * x + stats[3]).clamp_min(0.0), dt).to(F64)
    y, code = maxpool_ref(t, 3, 2, 1)
    return y, code, gather_at_code(x, code, 3, 2, 1)


def pool_fused_ref(gp, code, x, stats, gamma, dt):
    """iif_bn_backward_pool_fused: the pooled gradient scattered through ``code``, ROUNDED to the storage type (dt None: not
    rounded), gated by a x + b > 0, then the BN backward -> (dx, dgamma, dbeta, terms).  (The kernel forms its two column sums
    from the pooled gradients themselves, i.e. before that rounding; one rounding per element is what the eps l2 term of
    sum_bound stands for.)"""
    n, h, w, c = x.shape
    gy = maxpool_scatter(gp, code, (h, w), 3, 2, 1)
    if dt is not None:
        gy = rnd(gy, dt).to(F64)
    m = n * h * w
    x2 = x.reshape(m, c)
    mask = (stats[2] * x2 + stats[3]) > 0
    return bn_backward_ref(gy.reshape(m, c), x2, mask, gamma, stats[0], stats[1])


def sgd_ref(p, g, buf, lr, momentum, wd, nesterov):
    """One step of the recurrence of iif_sgd_step in float64 (in place)."""
    d = g + wd * p
    buf.mul_(momentum).add_(d)
    p.sub_(lr * ((d + momentum * buf) if nesterov else buf))


def rmsprop_ref(p, g, sq, buf, ga, lr, alpha, eps, wd, momentum):
    """One step of torch.optim.RMSprop's recurrence in float64 (in place); buf None: no momentum, ga None: not centred."""
    g = g + wd * p
    sq.mul_(alpha).add_((1 - alpha) * g * g)
    if ga is not None:
        ga.add_((1 - alpha) * (g - ga))
        avg = (sq - ga * ga).sqrt() + eps
    else:
        avg = sq.sqrt() + eps
    if buf is not None:
        buf.mul_(momentum).add_(g / avg)
        p.sub_(lr * buf)
    else:
        p.sub_(lr * (g / avg))


def im2col_ref(img, r, s, stride, pad, kp):
    """img [N, Cin, H, W] -> [N, Ho, Wo, kp], column (r * S + s) * Cin + c, zero padded to kp."""
    n, cin, h, w = img.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    z = torch.nn.functional.pad(img, (pad, pad, pad, pad))
    out = torch.zeros(n, ho, wo, kp, dtype=img.dtype, device=img.device)
    for a in range(r):
        for b in range(s):
            v = z[:, :, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride]
            out[..., (a * s + b) * cin:(a * s + b + 1) * cin] = v.permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------------ device comparisons
# (shared by tests/test_stream_paths_gpu.py and tests/stream_env_worker.py; everything below needs the GPU)
GUARD = 4096


def guarded(numel, dt, device):
    """(buffer, its first ``numel`` elements): NaN (0xAA for bytes) everywhere, GUARD elements behind the output."""
    buf = torch.empty(numel + GUARD, dtype=dt, device=device)
    buf.fill_(0xAA if dt == torch.uint8 else float("nan"))
    return buf, buf[:numel]


def _int_view(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def guard_intact(buf, numel):
    fresh, _ = guarded(0, buf.dtype, buf.device)
    return torch.equal(_int_view(buf[numel:]), _int_view(fresh))


def same_bits(got, ref):
    """bit identity over every element"""
    return got.shape == ref.shape and torch.equal(_int_view(got.contiguous()), _int_view(ref.contiguous()))


def check_bn_apply_exact(name, dt, device):
    """iif_bn_apply over relu x residual x bits against the float64 reference, bit for bit -> list of failed variants."""
    from iif_amd import ops
    m, c = bn_shape(name, dt)
    v = vec(dt)
    d = bn_case_inputs(name, dt, device)
    x, r = rnd(d["x"], dt), rnd(d["r"], dt)
    stats, stats2 = d["stats"].float(), d["stats2"].float()
    bad = []
    for res in ("none", "plain", "normalised"):
        rr = None if res == "none" else d["r"]
        s2 = d["stats2"] if res == "normalised" else None
        for relu in (True, False):
            y_ref, mask = bn_apply_ref(d["x"], d["stats"], relu, rr, s2)
            y_ref, bits_ref = rnd(y_ref, dt), pack_bits(mask, v)
            for with_bits in (True, False):
                ybuf, y = guarded(m * c, dt, device)
                bbuf, bits = guarded(m * c // v, torch.uint8, device)
                ops.bn_apply(x, stats, y.view(m, c), relu=relu, residual=None if rr is None else r,
                             residual_stats=None if s2 is None else stats2, relu_bits=bits if with_bits else None)
                ok = same_bits(y.view(m, c), y_ref) and guard_intact(ybuf, m * c) and guard_intact(bbuf, m * c // v)
                # the decision bytes are written by the ReLU forms only; otherwise the buffer stays as it was
                ok = ok and (same_bits(bits, bits_ref) if (with_bits and relu) else bool((bits == 0xAA).all()))
                if not ok:
                    bad.append(("apply", name, res, relu, with_bits))
    return bad


def check_bn_backward_exact(name, dt, device):
    """iif_bn_backward_apply_sums over mask x gmasked, and once in place, bit for bit -> list of failed variants."""
    from iif_amd import ops
    m, c = bn_shape(name, dt)
    v = vec(dt)
    d = bn_case_inputs(name, dt, device)
    x, gy = rnd(d["x"], dt), rnd(d["gy"], dt)
    stats = d["stats"].float()
    y64, mask = bn_apply_ref(d["x"], d["stats"], True)
    ymask, bits = rnd(y64, dt), pack_bits(mask, v)
    gamma, local, total = d["gamma"].float(), d["local"].float().contiguous(), d["total"].float().contiguous()
    assert torch.equal(gamma.double(), d["gamma"]) and torch.equal(total.double(), d["total"])
    bad = []

    def run(mode, with_gm, in_place=False):
        mk = None if mode == "none" else mask
        dx_ref, gm_ref = bn_bwd_apply_ref(d["gy"], d["x"], mk, d["k1"], d["k2"], d["k3"], d["stats"][0])
        dx_ref, gm_ref = rnd(dx_ref, dt), rnd(gm_ref, dt)
        dxbuf, dx = guarded(m * c, dt, device)
        gmbuf, gm = guarded(m * c, dt, device)
        src = gy
        if in_place:
            dx.copy_(gy.view(-1))
            src = dx.view(m, c)
        dg, db = torch.full((c,), float("nan"), device=device), torch.full((c,), float("nan"), device=device)
        coef = torch.full((3, c), float("nan"), device=device)
        ops.bn_backward_apply_sums(src, ymask if mode == "y" else None, x, stats, gamma, local, total, COUNT, dg, db, dx.view(m, c),
                                   coef, gmasked=gm.view(m, c) if with_gm else None, relu_bits=bits if mode == "bits" else None)
        ok = same_bits(dx.view(m, c), dx_ref) and guard_intact(dxbuf, m * c) and guard_intact(gmbuf, m * c)
        ok = ok and (same_bits(gm.view(m, c), gm_ref) if with_gm else bool(torch.isnan(gm).all()))
        ok = ok and same_bits(db, local[0]) and same_bits(dg, local[1])
        ok = ok and same_bits(coef, torch.stack([d["k1"], d["k2"], d["k3"]]).float())
        if not ok:
            bad.append(("backward", name, mode, with_gm, in_place))

    for mode in ("none", "y", "bits"):
        for with_gm in (False, True):
            run(mode, with_gm)
    run("bits", True, in_place=True)
    return bad
