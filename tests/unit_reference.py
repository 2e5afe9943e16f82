"""Per-unit float64 reference of the native ResNet training step (a test helper module, not a conftest).

Whole-network comparisons of two bf16 routes cannot get tighter than 1e-2 .. 3e-1 (a one-ulp difference flips ReLU decisions
and passes through BN-backward cancellation at every layer).  This module compares ONE conv+BN unit at a time instead: every
unit is evaluated in float64 from the inputs the real step itself used - its stored source, its bf16 weights, the statistics
it normalised with, its ReLU decisions and the gradient that arrived at it - so nothing compounds over layers and what is
left is fp32 accumulation and one rounding of each stored output.

``StepCapture`` wraps ``_Plan._unit_backward`` (clone of ``gy`` before the call, clone of the returned data gradient after
it, both on the stream current at the call); forward tensors stay valid after the step.  ``check_step`` returns
``{unit name: {metric: value}}``; ``failures`` compares that with a table of bounds.

Metrics (all dimensionless):
  mean    max |mean - mean_ref| * invstd_ref        invstd  max |invstd / invstd_ref - 1|
  x       max |x - x_ref| / max |x_ref| (stored convolution output, where stored)
  y       max |y - y_ref| / max |y_ref| (activated output), y_l2 its relative L2
  bits    fraction of stored ReLU bits that disagree with the stored y > 0 (exactly 0 expected)
  dgamma, dbeta, dw   relative L2 of the unit's parameter gradients in the arena
  dw_rdx  (units whose weight gradient the engine forms from its stored dx) relative L2 of dw against the weight gradient
          of the float64 dx rounded to the compute type: the weight-gradient kernel's own error, without the rounding
          of dx that every bf16 route stores
  dgrad   relative L2 of the unit's data gradient (the block-input gradient for a block's first unit: residual included),
          dgrad_max its max-abs error over the max; both gated by the upstream unit's ReLU (producers may store it gated)
  pool, pool_idx (stem of an ImageNet network): max-pooled output, and how far below its window's maximum the chosen
          element lies (relative to the window maximum)

Squeeze-and-excitation blocks (y = relu((a x + b) e + residual), e = sigmoid(W2 relu(W1 mean_hw(a x + b)))) add one entry
``<block>.se`` per block.  ``StepCapture`` also wraps ``_Plan._se_backward`` (the block-output gradient g as it arrives, the
same buffer after the in-place mask, the returned G), and every stage is evaluated from what the step stored for the stage
before it (``b["se"]``: sums, q, h, e, s1, s2, dz2, dz1, o), as ``check_head`` does, so one ReLU or sigmoid decision never
compounds:
  se_sums, se_s1, se_s2   the per-sample sums over the pixels of the stored x, of the masked g~ = g [y > 0] and of g~ x: worst
          |error| / bound per element, bound max((HW + 16) 2^-24 sum |term|, 4 |float32 CPU - float64|) (<= 1 passes)
  se_q    max |q - q_ref| / max |q_ref| from the stored sums and the unit's statistics (1e-5)
  se_h    max |h - h_ref| / max(1, max |h_ref|) from the stored q and the fp32 W1 (2e-5);  se_e  max |e - e_ref| from the
          stored h and the fp32 W2 (2e-6)
  y, y_l2, bits (under the last unit's name)  relu((a x + b) e + residual) from the stored x, statistics and e
  se_gmask   elements of the masked g left in place that are not g [y > 0] (exactly 0)
  se_dz2, se_dz1, se_o, se_dw1, se_dw2   relative L2 of each stage from the stored result of the stage before it, over
          max(2e-5, 4 x the relative L2 of the same stage in float32 on the CPU) (<= 1 passes)
  se_pad  non-zero elements in the pad columns of both SE gradient rows and the arena padding behind them (exactly 0)
  se_G    max |G - round(g~ e + o)| / max |G| from the masked g, the stored e and o
The last unit of an SE block then takes the captured G with no ReLU mask, and the identity path (identity, option-A shortcut
or the shortcut unit) takes the masked g.  ``SE_GATE`` keeps max |o| / max |G| per block from the float64 chain alone: how
visible the gate path is under one rounding of G.
"""
import contextlib

import torch
import torch.nn.functional as F

F64 = torch.float64


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


# ------------------------------------------------------------------ convolutions (NHWC activations, OIHW weights), float64
def _out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def conv_fwd(x, w, stride, pad, groups=1):
    """x [N, H, W, C], w [Co, C / groups, k, k] -> [N, Ho, Wo, Co] (matrix products over im2col columns)."""
    n, h, wd, c = x.shape
    co, cg, k, _ = w.shape
    ho, wo = _out_hw(h, wd, k, stride, pad)
    if k == 1 and pad == 0 and groups == 1:
        xs = x[:, ::stride, ::stride, :].reshape(-1, c)
        return (xs @ w.reshape(co, c).t()).view(n, ho, wo, co)
    cols = F.unfold(nchw(x), k, padding=pad, stride=stride).view(n, groups, cg * k * k, ho * wo)
    out = torch.matmul(w.reshape(1, groups, co // groups, cg * k * k), cols)          # [N, G, Co/G, L]
    return out.reshape(n, co, ho, wo).permute(0, 2, 3, 1)


def conv_wgrad(x, dy, wshape, stride, pad, groups=1):
    """d(loss)/dW [Co, C / groups, k, k] of conv_fwd(x, W) given dy [N, Ho, Wo, Co]."""
    n, h, wd, c = x.shape
    co, cg, k, _ = wshape
    ho, wo = dy.shape[1], dy.shape[2]
    if k == 1 and pad == 0 and groups == 1:
        xs = x[:, ::stride, ::stride, :].reshape(-1, c)
        return (dy.reshape(-1, co).t() @ xs).view(co, c, 1, 1)
    cols = F.unfold(nchw(x), k, padding=pad, stride=stride).view(n, groups, cg * k * k, ho * wo)
    d = nchw(dy).reshape(n, groups, co // groups, ho * wo)
    return torch.einsum("ngol,ngkl->gok", d, cols).reshape(co, cg, k, k)


def conv_dgrad(dy, w, in_shape, stride, pad, groups=1):
    """d(loss)/dx [N, H, W, C] of conv_fwd(x, w) given dy [N, Ho, Wo, Co]."""
    n, h, wd, c = in_shape
    co, cg, k, _ = w.shape
    ho, wo = dy.shape[1], dy.shape[2]
    if k == 1 and pad == 0 and groups == 1:
        dx = torch.zeros((n, h, wd, c), dtype=dy.dtype, device=dy.device)
        dx[:, ::stride, ::stride, :] = (dy.reshape(-1, co) @ w.reshape(co, c)).view(n, ho, wo, c)
        return dx
    d = nchw(dy).reshape(n, groups, co // groups, ho * wo)
    cols = torch.matmul(w.reshape(1, groups, co // groups, cg * k * k).transpose(2, 3), d)   # [N, G, cg*k*k, L]
    return nhwc(F.fold(cols.reshape(n, c * k * k, ho * wo), (h, wd), k, padding=pad, stride=stride))


# ------------------------------------------------------------------ batch norm (training mode), float64
def bn_stats(x, eps=1e-5):
    """Per-channel batch mean and 1 / sqrt(biased variance + eps) of x [..., C]."""
    x2 = x.reshape(-1, x.shape[-1])
    mean = x2.mean(0)
    var = (x2 - mean).square().mean(0)
    return mean, (var + eps).rsqrt()


def bn_act(x, a, b, res=None, relu=True):
    """y = act(a * x + b [+ res]) with the affine a = gamma * invstd, b = beta - mean * a of a statistics block."""
    pre = x * a + b
    if res is not None:
        pre = pre + res
    return pre.clamp_min(0) if relu else pre


def bn_backward(gy, mask, xhat, gamma, invstd, gy_sums=None):
    """BN backward with the statistics of the step: gt = gy * mask (mask None: no ReLU),
    dgamma = sum gt xhat, dbeta = sum gt, dx = gamma invstd (gt - mean(gt) - xhat mean(gt xhat)).
    gy_sums: the gradient the two sums are formed from where that is not gy itself (the stem behind the max pool: the sums
    come from the pooled gradients, unrounded, the normalisation pass from their gathered sum rounded to the storage type).
    Returns (dx, dgamma, dbeta, gt)."""
    c = gy.shape[-1]
    gt = gy if mask is None else gy * mask
    g2, xh = gt.reshape(-1, c), xhat.reshape(-1, c)
    m = g2.shape[0]
    gs = g2 if gy_sums is None else (gy_sums if mask is None else gy_sums * mask).reshape(-1, c)
    dbeta = gs.sum(0)
    dgamma = (gs * xh).sum(0)
    dx = (gamma * invstd) * (g2 - dbeta / m - xh * (dgamma / m))
    return dx.view(gt.shape), dgamma, dbeta, gt


def shortcut_a_fwd(x, cout):
    """Option-A shortcut (resnet_cifar.py LambdaLayer): x[:, ::2, ::2] zero-padded by (cout - cin) / 2 channels per side."""
    n, h, w, cin = x.shape
    p = (cout - cin) // 2
    out = torch.zeros((n, (h + 1) // 2, (w + 1) // 2, cout), dtype=x.dtype, device=x.device)
    out[..., p:p + cin] = x[:, ::2, ::2, :]
    return out


def shortcut_a_bwd(g, in_shape):
    n, h, w, cin = in_shape
    p = (g.shape[-1] - cin) // 2
    dx = torch.zeros(in_shape, dtype=g.dtype, device=g.device)
    dx[:, ::2, ::2, :] = g[..., p:p + cin]
    return dx


# ------------------------------------------------------------------ squeeze-and-excitation around a block's last BN
# o = a x + b (the last BN of the block), e = sigmoid(W2 relu(W1 mean_hw(o))), y = relu(o e + residual).  Every function is one
# stage of the engine's SE forward / backward and works in the dtype of its operands (float64 for the reference, float32 on the
# CPU for the error a stage has by itself).  x, g: [N, H, W, C]; everything else [N, C] / [N, hidden]; W1 [hidden, C],
# W2 [C, hidden].
def se_squeeze(x):
    """Per-sample channel sums over the pixels."""
    return x.sum((1, 2))


def se_q(sums, a, b, hw):
    """mean_hw(a x + b): the BN affine commutes with the mean."""
    return a * sums / hw + b


def se_h(q, w1):
    return (q @ w1.t()).clamp_min(0)


def se_e(h, w2):
    return torch.sigmoid(h @ w2.t())


def se_apply(x, a, b, e, res=None):
    """y = relu((a x + b) e [+ res])."""
    pre = (x * a + b) * e[:, None, None, :]
    if res is not None:
        pre = pre + res
    return pre.clamp_min(0)


def se_backward_sums(gt, x):
    """S1 = sum_hw g~, S2 = sum_hw g~ x of the masked block-output gradient g~ = g [y > 0]."""
    return gt.sum((1, 2)), (gt * x).sum((1, 2))


def se_dz2(s1, s2, a, b, e):
    """de = sum_hw g~ (a x + b) = a S2 + b S1, through the sigmoid."""
    return (a * s2 + b * s1) * e * (1 - e)


def se_dz1(dz2, w2, h):
    return (dz2 @ w2) * (h > 0).to(dz2.dtype)


def se_offset(dz1, w1, hw):
    """The gradient that reaches every pixel of the BN output through the squeeze."""
    return (dz1 @ w1) / hw


def se_dw(dz, v):
    """dW1 = dz1^T q, dW2 = dz2^T h."""
    return dz.t() @ v


def se_form(gt, e, o):
    """G = d(loss) / d(BN output) = g~ e + o."""
    return gt * e[:, None, None, :] + o[:, None, None, :]


def maxpool_windows(y, k=3, stride=2, pad=1):
    """[N, Ho, Wo, C, k*k] candidates of every pooling window (-inf outside the image), code kh * k + kw."""
    z = F.pad(nchw(y), (pad, pad, pad, pad), value=float("-inf"))
    win = z.unfold(2, k, stride).unfold(3, k, stride)                 # [N, C, Ho, Wo, k, k]
    return win.permute(0, 2, 3, 1, 4, 5).reshape(*win.shape[:1], win.shape[2], win.shape[3], win.shape[1], k * k)


def maxpool_scatter(g, idx, in_hw, k=3, stride=2, pad=1):
    """Backward of a max pool whose arg max codes (kh * k + kw, per output element) are ``idx``: g [N, Ho, Wo, C] -> [N, H, W, C]."""
    n, ho, wo, c = g.shape
    h, w = in_hw
    code = idx.long()
    hh = torch.arange(ho, device=g.device).view(1, ho, 1, 1) * stride - pad + code // k
    ww = torch.arange(wo, device=g.device).view(1, 1, wo, 1) * stride - pad + code % k
    nn_ = torch.arange(n, device=g.device).view(n, 1, 1, 1)
    cc = torch.arange(c, device=g.device).view(1, 1, 1, c)
    flat = ((nn_ * h + hh) * w + ww) * c + cc
    out = torch.zeros(n * h * w * c, dtype=g.dtype, device=g.device)
    out.index_add_(0, flat.reshape(-1), g.reshape(-1))
    return out.view(n, h, w, c)


def unpack_bits(bits, dt, shape):
    """ReLU decision bits of the engine (one byte per 16-byte channel vector: 8 bf16 / 4 fp32 channels, bit k = channel k)."""
    vec = 8 if dt == torch.bfloat16 else 4
    b = (bits.view(-1, 1).int() >> torch.arange(vec, device=bits.device).view(1, vec)) & 1
    return b.view(shape).bool()


# ------------------------------------------------------------------ metrics
def rel_l2(a, b):
    a, b = a.to(F64), b.to(F64)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def rel_max(a, b):
    a, b = a.to(F64), b.to(F64)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


# ------------------------------------------------------------------ capture harness
class StepCapture(object):
    """Records, per unit, the gradient that arrived at ``_Plan._unit_backward`` (``gy``, cloned before the call), the data
    gradient it returned (``out``, cloned after it) and whether the call went the BN3-algebra way (``alg``: the fused sums
    waiting for this unit came with their rows, ``_bn3_algebra``), and per SE block what went into and came out of
    ``_Plan._se_backward`` (``se_key``)."""

    def __init__(self):
        self.records = {}

    @contextlib.contextmanager
    def active(self):
        from iif_amd import resnet_engine
        orig = resnet_engine._Plan._unit_backward
        orig_se = resnet_engine._Plan._se_backward
        rec = self.records

        def wrapped(plan, u, gy, *args, **kw):
            ready = plan._bw_ready
            alg = ready is not None and ready[0] is u and len(ready) == 3
            g0 = gy.clone()
            out = orig(plan, u, gy, *args, **kw)
            rec[id(u)] = {"gy": g0, "out": None if out is None else out.clone(), "alg": alg}
            return out

        def wrapped_se(plan, b, last, g, *args, **kw):
            g0 = g.clone()
            G = orig_se(plan, b, last, g, *args, **kw)
            rec[se_key(last)] = {"g": g0, "gm": g.clone(), "G": G.clone()}
            return G

        resnet_engine._Plan._unit_backward = wrapped
        resnet_engine._Plan._se_backward = wrapped_se
        try:
            yield self
        finally:
            resnet_engine._Plan._unit_backward = orig
            resnet_engine._Plan._se_backward = orig_se


def se_key(last):
    """Record key of the SE block whose last unit is ``last`` (``g``: the block-output gradient as it arrived, ``gm``: the same
    buffer after ``_se_backward`` masked it in place, ``G``: the returned gradient of the BN output, before the unit's own BN
    backward overwrites that buffer)."""
    return ("se", id(last))


def run_step(net, x, y, crit, capture=None):
    """One real training step (forward, fused loss, backward); returns (loss, copy of the gradient arena)."""
    ctx = capture.active() if capture is not None else contextlib.nullcontext()
    with ctx:
        loss, _ = net.loss_and_backward(x, y, crit)
    torch.cuda.synchronize()
    return loss.item(), net._grad_arena.clone()


def unit_names(net):
    """id(conv) -> reference parameter prefix (``layer1.0.conv3``, ``layer2.0.downsample.0``, ``conv1``)."""
    return {id(m): n for n, m in net.named_modules()}


def routes(plan, cap):
    """Route inventory of the step the capture recorded."""
    alg = [u for u in plan.units if cap.records.get(id(u), {}).get("alg")]
    ds_alg = [b["ds"] for b in plan.blocks if "ds" in b and id(b["ds"]) not in cap.records]
    rs = [plan._route(b["units"][-1]) for b in plan.blocks]
    return {"alg3": len(alg), "alg3_pure": sum(1 for u in alg if plan._route(u).backward == "pure"),
            "rx": sum(1 for u in alg if plan._route(u).backward == "rx"), "nostore": sum(1 for r in rs if r.forward == "nostore"),
            "twopass": sum(1 for r in rs if r.forward == "twopass"), "pg": sum(1 for r in rs if r.gram == "producer"),
            "pro": sum(1 for r in rs if r.prologue), "pro_rows": sum(1 for r in rs if r.csum_rows),
            "se": sum(1 for b in plan.blocks if "se" in b and se_key(b["units"][-1]) in cap.records),
            "ds_alg": len(ds_alg), "pool_fused_bwd": bool(plan.pool_fused and plan.pool_x is not None),
            "wg_stream": plan.wg_stream is not None, "ds_stream": plan.ds_stream is not None}


# ------------------------------------------------------------------ the checker
SE_GATE = {}            # "<block>.se" -> max |o| / max |G| of the last check_step call, both from the float64 reference alone


def check_step(net, img, cap):
    """Evaluate every conv+BN unit of the last step in float64 from the inputs that step used; {name: {metric: value}}."""
    plan = net._saved
    dt = plan.dt
    names = unit_names(net)
    rec = cap.records
    res = {}

    def rnd(t):
        return t.to(dt).to(F64)

    def P(t):
        return t.detach().to(F64)

    def weight(cv):
        return cv.weight.detach().to(dt).to(F64)                 # the fp32 master parameters rounded to the compute type

    def dw_arena(cv):
        return cv._g2d[:, :cv.kdim].reshape(cv.cout, cv.k, cv.k, cv.cg).permute(0, 3, 1, 2).to(F64)

    def forward(u, src, x_stored, unrounded_stats, res_t=None, y_check=True, gate=None):
        """Statistics / stored output / activated output of unit u; returns (x_ref, the stats block as float64).
        gate: the stored excitation e [N, C] of an SE block's last unit (y = relu((a x + b) e + res))."""
        cv = u.conv
        m = {}
        xr = conv_fwd(src, weight(cv), cv.stride, cv.pad, cv.groups)
        mean_r, inv_r = bn_stats(xr if unrounded_stats else rnd(xr))
        st = P(u.stats)
        m["mean"] = ((st[0] - mean_r).abs() * inv_r).max().item()
        m["invstd"] = (st[1] / inv_r - 1).abs().max().item()
        if x_stored:
            m["x"] = rel_max(u.x, xr)
        if y_check and u.y is not None:
            xs = P(u.x) if x_stored else rnd(xr)
            yr = bn_act(xs, st[2], st[3], res_t) if gate is None else se_apply(xs, st[2], st[3], gate, res_t)
            m["y"] = rel_max(u.y, yr)
            m["y_l2"] = rel_l2(u.y, yr)
            pos = u.y > 0
            m["bits"] = (unpack_bits(u.bits, dt, pos.shape) != pos).double().mean().item()
        res[names[id(cv)]] = m
        return xr, st

    def backward(u, src, gy, mask, xsrc, st, stored_dx=True, gy_sums=None):
        """BN backward + weight gradient of unit u from the gradient that arrived at it; returns (dx, gt).  stored_dx: the
        engine forms the weight gradient from its stored (bf16) dx, not by algebra from fp32 P / Gram.  gy_sums: see bn_backward."""
        cv, bn = u.conv, u.bn
        xh = (xsrc - st[0]) * st[1]
        dx, dgam, dbet, gt = bn_backward(gy, mask, xh, P(bn.weight), st[1], gy_sums)
        m = res[names[id(cv)]]
        m["dgamma"] = rel_l2(bn._dgamma, dgam)
        m["dbeta"] = rel_l2(bn._dbeta, dbet)
        wshape = tuple(cv.weight.shape)
        got = dw_arena(cv)
        m["dw"] = rel_l2(got, conv_wgrad(src, dx, wshape, cv.stride, cv.pad, cv.groups))
        if stored_dx:
            m["dw_rdx"] = rel_l2(got, conv_wgrad(src, rnd(dx), wshape, cv.stride, cv.pad, cv.groups))
        return dx, gt

    def dgrad_metric(name, got, ref, up_mask):
        got = P(got)
        if up_mask is not None:
            got, ref = got * up_mask, ref * up_mask
        res[name]["dgrad"] = rel_l2(got, ref)
        res[name]["dgrad_max"] = rel_max(got, ref)

    def mask_of(u):
        return None if u is None else (u.y > 0).to(F64)

    def se_check(b, last, st):
        """The SE stages of block b around its last unit, each from the operands the step stored for it (b["se"], the capture's
        record); metrics under ``<block>.se``.  Returns the masked block-output gradient g~ (float64)."""
        from tests import head_cases as H
        S, se = b["se"], b["blk"].se
        l1, l2 = se.excitation[0], se.excitation[2]
        n, hw, c, hid = last.n, last.ho * last.wo, se.c, se.hidden
        bname = names[id(b["blk"])] + ".se"
        m = res[bname] = {}
        r = rec[se_key(last)]

        def C(t):
            return t.detach().to("cpu", F64)

        def rows(t):                          # [N, H, W, C] -> [N, C, pixels] on the CPU: the sums run over the last axis
            return C(t).reshape(n, hw, c).permute(0, 2, 1)

        def stage(key, got, fn, *ops):
            """Relative L2 of ``got`` against fn(*ops) in float64 over max(2e-5, 4 x the relative L2 of the same stage in
            float32 on the CPU from the same operands): <= 1 passes."""
            ref = fn(*ops)
            r32 = fn(*[o.float() if torch.is_tensor(o) else o for o in ops]).to(F64)
            m[key] = rel_l2(C(got), ref) / max(2e-5, 4 * rel_l2(r32, ref))
            return ref

        a, bb = C(st[2]), C(st[3])
        w1, w2 = C(l1.weight), C(l2.weight)
        xs = rows(last.x)
        ones = torch.ones_like(xs)
        # ---- forward: squeeze of the stored x, q / h / e each from the stored stage before it
        sref, sbnd = H.sum_bound(xs, ones, hw)
        m["se_sums"] = H.worst_ratio(C(S["sums"]), sref, sbnd)[0]
        qr = se_q(C(S["sums"]), a, bb, hw)
        m["se_q"] = ((C(S["q"]) - qr).abs().max() / qr.abs().max().clamp_min(1e-300)).item()
        hr = se_h(C(S["q"]), w1)
        m["se_h"] = ((C(S["h"]) - hr).abs().max() / max(1.0, hr.abs().max().item())).item()
        m["se_e"] = (C(S["e"]) - se_e(C(S["h"]), w2)).abs().max().item()
        # ---- backward: the in-place mask, the two sums over the masked gradient, the excitation's backward stage by stage
        m["se_gmask"] = float((r["gm"] != r["g"] * (last.y > 0)).sum().item())
        gm = rows(r["gm"])
        s1r, b1 = H.sum_bound(gm, ones, hw)
        s2r, b2 = H.sum_bound(gm, xs, hw)
        m["se_s1"] = H.worst_ratio(C(S["s1"]), s1r, b1)[0]
        m["se_s2"] = H.worst_ratio(C(S["s2"]), s2r, b2)[0]
        e_s, h_s, q_s = C(S["e"]), C(S["h"]), C(S["q"])
        stage("se_dz2", S["dz2"], se_dz2, C(S["s1"]), C(S["s2"]), a, bb, e_s)
        stage("se_dz1", S["dz1"], se_dz1, C(S["dz2"]), w2, h_s)
        stage("se_o", S["o"], se_offset, C(S["dz1"]), w1, hw)
        stage("se_dw1", l1._g2d[:, :c], se_dw, C(S["dz1"]), q_s)
        stage("se_dw2", l2._g2d[:, :hid], se_dw, C(S["dz2"]), h_s)
        pad = 0
        for lin in (l1, l2):                             # pad columns of the gradient rows and the arena's padding behind them
            o, nrow, pitch = net._offsets[(id(lin), "weight")]
            tail = net._grad_arena[o + nrow * pitch:o + (nrow * pitch + 15) // 16 * 16]
            pad += int((lin._g2d[:, lin.in_features:] != 0).sum().item()) + int((tail != 0).sum().item())
        m["se_pad"] = float(pad)
        gm64 = P(r["gm"])
        Gr = rnd(se_form(gm64, P(S["e"]), P(S["o"])))
        m["se_G"] = rel_max(r["G"], Gr)
        # how visible the gate path is in G, from float64 alone (the whole chain from the float64 sums and the stored e, h)
        o_chain = se_offset(se_dz1(se_dz2(s1r, s2r, a, bb, e_s), w2, h_s), w1, hw)
        G_chain = gm * e_s[:, :, None] + o_chain[:, :, None]
        SE_GATE[bname] = (o_chain.abs().max() / G_chain.abs().max().clamp_min(1e-300)).item()
        return gm64

    SE_GATE.clear()
    stem = plan.stem
    imagenet = net.style == "imagenet"
    c1 = net.conv1
    img64 = rnd(nhwc(img.to(F64)))
    # ---- blocks, in reverse (the block-input gradient of block bi is what arrived at block bi - 1's last unit)
    # (behind an SE block the last unit's record holds G, the gradient of the BN output: the block-output gradient is in the
    # SE record)
    g_in = {}
    for bi, b in enumerate(plan.blocks):
        if bi > 0:
            up_b = plan.blocks[bi - 1]
            up_last = up_b["units"][-1]
            g_in[bi] = rec[se_key(up_last)]["g"] if "se" in up_b else rec[id(up_last)]["gy"]
    b0 = plan.blocks[0]
    if id(stem) in rec:
        g_in[0] = rec[id(stem)]["gy"]
    elif "se" in b0 and "ds" in b0:
        g_in[0] = rec[id(b0["ds"])]["out"]       # the shortcut's data gradient runs last there and adds the first unit's
    else:
        g_in[0] = rec[id(b0["units"][0])]["out"]
    for bi, b in enumerate(plan.blocks):
        units = b["units"]
        last = units[-1]
        inp = P(b["inp"])
        lrec = rec[id(last)]
        alg = lrec["alg"]
        route = plan._route(last)
        unrounded_last = (route.forward == "nostore" and alg) or route.forward == "twopass"
        # forward
        xrs, sts = [], []
        for ui, u in enumerate(units[:-1]):
            xr, st = forward(u, P(u.src), True, False)
            xrs.append(xr)
            sts.append(st)
        du = b.get("ds")
        rres = None
        if du is not None:
            xr_d, st_d = forward(du, inp, True, False, y_check=False)
            rres = P(du.x) * st_d[2] + st_d[3]
        elif "sc" in b:
            rres = shortcut_a_fwd(inp, b["blk"].out_planes)
        else:
            rres = inp
        se = "se" in b
        xr, st = forward(last, P(last.src), not unrounded_last, unrounded_last, res_t=rres,
                         gate=P(b["se"]["e"]) if se else None)
        xrs.append(xr)
        sts.append(st)
        # an SE block: bn3 has no ReLU of its own, so G arrives at the last unit unmasked, and the identity path carries the
        # masked block-output gradient (the shortcut unit's record holds it already masked)
        gm = se_check(b, last, st) if se else None
        last_mask = None if se else mask_of(last)
        # backward, last unit: x-hat of the route ("sums from P": the unrounded product, the producer that recomputes conv3's
        # tile: that tile rounded, stored units: the stored output)
        if alg and route.backward == "pure":
            xsrc = xr
        elif alg and route.backward == "rx":
            xsrc = rnd(xr)
        else:
            xsrc = P(last.x)
        dx, gt = backward(last, P(last.src), P(lrec["gy"]), last_mask, xsrc, st, stored_dx=not alg)
        if se:
            gt = gm
        dxs = {len(units) - 1: dx}
        d_res = None
        if du is not None:
            drec = rec.get(id(du))
            # the shortcut's BN backward by algebra (not through _unit_backward) takes its sums from P = g~^T x_in: unrounded
            xs_d = P(du.x) if drec is not None else xr_d
            gy_d = P(drec["gy"]) if drec is not None else P(lrec["gy"])
            dx_d, _ = backward(du, inp, gy_d, last_mask, xs_d, st_d, stored_dx=drec is not None)
            d_res = conv_dgrad(dx_d, weight(du.conv), inp.shape, du.conv.stride, du.conv.pad)
        elif "sc" in b:
            d_res = shortcut_a_bwd(gt, inp.shape)
        else:
            d_res = gt
        for ui in range(len(units) - 2, -1, -1):
            u = units[ui]
            r = rec[id(u)]
            dx, _ = backward(u, P(u.src), P(r["gy"]), mask_of(u), P(u.x), sts[ui])
            dxs[ui] = dx
        for ui in range(len(units) - 1, 0, -1):
            u = units[ui]
            cv = u.conv
            d = conv_dgrad(dxs[ui], weight(cv), u.src.shape, cv.stride, cv.pad, cv.groups)
            dgrad_metric(names[id(cv)], rec[id(u)]["out"], d, mask_of(units[ui - 1]))
        f = units[0]
        d = conv_dgrad(dxs[0], weight(f.conv), f.src.shape, f.conv.stride, f.conv.pad, f.conv.groups) + d_res
        # behind an SE or option-A block the engine stores the block-input gradient ungated (no upstream unit fused into the
        # data gradient that completes it): compared ungated there
        up_b = plan.blocks[bi - 1] if bi > 0 else None
        up = up_b["units"][-1] if up_b is not None and "se" not in up_b and "sc" not in up_b else None
        dgrad_metric(names[id(f.conv)], g_in[bi], d, mask_of(up))
        del xrs, dxs
    # ---- stem
    if imagenet:
        xr, st = forward(stem, img64, True, False, y_check=False)
        m = res[names[id(c1)]]
        ys = rnd(bn_act(P(stem.x), st[2], st[3]))                    # bn1 + ReLU, rounded as the fused pool rounds candidates
        win = maxpool_windows(ys)
        wmax = win.max(-1).values
        chosen = win.gather(-1, plan.pool_idx.long().unsqueeze(-1)).squeeze(-1)
        m["pool"] = rel_max(plan.pool_out, wmax)
        m["pool_idx"] = ((wmax - chosen) / wmax.abs().clamp_min(1e-30)).max().item()
        # the gathered sum of up to four pooled gradients is rounded to the storage type before the normalisation pass: the fused
        # kernel rounds it in registers (bn.hip, pool_bn_bwd_apply_kernel), the unfused route stores that tensor.  The two
        # column sums are formed from the pooled gradients themselves (pool_bwd_sums_kernel): unrounded.
        gy = maxpool_scatter(P(g_in[0]), plan.pool_idx, (stem.ho, stem.wo))
        mask = ((P(stem.x) * st[2] + st[3]) > 0).to(F64)
        backward(stem, img64, rnd(gy), mask, P(stem.x), st, gy_sums=gy)
    else:
        xr, st = forward(stem, img64, True, False)
        backward(stem, img64, P(rec[id(stem)]["gy"]), mask_of(stem), P(stem.x), st)
    return res


def failures(metrics, bounds):
    """[(unit, metric, value, bound)] of every metric above its bound (``bounds``: metric -> bound, or a callable
    (unit, metric) -> bound)."""
    out = []
    for name, m in metrics.items():
        for k, v in m.items():
            bnd = bounds(name, k) if callable(bounds) else bounds.get(k)
            if bnd is not None and not (v <= bnd):
                out.append((name, k, v, bnd))
    return out


def worst(metrics):
    """metric -> (worst value, unit)."""
    w = {}
    for name, m in metrics.items():
        for k, v in m.items():
            if k not in w or v > w[k][0]:
                w[k] = (v, name)
    return w


# ------------------------------------------------------------------ the head: pooling, classifier, loss, and their backward
HEAD_ERRORS = {}                              # metric -> largest absolute error of the last check_head call (for reports)
FP32_TINY = 2.0 ** -126                       # below this fp32 results may be flushed to zero
HEAD_EXACT = ("w_cast", "wt", "w_t", "dl_cast", "dl_pad", "w_pad")          # counts / magnitudes that must be exactly 0


def _gemm_bound(a, b):
    """a [m, k] @ b [n, k]^T in float64 with the bound of an fp32-accumulated product (tests/head_cases.py: the reduction
    length k is the chain), or 4 x the error of the same product in float32 on the CPU."""
    from tests import head_cases as H
    ref = a @ b.t()
    s = a.abs() @ b.abs().t()
    cpu32 = (a.float() @ b.float().t()).to(F64)
    return ref, torch.maximum((a.shape[1] + 16) * H.U24 * s, 4 * (cpu32 - ref).abs())


def check_head(net, cap, targets, crit):
    """Everything between the last block and the loss of the last step, stage by stage in float64 on the CPU from the operands
    the step itself stored (``net._saved``), so each metric sees one rounding and one accumulation.  Returns {metric: value}.

    Unless noted a value is the worst |error| / bound over every element of the stage's output (<= 1 passes), with the
    per-element bounds of tests/head_cases.py: fp32 sums get max((L + 16) 2^-24 S, 4 |float32 CPU - float64|), an output that
    depends on a sum through a coefficient gets that bound times what multiplies it plus 16 * 2^-24 of its own terms, and
    every store in bf16 adds 2^-8 |ref|.
      pooled        mean over the pixels of ``final`` (L = pixels)
      ex, xnorm     the feature map of the cosine (x scale / (1 + |x|); lr_cosine: s^2, applied by a second in-place pass, so
                    two stores) and normed (x / max(|x|, eps)) heads and its stored row norms
      wn, wnorm     row-normalised weights (cosine: eps 0; normed: the columns, through the transpose ``w_t``, exact)
      w_pad         largest magnitude in the zero pad rows of the normalised weights (exactly 0)
      w_cast, wt    elements of ``head_w`` that are not the compute-type rounding of its fp32 source / of ``head_wt`` that are
                    not ``head_w`` transposed (exactly 0)
      logits        features x weights (+ bias), L = in_features
      loss, dlogits the closed form of oracle.iif_oracle.iif_ce_closed_form on the stored logits.  z = logit * table is one
                    fp32 product, exp(z - max) carries the rounding of its argument, 2^-24 (|z| + |max| + 3 |z - max| + 16)
                    relative (and may be flushed to 0 below 2^-126), the row sum L = C on top; the softmax and the row loss
                    inherit both
      dl_pad, dl_cast  pad columns of dlogits (exactly 0); elements of ``dlogits_t`` that are not the rounding of dlogits
      dwn           (cosine / normed) dlogits_t^T x ex, L = batch
      dw            the weight gradient against the float64 one formed from the stored dlogits_t and ex (pooled), taken back
                    through the row normalisation with the stored norms: the bound of dwn carried through g a - w <g, w> k
      dw_full       relative L2 of the weight gradient against the same from the unrounded dlogits (what bf16 storage of
                    dlogits costs; bounded like ``dw`` next to ``dw_rdx`` in the unit table)
      db, ds        (linear) column sums of dlogits, L = batch; (lr_cosine) (2 / s) <dlogits, logits>, double accumulation
      dex, dpooled  dlogits_t x weights, L = out_padded (lr_cosine: times s^2 by a second in-place pass); back through the map
      dgrad         the gradient that arrived at the last unit against the float64 dpooled / pixels at every pixel (the stored
                    dpooled's bound carried over, so an error in dpooled shows here too)
    """
    from oracle import iif_oracle as O
    from tests import head_cases as H
    plan, head = net._saved, net._head
    dt, kind = plan.dt, plan.head_kind
    n, C, op, D = plan.n, head.out_features, head.out_padded, head.in_features
    u24 = H.U24
    met = {}

    def P(t):
        return t.detach().to("cpu", F64)

    def ratio(name, got, ref, bound, store=None):
        met[name], HEAD_ERRORS[name] = H.worst_ratio(P(got), ref, H.stored(bound, ref, store) if store is not None else bound)

    def mismatch(name, a, b):
        met[name] = float((a.detach().cpu() != b.detach().cpu()).sum().item())

    lr = kind == "cosine" and head.lr_scale
    s = P(head._s1d[:1]).item() if lr else None
    # ---- pooling
    final = P(plan.final)
    hw = final.shape[1] * final.shape[2]
    fin = final.reshape(n, hw, D).permute(0, 2, 1)                            # [n, D, pixels]
    psum, b_psum = H.sum_bound(fin, torch.ones_like(fin), hw)
    pooled_ref = psum / hw
    ratio("pooled", plan.pooled, pooled_ref, b_psum / hw + 16 * u24 * pooled_ref.abs(), dt)
    pooled = P(plan.pooled)
    # ---- feature map and weights
    if kind == "linear":
        feat = pooled
        wsrc = P(head._w2d)
        bias = P(head._b1d)[:op]
    else:
        bias = None
        mode, eps = (1, 1e-12) if kind == "norm" else (0, 1e-12)
        scale = 1.0 if (kind == "norm" or lr) else float(head.scale)
        ex, b_ex, xn, b_xn = H.rowmap_forward_bounds(pooled, mode, scale, eps)
        if lr:                                          # stored once, then scaled in place by s^2 and stored again
            s2 = float(torch.tensor(s, dtype=torch.float32) ** 2)
            b_ex = s2 * H.stored(b_ex, ex, dt) + 16 * u24 * s2 * ex.abs()
            ex = ex * s2
        ratio("ex", plan.head_ex, ex, b_ex, dt)
        ratio("xnorm", plan.head_xnorm, xn, b_xn)
        feat = P(plan.head_ex)
        if kind == "cosine":
            wmaster, weps = P(head._w2d), 0.0
        else:
            mismatch("w_t", plan.head_wT, head._w2d.t())
            wmaster, weps = P(plan.head_wT), 1e-12
        wn, b_wn, wnorm, b_wnorm = H.rowmap_forward_bounds(wmaster, 1, 1.0, weps)
        ratio("wn", plan.head_wsrc, wn, b_wn)
        ratio("wnorm", plan.head_wnorm, wnorm, b_wnorm)
        met["w_pad"] = P(plan.head_wsrc)[C:].abs().max().item() if op > C else 0.0
        wsrc = P(plan.head_wsrc)
    mismatch("w_cast", plan.head_w, (head._w2d if kind == "linear" else plan.head_wsrc).to(dt))
    w = P(plan.head_w)
    if plan.head_wt is not None:
        mismatch("wt", plan.head_wt[:, :op], plan.head_w.t())
    # ---- logits
    lg, b_lg = _gemm_bound(feat, w)
    if bias is not None:
        lg, b_lg = lg + bias, b_lg + (D + 16) * u24 * bias.abs()
    ratio("logits", plan.logits, lg, b_lg)
    logits = P(plan.logits)
    # ---- loss and dlogits from the stored logits
    table = P(crit._table(plan.logits)).reshape(-1)[:C]
    tg = targets.detach().cpu().long()
    loss_ref, dl_ref, rows = O.iif_ce_closed_form(logits[:, :C], tg, table)
    z = logits[:, :C] * table
    zmax = z.max(1, keepdim=True).values
    e = torch.exp(z - zmax)
    ssum = e.sum(1, keepdim=True)
    rel_e = u24 * (z.abs() + zmax.abs() + 3 * (z - zmax).abs() + 16)
    b_e = e * rel_e + FP32_TINY                       # an exponential below fp32's normal range may come out as 0
    b_ssum = b_e.sum(1, keepdim=True) + (C + 16) * u24 * ssum
    soft = e / ssum
    b_soft = b_e / ssum + soft * (b_ssum / ssum + 2 * u24)
    onehot = torch.zeros_like(soft)
    onehot[torch.arange(n), tg] = 1.0
    b_dl = table.abs() / n * b_soft + 16 * u24 * table.abs() * (soft + onehot) / n + FP32_TINY
    zt = z[torch.arange(n), tg]
    b_row = (u24 * (zmax.abs() + zt.abs()[:, None]) + b_ssum / ssum
             + 16 * u24 * (zmax.abs() + ssum.log().abs() + zt.abs()[:, None])).squeeze(1)
    b_loss = b_row.sum() / n + (n + 16) * u24 * rows.abs().sum() / n
    ratio("loss", plan.loss, loss_ref, b_loss)
    ratio("dlogits", plan.dlogits[:, :C], dl_ref, b_dl)
    met["dl_pad"] = P(plan.dlogits)[:, C:].abs().max().item() if op > C else 0.0
    dl_full = P(plan.dlogits)
    if dt == torch.float32:
        dl = dl_full
        met["dl_cast"] = 0.0
    else:
        mismatch("dl_cast", plan.dlogits_t, plan.dlogits.to(dt))
        dl = P(plan.dlogits_t)
    # ---- weight gradient
    def through_norm(g, b_g):
        """Row-normalisation backward of g [op, D] (with its bound) from the master weights and the stored norms."""
        if kind == "linear":
            return g, b_g
        nrm = P(plan.head_wnorm)
        dx, t1, t2, k = H._rowmap_backward_terms(wmaster, nrm, g, 1, 1.0, weps)
        _, b = H.rowmap_backward_bounds(wmaster, nrm, g, 1, 1.0, weps)
        m = nrm.clamp_min(weps)
        a = torch.where(nrm > 0, 1 / torch.where(nrm > 0, m, torch.ones_like(m)), torch.zeros_like(nrm))
        carried = a[:, None] * b_g + wmaster.abs() * (k * (wmaster.abs() * b_g).sum(1))[:, None]
        return dx, b + carried

    dwn, b_dwn = _gemm_bound(dl.t().contiguous(), feat.t().contiguous())        # [op, D], L = batch
    if kind != "linear":
        ratio("dwn", plan.head_dwn, dwn, b_dwn)
    dw_ref, b_dw = through_norm(dwn, b_dwn)
    got_dw = P(head._g2d)
    if kind == "norm":
        got_dw = got_dw.t()
    ratio("dw", got_dw, dw_ref, b_dw)
    dw_full, _ = through_norm(dl_full.t() @ feat, torch.zeros_like(b_dwn))
    met["dw_full"] = rel_l2(got_dw, dw_full)
    if kind == "linear":
        ones = torch.ones_like(dl_full.t())
        db, b_db = H.sum_bound(dl_full.t().contiguous(), ones, n)
        ratio("db", head._gb1d[:op], db, b_db)
    if lr:
        ds, b_ds = H.dot_window(dl_full[:, :C], logits[:, :C], 2.0, s)
        ratio("ds", head._gs1d[:1], ds.reshape(1), b_ds.reshape(1))
    # ---- data gradient
    dex, b_dex = _gemm_bound(dl, w.t().contiguous())                             # [n, D], L = out_padded
    dpooled_t = plan._grad_pool[("dpooled",)].view(n, D)
    if kind == "linear":
        dp, b_dp = dex, b_dex
        ratio("dpooled", dpooled_t, dex, b_dex, dt)
    else:
        if lr:
            b_dex = s2 * H.stored(b_dex, dex, dt) + 16 * u24 * s2 * dex.abs()
            dex = dex * s2
        ratio("dex", plan.head_dex, dex, b_dex, dt)
        dp, b_dp = H.rowmap_backward_bounds(pooled, P(plan.head_xnorm), P(plan.head_dex), mode, scale, eps)
        ratio("dpooled", dpooled_t, dp, b_dp, dt)
    last = plan.blocks[-1]["units"][-1]
    gy = P(cap.records[id(last)]["gy"])
    dg = (dp / hw).view(n, 1, 1, D).expand(gy.shape)
    b_dg = (H.stored(b_dp, dp, dt) / hw).view(n, 1, 1, D).expand(gy.shape) + 16 * u24 * dg.abs()
    ratio("dgrad", gy, dg, b_dg, dt)
    return met


def head_failures(met, dt):
    """[(metric, value, bound)] above its bound: 1 for the error / bound ratios, 0 for the exact ones, and for ``dw_full`` the
    bound ``dw`` has next to ``dw_rdx`` in the unit table (2e-2 in bf16, 1e-5 in fp32)."""
    out = []
    for k, v in met.items():
        bnd = 0.0 if k in HEAD_EXACT else (2e-2 if dt == torch.bfloat16 else 1e-5) if k == "dw_full" else 1.0
        if not (v <= bnd):
            out.append((k, v, bnd))
    return out
