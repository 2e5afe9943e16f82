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


def bn_backward(gy, mask, xhat, gamma, invstd):
    """BN backward with the statistics of the step: gt = gy * mask (mask None: no ReLU),
    dgamma = sum gt xhat, dbeta = sum gt, dx = gamma invstd (gt - mean(gt) - xhat mean(gt xhat)).
    Returns (dx, dgamma, dbeta, gt)."""
    c = gy.shape[-1]
    gt = gy if mask is None else gy * mask
    g2, xh = gt.reshape(-1, c), xhat.reshape(-1, c)
    m = g2.shape[0]
    dbeta = g2.sum(0)
    dgamma = (g2 * xh).sum(0)
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
    waiting for this unit came with their rows, ``_bn3_algebra``)."""

    def __init__(self):
        self.records = {}

    @contextlib.contextmanager
    def active(self):
        from iif_amd import resnet_engine
        orig = resnet_engine._Plan._unit_backward
        rec = self.records

        def wrapped(plan, u, gy, *args, **kw):
            ready = plan._bw_ready
            alg = ready is not None and ready[0] is u and len(ready) == 3
            g0 = gy.clone()
            out = orig(plan, u, gy, *args, **kw)
            rec[id(u)] = {"gy": g0, "out": None if out is None else out.clone(), "alg": alg}
            return out

        resnet_engine._Plan._unit_backward = wrapped
        try:
            yield self
        finally:
            resnet_engine._Plan._unit_backward = orig


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
            "ds_alg": len(ds_alg), "pool_fused_bwd": bool(plan.pool_fused and plan.pool_x is not None),
            "wg_stream": plan.wg_stream is not None, "ds_stream": plan.ds_stream is not None}


# ------------------------------------------------------------------ the checker
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

    def forward(u, src, x_stored, unrounded_stats, res_t=None, y_check=True):
        """Statistics / stored output / activated output of unit u; returns (x_ref, the stats block as float64)."""
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
            yr = bn_act(xs, st[2], st[3], res_t)
            m["y"] = rel_max(u.y, yr)
            m["y_l2"] = rel_l2(u.y, yr)
            pos = u.y > 0
            m["bits"] = (unpack_bits(u.bits, dt, pos.shape) != pos).double().mean().item()
        res[names[id(cv)]] = m
        return xr, st

    def backward(u, src, gy, mask, xsrc, st, stored_dx=True):
        """BN backward + weight gradient of unit u from the gradient that arrived at it; returns (dx, gt).  stored_dx: the
        engine forms the weight gradient from its stored (bf16) dx, not by algebra from fp32 P / Gram."""
        cv, bn = u.conv, u.bn
        xh = (xsrc - st[0]) * st[1]
        dx, dgam, dbet, gt = bn_backward(gy, mask, xh, P(bn.weight), st[1])
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

    stem = plan.stem
    imagenet = net.style == "imagenet"
    c1 = net.conv1
    img64 = rnd(nhwc(img.to(F64)))
    # ---- blocks, in reverse (the block-input gradient of block bi is what arrived at block bi - 1's last unit)
    g_in = {}
    for bi, b in enumerate(plan.blocks):
        if bi > 0:
            g_in[bi] = rec[id(plan.blocks[bi - 1]["units"][-1])]["gy"]
    if id(stem) in rec:
        g_in[0] = rec[id(stem)]["gy"]
    else:
        g_in[0] = rec[id(plan.blocks[0]["units"][0])]["out"]
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
        xr, st = forward(last, P(last.src), not unrounded_last, unrounded_last, res_t=rres)
        xrs.append(xr)
        sts.append(st)
        # backward, last unit: x-hat of the route ("sums from P": the unrounded product, the producer that recomputes conv3's
        # tile: that tile rounded, stored units: the stored output)
        if alg and route.backward == "pure":
            xsrc = xr
        elif alg and route.backward == "rx":
            xsrc = rnd(xr)
        else:
            xsrc = P(last.x)
        dx, gt = backward(last, P(last.src), P(lrec["gy"]), mask_of(last), xsrc, st, stored_dx=not alg)
        dxs = {len(units) - 1: dx}
        d_res = None
        if du is not None:
            drec = rec.get(id(du))
            # the shortcut's BN backward by algebra (not through _unit_backward) takes its sums from P = g~^T x_in: unrounded
            xs_d = P(du.x) if drec is not None else xr_d
            gy_d = P(drec["gy"]) if drec is not None else P(lrec["gy"])
            dx_d, _ = backward(du, inp, gy_d, mask_of(last), xs_d, st_d, stored_dx=drec is not None)
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
        up = plan.blocks[bi - 1]["units"][-1] if bi > 0 else None
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
        gy = maxpool_scatter(P(g_in[0]), plan.pool_idx, (stem.ho, stem.wo))
        mask = ((P(stem.x) * st[2] + st[3]) > 0).to(F64)
        backward(stem, img64, gy, mask, P(stem.x), st)
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
