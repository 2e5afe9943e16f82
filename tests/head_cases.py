"""Float64 closed forms and error bounds of the head-side row kernels (a test helper module, not a conftest).

The closed forms restate the comments at the top of each kernel of iif_amd/csrc/norm_head.hip in plain float64 torch on the
CPU; tests/test_head_reference_host.py checks them against float64 autograd of ``F.normalize``, ``x * scale / (1 + norm)``
and the ``normed_predictor`` formula ``v * scale / (norm ** power + eps)``, so the yardstick does not depend on the code
under test.

Bounds (per element, nothing fitted to what the kernels give).  u = 2^-24.
  * a result the kernel forms as a sum of fp32 terms: max((L + 16) u S, 4 |float32 CPU evaluation - float64|), S the float64
    sum of the magnitudes of the terms, L the longest chain of sequential additions (``wave_chain``: one lane's strided chain
    plus the six shuffle steps of a 64-lane wave);
  * an output that depends on such a reduction through a coefficient: the reduction's bound times the magnitude of the
    derivative of the output with respect to the reduction, plus 16 u times the sum of the magnitudes of its own terms;
  * an output stored in bf16: 2^-8 |ref| on top (one round-to-nearest is 2^-9; the factor 2 is for an fp32 error that
    straddles a rounding boundary).
"""
import math

import torch

F64 = torch.float64
U24 = 2.0 ** -24
ROWS = (1, 3, 4, 5, 1001)                     # four rows per block: last blocks with 1, 3 and 4 live waves, many blocks
COLS = (1, 63, 64, 65, 640, 2048)             # below / at / above one lane chunk, ten and 32 chunks
PADS = (0, 1, 7)                              # leading dimension = cols + pad


def wave_chain(cols):
    return (cols + 63) // 64 + 6


def sum_bound(a, b, chain):
    """sum over the last dimension of a * b (float64 tensors holding fp32-representable values) -> (ref, bound)."""
    t = a * b
    ref = t.sum(-1)
    s = t.abs().sum(-1)
    cpu32 = (a.float() * b.float()).sum(-1).to(F64)
    return ref, torch.maximum((chain + 16) * U24 * s, 4 * (cpu32 - ref).abs())


def stored(bound, ref, dtype):
    """The bound of ``ref`` once stored as ``dtype``."""
    return bound + 2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else bound


def _safe_div(a, b):
    """a / b where b != 0, else 0 (the limit every use below wants: the numerator's bound is 0 there)."""
    return torch.where(b != 0, a / torch.where(b != 0, b, torch.ones_like(b)), torch.zeros_like(a))


# ------------------------------------------------------------------ rowmap (cosine / F.normalize feature maps)
def rowmap_forward(x, mode, scale, eps):
    """mode 0: x * scale / (1 + |x|);  mode 1: x / max(|x|, eps), rows of zeros stay zero.  -> (out, norms)."""
    n = (x * x).sum(-1).sqrt()
    if mode == 0:
        coef = scale / (1 + n)
    else:
        coef = _safe_div(torch.ones_like(n), n.clamp_min(eps)) * (n > 0)
    return x * coef[:, None], n


def rowmap_forward_bounds(x, mode, scale, eps):
    """-> (out, out_bound, norms, norms_bound) for fp32 outputs (``stored`` adds a bf16 rounding)."""
    ss, b_ss = sum_bound(x, x, wave_chain(x.shape[-1]))
    n = ss.sqrt()
    out, _ = rowmap_forward(x, mode, scale, eps)
    if mode == 0:
        dcoef = _safe_div(scale / (1 + n) ** 2, 2 * n)                         # |d coef / d ss|
    else:
        dcoef = _safe_div(torch.ones_like(n), 2 * n ** 3) * (n >= eps)
    b_out = (b_ss * dcoef)[:, None] * x.abs() + 16 * U24 * out.abs()
    b_n = _safe_div(b_ss, 2 * n) + 16 * U24 * n
    return out, b_out, n, b_n


def rowmap_backward(x, n, g, mode, scale, eps):
    """mode 0: scale (g / (1 + n) - x <g, x> / (n (1 + n)^2)), a row of zeros: scale g.
    mode 1: g / m - x <g, x> / m^3 with m = max(n, eps); no projection term where n < eps (there the map is x / eps);
    a row of zeros: 0 (the kernels' convention for the row the forward leaves at zero)."""
    return _rowmap_backward_terms(x, n, g, mode, scale, eps)[0]


def _rowmap_backward_terms(x, n, g, mode, scale, eps):
    dot = (g * x).sum(-1)
    if mode == 0:
        a = scale / (1 + n)
        k = _safe_div(scale / (1 + n) ** 2, n)
    else:
        m = n.clamp_min(eps)
        a = _safe_div(torch.ones_like(n), m) * (n > 0)
        k = _safe_div(torch.ones_like(n), m ** 3) * (n > 0) * (n >= eps)
    t1, t2 = g * a[:, None], x * (k * dot)[:, None]
    return t1 - t2, t1, t2, k


def rowmap_backward_bounds(x, n, g, mode, scale, eps):
    """-> (dx, bound) for an fp32 dx."""
    dx, t1, t2, k = _rowmap_backward_terms(x, n, g, mode, scale, eps)
    _, b_dot = sum_bound(g, x, wave_chain(x.shape[-1]))
    return dx, (b_dot * k)[:, None] * x.abs() + 16 * U24 * (t1.abs() + t2.abs())


# ------------------------------------------------------------------ rownorm (mmdet normed predictors)
def rownorm_forward(x, r, power, scale, eps):
    """v = r x (r per row, or None);  out = v scale / (|v|^power + eps).  -> (out, norms)."""
    v = x if r is None else x * r[:, None]
    n = (v * v).sum(-1).sqrt()
    return v * (scale / (n ** power + eps))[:, None], n


def rownorm_forward_bounds(x, r, power, scale, eps):
    v = x if r is None else x * r[:, None]
    ss, b_ss = sum_bound(v, v, wave_chain(x.shape[-1]))
    n = ss.sqrt()
    den = n ** power + eps
    out = v * (scale / den)[:, None]
    # coef = scale / (ss^(p/2) + eps):  |d coef / d ss| = scale p n^(p-2) / (2 den^2)
    dcoef = torch.where(n > 0, abs(scale) * power * n.clamp_min(1e-300) ** (power - 2) / (2 * den ** 2), torch.zeros_like(n))
    b_out = (b_ss * dcoef)[:, None] * v.abs() + 16 * U24 * out.abs()
    return out, b_out, n, _safe_div(b_ss, 2 * n) + 16 * U24 * n


def _rownorm_backward_terms(x, r, n, g, power, scale, eps):
    v = x if r is None else x * r[:, None]
    rr = torch.ones_like(n) if r is None else r
    dot = (g * v).sum(-1)
    den = n ** power + eps
    a = scale / den
    k = torch.where(n > 0, scale * power * n.clamp_min(1e-300) ** (power - 2) / den ** 2, torch.zeros_like(n))
    t1, t2 = g * (rr * a)[:, None], v * (rr * k * dot)[:, None]
    return t1 - t2, t1, t2, k, v, rr


def rownorm_backward(x, r, n, g, power, scale, eps):
    """dv = g a - v b,  a = scale / den,  b = scale power n^(power - 2) <g, v> / den^2 (0 for a row of zeros);  dx = r dv."""
    return _rownorm_backward_terms(x, r, n, g, power, scale, eps)[0]


def rownorm_backward_bounds(x, r, n, g, power, scale, eps):
    dx, t1, t2, k, v, rr = _rownorm_backward_terms(x, r, n, g, power, scale, eps)
    _, b_dot = sum_bound(g, v, wave_chain(x.shape[-1]))
    return dx, (b_dot * k.abs() * rr.abs())[:, None] * v.abs() + 16 * U24 * (t1.abs() + t2.abs())


# ------------------------------------------------------------------ dot over a window (double accumulation)
def dot_window(a, b, alpha, alpha_div=None):
    """alpha sum(a b) / alpha_div -> (ref, bound): the final fp32 rounding plus (rows cols) 2^-53 S."""
    t = a * b
    f = alpha / (1.0 if alpha_div is None else alpha_div)
    ref = t.sum() * f
    return ref, U24 * ref.abs() + t.numel() * 2.0 ** -53 * t.abs().sum() * abs(f)


# ------------------------------------------------------------------ inputs
def rows_matrix(rows, cols, seed, dtype=torch.float32, special=True, tiny=True):
    """A random [rows, cols] matrix rounded to ``dtype`` and widened to float64.  With ``special`` and enough rows: row 1 is
    zero and (``tiny``) row 3 has norm 1e-13, below the eps of F.normalize.  Callers pass ``tiny=False`` with eps = 0: the
    cube of such a norm is below fp32's normal range, which no fp32 bound describes and no head produces."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, cols, generator=g, dtype=F64) * 1.5 + 0.25)
    if special and rows >= 3:
        x[1] = 0
    if special and tiny and rows >= 5:
        x[3] = x[3] / x[3].norm() * 1e-13
    return x.to(dtype).to(F64)


def padded(values, pad, dtype, fill, device):
    """A [rows + 2, cols + pad] buffer of ``fill`` on the device whose window [1 : rows + 1, : cols] holds ``values`` (None: the
    window keeps ``fill``) -> (buffer, window view).  The window's leading dimension is cols + pad."""
    rows, cols = values.shape if isinstance(values, torch.Tensor) else values
    buf = torch.full((rows + 2, cols + pad), fill, dtype=dtype, device=device)
    win = buf[1:rows + 1, :cols]
    if isinstance(values, torch.Tensor):
        win.copy_(values.to(dtype))
    return buf, win


def outside_untouched(buf, rows, cols, fill):
    """Nothing but the window [1 : rows + 1, : cols] of a ``padded`` buffer differs from ``fill``."""
    probe = buf.clone()
    probe[1:rows + 1, :cols] = fill
    return bool((probe == fill).all().item())


def worst_ratio(got, ref, bound):
    """max over every element of |got - ref| / bound (0 / 0 counts as 0, anything / 0 as inf) and the max error."""
    err = (got.to(F64) - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    return ratio.max().item(), err.max().item()
