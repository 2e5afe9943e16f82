"""Cases of tests/golden/g19_focal.npz and an fp64 closed form of the reference's FocalLoss
(classification/custom.py:42-89), shared by the CPU and the GPU tests of the sigmoid BCE / focal head.

The closed form is the exact function (stable softplus forms), so it also serves where the reference's fp32
nn.BCELoss saturates (|x| above ~16.6, DESIGN.md "Sigmoid BCE / focal head")."""
import numpy as np

REDUCTIONS = ("mean", "sum", "none")


def softplus(v):
    return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))


def closed_form(x, targets, gamma, alpha=None, weights=None, reduction="mean", targets_b=None, lam=1.0):
    """(loss, d loss / d x) in float64 for logits x [B, C]; mixup when targets_b is given."""
    x = np.asarray(x, dtype=np.float64)
    B, C = x.shape

    def one(t):
        y = np.zeros((B, C))
        y[np.arange(B), np.asarray(t)] = 1.0
        sp, spn = softplus(x), softplus(-x)
        s = np.exp(-spn)                    # sigmoid(x)
        q = np.exp(-sp)                     # 1 - sigmoid(x)
        if gamma == 0:
            l = sp - x * y
            d = s - y
        else:
            l = np.where(y > 0, q ** gamma * spn, s ** gamma * sp)
            d = np.where(y > 0, -(q ** gamma) * (gamma * s * spn + q), s ** gamma * (s + gamma * q * sp))
            if alpha:
                at = alpha * y + (1 - alpha) * (1 - y)
                l, d = l * at, d * at
        if weights is not None:
            w = np.asarray(weights, dtype=np.float64).reshape(1, C)
            l, d = l * w, d * w
        k = 1.0 / B if reduction == "sum" else 1.0 / (B * C)
        return l.sum() * k, d * k

    la, da = one(targets)
    if targets_b is None:
        return la, da
    lb, db = one(targets_b)
    return lam * la + (1 - lam) * lb, lam * da + (1 - lam) * db


# The fixture's inputs: (name, B, C, rows whose gradient it keeps).  Rows are independent, so a few rows of the
# reference's gradient pin it as well as all of them would; the loss covers every element.
SHAPES = (("r7x13", 7, 13, tuple(range(7))), ("m128x100", 128, 100, (0, 1, 3, 127)),
          ("l256x1000", 256, 1000, (0, 5)))
MIX_ROWS = tuple(range(8))


def _mix64(v):
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic): a generator that no library version changes."""
    v = (v + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    v = ((v ^ (v >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)).astype(np.uint64)
    v = ((v ^ (v >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)).astype(np.uint64)
    return v ^ (v >> np.uint64(31))


def make_inputs(B, C, salt):
    """Deterministic logits [B, C] (float32, multiples of 1/256, bell-shaped with sd 3, |x| <= 12) and targets [B].
    Every third row has a confident target logit of either sign.  Regenerated, not stored, by the fixture's users."""
    with np.errstate(over="ignore"):
        idx = np.arange(B * C, dtype=np.uint64).reshape(B, C) + np.uint64(salt << 40)
        h = _mix64(idx)
        m = np.uint64(0xFFFF)
        s = (h & m).astype(np.int64) + ((h >> np.uint64(16)) & m).astype(np.int64) + ((h >> np.uint64(32)) & m).astype(np.int64)
        code = (s - 3 * 32768) * 1536 // 65536                      # sum of three uniforms: sd 768 = 3.0 in units of 1/256
        th = _mix64(np.arange(B, dtype=np.uint64) + np.uint64((salt + 1) << 40))
    t = (th % np.uint64(C)).astype(np.int64)
    conf = ((th >> np.uint64(32)) % np.uint64(6145)).astype(np.int64) - 3072
    rows = np.arange(0, B, 3)
    code[rows, t[rows]] = conf[rows]
    return (code.astype(np.float32) / np.float32(256.0)), t


def shape_inputs(name):
    for si, (n, B, C, _) in enumerate(SHAPES):
        if n == name:
            return make_inputs(B, C, si + 1)
    raise KeyError(name)


def golden_cases(g):
    """Yield (name, x float32 [B, C], targets int64, kwargs for closed_form / FocalLoss, loss, grad [rows, C], rows)."""
    inputs = {}
    for name, _, _, _ in SHAPES:
        x, t = inputs[name] = shape_inputs(name)
        assert np.array_equal(t, g[name + "_targets"]), "input generator drifted from the fixture"
        assert float(x.astype(np.float64).sum()) == float(g[name + "_logit_sum"]), "input generator drifted"
    for i in range(len(g["case_shape"])):
        name, _, C, rows = SHAPES[int(g["case_shape"][i])]
        x, t = inputs[name]
        a = float(g["case_alpha"][i])
        kw = dict(gamma=float(g["case_gamma"][i]), alpha=None if np.isnan(a) else a,
                  weights=g[name + "_weights"] if g["case_w"][i] else None,
                  reduction=REDUCTIONS[int(g["case_red"][i])])
        yield "%s/%d" % (name, i), x, t, kw, float(g["case_loss"][i]), g["case%d_grad" % i], list(rows)


def golden_mixup(g):
    """(x, y_a, y_b, lam, kwargs, loss, grad [rows, C], rows) of the mixup case."""
    name = str(g["mix_shape"])
    x, ya = shape_inputs(name)
    yb = ya[g["mix_perm"]]
    a = float(g["mix_alpha"])
    kw = dict(gamma=float(g["mix_gamma"]), alpha=None if np.isnan(a) else a, weights=g[name + "_weights"],
              reduction="mean")
    return x, ya, yb, float(g["mix_lam"]), kw, float(g["mix_loss"]), g["mix_grad"], list(MIX_ROWS)
