"""Cases of tests/golden/g22_seesaw.npz and a float64 closed form of the reference's SeesawLoss
(instance_segmentation/mmdet/models/losses/seesaw_loss.py), shared by the CPU and the GPU tests of the Seesaw head.

The closed form is written in the log domain (no [C, C] ratio matrix, no pow):
    a_j = min(0, p (log max(cum_j, 1) - log max(cum_t, 1)))
    b_j = max(0, q (z_j - lse(z) - max(z_t - lse(z), log eps)))
    z'_j = z_j + a_j + b_j (j != t),  loss_i = w_i (lse(z') - z_t),  d z = w_i (softmax(z') - onehot_t)
which is what log(seesaw_weights) of the reference equals where its float32 softmax does not underflow."""
import numpy as np

REDUCTIONS = ("mean", "sum", "none")
PQ = ((0.8, 2.0), (0.0, 2.0), (0.8, 0.0), (0.0, 0.0))
EPS = 1e-2
AVG_FACTOR = 37.0
LOSS_WEIGHT = 1.0

# (name, N, C, rows whose gradient / activation the fixture keeps).  Rows are independent, so a few rows of the
# reference's gradient pin it as well as all of them would; the losses cover every row.
SHAPES = (("s9x5", 9, 5, tuple(range(9))),            # 7 columns: every row on another 16-byte phase, odd row count
          ("m64x80", 64, 80, (1, 6, 63)),             # 82 columns: pitch = 2 mod 4
          ("l70x1203", 70, 1203, (1, 69)),            # the LVIS row: 1205 columns, ragged last chunk
          ("c16400x5", 16400, 5, (0, 1)))             # more labels than one histogram block takes
SCALES = (1, 6)        # x1: some target scores fall below eps; x6: the clamp binds on most rows


def _mix64(v):
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic): a generator that no library version changes."""
    with np.errstate(over="ignore"):
        v = (v + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
        v = ((v ^ (v >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)).astype(np.uint64)
        v = ((v ^ (v >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)).astype(np.uint64)
        return v ^ (v >> np.uint64(31))


def make_inputs(N, C, salt, scale=1):
    """Deterministic (logits [N, C + 2] float32: multiples of 1/256, bell-shaped with sd 3 x scale; labels int64 [N] in
    [0, C], about a quarter background; weights float32 [N]: multiples of 1/4 in [0, 2], about one in five zero)."""
    with np.errstate(over="ignore"):
        idx = np.arange(N * (C + 2), dtype=np.uint64).reshape(N, C + 2) + np.uint64(salt << 40)
        h = _mix64(idx)
        m = np.uint64(0xFFFF)
        s = (h & m).astype(np.int64) + ((h >> np.uint64(16)) & m).astype(np.int64) + ((h >> np.uint64(32)) & m).astype(np.int64)
        code = (s - 3 * 32768) * 1536 // 65536                      # sum of three uniforms: sd 768 = 3.0 in units of 1/256
        th = _mix64(np.arange(N, dtype=np.uint64) + np.uint64((salt + 1) << 40))
    labels = (th % np.uint64(C)).astype(np.int64)
    labels[((th >> np.uint64(20)) % np.uint64(4)) == 0] = C          # background
    wq = ((th >> np.uint64(32)) % np.uint64(10)).astype(np.int64)    # 0, 1 -> weight 0
    weights = np.where(wq < 2, 0, wq - 1).astype(np.float32) / np.float32(4.0)
    x = code.astype(np.float32) * np.float32(scale) / np.float32(256.0)
    return x, labels, weights


def make_cum(C, salt):
    """cum_samples [C + 1] float32 before the call: integers with a 1000:1 spread (1 and 1000 are
    always there), every seventh class never seen (0)."""
    h = _mix64(np.arange(C + 1, dtype=np.uint64) + np.uint64((salt + 7) << 40))
    u = (h % np.uint64(1024)).astype(np.float64) / 1024.0
    cum = np.floor(10.0 ** (3.0 * u))
    cum[::7] = 0.0
    cum[1], cum[(C + 1) // 2] = 1.0, 1000.0
    return cum.astype(np.float32)


def shape_index(name):
    return [s[0] for s in SHAPES].index(name)


def shape_inputs(name, scale=1):
    si = shape_index(name)
    _, N, C, _ = SHAPES[si]
    return make_inputs(N, C, si + 1, scale)


def count_labels(labels, C):
    """Per-class counts [C + 1] of the labels inside [0, C] (an out-of-range label counts nowhere)."""
    l = np.asarray(labels)
    return np.bincount(l[(l >= 0) & (l <= C)], minlength=C + 1)


def updated_cum(cum, labels, C):
    """cum_samples after a call: ONE float32 addition of the integer count per class (seesaw_loss.py:230-233)."""
    n = count_labels(labels, C)
    out = np.asarray(cum, dtype=np.float32).copy()
    nz = n > 0
    out[nz] = out[nz] + n[nz].astype(np.float32)
    return out


def _lse(v, axis=-1):
    m = v.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(v - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def closed_form(x, labels, cum, C, p=0.8, q=2.0, eps=EPS, weights=None, reduction="mean", avg_factor=None,
                loss_weight=LOSS_WEIGHT):
    """float64 (loss_classes, loss_objectness, gradient [N, C + 2]) for cls_score x with the UPDATED cum_samples.

    'none' returns the per-positive-row and the per-row vectors; its gradient is that of the sum of both.  Otherwise the
    gradient is that of loss_classes + loss_objectness.  Labels outside [0, C] contribute nothing."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    N = x.shape[0]
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    valid = (labels >= 0) & (labels <= C)
    pos = valid & (labels < C)
    w = np.where(valid, w, 0.0)
    grad = np.zeros((N, C + 2))
    # objectness: every (valid) row, label (labels == C)
    o = x[:, C:]
    ol = (labels == C).astype(np.int64)
    rows_obj = w * (_lse(o) - o[np.arange(N), ol]) if N else np.zeros(0)
    if N:
        so = np.exp(o - _lse(o)[:, None])
        so[np.arange(N), ol] -= 1.0
        grad[:, C:] = so * w[:, None]
    # classes: positive rows
    rows_cls = np.zeros(N)
    if pos.any():
        z = x[pos][:, :C]
        t = labels[pos]
        n = z.shape[0]
        ar = np.arange(n)
        lc = np.log(np.maximum(np.asarray(cum, dtype=np.float64)[:C], 1.0))
        add = np.zeros_like(z)
        if p > 0:
            add += np.minimum(0.0, p * (lc[None, :] - lc[t][:, None]))
        if q > 0:
            lse = _lse(z)
            thr = np.maximum(z[ar, t] - lse, np.log(eps))
            add += np.maximum(0.0, q * (z - lse[:, None] - thr[:, None]))
        add[ar, t] = 0.0
        z2 = z + add
        l2 = _lse(z2)
        rows_cls[pos] = w[pos] * (l2 - z[ar, t])
        sm = np.exp(z2 - l2[:, None])
        sm[ar, t] -= 1.0
        gp = np.zeros((n, C + 2))
        gp[:, :C] = sm * w[pos][:, None]
        gp[:, C:] = grad[pos][:, C:]
        grad[pos] = gp
    npos = int(pos.sum())
    if reduction == "none":
        return loss_weight * rows_cls[labels < C], loss_weight * rows_obj, loss_weight * grad
    if reduction == "sum":
        if avg_factor is not None:
            raise ValueError('avg_factor can not be used with reduction="sum"')
        kc = ko = loss_weight
    elif avg_factor is not None:
        kc = ko = loss_weight / avg_factor
    else:
        kc = loss_weight / npos if npos else 0.0
        ko = loss_weight / N if N else float("nan")
    grad[:, :C] *= kc
    grad[:, C:] *= ko
    return kc * rows_cls.sum(), ko * rows_obj.sum(), grad


def activation(x, C):
    """float64 [N, C + 1]: softmax(classes) * softmax(objectness)[0], then softmax(objectness)[1]."""
    x = np.asarray(x, dtype=np.float64)
    sc = np.exp(x[:, :C] - _lse(x[:, :C])[:, None])
    so = np.exp(x[:, C:] - _lse(x[:, C:])[:, None])
    return np.concatenate([sc * so[:, :1], so[:, 1:]], axis=1)


def accuracy(x, labels, C):
    """(acc_objectness, acc_classes) float32 as accuracy.py computes them: float32 hit count times float32(100 / rows),
    a hit when no column beats the target's and no equal one has a lower index; 0 without rows."""
    x = np.asarray(x)
    labels = np.asarray(labels)

    def top1(v, t):
        if v.shape[0] == 0:
            return np.float32(0.0)
        vt = v[np.arange(v.shape[0]), t][:, None]
        col = np.arange(v.shape[1])[None, :]
        beaten = ((v > vt) | ((v == vt) & (col < t[:, None]))).any(axis=1)
        return np.float32((~beaten).sum()) * np.float32(100.0 / v.shape[0])
    pos = (labels >= 0) & (labels < C)
    return top1(x[:, C:], (labels == C).astype(np.int64)), top1(x[pos][:, :C], labels[pos])


def grid_cases():
    """The fixture's case list: (shape index, scale, p, q, weights?, avg_factor?, reduction).  The full product on the two
    small shapes (avg_factor with 'sum' is an error and is left out); on the LVIS shape and the many-label shape every
    (p, q) x scale with the other options cycled."""
    out = []
    for si, (name, _, _, _) in enumerate(SHAPES):
        k = 0
        for scale in SCALES:
            for (p, q) in PQ:
                if name in ("s9x5", "m64x80"):
                    for wf in (0, 1):
                        for af in (0, 1):
                            for red in REDUCTIONS:
                                if af and red == "sum":
                                    continue
                                out.append((si, scale, p, q, wf, af, red))
                elif name == "l70x1203":
                    red = REDUCTIONS[k % 3]
                    out.append((si, scale, p, q, k % 2, 0 if red == "sum" else (k // 2) % 2, red))
                    k += 1
                elif (p, q) == PQ[0] and scale == 1:
                    out.append((si, scale, p, q, 1, 0, "mean"))
    return out


# label overrides on the s9x5 inputs: (name, labels)
def special_labels(name, C=5, N=9):
    if name == "allbg":
        return np.full(N, C, dtype=np.int64)
    if name == "allpos":
        return (np.arange(N, dtype=np.int64) * 2) % C
    if name == "big":          # three labels of class 2 onto cum_samples[2] = 2^24
        return np.array([2, 2, 2, 0, 5, 1, 5, 4, 3], dtype=np.int64)
    raise KeyError(name)


SPECIALS = ("allbg", "allpos", "big")
STATE_CALLS = 3            # consecutive calls on one module (shape m64x80, salts 11, 12, 13)


def state_inputs(k):
    return make_inputs(64, 80, 11 + k, 1)


def special_cum(name, C=5):
    cum = make_cum(C, 1)
    if name == "big":
        cum[2] = np.float32(16777216.0)
    return cum


def unpack(g, key):
    """The per-case arrays of quantity ``key`` (flat; the fixture stores one concatenated array and the lengths)."""
    data, ln = g[key + "_data"], g[key + "_len"]
    off = np.concatenate([[0], np.cumsum(ln)])
    return [data[off[i]:off[i + 1]] for i in range(len(ln))]


def check_generator(g):
    """The fixture was written from these very inputs."""
    for name, _, _, _ in SHAPES:
        for scale in SCALES:
            x, labels, weights = shape_inputs(name, scale)
            assert np.array_equal(labels, g[name + "_labels"]), "input generator drifted from the fixture"
            assert np.array_equal(weights, g[name + "_weights"]), "input generator drifted from the fixture"
            assert float(x.astype(np.float64).sum()) == float(g["%s_x%d_logit_sum" % (name, scale)]), "input generator drifted"
