"""The ticketed scalar-loss reduction shared by the fused loss heads (iif_amd/csrc/loss_reduce.h), through all nine entries
that finish with it: iif_ce_fwd_bwd, iif_sigmoid_focal_fwd_bwd, iif_bce_det_fwd_bwd, iif_bbox_reg_fwd and the Seesaw loss
(float sums), and the read-free BBoxHead.loss entries iif_head_loss_fwd, iif_head_loss_cums_fwd, iif_head_bce_loss_fwd and
iif_seesaw_head_fwd, whose integer counts travel beside the loss.

The finish has three regimes, and every entry runs in each of them with the smallest input that gets there (fp32, a tiny
class count; the block counts are read off each head's launch code):

  one   one block: the block that publishes is the block that sums.
  few   2 .. 255 blocks: a last block of 256 threads reads at most one partial per thread.
  many  more than 256 blocks: the last block's strided loop over the partials takes a second trip.

  entry                      grid                                                          one      few      many
  iif_ce_fwd_bwd             ceil(B / 4) (four rows per block; cap 512)                    B = 4    37: 10   1200: 300
  iif_sigmoid_focal_fwd_bwd  ceil(B / 4) (cap: the workspace's partial slots)              B = 4    37: 10   1200: 300
  iif_bce_det_fwd_bwd        b = ceil(N C / 4 / 256) one-vector blocks, spread over at     N C =    10240:   1048580:
                             most 256 blocks while a thread has <= 4 vectors; beyond       15       10       257
                             (b > 1024) ceil(b / 4) blocks of whole four-vector steps
  iif_bbox_reg_fwd           ceil(n / 4 / 256) (a box per lane; cap 1024)                  n = 8    10240:   262148:
                                                                                                    10       257
  Seesaw (SeesawLoss)        ceil(N / 4) (cap 512)                                         N = 4    37: 10   1200: 300
  iif_head_loss_fwd, iif_head_loss_cums_fwd, iif_head_bce_loss_fwd, iif_seesaw_head_fwd
                             ceil(N / 4) (cap 512)                                         N = 4    37: 10   1200: 300

(The detection BCE kernel has a one-element-per-lane form for pitched rows that reaches 257 blocks at a quarter of the
elements; the contiguous 16-byte form is the one mmdet's tensors take, so that one is run.)

Per case: the scalar equals scale times the float64 sum of the per-row / per-element losses the SAME launch wrote, within the
relative bound the head's own test file puts on its scalar loss (test_iif_head_gpu.py 2e-6, test_focal_head_gpu.py 1e-5,
test_mmdet_ce_gpu.py / test_bbox_reg_gpu.py / test_seesaw_gpu.py REL = 1e-4); a second call on the same workspace is
bit-identical in loss, rows and gradient; the ticket word reads 0 afterwards.  And the contract custom._workspace relies on
when it hands one ticket buffer to every head: the four CE-workspace entries back to back on one workspace, zeroed once,
give the bits they give on a fresh one.

The four BBoxHead.loss entries (fp32; 8 softmax, 4 sigmoid, 3 + 2 Seesaw columns; one row in four of weight 0 and a few
negative weights, so that the rows that count are not N and the three sums differ) are held to the float64 restatements of
their own test files: avg_factor and the accuracies exactly, each loss within (columns + 16) 2^-24 sum|term| (the
fixture-free bound of test_head_loss_kinds_gpu.py's 16400-row case), a second call bit-identical in every output, the ticket
word 0 afterwards.  The three of head_loss.hip run on the CE workspace in production with a partial layout of their own (word
4 onwards, three words per block), so they take part in the back-to-back test."""
import functools

import numpy as np
import pytest
import torch

from . import bbox_head_loss_cases as bc
from . import fasa_head_cases as fc
from . import head_loss_kinds_cases as kc

pytestmark = pytest.mark.gpu
DEV = "cuda"
REGIMES = ("one", "few", "many")
SCALE = 0.37
#           one  few    many      (rows for CE / focal / Seesaw and for BCE, whose rows have 3 / 4 / 4 columns; elements for bbox)
SIZES = {"ce": (4, 37, 1200), "focal": (4, 37, 1200), "bce": (5, 2560, 262145), "bbox": (8, 10240, 262148),
         "seesaw": (4, 37, 1200)}
TOL = {"ce": 2e-6, "focal": 1e-5, "bce": 1e-4, "bbox": 1e-4, "seesaw": 1e-4}
CE_HEADS = ("ce", "focal", "bce", "bbox")
HEAD_ROWS = (4, 37, 1200)
HEAD_COLS = {"head_ce": 8, "head_cums": 8, "head_bce": 4, "head_seesaw": 3 + 2}
HEADS = tuple(HEAD_COLS)
HEADS_ON_CE_WORKSPACE = ("head_ce", "head_cums", "head_bce")
SEESAW_CUM = (900.0, 30.0, 2.0, 5000.0)
SEESAW_P, SEESAW_Q = 0.8, 2.0


def _ce_workspace():
    from iif_amd.loss_reduction import CE_WORKSPACE_WORDS
    return torch.zeros(CE_WORKSPACE_WORDS, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _inputs(head, regime):
    """Device inputs of one case, made once and never written."""
    n = SIZES[head][REGIMES.index(regime)]
    g = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + sorted(SIZES).index(head))
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)                       # noqa: E731
    if head == "ce":
        return rnd(n, 8) * 3, torch.randint(0, 8, (n,), generator=g).to(DEV), torch.ones(8, device=DEV)
    if head == "focal":
        return rnd(n, 5) * 3, torch.randint(0, 5, (n,), generator=g).to(DEV)
    if head == "bce":
        C = 3 if regime == "one" else 4
        return rnd(n, C) * 3, torch.randint(0, C + 1, (n,), generator=g).to(DEV)      # label C: a background row
    if head == "bbox":
        return rnd(n), rnd(n), torch.rand(n, generator=g).to(DEV)
    return rnd(n, 3 + 2) * 3, (torch.arange(n) % 4).to(DEV)                           # Seesaw: C = 3, label 3 the background


def _run(head, regime, ws):
    """One launch on the workspace ``ws``.  Returns (scalar losses [K], rows or elements [K, n], gradient, scales [K])."""
    from iif_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    inp = _inputs(head, regime)
    x = inp[0]
    loss = torch.full((1,), -1.0, device=DEV)
    if head == "ce":
        B, C = x.shape
        rows, d = torch.empty(B, device=DEV), torch.empty_like(x)
        rc = L.iif_ce_fwd_bwd(p(x), 0, C, p(inp[2]), p(inp[1]), None, 1.0, None, None, -100, SCALE, B, C, p(rows), p(loss), p(d),
                              C, None, p(ws), st)
    elif head == "focal":
        B, C = x.shape
        rows, d = torch.empty(B, device=DEV), torch.empty_like(x)
        rc = L.iif_sigmoid_focal_fwd_bwd(p(x), 0, C, p(inp[1]), None, 1.0, None, 2.0, 1, 0.25, SCALE, B, C, p(rows), p(loss),
                                         p(d), C, None, p(ws), st)
    elif head == "bce":
        N, C = x.shape
        rows, d = torch.empty_like(x), torch.empty_like(x)
        rc = L.iif_bce_det_fwd_bwd(p(x), 0, C, p(inp[1]), None, -100, None, None, None, SCALE, N, C, p(rows), p(loss), p(d), C,
                                   p(ws), st)
    else:
        n = x.numel()
        rows, d = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        rc = L.iif_bbox_reg_fwd(p(x), 0, 4, None, 1, 1, p(inp[1]), p(inp[2]), 1.0 / 9.0, SCALE, n, 0, p(rows), p(loss), p(d),
                                p(ws), st)
    assert rc == 0
    return loss, rows.reshape(1, -1), d, (SCALE,)


def _run_seesaw(regime):
    """The Seesaw loss launch of a SeesawLoss module (its parameters and counters; the counters are not updated, so that
    the second call sees the first one's).  Scales: 'sum' with a loss weight for the classes, a mean for the objectness."""
    from iif_amd import mmdet_seesaw_loss as S
    x, lab = _inputs("seesaw", regime)
    m = _seesaw_module()
    scales = (SCALE, 1.7 / x.shape[0])
    losses, rows, d = S._launch(x, lab, None, m.cum_samples, False, m.p, m.q, m.eps, scales[0], False, scales[1], m.num_classes,
                                True)
    return losses, rows, d, scales


@functools.lru_cache(maxsize=None)
def _seesaw_module():
    from iif_amd.mmdet_seesaw_loss import SeesawLoss
    m = SeesawLoss(num_classes=3, device=DEV)
    m.cum_samples.copy_(torch.tensor([900.0, 30.0, 2.0, 5000.0]))
    return m


def _seesaw_ticket():
    from iif_amd import _lib
    from iif_amd import mmdet_seesaw_loss as S
    return S._workspace(_inputs("seesaw", "one")[0].device, _lib.stream_ptr())["loss"]


@functools.lru_cache(maxsize=None)
def _fresh(head, regime):
    """The case on a workspace of its own, zeroed: (first call, second call, ticket word after each)."""
    ws = _ce_workspace()
    a = _run(head, regime, ws)
    ta = int(ws[0].item())
    b = _run(head, regime, ws)
    return a, b, (ta, int(ws[0].item()))


def _check(head, a, b, tickets):
    loss, rows, d, scales = a
    for k, s in enumerate(scales):
        want = s * float(rows[k].double().sum().item())
        got = float(loss[k].item())
        print("%s sum %d: loss %.9g, scale x float64 sum of the rows %.9g, relative difference %.3g"
              % (head, k, got, want, abs(got - want) / abs(want)))
        assert want != 0.0 and abs(got - want) <= TOL[head] * abs(want)
    assert torch.equal(loss, b[0]) and torch.equal(rows, b[1]) and torch.equal(d, b[2])
    assert tickets == (0, 0)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("head", CE_HEADS)
def test_scalar_is_the_sum_of_the_rows_repeats_bitwise_and_rezeroes_the_ticket(head, regime):
    _check(head, *_fresh(head, regime))


@pytest.mark.parametrize("regime", REGIMES)
def test_seesaw_both_scalars(regime):
    """K = 2: the class and the objectness loss leave the launch together (ticket at word 0 of the Seesaw workspace)."""
    ws = _seesaw_ticket()
    a = _run_seesaw(regime)
    ta = int(ws[0].item())
    b = _run_seesaw(regime)
    _check("seesaw", a, b, (ta, int(ws[0].item())))
    # and through the module's forward, which also counts the batch: the same counters give the same bits
    m = _seesaw_module()
    x, lab = _inputs("seesaw", regime)
    cum = m.cum_samples.clone()
    outs = []
    for _ in range(2):
        outs.append(m(x, lab, reduction_override="sum"))
        m.cum_samples.copy_(cum)
        assert int(ws[0].item()) == 0
    for key in ("loss_cls_classes", "loss_cls_objectness"):
        assert torch.isfinite(outs[0][key]) and torch.equal(outs[0][key], outs[1][key])


# ---------------------------------------------------------------------------------------- the BBoxHead.loss entries
@functools.lru_cache(maxsize=None)
def _head_inputs(head, regime):
    """Host inputs of one case, made once and never written: scores, labels, label weights, the softmax table."""
    n, cols = HEAD_ROWS[REGIMES.index(regime)], HEAD_COLS[head]
    g = torch.Generator().manual_seed(7000 + 10 * REGIMES.index(regime) + HEADS.index(head))
    x = torch.randn(n, cols, generator=g) * 3
    classes = cols - 2 if head == "head_seesaw" else cols
    top = classes if head in ("head_ce", "head_cums") else classes + 1               # sigmoid / Seesaw: label C is the background
    lab = torch.randint(0, top, (n,), generator=g)
    lab[1], lab[2] = 0, 1                                                            # the four-row case has rows with a class target
    w = 0.5 + torch.rand(n, generator=g)
    w[3::7] = -w[3::7]
    w[0::4] = 0.0
    return x, lab, w, 0.5 + torch.rand(cols, generator=g)


@functools.lru_cache(maxsize=None)
def _head_device_inputs(head, regime):
    return tuple(t.to(DEV) for t in _head_inputs(head, regime))


@functools.lru_cache(maxsize=None)
def _head_restated(head, regime):
    """dict(avg, acc: the float32 accuracies, losses: (float64 loss, the sum of its |terms|) each)."""
    x, lab, w, tab = (t.numpy() for t in _head_inputs(head, regime))
    if head == "head_ce":
        r = bc.restate64(x, tab, lab, w, None, -100, SCALE)
        return dict(avg=r["avg"], acc=[r["acc"]], losses=[(r["loss"], r["sum_abs"])])
    if head == "head_cums":
        r = fc.cums_restate(x, tab, lab, w, SCALE)
        return dict(avg=r["avg"], acc=[r["acc"]], losses=[(r["loss"], r["sum_abs"])])
    if head == "head_bce":
        r = kc.restate_sigmoid(x, lab, w, None, -100, SCALE)
        return dict(avg=r["avg"], acc=[r["acc"][0]], losses=[(r["loss"], r["sum_abs"])])
    r = kc.restate_seesaw(x, lab, w, np.array(SEESAW_CUM, dtype=np.float32), HEAD_COLS[head] - 2, SEESAW_P, SEESAW_Q, SCALE)
    return dict(avg=r["avg"], acc=[r["acc_obj"][0], r["acc_cls"][0]],
                losses=[(r["loss_cls"], r["sum_abs_cls"]), (r["loss_obj"], r["sum_abs_obj"])])


def _head_workspace(head):
    if head == "head_seesaw":
        from iif_amd.mmdet_bbox_head_loss import SEESAW_HEAD_WORKSPACE_WORDS
        return torch.zeros(SEESAW_HEAD_WORKSPACE_WORDS, dtype=torch.int32, device=DEV)
    return _ce_workspace()


def _run_head(head, regime, ws):
    """One call on the workspace ``ws``: every output tensor - (losses, acc, avg, gradient, ...) - with accumulators that start
    from the same values each time."""
    from iif_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    x, lab, w, tab = _head_device_inputs(head, regime)
    N, C = x.shape
    f = lambda *shape: torch.full(shape, -1.0, device=DEV)                        # noqa: E731
    acc, avg, d, status = f(2), f(1), torch.empty_like(x), torch.zeros(1, dtype=torch.int32, device=DEV)
    if head == "head_ce":
        loss = f(1)
        rc = L.iif_head_loss_fwd(p(x), 0, C, p(tab), p(lab), p(w), None, -100, SCALE, N, C, p(d), C, p(loss), p(acc), p(avg), p(status),
                                 p(ws), st)
        out = (loss, acc[:1], avg, d)
    elif head == "head_cums":
        loss, rows, cl, cn = f(1), f(N), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        rc = L.iif_head_loss_cums_fwd(p(x), 0, C, p(tab), p(lab), p(w), None, -100, SCALE, N, C, p(d), C, p(rows), p(cl), p(cn), p(loss),
                                      p(acc), p(avg), p(status), p(ws), st)
        out = (loss, acc[:1], avg, d, rows, cl, cn)
    elif head == "head_bce":
        loss = f(1)
        rc = L.iif_head_bce_loss_fwd(p(x), 0, C, p(lab), p(w), None, -100, SCALE, N, C, p(d), C, p(loss), p(acc), p(avg), p(ws), st)
        out = (loss, acc[:1], avg, d)
    else:
        loss, cum = f(3), torch.tensor(SEESAW_CUM, device=DEV)
        rc = L.iif_seesaw_head_fwd(p(x), 0, C, p(lab), p(w), p(cum), SEESAW_P, SEESAW_Q, kc.EPS, SCALE, N, C - 2, p(d), C, p(loss), p(acc),
                                   p(avg), p(status), p(ws), st)
        out = (loss, acc, avg, d, cum)
    assert rc == 0 and int(status.item()) == 0
    return out


@functools.lru_cache(maxsize=None)
def _fresh_head(head, regime):
    """The case on a workspace of its own, zeroed: (first call, second call, ticket word after each)."""
    ws = _head_workspace(head)
    a = _run_head(head, regime, ws)
    ta = int(ws[0].item())
    b = _run_head(head, regime, ws)
    return a, b, (ta, int(ws[0].item()))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("head", HEADS)
def test_head_loss_entries_carry_their_counts_beside_the_loss(head, regime):
    a, b, tickets = _fresh_head(head, regime)
    want = _head_restated(head, regime)
    n = HEAD_ROWS[REGIMES.index(regime)]
    assert 1 < want["avg"] < n                                       # rows of weight 0 are there: the rows that count are not N
    assert float(a[2].item()) == want["avg"]
    assert np.array_equal(a[1].cpu().numpy(), np.array(want["acc"], dtype=np.float32))
    for k, (loss, sum_abs) in enumerate(want["losses"]):
        got = float(a[0][k].item())
        bound = (HEAD_COLS[head] + 16) * 2.0 ** -24 * sum_abs
        print("%s %s loss %d: %.9g, float64 restatement %.9g, difference %.3g of the bound %.3g"
              % (head, regime, k, got, loss, abs(got - loss) / bound, bound))
        assert sum_abs > 0.0 and abs(got - loss) <= bound
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    assert tickets == (0, 0)


def test_one_workspace_serves_every_head_back_to_back():
    """CE, sigmoid focal, detection BCE and box regression, then the three head_loss.hip entries, in turn on ONE workspace,
    zeroed once, one stream, large grids before small ones (stale partials of a larger grid sit behind a smaller one's, and
    those of one layout - a float per block from word 1, or three words per block from word 4 - under the other): every call
    gives the bits it gives on a fresh workspace."""
    ws = _ce_workspace()
    for regime in reversed(REGIMES):
        for head in CE_HEADS:
            got = _run(head, regime, ws)
            want = _fresh(head, regime)[0]
            assert all(torch.equal(g, w) for g, w in zip(got[:3], want[:3])), (head, regime)
        for head in HEADS_ON_CE_WORKSPACE:
            got = _run_head(head, regime, ws)
            want = _fresh_head(head, regime)[0]
            assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want)), (head, regime)
    assert int(ws[0].item()) == 0
