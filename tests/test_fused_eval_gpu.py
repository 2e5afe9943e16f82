"""The fused inference forward on the device.

Bit-identity to the present route is the tolerance everywhere: iif_conv_igemm_affine against iif_conv_igemm followed by
iif_bn_apply per kernel family (each case pins the family through iif_conv_affine_route - the launch routing walked without
launching - under the IIF_CONV_* switches it sets), iif_bn_fold against the torch arithmetic of the present route, whole
networks fused against unfused on the same model object, and evaluate() with --fused-eval against the run without it."""
import os
import subprocess
import sys

import pytest
import torch

from tests.fused_eval_cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BF = torch.bfloat16


@pytest.fixture
def conv_env(monkeypatch):
    """Set convolution switches AND make the library read them again (it caches them when it is loaded)."""
    from iif_amd import _lib

    def set_(**kw):
        for k, v in kw.items():
            monkeypatch.setenv(k, v)
        _lib.check(_lib.lib().iif_conv_reload_env(), "iif_conv_reload_env")
    yield set_
    monkeypatch.undo()
    _lib.lib().iif_conv_reload_env()


def _pack_frag(w2d, rows, taps, k):
    from iif_amd import ops
    tab, blocks = ops.pack_table([(0, 0, rows, taps, k, w2d.shape[1])], DEV)
    return ops.pack_fragments(w2d, tab, 1, blocks, torch.empty(rows * taps * k, dtype=w2d.dtype, device=DEV))


def _pack_g16(w2d, width):
    from iif_amd import ops
    tab, blocks = ops.pack_table_g16([(0, 0, width, 9, 64, w2d.shape[1])], DEV)
    return ops.pack_fragments_g16(w2d, tab, 1, blocks, torch.empty(width // 64 * 20 * 512, dtype=w2d.dtype, device=DEV)), 1


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_affine_epilogue_is_bit_identical_to_conv_then_bn_apply(case, conv_env):
    from iif_amd import ops
    name, n, hw, cin, cout, k, stride, chunks, frag, env, expect = case
    conv_env(**env)
    pad = k // 2
    ho, wo = ops.conv_out_hw(hw, hw, k, k, stride, pad)
    m = n * ho * wo
    cs, cd = cin // chunks, cout // chunks
    ldw = k * k * cs
    g = torch.Generator().manual_seed(len(name) * 1009 + n + hw + cin + cout)
    x = torch.relu(torch.randn(n, hw, hw, cin, generator=g)).to(BF).to(DEV)
    w = (torch.randn(cout, ldw, generator=g) / ldw ** 0.5).to(BF).to(DEV)
    res = torch.randn(n, ho, wo, cout, generator=g).to(BF).to(DEV)
    stats, stats2 = torch.zeros(4, cout), torch.zeros(4, cout)
    for s_ in (stats, stats2):                      # a of both signs and magnitudes, b around the activation's scale
        s_[2] = (torch.rand(cout, generator=g) + 0.25) * torch.where(torch.rand(cout, generator=g) < 0.2, -1.0, 1.0)
        s_[3] = torch.randn(cout, generator=g) * 0.3
    stats, stats2 = stats.to(DEV), stats2.to(DEV)
    wf = None
    if frag == "frag":
        wf = _pack_frag(w, cout, 9, cs)
    elif frag == "g16":
        wf = _pack_g16(w, cout)
    y = ops.conv_forward(x, w, k, k, stride, pad, groups=chunks, w_frag=wf)
    assert tuple(y.shape) == (n, ho, wo, cout)
    ref, bits_ref = torch.empty_like(y), torch.zeros(m * cout // 8, dtype=torch.uint8, device=DEV)
    for r_, rs_ in ((None, None), (res, None), (res, stats2)):
        ops.bn_apply(y.view(m, cout), stats, ref.view(m, cout), relu=True, residual=None if r_ is None else r_.view(m, cout),
                     residual_stats=rs_, relu_bits=bits_ref)
        for want_bits in (False, True):
            route = ops.conv_affine_route(n, hw, hw, cs, ho, wo, cd, k, k, stride, pad, ldw, groups=chunks, has_res=r_ is not None,
                                          has_res_affine=rs_ is not None, has_relu_bits=want_bits, w_frag=wf)
            assert route == expect[(rs_ is not None, want_bits)], (route, r_ is not None, rs_ is not None, want_bits)
            out = torch.full_like(y, float("nan"))
            bits = torch.full_like(bits_ref, 0xAA) if want_bits else None
            ops.conv_forward_affine(x, w, k, k, stride, pad, out, stats, res=r_, res_affine=rs_, relu_bits=bits, groups=chunks,
                                    w_frag=wf)
            assert torch.equal(out, ref), (route, r_ is not None, rs_ is not None, want_bits)
            if want_bits:
                assert torch.equal(bits, bits_ref), (route, r_ is not None, rs_ is not None)
    assert (ref != 0).float().mean().item() > 0.05           # (the comparison is not one of all-zero tensors)


def test_affine_entry_refuses_what_it_has_no_instance_for():
    from iif_amd import _lib, ops
    x = torch.zeros(2, 8, 8, 64, device=DEV)
    w = torch.zeros(64, 576, device=DEV)
    out, stats = torch.empty(2, 8, 8, 64, device=DEV), torch.zeros(4, 64, device=DEV)
    with pytest.raises(_lib.IIFNativeError, match="UNSUPPORTED"):
        ops.conv_forward_affine(x, w, 3, 3, 1, 1, out, stats)                       # fp32
    assert ops.conv_affine_route(2, 8, 8, 60, 8, 8, 64, 3, 3, 1, 1, 540) == "none"


def test_bn_fold_matches_the_torch_arithmetic_bit_for_bit():
    """iif_bn_fold against _eval_stats (the present route) over a few thousand channels in layers of every width class,
    variances from denormal-small to huge, gains of both signs."""
    from iif_amd import ops
    from iif_amd.resnet_engine import BN_EPS, BNParam, _eval_stats
    g = torch.Generator().manual_seed(77)
    widths = [16, 32, 64, 64, 128, 256, 512, 1024, 2048, 40, 8, 1000]
    bns, stats = [], []
    for i, c in enumerate(widths):
        bn = BNParam(c).to(DEV)
        with torch.no_grad():
            bn.weight.copy_(torch.randn(c, generator=g) * (10.0 ** torch.randint(-3, 3, (c,), generator=g).float()))
            bn.bias.copy_(torch.randn(c, generator=g) * 3)
            bn.running_mean.copy_(torch.randn(c, generator=g) * (10.0 ** torch.randint(-4, 4, (c,), generator=g).float()))
            rv = torch.rand(c, generator=g) * (10.0 ** torch.randint(-12, 12, (c,), generator=g).float())
            rv[::7] = 0.0
            rv[1::11] = 1e-38
            rv[2::13] = 3e38
            bn.running_var.copy_(rv)
        bns.append(bn)
        stats.append(torch.full((4, c), float("nan"), device=DEV))
    table = ops.bn_fold_table([(b.weight.detach(), b.bias.detach(), b.running_mean, b.running_var, s) for b, s in zip(bns, stats)], DEV)
    ops.bn_fold(table, len(bns), BN_EPS)
    torch.cuda.synchronize()
    assert sum(widths) > 5000
    for b, s in zip(bns, stats):
        ref = torch.empty_like(s)
        _eval_stats(b, ref)
        assert torch.equal(s, ref), (b.num_features, (s != ref).nonzero()[:4].tolist())


# ------------------------------------------------------------------------------------------------ whole networks
def _build(arch, num_classes=100):
    from iif_amd import resnet_cifar, resnet_pytorch
    torch.manual_seed(1234)
    if hasattr(resnet_cifar, arch):
        net = getattr(resnet_cifar, arch)(num_classes=num_classes, use_norm="None", compute_dtype=BF)
    else:
        net = getattr(resnet_pytorch, arch)(num_classes=num_classes, use_norm="None", pretrained="None", compute_dtype=BF)
    return net


def seed_bn(net, seed=5):
    """Running statistics and BN gains / offsets set to seeded non-trivial values (a freshly built model has mean 0, var 1)."""
    from iif_amd.resnet_engine import BNParam
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, BNParam):
                c = m.num_features
                m.running_mean.copy_((torch.randn(c, generator=g) * 0.2).to(DEV))
                m.running_var.copy_((torch.rand(c, generator=g) * 1.5 + 0.25).to(DEV))
                m.weight.copy_((torch.rand(c, generator=g) * 0.8 + 0.4).to(DEV))
                m.bias.copy_((torch.randn(c, generator=g) * 0.1).to(DEV))


def _eval_logits(net, x, fused):
    net.eval()
    net.set_fused_eval(fused)
    with torch.no_grad():
        out = net(x)
    torch.cuda.synchronize()
    return out


NETWORKS = [("resnet32", 8, 32), ("se_resnet32", 8, 32), ("resnet18", 8, 64), ("resnet50", 8, 64), ("wide_resnet50_2", 4, 64),
            ("resnext50_32x4d", 8, 64), ("se_resnet50", 4, 64), ("resnet50", 256, 224), ("resnet32", 128, 32)]


@pytest.mark.parametrize("arch,B,hw", NETWORKS, ids=["%s_%dx%d" % c for c in NETWORKS])
def test_fused_eval_logits_equal_the_unfused_ones(arch, B, hw):
    net = _build(arch)
    seed_bn(net)
    x = torch.randn(B, 3, hw, hw, generator=torch.Generator().manual_seed(B + hw)).to(DEV)
    plain = _eval_logits(net, x, False)
    fused = _eval_logits(net, x, True)
    assert torch.isfinite(plain).all() and plain.abs().max().item() > 0
    assert torch.equal(fused, plain)
    # the routing list is what ran: every unit it calls fused went through the affine entry, nothing else did
    from iif_amd import ops
    calls = []
    orig = ops.conv_forward_affine
    try:
        ops.conv_forward_affine = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        again = _eval_logits(net, x, True)
    finally:
        ops.conv_forward_affine = orig
    assert torch.equal(again, plain)
    assert len(calls) == sum(r == "fused" for _, r in net.eval_route(B, hw, hw)) > 0
    # a write to the running statistics is seen by the next forward (nothing cached)
    with torch.no_grad():
        net.bn1.running_mean.add_(0.5)
    moved_f = _eval_logits(net, x, True)
    moved_p = _eval_logits(net, x, False)
    assert torch.equal(moved_f, moved_p) and not torch.equal(moved_p, plain)


@pytest.mark.parametrize("arch,B,hw", [("resnet50", 8, 64), ("resnet32", 16, 32), ("resnext50_32x4d", 4, 64)])
def test_fused_eval_between_training_steps_leaves_the_trajectory_alone(arch, B, hw):
    """The plan's buffers are shared with the training route: train 2 steps -> fused eval -> train 2 steps gives the same four
    losses and final weights, bit for bit, as four uninterrupted steps."""
    from iif_amd.custom import IIFLoss

    class DS:
        def get_cls_num_list(self):
            return [max(int(500 * 0.97 ** i), 2) for i in range(100)]

    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, 3, hw, hw, generator=g).to(DEV)
    y = torch.randint(0, 100, (B,), generator=g).to(DEV)
    runs = []
    for interrupt in (False, True):
        net = _build(arch)
        seed_bn(net)
        net.set_fused_eval(True)
        crit = IIFLoss(DS(), variant="raw")
        losses = []
        for it in range(4):
            if interrupt and it == 2:
                net.eval()
                with torch.no_grad():
                    net(x)
            net.train()
            loss, _ = net.loss_and_backward(x, y, crit)
            net.sgd_step(0.05)
            losses.append(loss.item())
        torch.cuda.synchronize()
        runs.append((losses, net._arena.clone(), net._rstat.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


# ------------------------------------------------------------------------------------------------ evaluate()
def test_evaluate_with_fused_eval_reports_the_same_numbers():
    sys.path.insert(0, HERE)
    import fused_eval_ddp_worker as W
    plain, fused = W.run(False), W.run(True)
    assert plain["lines"] == fused["lines"] and len(plain["lines"]) == 3, (plain, fused)
    assert fused["fused"] is True and plain["fused"] is False


def test_evaluate_with_fused_eval_on_two_ranks(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", IIF_REHEARSE_ONE_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29583", os.path.join(HERE, "fused_eval_ddp_worker.py"), str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    got = torch.load(tmp_path / "rank0.pt")
    assert got["plain"]["lines"] == got["fused"]["lines"] and len(got["fused"]["lines"]) == 3, got
    assert got["fused"]["fused"] is True and got["world"] == 2
