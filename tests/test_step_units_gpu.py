"""Every conv+BN unit of the REAL bf16 training step against a float64 evaluation of that unit alone (tests/unit_reference.py).

The whole-network comparisons in tests/test_resnet_gpu.py bound each tensor by bf16-route noise (3e-2 .. 0.75): a missing
or mis-scaled term of 20-25 % in one tensor passes them.  Here each unit is evaluated from the inputs the step itself used
(stored bf16 source, bf16 weights, the step's statistics and ReLU decisions, the gradient that arrived at it), so nothing
compounds over layers and the bounds sit at fp32-accumulation / one-bf16-rounding level.  Each configuration first asserts
its route inventory (a later change to the plan cannot silently empty a test) and that the capture is transparent (the
same step with and without it: bit-identical loss and gradient arena)."""
import os
import time

import pytest
import torch

from tests import unit_reference as U
from tests.test_resnet_gpu import DS, _build, _data, damp_residual_branches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, FP32 = torch.bfloat16, torch.float32

# name: (arch, classes, batch, image size, compute dtype, environment)
CONFIGS = {
    # the benchmark's mix of routes at batch 64: 56 x 56 / 28 x 28 stages never store conv3's output and take the producer that
    # recomputes its tile (P / Gram as its by-products at 56 x 56), the 14 x 14 stage takes the stored "sums from the producer"
    "r50_bench_mix": ("resnet50", 1000, 64, 224, BF16, {"IIF_BN3_ALGEBRA_PURE_MIN_ELEMS": "5e7"}),
    # "sums from P" wherever the producer does not recompute the tile, never-stored forward in downsample blocks too
    "r50_sums_from_p": ("resnet50", 1000, 32, 128, BF16, {"IIF_BN3_ALGEBRA_PURE_MIN_ELEMS": "0"}),
    # one stream: no P / Gram by-products, shortcut backward on the compute stream, the pending fused sums set aside
    "r50_one_stream": ("resnet50", 1000, 64, 224, BF16, {"IIF_NO_WGRAD_STREAM": "1"}),
    # grouped 3 x 3 on the fragment kernel, group pack / unpack of the weight gradient
    "rx50_grouped": ("resnext50_32x4d", 365, 32, 128, BF16, {}),
    # BASELINE config 1: basic blocks, option-A shortcut, one stream (the engine's own choice at this size)
    "r32_cifar": ("resnet32", 100, 128, 32, BF16, {"IIF_SIDE_STREAMS": "0"}),
    # exact-fp32 arithmetic: the harness's own conventions (gating, residuals, statistics) must hold to 1e-5
    "r50_fp32": ("resnet50", 1000, 8, 64, FP32, {}),
}

# expected route inventory per configuration (unit_reference.routes)
INVENTORY = {
    "r50_bench_mix": {"alg3": 13, "rx": 7, "nostore": 7, "ds_alg": 1, "pool_fused_bwd": True, "wg_stream": True},
    "r50_sums_from_p": {"alg3": 13, "nostore": 13, "ds_alg": 1, "pool_fused_bwd": True},
    "r50_one_stream": {"alg3": 13, "pg": 0, "ds_alg": 0, "wg_stream": False, "ds_stream": False, "pool_fused_bwd": True},
    "rx50_grouped": {"pool_fused_bwd": True},
    "r32_cifar": {"alg3": 0, "wg_stream": False, "pool_fused_bwd": False},
    "r50_fp32": {"alg3": 0, "rx": 0, "nostore": 0, "pg": 0, "pro": 0, "ds_alg": 0, "pool_fused_bwd": False},
}

# bf16 bounds: the measured worst case over the five bf16 configurations (MI355X; the step is bit-reproducible, so these are
# exact) with 2-4x headroom.  Statistics: mean 3.6e-5, invstd 6.3e-5 (layer4 at batch 32 / 128 x 128: 512 rows, the size of
# one bf16 rounding per element over sqrt(rows); everywhere else <= 1e-6); stored output x 3.7e-3 and activated output y
# 3.3e-3 of the tensor's max (one bf16 rounding), y 1.7e-3 relative L2; ReLU bits: no element disagrees with y > 0;
# dbeta 7.1e-8, dgamma 2.2e-5 (both "sums from P" and the producer's sums); dgrad 2.9e-3 relative L2, 5.7e-3 max;
# the pooled stem: value and arg max exact.
BF16_BOUNDS = {"mean": 1e-4, "invstd": 2e-4, "x": 2 ** -7, "y": 2 ** -7, "y_l2": 4e-3, "bits": 0.0, "dbeta": 3e-7,
               "dgamma": 8e-5, "dw": 2e-2, "dw_rdx": 2e-4, "dgrad": 1e-2, "dgrad_max": 2 ** -6, "pool": 2 ** -8,
               "pool_idx": 2 ** -8}
# dw: 6.9e-3 at most, except the two 1 x 1 convolutions that read the max-pooled stem output (layer1.0.conv1 and, where its
# BN backward is not taken by algebra, layer1.0.downsample.0): 3.1e-2 at batch 64 / 224 x 224 (6.9e-3 at batch 32 / 128).
# That is the bf16 storage of their dx, not the kernel: dw_rdx (the same weight gradient from dx rounded to bf16) is at
# fp32-summation level for them, and the shortcut's weight gradient formed by algebra from fp32 P / Gram is 1e-6 away.
# dW = sum_rows dx (x - mean x) while the rounding error of dx multiplies x itself: the pooled stem output (a max over nine
# ReLU outputs) has a mean large against its spread, and 200 704 rows of independent roundings do not cancel.
# dw_rdx: 4.9e-5 at most over every unit (the weight-gradient kernels reproduce the product of their stored operands), the stem
# included: the space-to-depth 7 x 7 stem of the ImageNet networks is 1.2e-5 .. 2.3e-5 away (fp32 mode 2.3e-7; the CIFAR 3 x 3 stem
# 1.5e-5).  Until the reference rounded the gradient behind the max pool it read 2.2e-3 .. 2.3e-3 in every bf16 configuration:
# a pixel that is the arg max of several windows receives the SUM of up to four pooled gradients, and the step rounds that sum
# to bf16 before the normalisation pass (in registers in iif_bn_backward_pool_fused, by storing the tensor on the unfused
# route) while the reference kept it in float64.  With the rounding alone (sums taken from the rounded tensor as well) the stem
# measured 2.0e-4 .. 2.5e-4, dgamma 3.7e-3 .. 4.8e-3 and dbeta 1.8e-2 .. 2.6e-2: the kernels form the two column sums from the
# pooled gradients themselves, unrounded, and the reference now does the same (unit_reference.bn_backward, gy_sums).
POOL_FED = ("layer1.0.conv1", "layer1.0.downsample.0")


def bf16_bound(unit, metric):
    if metric == "dw" and unit in POOL_FED:
        return 8e-2
    return BF16_BOUNDS.get(metric)


FP32_BOUND = 1e-5


def run_config(name, monkeypatch):
    """Build the configuration, take one step without and one with the capture; returns (net, capture, inventory, metrics)."""
    from iif_amd.custom import IIFLoss
    arch, C, B, hw, dt, env = CONFIGS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    counts = [max(int(1000 * (5 / 1000) ** (i / (C - 1.0))), 1) for i in range(C)]
    net, sd = _build(arch, C, dt)
    if not arch.startswith("resnet3") and not arch.startswith("resnet2"):
        net.load_state_dict(damp_residual_branches(sd, arch))
    x, y = _data(B, hw, counts, seed=41)
    xd, yd = x.to(DEV), y.to(DEV)
    crit = IIFLoss(DS(counts), variant="raw")
    net.train()
    loss0, g0 = U.run_step(net, xd, yd, crit)
    cap = U.StepCapture()
    loss1, g1 = U.run_step(net, xd, yd, crit, capture=cap)
    # the capture only adds clones on the streams: the step it observes is the step without it
    assert loss1 == loss0 and torch.equal(g1, g0), name
    del g0, g1
    inv = U.routes(net._saved, cap)
    t0 = time.time()
    met = U.check_step(net, xd, cap)
    torch.cuda.synchronize()
    print("\n[%s] routes %s, reference %.1f s, peak %.1f GB" % (name, inv, time.time() - t0,
                                                               torch.cuda.max_memory_allocated() / 2 ** 30))
    for k, (v, unit) in sorted(U.worst(met).items()):
        print("  worst %-10s %.3e  %s" % (k, v, unit))
    if os.environ.get("UNIT_REF_VERBOSE"):
        for unit, m in met.items():
            print("  %-26s %s" % (unit, " ".join("%s=%.2e" % kv for kv in sorted(m.items()))))
    return net, cap, inv, met, (xd, yd, crit)


def _check_inventory(name, inv):
    for k, v in INVENTORY[name].items():
        assert inv[k] == v, (name, k, inv[k], v, inv)
    if name == "r50_bench_mix":
        assert inv["pg"] >= 1 and inv["pro_rows"] >= 1 and inv["alg3_pure"] == 0


@pytest.mark.parametrize("name", [n for n in CONFIGS if CONFIGS[n][4] == BF16])
def test_bf16_units_against_float64(name, monkeypatch):
    """Measured worst cases per configuration (MI355X; dw: the pooled-stem units at 224 x 224; the stem's dw_rdx in brackets):
        r50_bench_mix    dgamma 2.0e-5  dw 3.1e-2  dw_rdx 3.2e-5 (1.2e-5)  dgrad 2.9e-3  invstd 2.9e-5  y 3.2e-3
        r50_sums_from_p  dgamma 2.2e-5  dw 6.9e-3  dw_rdx 4.9e-5 (2.1e-5)  dgrad 2.9e-3  invstd 6.3e-5  y 3.3e-3
        r50_one_stream   dgamma 2.0e-5  dw 3.1e-2  dw_rdx 3.7e-5 (1.5e-5)  dgrad 2.9e-3  invstd 2.9e-5  y 3.2e-3
        rx50_grouped     dgamma 1.1e-5  dw 6.3e-3  dw_rdx 2.9e-5 (2.3e-5)  dgrad 2.9e-3  invstd 5.9e-5  y 3.2e-3
        r32_cifar        dgamma 1.5e-7  dw 3.8e-3  dw_rdx 3.1e-5 (1.5e-5)  dgrad 2.6e-3  invstd 4.7e-6  y 3.3e-3"""
    net, cap, inv, met, _ = run_config(name, monkeypatch)
    _check_inventory(name, inv)
    assert len(met) == len(net._saved.units), (len(met), len(net._saved.units))
    bad = U.failures(met, bf16_bound)
    assert not bad, bad


def test_fp32_units_against_float64(monkeypatch):
    """Self-check of the harness: exact-fp32 arithmetic agrees with the float64 evaluation of every unit to 1e-5
    (measured: 2.1e-6 at worst, the stored convolution output of layer4.0.conv2; every gradient <= 8.3e-7)."""
    net, cap, inv, met, _ = run_config("r50_fp32", monkeypatch)
    _check_inventory("r50_fp32", inv)
    assert len(met) == len(net._saved.units)
    bad = U.failures(met, lambda unit, k: FP32_BOUND)
    assert not bad, bad


def test_negative_controls_flag_exactly_the_affected_unit(monkeypatch):
    """The bounds catch what the whole-network comparisons cannot: (a) one algebra unit's weight gradient scaled by 0.8,
    (b) one unit's invstd row shifted by 5 %, (c) the column sums that bn2's prologue left for one algebra unit dropped before
    backward (its weight gradient then misses the D (x) colsum(a2) term).  Each is reported for that unit and no other."""
    from iif_amd import resnet_engine
    net, cap, inv, met, (xd, yd, crit) = run_config("r50_sums_from_p", monkeypatch)
    assert not U.failures(met, bf16_bound)
    plan = net._saved
    names = U.unit_names(net)
    alg = [u for u in plan.units if cap.records.get(id(u), {}).get("alg")]
    flagged = lambda m: {unit for unit, _, _, _ in U.failures(m, bf16_bound)}      # noqa: E731
    # (a) the result of one alg3 unit scaled by 0.8
    u = alg[len(alg) // 2]
    u.conv._g2d.mul_(0.8)
    m1 = U.check_step(net, xd, cap)
    assert flagged(m1) == {names[id(u.conv)]}, U.failures(m1, bf16_bound)
    u.conv._g2d.div_(0.8)
    # (b) one statistics row shifted by 5 %
    v = plan.blocks[5]["units"][1]
    v.stats[1].mul_(1.05)
    m2 = U.check_step(net, xd, cap)
    assert flagged(m2) == {names[id(v.conv)]}, U.failures(m2, bf16_bound)
    v.stats[1].div_(1.05)
    # (c) one prologue column-sum compensation dropped between forward and backward
    target = next(w for w in alg if plan._route(w).csum_rows)
    orig = resnet_engine._Plan.backward

    def backward(self, reducer=None):
        self.c3[target].sums.zero_()
        return orig(self, reducer)

    monkeypatch.setattr(resnet_engine._Plan, "backward", backward)
    cap2 = U.StepCapture()
    U.run_step(net, xd, yd, crit, capture=cap2)
    m3 = U.check_step(net, xd, cap2)
    assert flagged(m3) == {names[id(target.conv)]}, U.failures(m3, bf16_bound)

