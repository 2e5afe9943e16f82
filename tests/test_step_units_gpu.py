"""Every conv+BN unit of the REAL bf16 training step against a float64 evaluation of that unit alone (tests/unit_reference.py).

The whole-network comparisons in tests/test_resnet_gpu.py bound each tensor by bf16-route noise (3e-2 .. 0.75): a missing
or mis-scaled term of 20-25 % in one tensor passes them.  Here each unit is evaluated from the inputs the step itself used
(stored bf16 source, bf16 weights, the step's statistics and ReLU decisions, the gradient that arrived at it), so nothing
compounds over layers and the bounds sit at fp32-accumulation / one-bf16-rounding level.  Each configuration first asserts
its route inventory (a later change to the plan cannot silently empty a test) and that the capture is transparent (the
same step with and without it: bit-identical loss and gradient arena).

Squeeze-and-excitation blocks get one more entry each (``<block>.se``): how ``_Plan`` wires the SE kernels inside a step - the
squeeze of the stored x, the BN affine folded into the excitation, the apply fused with the identity or the normalised
shortcut, the in-place mask of g, the sums, the excitation's backward and both weight gradients, and G = g~ e + o - stage by
stage from what the step stored (SE_BOUNDS).  Their excitation weights are scaled (SE_GATE_SCALE: 8 for se_resnet50, 2 for
se_resnet32) so that the gate path o is visible under one bf16 rounding of G; the SE controls show that a scaled weight
gradient, a stale gate and a dropped o are each reported for their block and nothing else."""
import os
import time

import pytest
import torch

from oracle import resnet_oracle as R
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
    # squeeze-and-excitation bottlenecks: the smallest size at which BF16_BOUNDS were measured (layer4 has 512 rows, and invstd
    # scales with 1 / sqrt(rows)); SE around the identity and around the normalised shortcut
    "se_r50": ("se_resnet50", 1000, 32, 128, BF16, {}),
    # SE basic blocks behind the option-A shortcut, reduction 4, one stream (as r32_cifar)
    "se_r32_cifar": ("se_resnet32", 100, 128, 32, BF16, {"IIF_SIDE_STREAMS": "0"}),
    # ImageNet basic blocks: a 3 x 3 block-closing unit meets a convolutional shortcut (on the shortcut stream) and the
    # fused stem pool
    "r18_basic": ("resnet18", 365, 32, 128, BF16, {}),
    # exact-fp32 arithmetic for the SE conventions (gate, residual, masked identity path, ungated block-input gradient)
    "se_r50_fp32": ("se_resnet50", 1000, 8, 64, FP32, {}),
    # the benchmark's mix of routes under a compute-unit budget (CU_BUDGET), forward and backward: the persistent kernels launch
    # smaller grids - other tile sequences, other partial-row, column-sum and P / Gram slab counts - for the same plan
    "r50_budget_240": ("resnet50", 1000, 32, 128, BF16, {"IIF_BN3_ALGEBRA_PURE_MIN_ELEMS": "5e7"}),
    "r50_budget_64": ("resnet50", 1000, 32, 128, BF16, {"IIF_BN3_ALGEBRA_PURE_MIN_ELEMS": "5e7"}),
}
# iif_set_cu_budget around the whole configuration: 240 of 256 CUs is what a rank with an active gradient reducer sets, 64 the
# smallest budget there is
CU_BUDGET = {"r50_budget_240": 240, "r50_budget_64": 64}

# The gate path must be visible.  At the oracle's initialisation every e is 0.5 +- 0.016 and the offset o = (dz1 W1) / HW is
# 1e-4 .. 1.2e-2 of max |G| (se_resnet50, batch 32 / 128 x 128, the oracle in float64 on the CPU): a dropped o would hide
# under one bf16 rounding of G (2^-8).  The se.excitation.*.weight entries of the state dict are scaled by this factor.
# max |o| / max |G| per block of se_resnet50 in the float64 oracle, layer1 .. layer4:
#   x 1   1e-4       3e-4 .. 4e-4   1.2e-3 .. 1.8e-3  7.1e-3 .. 1.3e-2        e in [0.48, 0.52]
#   x 8   5.6e-3 ..  2.2e-2 ..      6.3e-2 .. 9.9e-2  0.21 .. 0.39            e in [0.015, 0.98]
#   x 32  4.6e-2 ..  0.21 ..        0.35 ..           0.89                    e reaches 0.000 and 1.000 in every stage
# No single factor serves every block: o carries 1 / HW (1024 pixels in layer1 against 16 in layer4), and the factor that
# lifts layer1 over 4 x 2^-7 (32; 20 .. 28 leave layer1 at 2.8e-2 .. 4.4e-2) saturates the gates: logits a thousand times
# those of the initialisation, where the 2e-6 bound of se_e (set for logits of order 1) no longer describes an fp32
# accumulation, and gates at 0 or 1 that switch the term under test off.  8 keeps every gate inside
# (0.01, 0.99) and the nine blocks of layer3 and layer4 over the condition; the SE control (c) targets one of them.
# se_resnet32 (kaiming-normal SE weights, reduction 4, no damped gains) has 1e-2 .. 0.15 at its own initialisation and
# 3.4e-2 .. 0.44 (every block over the condition) at 2.
SE_GATE_SCALE = {"se_resnet50": 8.0, "se_resnet32": 2.0}
SE_GATE_MIN = 4 * 2.0 ** -7

# expected route inventory per configuration (unit_reference.routes)
INVENTORY = {
    "r50_bench_mix": {"alg3": 13, "rx": 7, "nostore": 7, "ds_alg": 1, "pool_fused_bwd": True, "wg_stream": True},
    "r50_sums_from_p": {"alg3": 13, "nostore": 13, "ds_alg": 1, "pool_fused_bwd": True},
    "r50_one_stream": {"alg3": 13, "pg": 0, "ds_alg": 0, "wg_stream": False, "ds_stream": False, "pool_fused_bwd": True},
    "rx50_grouped": {"pool_fused_bwd": True},
    "r32_cifar": {"alg3": 0, "wg_stream": False, "pool_fused_bwd": False},
    "r50_fp32": {"alg3": 0, "rx": 0, "nostore": 0, "pg": 0, "pro": 0, "ds_alg": 0, "pool_fused_bwd": False},
    # SE blocks: conv3's output is stored (the squeeze needs all of it before any element is scaled), no BN backward by algebra
    "se_r50": {"se": 16, "alg3": 0, "rx": 0, "nostore": 0, "pg": 0, "pro": 0, "ds_alg": 0, "pool_fused_bwd": True,
               "wg_stream": True, "ds_stream": True},
    "se_r32_cifar": {"se": 15, "alg3": 0, "nostore": 0, "wg_stream": False, "ds_stream": False, "pool_fused_bwd": False},
    "r18_basic": {"se": 0, "alg3": 0, "nostore": 0, "ds_alg": 0, "pool_fused_bwd": True, "wg_stream": True, "ds_stream": True},
    "se_r50_fp32": {"se": 16, "alg3": 0, "rx": 0, "nostore": 0, "pg": 0, "pro": 0, "ds_alg": 0, "pool_fused_bwd": False},
    "r50_budget_240": {"alg3": 13, "rx": 7, "nostore": 7, "pg": 3, "ds_alg": 1, "pool_fused_bwd": True, "wg_stream": True},
    "r50_budget_64": {"alg3": 13, "rx": 7, "nostore": 7, "pg": 3, "ds_alg": 1, "pool_fused_bwd": True, "wg_stream": True},
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


FP32_BOUND = 1e-5

# the metrics of an SE block (unit_reference, "Squeeze-and-excitation blocks").  1: the metric is an error / bound ratio whose
# bound is formed per element or per stage from the float64 reference (fp32 sums over HW terms; a stage in float32 on the CPU);
# se_q, se_h, se_e: the tolerances of tests/test_layers_gpu.py::test_se_excitation_native_against_torch; se_G: one rounding of
# the stored gradient with 2x headroom, as x and y
SE_BOUNDS = {"se_sums": 1.0, "se_q": 1e-5, "se_h": 2e-5, "se_e": 2e-6, "se_gmask": 0.0, "se_s1": 1.0, "se_s2": 1.0,
             "se_dz2": 1.0, "se_dz1": 1.0, "se_o": 1.0, "se_dw1": 1.0, "se_dw2": 1.0, "se_pad": 0.0, "se_G": 2 ** -7}
SE_BOUNDS_FP32 = dict(SE_BOUNDS, se_G=FP32_BOUND)


def bf16_bound(unit, metric):
    if metric == "dw" and unit in POOL_FED:
        return 8e-2
    return BF16_BOUNDS.get(metric, SE_BOUNDS.get(metric))


def fp32_bound(unit, metric):
    return SE_BOUNDS_FP32.get(metric, FP32_BOUND)


def condition_gates(sd, arch):
    """Scale every SE excitation weight by SE_GATE_SCALE (see there)."""
    for k in sd:
        if ".se.excitation." in k and k.endswith(".weight"):
            sd[k] = sd[k] * SE_GATE_SCALE[arch]
    return sd


def run_config(name, monkeypatch):
    """Build the configuration, take one step without and one with the capture; returns (net, capture, inventory, metrics)."""
    from iif_amd.custom import IIFLoss
    arch, C, B, hw, dt, env = CONFIGS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    counts = [max(int(1000 * (5 / 1000) ** (i / (C - 1.0))), 1) for i in range(C)]
    net, sd = _build(arch, C, dt)
    if not arch.startswith("resnet3") and not arch.startswith("resnet2") and arch not in R.CIFAR_ARCHS:
        net.load_state_dict(damp_residual_branches(sd, arch))
    if R.is_se(arch):
        net.load_state_dict(condition_gates(sd, arch))
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
    if U.SE_GATE:
        print("  max|o| / max|G| per SE block: " + " ".join("%s=%.3f" % (k[:-3], v) for k, v in U.SE_GATE.items()))
    if os.environ.get("UNIT_REF_VERBOSE"):
        for unit, m in met.items():
            print("  %-26s %s" % (unit, " ".join("%s=%.2e" % kv for kv in sorted(m.items()))))
    return net, cap, inv, met, (xd, yd, crit)


def _check_inventory(name, inv):
    for k, v in INVENTORY[name].items():
        assert inv[k] == v, (name, k, inv[k], v, inv)
    if name == "r50_bench_mix":
        assert inv["pg"] >= 1 and inv["pro_rows"] >= 1 and inv["alg3_pure"] == 0
    if name in CU_BUDGET:           # the routes whose launches a budget resizes: recomputing producer, its slabs, never-stored forward
        assert inv["rx"] >= 1 and inv["pg"] >= 1 and inv["nostore"] >= 1, (name, inv)


@pytest.fixture
def cu_budget():
    """set_(cus): iif_set_cu_budget for the rest of the test; budget 0 (the whole device) is restored whatever happens."""
    from iif_amd import _lib
    L = _lib.lib()

    def set_(cus):
        L.iif_set_cu_budget(0)
        if L.iif_get_cu_budget() != 256:
            pytest.skip("the budgets of CU_BUDGET are meant for 256 compute units")
        _lib.check(L.iif_set_cu_budget(cus), "iif_set_cu_budget")
        assert L.iif_get_cu_budget() == cus
    try:
        yield set_
    finally:
        L.iif_set_cu_budget(0)


@pytest.mark.parametrize("name", [n for n in CONFIGS if CONFIGS[n][4] == BF16])
def test_bf16_units_against_float64(name, monkeypatch, cu_budget):
    """Measured worst cases per configuration (MI355X; dw: the pooled-stem units at 224 x 224; the stem's dw_rdx in brackets):
        r50_bench_mix    dgamma 2.0e-5  dw 3.1e-2  dw_rdx 3.2e-5 (1.2e-5)  dgrad 2.9e-3  invstd 2.9e-5  y 3.2e-3
        r50_sums_from_p  dgamma 2.2e-5  dw 6.9e-3  dw_rdx 4.9e-5 (2.1e-5)  dgrad 2.9e-3  invstd 6.3e-5  y 3.3e-3
        r50_one_stream   dgamma 2.0e-5  dw 3.1e-2  dw_rdx 3.7e-5 (1.5e-5)  dgrad 2.9e-3  invstd 2.9e-5  y 3.2e-3
        rx50_grouped     dgamma 1.1e-5  dw 6.3e-3  dw_rdx 2.9e-5 (2.3e-5)  dgrad 2.9e-3  invstd 5.9e-5  y 3.2e-3
        r32_cifar        dgamma 1.5e-7  dw 3.8e-3  dw_rdx 3.1e-5 (1.5e-5)  dgrad 2.6e-3  invstd 4.7e-6  y 3.3e-3
        se_r50           dgamma 3.3e-7  dw 6.7e-3  dw_rdx 4.3e-5 (5.6e-6)  dgrad 2.9e-3  invstd 1.8e-4  y 3.4e-3
        se_r32_cifar     dgamma 1.4e-7  dw 1.5e-2  dw_rdx 2.1e-5 (2.1e-5)  dgrad 2.4e-3  invstd 6.5e-6  y 3.6e-3
        r18_basic        dgamma 3.0e-7  dw 5.7e-3  dw_rdx 1.7e-5 (1.6e-5)  dgrad 2.9e-3  invstd 1.3e-4  y 3.4e-3
        r50_budget_240   dgamma 1.8e-5  dw 9.5e-3  dw_rdx 3.3e-5           dgrad 2.9e-3  invstd 8.2e-5  y 3.4e-3
        r50_budget_64    dgamma 2.4e-5  dw 1.2e-2  dw_rdx 3.6e-5           dgrad 2.9e-3  invstd 6.4e-5  y 3.3e-3
    (the two budget configurations: dw at layer1.0.conv1, a pooled-stem unit; dgrad_max 5.0e-3 / 6.5e-3, x 3.7e-3 / 3.5e-3,
    mean 3.5e-5 / 4.2e-5, dbeta 4.0e-8 / 4.3e-8.)
    (invstd: layer4.0.downsample.0 of se_r50, layer4.1.conv2 of r18_basic, both 512 rows; the bound is 2e-4.)
    The SE metrics, measured worst case (bound), se_r50 / se_r32_cifar: se_sums 2.9e-2 / 1.5e-2 (1), se_s1 3.4e-2 / 1.2e-2 (1),
    se_s2 5.3e-2 / 3.0e-2 (1), se_q 8.1e-7 / 3.6e-7 (1e-5), se_h 1.0e-7 / 1.0e-7 (2e-5), se_e 2.2e-7 / 1.0e-7 (2e-6), se_dz2
    4.4e-3 / 4.8e-3 (1), se_dz1 4.9e-3 / 3.8e-3 (1), se_o 7.5e-3 / 3.2e-3 (1), se_dw1 4.0e-3 / 9.6e-3 (1), se_dw2 4.0e-3 /
    7.4e-3 (1), se_G 0 / 0 (2^-7: the reference's one rounding of g~ e + o is the kernel's), se_gmask and se_pad 0 / 0 (0).
    max |o| / max |G| from the float64 reference: se_r50 6e-3 .. 8e-3 in layer1, 1.9e-2 .. 2.4e-2 in layer2, 6.0e-2 .. 9.6e-2 in
    layer3, 0.22 .. 0.39 in layer4; se_r32_cifar 3.7e-2 .. 0.46."""
    if name in CU_BUDGET:
        cu_budget(CU_BUDGET[name])
    net, cap, inv, met, _ = run_config(name, monkeypatch)
    _check_inventory(name, inv)
    assert len(met) == len(net._saved.units) + _se_blocks(net), (len(met), len(net._saved.units))
    bad = U.failures(met, bf16_bound)
    assert not bad, bad


def _se_blocks(net):
    return sum(1 for b in net._saved.blocks if "se" in b)


def test_fp32_units_against_float64(monkeypatch):
    """Self-check of the harness: exact-fp32 arithmetic agrees with the float64 evaluation of every unit to 1e-5
    (measured: 2.1e-6 at worst, the stored convolution output of layer4.0.conv2; every gradient <= 8.3e-7)."""
    net, cap, inv, met, _ = run_config("r50_fp32", monkeypatch)
    _check_inventory("r50_fp32", inv)
    assert len(met) == len(net._saved.units)
    bad = U.failures(met, lambda unit, k: FP32_BOUND)
    assert not bad, bad


def test_fp32_se_units_against_float64(monkeypatch):
    """The same self-check for the SE conventions: every unit metric to 1e-5 and every SE metric at its fp32 bound (SE_BOUNDS_FP32:
    se_G to 1e-5 as well).  A convention error of the reference (the gate in y, the unmasked G at the last unit, the masked g on
    the identity path, the ungated block-input gradient behind an SE block) shows here at 1e-5, not under a bf16 rounding.
    Measured: 2.1e-6 at worst over the unit metrics (dgrad_max of layer3.5.conv2; y 8.4e-8); se_sums 0.11, se_s1 9.7e-2, se_s2
    0.13, se_dz2 3.7e-3, se_dz1 5.4e-3, se_o 7.6e-3, se_dw1 2.5e-3, se_dw2 2.4e-3 of their bounds, se_q 4.2e-7, se_h 1.2e-7,
    se_e 2.6e-7, se_G, se_gmask and se_pad 0."""
    net, cap, inv, met, _ = run_config("se_r50_fp32", monkeypatch)
    _check_inventory("se_r50_fp32", inv)
    assert _se_blocks(net) == 16 and len(met) == len(net._saved.units) + 16
    bad = U.failures(met, fp32_bound)
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


# blocks of se_resnet50 (plan.blocks index) the SE controls target: an identity block of layer3, the last block of layer4,
# and the stride-2 block of layer3 (HW changes behind its stride, its residual is the normalised shortcut)
SE_CONTROL_BLOCKS = {"a": 9, "b": 15, "c": 7}


def test_se_negative_controls_flag_exactly_the_affected_block(monkeypatch):
    """The SE twin of the controls above, on se_r50: (a) one block's excitation[0] weight gradient scaled by 0.8: only its se_dw1;
    (b) one block's stored e scaled by 1.05: what is evaluated FROM that e against what the step made with the true one (se_e,
    the last unit's y, se_G; se_dz2 = de e (1 - e) reads the stored e as well), nothing else; (c) ops.se_backward_form patched so
    that one block receives a zeroed offset, a new step and a new capture: only that block's se_G, and every unit downstream of
    it stays clean, since each is checked from the gradient that arrived at it.  For the block of (c) the float64 reference
    alone has max |o| >= 4 x 2^-7 max |G| (SE_GATE_SCALE)."""
    from iif_amd import ops
    net, cap, inv, met, (xd, yd, crit) = run_config("se_r50", monkeypatch)
    assert not U.failures(met, bf16_bound)
    gate = dict(U.SE_GATE)
    plan = net._saved
    names = U.unit_names(net)
    flagged = lambda m: {(unit, k) for unit, k, _, _ in U.failures(m, bf16_bound)}      # noqa: E731
    blk = lambda key: plan.blocks[SE_CONTROL_BLOCKS[key]]                                # noqa: E731
    se_name = lambda b: names[id(b["blk"])] + ".se"                                      # noqa: E731
    # (a) one SE weight gradient scaled by 0.8
    b = blk("a")
    g1 = b["blk"].se.excitation[0]._g2d
    keep = g1.clone()
    g1.mul_(0.8)
    m1 = U.check_step(net, xd, cap)
    print("\n(a)", sorted(flagged(m1)))
    assert flagged(m1) == {(se_name(b), "se_dw1")}, U.failures(m1, bf16_bound)
    g1.copy_(keep)
    # (b) one stored gate scaled by 1.05
    b = blk("b")
    e = b["se"]["e"]
    keep = e.clone()
    e.mul_(1.05)
    m2 = U.check_step(net, xd, cap)
    last = names[id(b["units"][-1].conv)]
    print("(b)", sorted(flagged(m2)))
    assert flagged(m2) == {(se_name(b), "se_e"), (last, "y"), (last, "y_l2"), (se_name(b), "se_G"),
                           (se_name(b), "se_dz2")}, U.failures(m2, bf16_bound)
    e.copy_(keep)
    # (c) the offset dropped from one block's G
    b = blk("c")
    assert gate[se_name(b)] >= SE_GATE_MIN, gate
    orig, o_t = ops.se_backward_form, b["se"]["o"]

    def form(g, excite, offset, out):
        if offset.data_ptr() == o_t.data_ptr():
            offset = torch.zeros_like(offset)
        return orig(g, excite, offset, out)

    monkeypatch.setattr(ops, "se_backward_form", form)
    cap2 = U.StepCapture()
    U.run_step(net, xd, yd, crit, capture=cap2)
    m3 = U.check_step(net, xd, cap2)
    print("(c)", sorted(flagged(m3)))
    assert flagged(m3) == {(se_name(b), "se_G")}, U.failures(m3, bf16_bound)

