"""bench.py --dump-outputs: what the last timed step computed, as float32 .npy files under 64 MB, so that two builds can be
compared output for output; --steps sets the number of timed steps and the result line reports ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bench.py is imported in a child process: importing it sets a HIP environment default that must not leak into the suite
_CPU_DUMP = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import bench
from iif_amd import resnet_cifar
torch.manual_seed(0)
net = resnet_cifar.resnet20(num_classes=10, device="cpu", compute_dtype=torch.float32)
with torch.no_grad():
    net._mom_arena.copy_(torch.arange(net._mom_arena.numel(), dtype=torch.float32))
bench.dump_outputs(sys.argv[2], net, torch.tensor(2.5), torch.arange(40, dtype=torch.float32).view(4, 10))
torch.save({"params": torch.cat([p.detach().reshape(-1) for p in net.parameters()]),
            "momentum": torch.cat([v.reshape(-1) for v in net._arena_views(net._mom_arena)]),
            "sample": bench._seeded_sample(torch.arange(1000), 100), "sample2": bench._seeded_sample(torch.arange(1000), 100)},
           sys.argv[2] + "/expect.pt")
"""


def test_dump_outputs_writes_the_step_results(tmp_path):
    import torch
    r = subprocess.run([sys.executable, "-c", _CPU_DUMP, ROOT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    want = torch.load(tmp_path / "expect.pt")
    names = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npy"))
    assert names == ["bn_running.npy", "logits.npy", "loss.npy", "momentum.npy", "params.npy"]
    arrays = {f[:-4]: np.load(tmp_path / f) for f in names}
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert arrays["loss"].tolist() == [2.5]
    assert np.array_equal(arrays["logits"], np.arange(40, dtype=np.float32).reshape(4, 10))
    # fewer parameters than the sample size: everything, in parameters() order
    assert np.array_equal(arrays["params"], want["params"].numpy())
    assert np.array_equal(arrays["momentum"], want["momentum"].numpy())
    assert arrays["bn_running"].size > 0
    # a larger array: a fixed sample in index order, the same on every call
    s = want["sample"]
    assert s.numel() == 100 and torch.equal(s, want["sample2"]) and bool((s[1:] > s[:-1]).all())


@pytest.mark.gpu
def test_bench_steps_and_dump(tmp_path):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None); e.pop("RANK", None); e.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--model", "resnet32", "--image", "32", "--classes", "100", "--batch", "32", "--no-cpu-baseline",
                        "--no-fp32-step", "--dump-outputs", str(tmp_path)], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1
    out = json.loads(line[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    arrays = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith(".npy")}
    assert sorted(arrays) == ["bn_running", "logits", "loss", "momentum", "params"]
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["logits"].shape == (32, 100) and np.isfinite(arrays["logits"]).all()
    assert abs(float(arrays["loss"][0]) - out["config"]["final_loss"]) <= 1e-4 * max(1.0, abs(out["config"]["final_loss"]))
