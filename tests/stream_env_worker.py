"""Worker of tests/test_stream_paths_gpu.py: the exact forward and backward comparisons of the BN normalisation passes in a FRESH
process, because bn.hip's stream_grid reads IIF_BN_GRID_CAP / IIF_BN_NT_STORES / IIF_BN_UNROLL once per process.

    python -m tests.stream_env_worker [u=<U>] [nts=<0|1>] [trips=<minimum>] <case> [<case> ...]

The expectations are held against the planning query first (a switch that did not reach the library fails here, not silently);
then every case runs in bf16 and fp32, one line each.  Exit status 0 only if everything is bit-identical."""
import sys

import torch

from tests import stream_cases as S


def main(argv):
    expect = dict(a.split("=") for a in argv if "=" in a)
    cases = [a for a in argv if "=" not in a]
    status = 0
    for name in cases:
        blocks, u, nts, trips = S.plan("bn", S.bn_vectors(name))
        ok = ("u" not in expect or u == int(expect["u"])) and ("nts" not in expect or nts == int(expect["nts"]))
        ok = ok and trips >= int(expect.get("trips", 1))
        print("%-8s plan blocks=%d u=%d nts=%d trips=%d %s" % (name, blocks, u, nts, trips, "ok" if ok else "UNEXPECTED"), flush=True)
        if not ok:
            return 2
        for key, dt in S.DTYPES.items():
            bad = S.check_bn_apply_exact(name, dt, "cuda:0") + S.check_bn_backward_exact(name, dt, "cuda:0")
            torch.cuda.synchronize()
            print("%-8s %-4s %s" % (name, key, "bit-identical" if not bad else "MISMATCH %s" % bad), flush=True)
            if bad:
                status = 1
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
