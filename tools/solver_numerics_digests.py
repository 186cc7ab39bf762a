"""Records tests/golden/solver_numerics_parent_digests.json: SHA-256 of the raw bytes of every result of the cases of
tests/test_gpu_solver_numerics_parent_digests.py (smoother set-up, CG solves, residual updates and timers of the FE_Q,
DG-on-FE_Q and plain DG solvers), with the library that is loaded.  Run it on the GPU with a build of the commit BEFORE
a change to the host numerics (mgx_krylov.hpp and its callers in mgx_api.cpp and mgx_dg_api.cpp), twice, one process
each, and keep what both runs agree on:
    python tools/solver_numerics_digests.py first.json
    python tools/solver_numerics_digests.py second.json
    python tools/solver_numerics_digests.py --keep-equal first.json second.json [out.json]
The file holds names with digests and, for the FE_Q CG solves, residual histories."""
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "tests")]


def write(digests, out):
    with open(out, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(digests), out))


if len(sys.argv) > 1 and sys.argv[1] == "--keep-equal":
    with open(sys.argv[2]) as f:
        first = json.load(f)
    with open(sys.argv[3]) as f:
        second = json.load(f)
    # (a residual history, a list of numbers, is kept from the first run: the test compares it within a tolerance)
    dropped = sorted(k for k in set(first) | set(second) if first.get(k) != second.get(k) and not isinstance(first.get(k), list))
    print("dropped (the two runs differ):", dropped if dropped else "none")
    golden = os.path.join(root, "tests", "golden", "solver_numerics_parent_digests.json")
    write({k: v for k, v in first.items() if k not in dropped}, sys.argv[4] if len(sys.argv) > 4 else golden)
else:
    import conftest  # noqa: E402,F401  the scheduling thresholds the suite runs under (they select the kernels of small levels)
    import test_gpu_solver_numerics_parent_digests as cases  # noqa: E402
    write(cases.all_digests(), sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN)
