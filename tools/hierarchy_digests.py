"""Records tests/golden/hierarchy_parent_digests.json: SHA-256 of the raw bytes of every result of the cases of
tests/test_gpu_hierarchy_parent_digests.py (what MultigridSolver holds and computes on a Square and on a Cube: right-hand
sides, coefficients, prolongation, state interpolation, coefficient refresh, nonlinear residual, one 2D solve), with the
package and library that are loaded.  Run it on the GPU in a checkout of the commit BEFORE a change to the hierarchy
set-up (mgx_hierarchy.cpp, the solver-create functions of mgx_cube.cpp and mgx_square.cpp, MultigridSolver.__init__),
twice, in two processes, and compare the two files: every case is free of atomics.
    python tools/hierarchy_digests.py [out.json [root of the checkout to load multigrid_amd from]]
The file holds names and digests only."""
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [sys.argv[2] if len(sys.argv) > 2 else root, os.path.join(root, "tests")]
import test_gpu_hierarchy_parent_digests as cases  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
digests = cases.all_digests()
with open(out, "w") as f:
    json.dump(digests, f, indent=1, sort_keys=True)
    f.write("\n")
print("%d digests -> %s" % (len(digests), out))
