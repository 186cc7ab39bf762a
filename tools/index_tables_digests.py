"""Records tests/golden/index_tables_parent_digests.json: SHA-256 of the raw bytes of every result of the cases of
tests/test_gpu_index_tables_parent_digests.py (FE_Q operators, transfers, state interpolation, nonlinear residual and
coefficient refresh in 2D; the DG <-> FE_Q transfers of the 2D DG solver; prolongation, interpolation and refresh in 3D),
with the library that is loaded.  Run it on the GPU with a build of the commit BEFORE a change to the index-table
set-up or the cell-list launches (mgx_index_tables.hpp, mgx_transfer_create, the 2D launchers), twice, in two
processes, and compare the two files: every case is free of atomics.
    MGX_LIB_PATH=/path/to/libmgx_of_the_parent.so python tools/index_tables_digests.py [out.json]
The file holds names and digests only."""
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "tests")]
import test_gpu_index_tables_parent_digests as cases  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
digests = cases.all_digests()
with open(out, "w") as f:
    json.dump(digests, f, indent=1, sort_keys=True)
    f.write("\n")
print("%d digests -> %s" % (len(digests), out))
