"""Records tests/golden/transfer_tables_parent_digests.json: SHA-256 of the raw bytes of every result of the cases of
tests/test_gpu_transfer_tables_parent_digests.py (3D: ordered assembly, restriction in colour launches, V-cycle and
diagonal on brick levels under the three schedules) and the route lines of their set-up trace, with the library that
is loaded.  Run it on the GPU with a build of the commit BEFORE a change to the assembly or transfer tables
(mgx_transfer_tables.hpp, the node rule of mgx_index_tables.hpp, the stages of mgx_operator_create and
mgx_transfer_create that call them), twice, in two processes, and compare the two files: every case is free of atomics.
    MGX_LIB_PATH=/path/to/libmgx_of_the_parent.so python tools/transfer_tables_digests.py [out.json]
The file holds names, digests and trace lines only."""
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "tests")]
import test_gpu_transfer_tables_parent_digests as cases  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
digests = cases.all_digests()
with open(out, "w") as f:
    json.dump(digests, f, indent=1, sort_keys=True)
    f.write("\n")
print("%d digests -> %s" % (len(digests), out))
