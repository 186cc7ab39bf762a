"""Records tests/golden/dg_transfer_parent_digests.json: SHA-256 of the raw bytes of every result of the cases of
tests/test_gpu_dg_transfer_parent_digests.py (DG-to-DG mesh and degree transfers in both directions, one V-cycle of the
plain solver from either entry point), with the library that is loaded.  Run it on the GPU with a build of the commit
BEFORE a change to mgx_dg_transfer.hip or to the transfer and plain-solver part of mgx_dg_api.cpp:
    MGX_LIB_PATH=/path/to/libmgx_of_the_parent.so python tools/dg_transfer_digests.py [out.json]
The file holds names and digests only."""
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "tests")]
import test_gpu_dg_transfer_parent_digests as cases  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
digests = cases.all_digests()
with open(out, "w") as f:
    json.dump(digests, f, indent=1, sort_keys=True)
    f.write("\n")
print("%d digests -> %s" % (len(digests), out))
