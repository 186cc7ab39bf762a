"""Records tests/golden/cheb_init_parent_digests.json: SHA-256 of the raw bytes of smoother.vmult from a zero start and of
the following smoother.step for every case of tests/test_gpu_cheb_init_rhs_once.py, with the library that is loaded.
Run it on the GPU with a build of the commit BEFORE a change to the first-iterate form (kChebInit):
    MGX_LIB_PATH=/path/to/libmgx_of_the_parent.so python tools/cheb_init_digests.py [out.json [case-name-prefix ...]]
With prefixes only those cases are run and their entries replace the ones in an existing file.  The file holds names and
digests only.

The cases "5-1-3-f64-*" were recorded from the parent commit with ONE change applied, the collect pass of
diag_table_kernel (mgx_macro.hip) as it is now: until then the per-item table of the inverse diagonal took, item by
item, whichever brick wrote last, the bricks differ in the last bits on that mesh, and the parent reproduces none of
its own results there from one set-up to the next.  That build reproduces every other digest of the plain parent."""
import json
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the thresholds the test suite runs with (tests/conftest.py)
os.environ.setdefault("MGX_BRICK_MIN", "1")
os.environ.setdefault("MGX_RESTRICT_COLOUR_MIN", "8")
sys.path[:0] = [root, os.path.join(root, "tests")]
import test_gpu_cheb_init_rhs_once as cases  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
only = tuple(sys.argv[2:])
digests = {}
if only and os.path.exists(out):
    with open(out) as f:
        digests = json.load(f)
digests.update(cases.all_digests(only))
with open(out, "w") as f:
    json.dump(digests, f, indent=1, sort_keys=True)
    f.write("\n")
print("%d digests -> %s" % (len(digests), out))
