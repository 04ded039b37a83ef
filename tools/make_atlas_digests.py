"""tests/golden/atlas_record_digests.json: the record digests of tests/test_atlas_host.py's frames (build_frames), made with the library of
the commit BEFORE the atlas moved out of Context -- build that commit's figdraw_amd/csrc elsewhere and point FIGDRAW_HIP_LIB at its
libfigdraw_hip.so:   FIGDRAW_HIP_LIB=/path/to/parent/libfigdraw_hip.so python tools/make_atlas_digests.py <parent commit hash>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from figdraw_amd.context import HipContext  # noqa: E402
from test_atlas_host import build_frames  # noqa: E402

assert len(sys.argv) == 2 and len(sys.argv[1]) == 40 and "FIGDRAW_HIP_LIB" in os.environ, __doc__
ctx = HipContext(atlas_size=256, record_only=True)
digests = {name: f"{d:016x}" for name, d in build_frames(ctx).items()}
ctx.close()
with open(os.path.join(ROOT, "tests", "golden", "atlas_record_digests.json"), "w") as f:
    json.dump({"parent_commit": sys.argv[1], "library": "libfigdraw_hip.so built from parent_commit; frames: tests/test_atlas_host.py build_frames()",
               "digests": digests}, f, indent=1)
    f.write("\n")
print(len(digests), "digests")
