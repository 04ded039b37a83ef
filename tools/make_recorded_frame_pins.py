"""tests/golden/recorded_frame_pins.json (and, with --gpu, recorded_frame_gpu_pins.json): what the cases of tests/test_recorded_frame_host.py
(--gpu: tests/test_recorded_frame.py, on the MI355X) give with the library of the commit BEFORE the recorded frame moved out of Context --
build that commit's figdraw_amd/csrc elsewhere and point FIGDRAW_HIP_LIB at its libfigdraw_hip.so:
    FIGDRAW_HIP_LIB=/path/to/parent/libfigdraw_hip.so python tools/make_recorded_frame_pins.py [--gpu] <parent commit hash> [output file]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

args = [a for a in sys.argv[1:] if a != "--gpu"]
gpu = "--gpu" in sys.argv[1:]
assert len(args) in (1, 2) and len(args[0]) == 40 and "FIGDRAW_HIP_LIB" in os.environ, __doc__
if gpu:
    import test_recorded_frame as T  # noqa: E402
else:
    import test_recorded_frame_host as T  # noqa: E402

cases = {name: fn() for name, fn in sorted(T.CASES.items())}
out = args[1] if len(args) == 2 else T.PIN_FILE
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump({"parent_commit": args[0], "library": "libfigdraw_hip.so built from parent_commit; cases: tests/" + os.path.basename(T.__file__) + " CASES",
               "cases": cases}, f, indent=1, sort_keys=True)
    f.write("\n")
print(len(cases), "cases ->", out)
