"""class RetainedScene (figdraw_amd/csrc/fdh_retained.h) on its own: tests/retained_host/model.cpp drives it against a naive mirror of the
tree -- every node owning private copies of its glyphs, variant ids, ops and text rectangles -- through a seeded script of edits, as a
stand-alone program under AddressSanitizer and UBSan.  No context, no device, no library: the class is plain C++."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "figdraw_amd", "csrc")


def test_retained_scene_against_a_naive_mirror(tmp_path):
    exe = tmp_path / "model"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "retained_host", "model.cpp"), os.path.join(CSRC, "fdh_retained.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), f"{r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    # the script really took every kind of step (the program checks its invariants after each one)
    n = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", r.stdout.splitlines()[-2])}
    assert n["steps"] >= 300
    assert n["failed_update_last_node"] >= 2  # the bad side range at the last node of an update_nodes edit: once outside the random script, and in it
    for kind in ("updates", "reparents", "late_roots", "replaces", "inserts", "removes", "failed", "failed_replace_side", "failed_insert_side", "failed_update_last_node",
                 "failed_slot", "failed_parent", "compactions", "tables"):
        assert n[kind] > 0, (kind, n)
