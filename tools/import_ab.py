#!/usr/bin/env python3
"""The host cost of the image and video imports, or of the video exports, this tree's library against another build's (the parent
commit's), on one MI355X in one session -> the timing part of profiles/import_refactor.txt, profiles/video_out_refactor.txt.

  import_ab.py OUT --parent-lib LIB [--rows import|out] [--rounds N] [--warmup W] [--bench-runs K]
  import_ab.py --first                       one process: the first imports of a context that has made glyphs; one JSON line

The rows are steps of the import benchmarks -- tools/device_image_bench.py (single and batch), tools/video_frame_bench.py,
tools/video_frame_batch_bench.py, tools/video_alpha_bench.py -- at their smallest sizes, where the host side is the larger share of a call,
each step a process of its own on the library FIGDRAW_HIP_LIB names (--rows out: the way out of tools/video_out_bench.py,
tools/video_planar_bench.py, tools/video_422_bench.py and tools/video_alpha_bench.py at 256 x 256 instead, and no first-call rows); then
bench.py --gpus 1 --steps 200 --warmup 20.  A row runs parent, tree, parent, tree, parent: the yardstick is the parent against itself.  A leg is marked only where every run of the tree is slower than
every run of the parent; whatever comes out is written down.  The first-call rows are numbers, not verdicts: the tree's importer allocates
its own scratch there.  Every step runs under its own time limit and nothing is started after a failure."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = {"import": [("device_image_bench.py", s) for s in ("32:put:device", "32:update:device", "256:put:device", "256:update:device", "batch:32:put:batch", "batch:32:update:batch")]}
ROWS["import"] += [("video_frame_bench.py", s) for s in ("256x256:put:video", "256x256:update:video")]
ROWS["import"] += [("video_frame_batch_bench.py", s) for s in ("thumbs:put:batch", "thumbs:update:batch")]
ROWS["import"] += [("video_alpha_bench.py", "256x256:in")]
ROWS["out"] = [("video_out_bench.py", "256x256:video"), ("video_planar_bench.py", "256x256:out"), ("video_422_bench.py", "256x256:out"), ("video_alpha_bench.py", "256x256:out")]
ORDER = ("parent", "tree", "parent", "tree", "parent")


def first():
    """glyph puts first, so that the glyph maker's buffers have grown; then the first and the second call of a single import and of a batch"""
    import numpy as np
    from figdraw_amd.context import HipContext

    hip = C.CDLL("libamdhip64.so")

    def device(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    nan = float("nan")
    box = np.array([[2, 2, nan, nan, 17, 2], [17, 2, nan, nan, 17, 18], [17, 18, nan, nan, 2, 18], [2, 18, nan, nan, 2, 2]], np.float32)
    rng = np.random.default_rng(1)
    y, uv = device(rng.integers(0, 256, size=(256, 256)).astype(np.uint8)), device(rng.integers(0, 256, size=(128, 128, 2)).astype(np.uint8))
    rgba = device(rng.integers(0, 256, size=(32, 32, 4)).astype(np.uint8))
    ctx = HipContext(atlas_size=2048, device=0)
    ctx.put_glyph_outline(1, box, 20, 20)
    ctx.put_glyph_outlines([(10 + k, box, 20, 20) for k in range(16)])
    out = {}
    for name, call in (("put_video_frame 256 x 256", lambda k: ctx.put_video_frame(100 + k, y, uv, 256, 256, 256, 256)),
                       ("put_images_device 4 of 32 x 32", lambda k: ctx.put_images_device([(200 + 4 * k + i, rgba, 32, 32, 128) for i in range(4)]))):
        for k, which in enumerate(("first", "second")):
            ctx.sync()
            t1 = time.perf_counter()
            call(k)
            out[f"{name}, {which}"] = (time.perf_counter() - t1) * 1e6
    ctx.close()
    print(json.dumps(out))


def child(cmd, lib, limit):
    """-> the last JSON line the command prints, or None: it failed"""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=dict(os.environ, FIGDRAW_HIP_LIB=os.path.abspath(lib)), cwd=ROOT)
    found = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not found:
        print(f"{' '.join(cmd)} failed with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-4000:]}", flush=True)
        return None
    return json.loads(found[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--first", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rows", choices=sorted(ROWS), default="import")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-runs", type=int, default=3)
    args = ap.parse_args()
    if args.first:
        first()
        return 0
    if not args.out or not args.parent_lib:
        ap.error("OUT and --parent-lib")
    from figdraw_amd import context

    libs = {"parent": args.parent_lib, "tree": os.environ.get("FIGDRAW_HIP_LIB", context.LIB_PATH)}
    lines = [f"whole calls, host clock, median of {args.rounds} rounds after {args.warmup} in microseconds; one process per run, in the order {', '.join(ORDER)}",
             "per leg: the parent's runs | the tree's runs"]
    ok, marked = True, []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def verdict(where, parent, tree, slower_is_more=True):
        worst = min(tree) > max(parent) if slower_is_more else max(tree) < min(parent)
        if worst:
            marked.append(where)
        return "   EVERY RUN OF THE TREE SLOWER THAN EVERY RUN OF THE PARENT" if worst else ""

    for tool, step in ROWS[args.rows]:
        cmd = [sys.executable, os.path.join(ROOT, "tools", tool), "--step", step, "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        runs = []
        for side in ORDER:
            got = child(cmd, libs[side], 300) if ok else None
            ok = ok and got is not None
            runs.append((side, got))
        say(f"{tool} --step {step}" + ("" if ok else ": not measured"))
        if not ok:
            continue
        for leg, v in runs[0][1].items():
            if not isinstance(v, list):
                continue
            parent, tree = [g[leg][0] for s, g in runs if s == "parent"], [g[leg][0] for s, g in runs if s == "tree"]
            say(f"    {leg:22s} {'  '.join(f'{x:8.1f}' for x in parent)}  | {'  '.join(f'{x:8.1f}' for x in tree)}{verdict(f'{step} {leg}', parent, tree)}")
    runs = []
    if args.rows == "import":
        say("first imports on a context that has made glyphs (tools/import_ab.py --first), microseconds; numbers, not verdicts")
        for side in ORDER:
            got = child([sys.executable, os.path.abspath(__file__), "--first"], libs[side], 120) if ok else None
            ok = ok and got is not None
            runs.append((side, got))
    for leg in (runs[0][1] or {}) if ok and runs else ():
        say(f"    {leg:40s} {'  '.join(f'{g[leg]:8.1f}' for s, g in runs if s == 'parent')}  | {'  '.join(f'{g[leg]:8.1f}' for s, g in runs if s == 'tree')}")
    say("bench.py --gpus 1 --steps 200 --warmup 20: value (Mpixels/s), parent and tree by turns")
    values = {"parent": [], "tree": []}
    for k in range(2 * args.bench_runs + 1):
        side = "parent" if k % 2 == 0 else "tree"
        got = child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20"], libs[side], 300) if ok else None
        ok = ok and got is not None
        if ok:
            values[side].append(float(got["value"]))
            say(f"    {side:7s} {got['value']}")
    if ok:
        say(f"    parent {values['parent']} | tree {values['tree']}{verdict('bench.py value', values['parent'], values['tree'], slower_is_more=False)}")
    say("legs on which every run of the tree is slower than every run of the parent: " + (", ".join(marked) if marked else "none"))
    if not ok:
        say("INCOMPLETE: a step failed; nothing was started after it")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
