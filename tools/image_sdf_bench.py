#!/usr/bin/env python3
"""What a distance field of a coverage image costs (fdh_put_image_sdf, fdh_put_image_sdf_of; include_glyphs/figdraw_hip_image_sdf.h) on an
MI355X -> profiles/image_sdf.txt.

  image_sdf_bench.py OUT [--rounds N] [--warmup W] [--nocull-lib LIB] [--trace-dir DIR]
  image_sdf_bench.py --step NAME [--rounds N] [--warmup W]           one step in this process; one JSON line

A measurement is the host clock around whole calls -- every call ends in a device synchronise -- on one context, N timed rounds after W;
the 2048 atlas is reset, and the sources of the atlas-to-atlas call are put again, before every round outside the clock.  In the same
step fdh_put_image of an image of the output's size gives the floor: placement, upload and level chain; the two alternate.  --nocull-lib
names the variant library without the walk's exit and the two shortcuts (make variant NAME=image_sdf_nocull
DEFS=-DFDH_IMAGE_SDF_NO_CULL=1): the steps run again on it, and the difference is what the exit is worth.  --trace-dir: every step once
more under rocprofv3 --kernel-trace --stats, runs of their own, for k_image_sdf_generate's own time per launch.  Every step is a child process
under its own time limit, nothing is started after a failure, and what was not reached is written down as "not measured".  There is no
CPU fallback: without a device the context cannot be made and the step fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNEL = "k_image_sdf_generate"
STEPS = {  # name -> (what, call, R, pad)
    "glyphs": ("the 94 glyphs at R = 8, pad = 4 (94 calls)", "put", 8, 4),
    "icon 8": ("a 256 x 256 icon at R = 8, pad = 4", "put", 8, 4),
    "icon 64": ("a 256 x 256 icon at R = 64, pad = 32", "put", 64, 32),
    "image 16": ("a 1024 x 1024 image at R = 16, pad = 8", "put", 16, 8),
    "glyphs of": ("the same glyphs from the atlas, fdh_put_image_sdf_of (94 calls)", "of", 8, 4),
}


def images(name):
    import image_sdf_cases as IC

    if name.startswith("glyphs"):
        return list(IC.glyph_images().values())
    side = 1024 if name.startswith("image") else 256
    cov = IC.disc(side, side, side * 0.47, side * 0.52, side * 0.33, ss=4)
    cov[side // 3:side // 3 + side // 16] = 0  # a slit through it
    return [IC.white(cov)]


def step(name, rounds, warmup):
    import numpy as np
    from figdraw_amd.context import HipContext

    _, call, R, pad = STEPS[name]
    imgs = images(name)
    plain = [np.full((m.shape[0] + 2 * pad, m.shape[1] + 2 * pad, 4), 77, np.uint8) for m in imgs]
    ctx = HipContext(atlas_size=2048, device=0)
    us = {"field": [], "floor": []}
    for k in range(warmup + rounds):
        for leg in ("field", "floor"):
            ctx.reset_atlas()
            if call == "of" and leg == "field":
                for i, m in enumerate(imgs):
                    ctx.put_image(1 + i, m)
            ctx.sync()
            t1 = time.perf_counter()
            if leg == "floor":
                for i, m in enumerate(plain):
                    ctx.put_image(1000 + i, m)
            elif call == "of":
                for i in range(len(imgs)):
                    ctx.put_image_sdf_of(1 + i, 1000 + i, 3, pad, R)
            else:
                for i, m in enumerate(imgs):
                    ctx.put_image_sdf(1000 + i, m, 3, pad, R)
            t2 = time.perf_counter()
            if k >= warmup:
                us[leg].append((t2 - t1) * 1e6)
    assert ctx.atlas_size() == 2048
    ctx.close()
    q = lambda v, f: sorted(v)[int(f * (len(v) - 1))]  # noqa: E731
    print(json.dumps({"step": name, "calls": len(imgs), **{leg: [statistics.median(v), q(v, 0.1), q(v, 0.9)] for leg, v in us.items()}}))


def run_child(name, rounds, warmup, lib, limit=240, trace_dir=None):
    """one step as a process of its own -> its JSON line; under the profiler: (launches, mean, least, most) of the kernel in us; None: it failed"""
    env = dict(os.environ, FIGDRAW_HIP_LIB=os.path.abspath(lib)) if lib else None
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--rounds", str(rounds), "--warmup", str(warmup)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", trace_dir, "-o", "t", "--"] + cmd
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        print(f"step {name!r} failed with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-4000:]}", flush=True)
        return None
    if not trace_dir:
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    import csv
    import glob

    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if KERNEL in row["Name"]:
                return int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3
    print(f"step {name!r}: no {KERNEL} in the trace", flush=True)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nocull-lib")
    ap.add_argument("--trace-dir")
    args = ap.parse_args()
    if args.step:
        step(args.step, args.rounds, args.warmup)
        return 0
    if not args.out:
        ap.error("nothing to do")
    fmt = lambda v: f"{v[0]:10.1f} ({v[1]:9.1f} .. {v[2]:9.1f})"  # noqa: E731
    lines = ["tools/image_sdf_bench.py -- distance fields from coverage images (k_image_sdf_generate), MI355X.",
             "whole calls = host clock around the calls of a row (each ends in a device synchronise), profiler off, one context, atlas 2048 reset before",
             f"every round outside the clock, {args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds.  floor = fdh_put_image of an image of the",
             "output's size, alternating with the field in the same process: placement, upload and level chain.  no cull = the variant library built",
             "with -DFDH_IMAGE_SDF_NO_CULL=1 (no exit from the walk, no shortcut), a process of its own.", ""]
    lines.append(f"{'row':66s} {'field us':>34s} {'floor us':>34s} {'field - floor':>14s} {'no cull, field us':>34s}")
    ok = True
    for name, (what, _, _, _) in STEPS.items():
        got = run_child(name, args.rounds, args.warmup, None) if ok else None
        ok = ok and got is not None
        bare = run_child(name, args.rounds, args.warmup, args.nocull_lib) if ok and args.nocull_lib else None
        ok = ok and (bare is not None or not args.nocull_lib)
        if got is None:
            lines.append(f"{what:66s} not measured")
        else:
            lines.append(f"{what:66s} {fmt(got['field']):>34s} {fmt(got['floor']):>34s} {got['field'][0] - got['floor'][0]:14.1f} {fmt(bare['field']) if bare else 'not measured':>34s}")
        print(lines[-1], flush=True)
    lines += ["", f"{KERNEL} alone, us per launch: mean (least .. most) over the launches of a step, rocprofv3 --kernel-trace --stats, a run of its own per step"]
    for name, (what, _, _, _) in STEPS.items():
        got = run_child(name, args.rounds, args.warmup, None, trace_dir=os.path.join(args.trace_dir, name.replace(" ", "_"))) if ok and args.trace_dir else None
        ok = ok and (got is not None or not args.trace_dir)
        lines.append(f"{what:66s} " + (f"{got[1]:10.1f} ({got[2]:9.1f} .. {got[3]:9.1f}) over {got[0]} launches" if got else "not measured"))
        print(lines[-1], flush=True)
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
