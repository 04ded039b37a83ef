#!/usr/bin/env python3
"""What a decoded video frame costs on its way into the atlas (fdh_put_video_frame, fdh_update_video_frame;
include_glyphs/figdraw_hip_video_frame.h) on an MI355X, against the conversion-free path an application has without them
-> profiles/video_frame.txt.

  video_frame_bench.py OUT --parent-lib LIB [--rounds N] [--warmup W] [--trace-dir DIR]
  video_frame_bench.py --step WxH:OP:SIDE [--rounds N] [--warmup W]      one step in this process; one JSON line

The protocol is tools/device_image_bench.py's: a measurement is the host clock around whole calls -- every call ends in a device
synchronise -- on one context, N timed rounds after W, median (p10 .. p90).  A row is a size (256 x 256, 1920 x 1080, 3840 x 2160) and an
operation (put, update).  Its video side is a process on this tree's library: BGRA8, NV12 and P010 frames in device memory, the two planar
formats with and without FDH_VIDEO_CHROMA_LINEAR, and fdh_*_image_device of the RGBA8 source as a control, alternating round by round.  Its yardstick is a process on --parent-lib, the parent
commit's library: fdh_put_image_device / fdh_update_image_device of an RGBA8 source of the same size in device memory -- what an
application that has converted the frame by itself calls today; the conversion pass itself is NOT in that row.  The two processes of a
row run one after the other, video first for even rows, yardstick first for odd ones.  For a put the atlas (4096) is reset before every
round outside the clock; an update goes to the entry a put made once.  --trace-dir: the video side of every row once more under
rocprofv3 --kernel-trace --stats, runs of their own, for the kernels' own times.  Every step is a child process under its own time limit,
nothing is started after a failure, and what was not reached is written down as "not measured".  There is no CPU fallback: without a
device the context cannot be made and the step fails.

The hypothesis, stated before measuring: an NV12 update is not slower than the RGBA8 one -- it reads 1.5 bytes per pixel against 4 and
stores the same.  Whatever comes out is written down; nothing here gates a test."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((256, 256), (1920, 1080), (3840, 2160))
OPS = ("put", "update")
KERNELS = ("k_video_import<", "k_image_import<", "k_image_import_tail", "k_minify2", "k_atlas_blit")


def step(w, h, op, side, rounds, warmup):
    import numpy as np
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(w)
    hip = C.CDLL("libamdhip64.so")

    def device(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0  # (a bare int would travel as 32 bits)
        return p.value

    ctx = HipContext(atlas_size=4096, device=0)
    texels = device(rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8))
    legs = {}
    if side == "rgba8":
        call = ctx.put_image_device if op == "put" else ctx.update_image_device
        legs["rgba8, image_device"] = lambda: call(1, texels, w, h, 4 * w)
    else:
        cw, ch = (w + 1) // 2, (h + 1) // 2
        y8, c8 = device(rng.integers(0, 256, size=(h, w)).astype(np.uint8)), device(rng.integers(0, 256, size=(ch, cw, 2)).astype(np.uint8))
        y16, c16 = device(rng.integers(0, 65536, size=(h, w)).astype(np.uint16)), device(rng.integers(0, 65536, size=(ch, cw, 2)).astype(np.uint16))
        call = ctx.put_video_frame if op == "put" else ctx.update_video_frame
        same = ctx.put_image_device if op == "put" else ctx.update_image_device
        legs["rgba8, same process"] = lambda: same(1, texels, w, h, 4 * w)  # the yardstick's call among the others: what alternating sources cost
        legs["bgra8"] = lambda: call(1, texels, 0, w, h, 4 * w, 0, format=0, matrix=0, range=0)
        for linear in (0, 1):
            legs["nv12" + (", linear" if linear else "")] = lambda linear=linear: call(1, y8, c8, w, h, w, 2 * cw, format=1, flags=linear)
            legs["p010" + (", linear" if linear else "")] = lambda linear=linear: call(1, y16, c16, w, h, 2 * w, 4 * cw, format=2, flags=linear)
    us = {leg: [] for leg in legs}
    if op == "update":
        ctx.put_image_device(1, texels, w, h, 4 * w)
    for k in range(warmup + rounds):
        for leg, f in legs.items():
            if op == "put":
                ctx.reset_atlas()
            ctx.sync()
            t1 = time.perf_counter()
            f()
            t2 = time.perf_counter()
            if k >= warmup:
                us[leg].append((t2 - t1) * 1e6)
    ctx.close()
    q = lambda v, f: sorted(v)[int(f * (len(v) - 1))]  # noqa: E731
    print(json.dumps({"step": f"{w}x{h}:{op}:{side}", **{leg: [statistics.median(v), q(v, 0.1), q(v, 0.9)] for leg, v in us.items()}}))


def run_child(name, rounds, warmup, lib, limit=240, trace_dir=None):
    """one step as a process of its own -> its JSON line; under the profiler: {kernel: (launches, mean, least, most)} in us; None: it failed"""
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

    found = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for kernel in KERNELS:
                if kernel in row["Name"]:
                    found[row["Name"].split("(")[0]] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3)
    return found or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--step")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--trace-dir")
    args = ap.parse_args()
    if args.step:
        size, op, side = args.step.split(":")
        w, h = (int(v) for v in size.split("x"))
        step(w, h, op, side, args.rounds, args.warmup)
        return 0
    if not args.out or not args.parent_lib:
        ap.error("OUT and --parent-lib")
    fmt = lambda v: f"{v[0]:9.1f} ({v[1]:8.1f} .. {v[2]:8.1f})"  # noqa: E731
    lines = ["tools/video_frame_bench.py -- decoded video frames into the atlas (k_video_import, k_image_import_tail), MI355X.",
             "whole calls = host clock around the call (each ends in a device synchronise), profiler off, one context, atlas 4096; a put's atlas is reset",
             f"before every round outside the clock; {args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds.  video rows: this tree's library,",
             "the planes in device memory, the five kinds and the yardstick's own call (rgba8, same process) alternating in one process.  yardstick row: the PARENT commit's library, fdh_put_image_device /",
             "fdh_update_image_device of an RGBA8 source of the same size in device memory (the conversion an application would run first is not in it),",
             "a process of its own; the two processes of a row alternate their order from row to row.",
             "hypothesis, stated before measuring: an NV12 update is not slower than the RGBA8 one (1.5 bytes read per pixel against 4, the same stored).", ""]
    ok = True
    slower = []
    for n, ((w, h), op) in enumerate((s, o) for s in SIZES for o in OPS):
        order = ("video", "rgba8") if n % 2 == 0 else ("rgba8", "video")
        got = {}
        for side in order:
            got[side] = run_child(f"{w}x{h}:{op}:{side}", args.rounds, args.warmup, args.parent_lib if side == "rgba8" else None) if ok else None
            ok = ok and got[side] is not None
        lines.append(f"{w} x {h}, {op}")
        if not ok:
            lines.append("    not measured")
            continue
        base = got["rgba8"]["rgba8, image_device"]
        lines.append(f"    {'rgba8, parent commit':24s} {fmt(base)}")
        for leg, v in got["video"].items():
            if leg == "step":
                continue
            note = ""
            if v[0] > base[0] + (base[2] - base[1]):
                note = "   SLOWER than the yardstick beyond its spread"
                slower.append(f"{w} x {h} {op} {leg}")
            lines.append(f"    {leg:24s} {fmt(v)}   yardstick / this = {base[0] / v[0]:5.2f}{note}")
        print("\n".join(lines[-7:]), flush=True)
    lines += ["", "rows slower than their yardstick beyond the yardstick's own spread (p90 - p10): " + (", ".join(slower) if slower else "none")]
    lines += ["", "the kernels alone, us per launch: mean (least .. most), rocprofv3 --kernel-trace --stats, a run of its own per row"]
    for (w, h) in SIZES:
        for op in OPS:
            got = run_child(f"{w}x{h}:{op}:video", args.rounds, args.warmup, None, trace_dir=os.path.join(args.trace_dir, f"{w}_{op}")) if ok and args.trace_dir else None
            ok = ok and (got is not None or not args.trace_dir)
            lines.append(f"{w} x {h}, {op}" + ("" if got else ": not measured"))
            for kernel, v in sorted((got or {}).items()):
                lines.append(f"    {kernel:56s} {v[1]:9.1f} ({v[2]:8.1f} .. {v[3]:8.1f}) over {v[0]} launches")
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
