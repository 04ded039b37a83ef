#!/usr/bin/env python3
"""What 4:2:2 video costs on its way into the atlas and out of the frame (fdh_update_video_422, fdh_read_video_422;
include_video/figdraw_hip_video_422.h) on an MI355X, against the three-plane calls on either side of it -> profiles/video_422.txt.

  video_422_bench.py OUT [--rounds N] [--warmup W] [--trace-dir DIR]
  video_422_bench.py --step WxH:in|out [--rounds N] [--warmup W]      one step in this process; one JSON line

The protocol is that of tools/video_planar_bench.py: a measurement is the host clock around whole calls -- every call ends in a device
synchronise -- on one context (atlas 4096 for the way in; one rendered frame for the way out), N timed rounds after W, median
(p10 .. p90), the legs of a step alternating round by round in one process, at 1920 x 1080 and 3840 x 2160, planes tightly packed in
device memory.  The legs:
  the measuring stick: fdh_update_video_planes / fdh_read_video_planes as the parent commit has them (their translation units are
      untouched here) for I420 and I444, and for I010 and I410;
  the new calls: I422, YUY2, UYVY beside the 8-bit stick, I210 beside the 10-bit one.
--trace-dir: every step once more under rocprofv3 --kernel-trace --stats, runs of their own, for the kernels' own times.  Every step is
a child process under its own time limit, nothing is started after a failure, and what was not reached is written down as "not
measured".  There is no CPU fallback.

The hypothesis, stated before measuring: a 4:2:2 frame moves 2 bytes per pixel (4 for I210) beside the surface's or the atlas's 4,
between 4:2:0's 1.5 (3) and 4:4:4's 3 (6), and the kernels have their siblings' shape: the time of a 4:2:2 call lies between the
4:2:0 call's and the 4:4:4 call's of the same bit depth, the spread allowed for -- its median is not below the 4:2:0 leg's p10 and not
above the 4:4:4 leg's p90.  Whatever comes out is written down; nothing here gates a test."""
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

SIZES = ((1920, 1080), (3840, 2160))
KERNELS = ("k_video_422_import<", "k_video_422_export<", "k_video_planar_import<", "k_video_planar_export<", "k_image_import_tail")
# leg -> (the call's family, format, bit depth, chroma: 0 = 4:2:0, 1 = 4:2:2, 2 = 4:4:4, 3 = packed)
LEGS = {"i420": ("planes", 3, 8, 0), "i422": ("422", 7, 8, 1), "yuy2": ("422", 9, 8, 3), "uyvy": ("422", 10, 8, 3), "i444": ("planes", 5, 8, 2),
        "i010": ("planes", 4, 10, 0), "i210": ("422", 8, 10, 1), "i410": ("planes", 6, 10, 2)}
BETWEEN = (("i422", "i420", "i444"), ("yuy2", "i420", "i444"), ("uyvy", "i420", "i444"), ("i210", "i010", "i410"))


def step(w, h, side, rounds, warmup):
    import numpy as np
    from figdraw_amd.context import HipContext

    hip = C.CDLL("libamdhip64.so")

    def device(n, data=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
        if data is not None:
            assert hip.hipMemcpy(p, C.c_void_p(data.ctypes.data), C.c_size_t(n), 1) == 0
        return p.value

    ctx = HipContext(atlas_size=4096 if side == "in" else 512, device=0)
    assert w % 16 == 0 and h % 2 == 0
    rng = np.random.default_rng(w)
    legs = {}
    if side == "in":
        first = device(w * h * 4, rng.integers(0, 256, size=(h, 4 * w)).astype(np.uint8))
        ctx.put_video_422(1, (first, 0, 0), w, h, (2 * w, 0, 0), format=9)  # one entry, key 1: every leg is an update of it
    else:
        ctx.put_image(1, rng.integers(0, 256, size=(256, 256, 4)).astype(np.uint8))
        ctx.begin_frame(w, h, True, (0.1, 0.2, 0.3, 1.0))
        ctx.draw_rect((0.0, 0.0, w * 0.6, h * 0.5), (200, 40, 90, 255))
        for y in range(0, h, 256):
            for x in range(0, w, 256):
                ctx.draw_image(1, (float(x), float(y)), [(255, 255, 255, 255)] * 4, (256.0, 256.0))
        ctx.end_frame()
        ctx.sync()
    for name, (family, fmt, bits, chroma) in LEGS.items():
        es, dt = (1, np.uint8) if bits == 8 else (2, np.uint16)
        if chroma == 3:
            shapes, pitches = [(h, 2 * w)], (2 * w, 0, 0)
        else:
            cw, ch = (w, h) if chroma == 2 else (w // 2, h) if chroma == 1 else (w // 2, h // 2)
            shapes, pitches = [(h, w), (ch, cw), (ch, cw)], (w * es, cw * es, cw * es)
        mk = (lambda s: device(int(np.prod(s)) * es, rng.integers(0, 1 << bits, size=s).astype(dt))) if side == "in" else (lambda s: device(int(np.prod(s)) * es))
        ptrs = tuple([mk(s) for s in shapes] + [0] * (3 - len(shapes)))
        if side == "in":
            call = ctx.update_video_422 if family == "422" else ctx.update_video_planes
            legs[name] = lambda call=call, ptrs=ptrs, pitches=pitches, fmt=fmt: call(1, ptrs, w, h, pitches, format=fmt)
        else:
            call = ctx.read_video_422 if family == "422" else ctx.read_video_planes
            legs[name] = lambda call=call, ptrs=ptrs, pitches=pitches, fmt=fmt: call(ptrs, pitches, format=fmt)
    us = {leg: [] for leg in legs}
    for k in range(warmup + rounds):
        for leg, f in legs.items():
            ctx.sync()
            t1 = time.perf_counter()
            f()
            t2 = time.perf_counter()
            if k >= warmup:
                us[leg].append((t2 - t1) * 1e6)
    ctx.close()
    q = lambda v, f: sorted(v)[int(f * (len(v) - 1))]  # noqa: E731
    print(json.dumps({"step": f"{w}x{h}:{side}", **{leg: [statistics.median(v), q(v, 0.1), q(v, 0.9)] for leg, v in us.items()}}))


def run_child(name, rounds, warmup, limit=240, trace_dir=None):
    """one step as a process of its own -> its JSON line; under the profiler: {kernel: (launches, mean, least, most)} in us; None: it failed"""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--rounds", str(rounds), "--warmup", str(warmup)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", trace_dir, "-o", "t", "--"] + cmd
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
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
            if any(kernel in row["Name"] for kernel in KERNELS):
                found[row["Name"].split("(")[0]] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3)
    return found or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--step")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-dir")
    args = ap.parse_args()
    if args.step:
        size, side = args.step.split(":")
        w, h = (int(v) for v in size.split("x"))
        step(w, h, side, args.rounds, args.warmup)
        return 0
    if not args.out:
        ap.error("OUT")
    fmt = lambda v: f"{v[0]:9.1f} ({v[1]:8.1f} .. {v[2]:8.1f})"  # noqa: E731
    lines = ["tools/video_422_bench.py -- 4:2:2 video in (k_video_422_import, k_image_import_tail) and out (k_video_422_export), MI355X.",
             "whole calls = host clock around the call (each ends in a device synchronise), profiler off, one context; the way in: fdh_update_* of an",
             "entry in an atlas of 4096; the way out: one rendered frame; planes tightly packed in device memory;",
             f"{args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds; the legs of a step alternate round by round in one process.",
             "i420, i444, i010, i410: fdh_update_video_planes / fdh_read_video_planes as the parent commit has them (their translation units are",
             "untouched), the measuring stick; i422, yuy2, uyvy, i210: the new calls.",
             "hypothesis, stated before measuring: a 4:2:2 call's time lies between the 4:2:0 call's and the 4:4:4 call's of the same bit depth, the",
             "spread allowed for: its median is not below the 4:2:0 leg's p10 and not above the 4:4:4 leg's p90.", ""]
    ok, verdicts = True, []
    for (w, h) in SIZES:
        for side in ("in", "out"):
            got = run_child(f"{w}x{h}:{side}", args.rounds, args.warmup) if ok else None
            ok = ok and got is not None
            lines.append(f"{w} x {h}, the way {side}" + ("" if got else ": not measured"))
            if not got:
                continue
            legs = {k: v for k, v in got.items() if k != "step"}
            for leg, v in legs.items():
                lines.append(f"    {leg:8s} {fmt(v)}")
            for mine, lo, hi in BETWEEN:
                m, a, b = legs[mine], legs[lo], legs[hi]
                where = "between" if a[1] <= m[0] <= b[2] else "BELOW the 4:2:0 call" if m[0] < a[1] else "ABOVE the 4:4:4 call"
                verdicts.append(f"{w} x {h} {side} {mine}: {m[0]:.1f} us, {where} ({lo} {a[0]:.1f}, {hi} {b[0]:.1f}); {mine} / {lo} = {m[0] / a[0]:.2f}, {mine} / {hi} = {m[0] / b[0]:.2f}")
            print("\n".join(lines[-9:]), flush=True)
    lines += ["", "the kernels alone, us per launch: mean (least .. most), rocprofv3 --kernel-trace --stats, a run of its own per step"]
    for (w, h) in SIZES:
        for side in ("in", "out"):
            got = run_child(f"{w}x{h}:{side}", args.rounds, args.warmup, trace_dir=os.path.join(args.trace_dir, f"{w}_{side}")) if ok and args.trace_dir else None
            ok = ok and (got is not None or not args.trace_dir)
            lines.append(f"{w} x {h}, the way {side}" + ("" if got else ": not measured"))
            for kernel, v in sorted((got or {}).items()):
                lines.append(f"    {kernel:64s} {v[1]:9.1f} ({v[2]:8.1f} .. {v[3]:8.1f}) over {v[0]} launches")
    lines += ["", "verdict on the hypothesis:"] + (["    " + v for v in verdicts] or ["    not measured"])
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
