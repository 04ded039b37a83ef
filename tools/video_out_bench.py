#!/usr/bin/env python3
"""What the rendered frame costs on its way out as NV12, P010 or BGRA8 (fdh_read_video_frame; include_video/figdraw_hip_video_out.h) on
an MI355X, against a plain device-to-device copy of the frame and against what an application does without the call
-> profiles/video_out.txt.

  video_out_bench.py OUT --parent-lib LIB [--rounds N] [--warmup W] [--trace-dir DIR]
  video_out_bench.py --step WxH:SIDE [--rounds N] [--warmup W]      one step in this process; one JSON line

The protocol is tools/video_frame_bench.py's: a measurement is the host clock around whole calls -- every call ends in a device
synchronise -- on one context that holds one rendered frame, N timed rounds after W, median (p10 .. p90).  A row is a size (256 x 256,
1920 x 1080, 3840 x 2160).  Its video side is a process on this tree's library: the frame out as BGRA8, NV12 and P010 into device
memory, the two planar formats with and without FDH_VIDEO_CHROMA_LINEAR, alternating round by round with two yardsticks in the same
process: a device-to-device hipMemcpy2DAsync of the frame (fdh_frame_device_ptr) on the context's stream plus a synchronise -- the floor
of a call that ends in a synchronise -- and fdh_read_pixels of the whole frame.  Its other yardstick is a process on --parent-lib, the
parent commit's library, doing what an application does today: fdh_read_pixels of the whole frame into pageable host memory (the
conversion it would run on the CPU afterwards is NOT in that row).  The two processes of a row run one after the other, video first for
even rows, parent first for odd ones.  --trace-dir: the video side of every row once more under rocprofv3 --kernel-trace --stats, runs of
their own, for the kernels' own times.  Every step is a child process under its own time limit, nothing is started after a failure, and
what was not reached is written down as "not measured".  There is no CPU fallback: without a device the context cannot be made and the
step fails.

The hypothesis, stated before measuring: the NV12 export at 3840 x 2160 lies within the spread of k_video_import<BGRA8>'s 24.3 us update
launch (profiles/video_frame.txt) -- it reads the same 33 MB and stores 12 where that stores 33; that file also records that reading fewer
bytes did not make the import faster.  Whatever comes out is written down; nothing here gates a test."""
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
KERNELS = ("k_video_export<",)
HYPOTHESIS_US = 24.3  # k_video_import<BGRA8>'s update launch at 3840 x 2160 (profiles/video_frame.txt)


def step(w, h, side, rounds, warmup):
    import numpy as np
    from figdraw_amd.context import HipContext

    hip = C.CDLL("libamdhip64.so")

    def device(n):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
        return p.value

    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx = HipContext(atlas_size=512, device=0)
    ctx.set_stream(stream.value)
    ctx.put_image(1, np.random.default_rng(w).integers(0, 256, size=(256, 256, 4)).astype(np.uint8))
    ctx.begin_frame(w, h, True, (0.1, 0.2, 0.3, 1.0))
    ctx.draw_rect((0.0, 0.0, w * 0.6, h * 0.5), (200, 40, 90, 255))
    for y in range(0, h, 256):
        for x in range(0, w, 256):
            ctx.draw_image(1, (float(x), float(y)), [(255, 255, 255, 255)] * 4, (256.0, 256.0))
    ctx.end_frame()
    ctx.sync()
    legs = {}
    host = np.empty((h, w, 4), np.uint8)
    legs["read_pixels, parent commit" if side == "parent" else "read_pixels, same process"] = lambda: ctx.L.fdh_read_pixels(ctx.h, 0, 0, w, h, host.ctypes.data)
    if side == "video":
        cw, ch = (w + 1) // 2, (h + 1) // 2
        rgba, y8, c8, y16, c16 = device(4 * w * h), device(w * h), device(2 * cw * ch), device(2 * w * h), device(4 * cw * ch)
        surface = ctx.frame_device_ptr()[0]
        hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]

        def copy():
            assert hip.hipMemcpy2DAsync(rgba, 4 * w, surface, 4 * w, 4 * w, h, 3, stream) == 0  # device -> device
            assert hip.hipStreamSynchronize(stream) == 0

        legs["memcpy2d, device to device"] = copy
        legs["bgra8"] = lambda: ctx.read_video_frame(rgba, 0, 4 * w, 0, format=0, matrix=0, range=0)
        for linear in (0, 1):
            legs["nv12" + (", linear" if linear else "")] = lambda linear=linear: ctx.read_video_frame(y8, c8, w, 2 * cw, format=1, flags=linear)
            legs["p010" + (", linear" if linear else "")] = lambda linear=linear: ctx.read_video_frame(y16, c16, 2 * w, 4 * cw, format=2, flags=linear)
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
        size, side = args.step.split(":")
        w, h = (int(v) for v in size.split("x"))
        step(w, h, side, args.rounds, args.warmup)
        return 0
    if not args.out or not args.parent_lib:
        ap.error("OUT and --parent-lib")
    fmt = lambda v: f"{v[0]:9.1f} ({v[1]:8.1f} .. {v[2]:8.1f})"  # noqa: E731
    lines = ["tools/video_out_bench.py -- the rendered frame out as NV12, P010 or BGRA8 (k_video_export), MI355X.",
             "whole calls = host clock around the call (each ends in a device synchronise), profiler off, one context holding one rendered frame;",
             f"{args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds.  video rows: this tree's library, the planes in device memory, the five kinds,",
             "a device-to-device hipMemcpy2DAsync of the frame on the context's stream plus a synchronise (the floor of a call that ends in one) and",
             "fdh_read_pixels alternating in one process.  parent row: the PARENT commit's library doing what an application does today, fdh_read_pixels",
             "of the whole frame into pageable host memory (the conversion on the CPU that would follow is not in it), a process of its own; the two",
             "processes of a row alternate their order from row to row.",
             f"hypothesis, stated before measuring: the NV12 export's kernel at 3840 x 2160 lies within the spread of k_video_import<BGRA8>'s {HYPOTHESIS_US} us update",
             "launch (profiles/video_frame.txt): the same 33 MB read, 12 MB stored where that stores 33.", ""]
    ok = True
    for n, (w, h) in enumerate(SIZES):
        order = ("video", "parent") if n % 2 == 0 else ("parent", "video")
        got = {}
        for side in order:
            got[side] = run_child(f"{w}x{h}:{side}", args.rounds, args.warmup, args.parent_lib if side == "parent" else None) if ok else None
            ok = ok and got[side] is not None
        lines.append(f"{w} x {h}")
        if not ok:
            lines.append("    not measured")
            continue
        base, floor = got["parent"]["read_pixels, parent commit"], got["video"]["memcpy2d, device to device"]
        lines.append(f"    {'read_pixels, parent commit':28s} {fmt(base)}")
        for leg, v in got["video"].items():
            if leg != "step":
                lines.append(f"    {leg:28s} {fmt(v)}   this / copy = {v[0] / floor[0]:5.2f}   read_pixels of the parent / this = {base[0] / v[0]:6.2f}")
        print("\n".join(lines[-9:]), flush=True)
    lines += ["", "the kernels alone, us per launch: mean (least .. most), rocprofv3 --kernel-trace --stats, a run of its own per row"]
    verdict = "not measured"
    for (w, h) in SIZES:
        got = run_child(f"{w}x{h}:video", args.rounds, args.warmup, None, trace_dir=os.path.join(args.trace_dir, f"{w}")) if ok and args.trace_dir else None
        ok = ok and (got is not None or not args.trace_dir)
        lines.append(f"{w} x {h}" + ("" if got else ": not measured"))
        for kernel, v in sorted((got or {}).items()):
            lines.append(f"    {kernel:56s} {v[1]:9.1f} ({v[2]:8.1f} .. {v[3]:8.1f}) over {v[0]} launches")
            if (w, h) == SIZES[-1] and "<1u, false>" in kernel.replace("(unsigned int)1", "1u"):
                verdict = f"the NV12 export's kernel takes {v[1]:.1f} us ({v[2]:.1f} .. {v[3]:.1f}) against {HYPOTHESIS_US} us"
    lines += ["", "verdict on the hypothesis: " + verdict]
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
