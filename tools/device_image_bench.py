#!/usr/bin/env python3
"""What an atlas image from device memory costs (fdh_put_image_device, fdh_update_image_device; include_glyphs/figdraw_hip_device_image.h)
on an MI355X, against the host calls it spares -> profiles/device_image.txt.

  device_image_bench.py OUT --parent-lib LIB [--rounds N] [--warmup W] [--trace-dir DIR]
  device_image_bench.py --step SIZE:OP:SIDE [--rounds N] [--warmup W]      one step in this process; one JSON line

The protocol is tools/image_sdf_bench.py's: a measurement is the host clock around whole calls -- every call ends in a device synchronise
-- on one context, N timed rounds after W, median (p10 .. p90).  A row is a size (32, 256, 1024, 2048 square) and an operation (put,
update).  Its device side is a process on this tree's library: the three formats (RGBA8, four float32 planes, four half planes) from
device memory, alternating round by round; at 32 x 32 also fdh_put_glyph_image, the library's cheapest put from the host.  Its host side
is a process on --parent-lib, the parent commit's library: fdh_put_image / fdh_update_image of the same texels from pageable memory.  The
two processes of a row run one after the other, device first for even rows, host first for odd ones.  For a put the atlas (2048; 4096 for
the 2048 image) is reset before every round outside the clock; an update goes to the entry a put made once.  --trace-dir: the device side
of every row once more under rocprofv3 --kernel-trace --stats, runs of their own, for the kernels' own times.  Every step is a child
process under its own time limit, nothing is started after a failure, and what was not reached is written down as "not measured".  There
is no CPU fallback: without a device the context cannot be made and the step fails."""
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

SIZES = (32, 256, 1024, 2048)
OPS = ("put", "update")
KERNELS = ("k_image_import<", "k_image_import_tail")


def step(size, op, side, rounds, warmup):
    import numpy as np
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(size)
    rgba = rng.integers(0, 256, size=(size, size, 4)).astype(np.uint8)
    ctx = HipContext(atlas_size=4096 if size > 2000 else 2048, device=0)
    legs = {}
    if side == "host":
        legs["host"] = (lambda: ctx.put_image(1, rgba)) if op == "put" else (lambda: ctx.update_image(1, rgba))
    else:
        hip = C.CDLL("libamdhip64.so")

        def device(a):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
            assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0  # (a bare int would travel as 32 bits)
            return p.value

        planes = np.ascontiguousarray(rgba.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0)
        sources = {"rgba8": (device(rgba), 4 * size, 0, 0, 4), "float32": (device(planes), 4 * size, 4 * size * size, 1, 4),
                   "float16": (device(planes.astype(np.float16)), 2 * size, 2 * size * size, 2, 4)}
        call = ctx.put_image_device if op == "put" else ctx.update_image_device
        for name, (ptr, pitch, plane, fmt, ch) in sources.items():
            legs[name] = (lambda ptr=ptr, pitch=pitch, plane=plane, fmt=fmt, ch=ch: call(1, ptr, size, size, pitch, format=fmt, channels=ch, plane_bytes=plane))
        if size == 32 and op == "put":
            legs["glyph image"] = lambda: ctx.put_glyph_image(1, rgba)
    us = {leg: [] for leg in legs}
    if op == "update":
        ctx.put_image(1, rgba)
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
    print(json.dumps({"step": f"{size}:{op}:{side}", **{leg: [statistics.median(v), q(v, 0.1), q(v, 0.9)] for leg, v in us.items()}}))


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
        step(int(size), op, side, args.rounds, args.warmup)
        return 0
    if not args.out or not args.parent_lib:
        ap.error("OUT and --parent-lib")
    fmt = lambda v: f"{v[0]:9.1f} ({v[1]:8.1f} .. {v[2]:8.1f})"  # noqa: E731
    lines = ["tools/device_image_bench.py -- atlas images from device memory (k_image_import, k_image_import_tail), MI355X.",
             "whole calls = host clock around the call (each ends in a device synchronise), profiler off, one context; a put's atlas is reset before every",
             f"round outside the clock; {args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds.  device rows: this tree's library, the source in device",
             "memory, the three formats alternating in one process.  host row: the PARENT commit's library, fdh_put_image / fdh_update_image of the same",
             "texels from pageable host memory, a process of its own; the two processes of a size alternate their order from row to row.", ""]
    ok = True
    slower = []
    for n, (size, op) in enumerate((s, o) for s in SIZES for o in OPS):
        order = ("device", "host") if n % 2 == 0 else ("host", "device")
        got = {}
        for side in order:
            got[side] = run_child(f"{size}:{op}:{side}", args.rounds, args.warmup, args.parent_lib if side == "host" else None) if ok else None
            ok = ok and got[side] is not None
        lines.append(f"{size} x {size}, {op}")
        if not ok:
            lines.append("    not measured")
            continue
        host = got["host"]["host"]
        lines.append(f"    {'host, parent commit':24s} {fmt(host)}")
        for leg, v in got["device"].items():
            if leg == "step":
                continue
            note = ""
            if leg != "glyph image" and v[0] > host[0] + (host[2] - host[1]):
                note = "   SLOWER than the host row beyond its spread"
                slower.append(f"{size} x {size} {op} {leg}")
            lines.append(f"    {leg:24s} {fmt(v)}   host / this = {host[0] / v[0]:5.2f}{note}")
        print("\n".join(lines[-6:]), flush=True)
    lines += ["", "rows slower than their host row beyond the host row's own spread (p90 - p10): " + (", ".join(slower) if slower else "none")]
    lines += ["", "the kernels alone, us per launch: mean (least .. most), rocprofv3 --kernel-trace --stats, a run of its own per row"]
    for size in SIZES:
        for op in OPS:
            got = run_child(f"{size}:{op}:device", args.rounds, args.warmup, None, trace_dir=os.path.join(args.trace_dir, f"{size}_{op}")) if ok and args.trace_dir else None
            ok = ok and (got is not None or not args.trace_dir)
            lines.append(f"{size} x {size}, {op}" + ("" if got else ": not measured"))
            for kernel, v in sorted((got or {}).items()):
                lines.append(f"    {kernel:40s} {v[1]:9.1f} ({v[2]:8.1f} .. {v[3]:8.1f}) over {v[0]} launches")
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
