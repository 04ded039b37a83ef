#!/usr/bin/env python3
"""What an atlas image from device memory costs (fdh_put_image_device, fdh_update_image_device; include_glyphs/figdraw_hip_device_image.h)
on an MI355X, against the host calls it spares -> profiles/device_image.txt.

  device_image_bench.py OUT --parent-lib LIB [--rounds N] [--warmup W] [--trace-dir DIR]
  device_image_bench.py --step SIZE:OP:SIDE [--rounds N] [--warmup W]      one step in this process; one JSON line
  device_image_bench.py --batch OUT --parent-lib LIB [--rounds N] [--warmup W]      the batch calls -> profiles/device_image_batch.txt

The protocol is tools/image_sdf_bench.py's: a measurement is the host clock around whole calls -- every call ends in a device synchronise
-- on one context, N timed rounds after W, median (p10 .. p90).  A row is a size (32, 256, 1024, 2048 square) and an operation (put,
update).  Its device side is a process on this tree's library: the three formats (RGBA8, four float32 planes, four half planes) from
device memory, alternating round by round; at 32 x 32 also fdh_put_glyph_image, the library's cheapest put from the host.  Its host side
is a process on --parent-lib, the parent commit's library: fdh_put_image / fdh_update_image of the same texels from pageable memory.  The
two processes of a row run one after the other, device first for even rows, host first for odd ones.  For a put the atlas (2048; 4096 for
the 2048 image) is reset before every round outside the clock; an update goes to the entry a put made once.  --trace-dir: the device side
of every row once more under rocprofv3 --kernel-trace --stats, runs of their own, for the kernels' own times.  Every step is a child
process under its own time limit, nothing is started after a failure, and what was not reached is written down as "not measured".  There
is no CPU fallback: without a device the context cannot be made and the step fails.

--batch (fdh_put_images_device, fdh_update_images_device; include_glyphs/figdraw_hip_device_images.h): the same protocol.  A row is a size (32,
128, 256 square), an operation, a format (RGBA8, four half planes) and n = 1, 4, 16, 64, 256 images; what is timed is ONE batch call of n
images on this tree's library against n single calls on --parent-lib, each side a process of its own per size and operation (the formats
and the n alternate inside it), the two processes alternating their order from row to row.  The n images share one source per format."""
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


BATCH_SIZES = (32, 128, 256)
BATCH_N = (1, 4, 16, 64, 256)
BATCH_HEAD = """tools/device_image_bench.py --batch -- n atlas images from device memory as ONE fdh_put_images_device / fdh_update_images_device (this tree's
library) against n single fdh_put_image_device / fdh_update_image_device calls of the PARENT commit's library, MI355X.

Hypotheses, written before the first number:
- a single call is launch plus synchronise, about 28 us for a put and 19 - 20 us for an update whatever the size up to 256 x 256
  (profiles/device_image.txt); n single calls cost n times that.
- a batch pays one copy of its tables, at most four launches and one synchronise, plus the host's work per image (validation, pointer
  attributes, placement, the tables, folding the ink blocks) and the device's work per tile.  Expected: at n = 1 the batch costs a single
  call plus the table copy, a few microseconds more; from n = 4 on it is faster, and the ratio grows with n until the per-image host work or
  the tiles' device time dominates -- 256 images of 256 x 256 are 16 384 tiles, tens of microseconds of device time.
- what would refute it: a batch of 4 no faster than 4 single calls (the table copy, a pageable hipMemcpyAsync, costing as much as the
  launches it saves), or a per-image host cost near a single call's (hipPointerGetAttributes per image is the suspect).
"""


def batch_step(size, op, side, rounds, warmup):
    """one size and operation on one side: "batch" -- one call of n images -- or "single" -- n calls; the formats and the n alternate"""
    import numpy as np
    from figdraw_amd.context import HipContext

    rng = np.random.default_rng(size)
    rgba = rng.integers(0, 256, size=(size, size, 4)).astype(np.uint8)
    atlas = 1024
    while atlas < 16 * (size + 8):
        atlas *= 2
    ctx = HipContext(atlas_size=atlas, device=0)
    hip = C.CDLL("libamdhip64.so")

    def device(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    planes = (np.ascontiguousarray(rgba.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0)).astype(np.float16)
    sources = {"rgba8": (device(rgba), size, size, 4 * size, 0, 4, 0), "float16": (device(planes), size, size, 2 * size, 2, 4, 2 * size * size)}
    legs = {}
    for name, src in sources.items():
        for n in BATCH_N:
            items = [(k + 1,) + src for k in range(n)]
            if side == "batch":
                legs[f"{name} {n}"] = (lambda items=items: ctx.put_images_device(items)) if op == "put" else (lambda items=items: ctx.update_images_device(items))
            else:
                call = ctx.put_image_device if op == "put" else ctx.update_image_device
                legs[f"{name} {n}"] = lambda items=items, call=call: [call(k, ptr, w, h, pitch, format=fmt, channels=ch, plane_bytes=plane) for k, ptr, w, h, pitch, fmt, ch, plane in items]
    us = {leg: [] for leg in legs}
    launches = {}
    if op == "update":
        for k in range(max(BATCH_N)):
            ctx.put_image_device(k + 1, *sources["rgba8"][:4])
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
            if side == "batch":
                launches[leg] = ctx.image_batch_stats()["launches"]
    ctx.close()
    q = lambda v, f: sorted(v)[int(f * (len(v) - 1))]  # noqa: E731
    print(json.dumps({"step": f"{size}:{op}:{side}", "launches": launches, **{leg: [statistics.median(v), q(v, 0.1), q(v, 0.9)] for leg, v in us.items()}}))


def batch_main(args):
    fmt = lambda v: f"{v[0]:9.1f} ({v[1]:8.1f} .. {v[2]:8.1f})"  # noqa: E731
    lines = [BATCH_HEAD, "whole calls = host clock around the call or the n calls (each call ends in a device synchronise), profiler off, one context; a put's atlas is",
             f"reset before every round outside the clock; {args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds.", ""]
    ok, findings = True, []
    for row, (size, op) in enumerate((s, o) for s in BATCH_SIZES for o in OPS):
        order = ("batch", "single") if row % 2 == 0 else ("single", "batch")
        got = {}
        for side in order:
            name = f"batch:{size}:{op}:{side}"
            got[side] = run_child(name, args.rounds, args.warmup, args.parent_lib if side == "single" else None) if ok else None
            ok = ok and got[side] is not None
        lines.append(f"{size} x {size}, {op}   ({order[0]} first)")
        if not ok:
            lines.append("    not measured")
            continue
        for leg, b in got["batch"].items():
            if leg in ("step", "launches"):
                continue
            s1 = got["single"][leg]
            n = int(leg.split()[1])
            spread = s1[2] - s1[1]
            note = ""
            if n >= 4 and not b[0] < s1[0] - spread:
                note = "   FINDING: not faster than the single calls by more than their spread"
            if n == 1 and b[0] > s1[0] + spread:
                note = "   FINDING: slower than the single call beyond its spread"
            if note:
                findings.append(f"{size} x {size} {op} {leg}")
            lines.append(f"    {leg:12s} batch {fmt(b)}   {n:3d} single calls, parent {fmt(s1)}   single / batch = {s1[0] / b[0]:6.2f}   launches {got['batch']['launches'][leg]}{note}")
        print("\n".join(lines[-11:]), flush=True)
    lines += ["", "rows that miss their condition (n >= 4: faster than the parent's n single calls by more than that row's p90 - p10; n = 1: no slower beyond it): "
              + (", ".join(findings) if findings else "none")]
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


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
    ap.add_argument("--batch", action="store_true", help="the batch calls against n single calls of --parent-lib")
    args = ap.parse_args()
    if args.step:
        if args.step.startswith("batch:"):
            _, size, op, side = args.step.split(":")
            batch_step(int(size), op, side, args.rounds, args.warmup)
            return 0
        size, op, side = args.step.split(":")
        step(int(size), op, side, args.rounds, args.warmup)
        return 0
    if not args.out or not args.parent_lib:
        ap.error("OUT and --parent-lib")
    if args.batch:
        return batch_main(args)
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
