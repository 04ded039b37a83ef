#!/usr/bin/env python3
"""Exact damage readback (include/figdraw_hip_exact.h): what a read costs with the mode off and on, raw and coded.

  raw off    fdh_read_damage, fdh_set_damage_exact(ctx, 0)        coded off    fdh_read_damage_coded, mode off
  raw on     fdh_read_damage, fdh_set_damage_exact(ctx, 1)        coded on     fdh_read_damage_coded, mode on

Cases: tools/damage_readback_bench.py's (a), (c) and (s); (t) = (s) with a static frame; (h) the bench tree at 1080p with its middle
root, which is fully hidden, moved as tests/test_damage_exact.py moves it; (w) two distant frames of the bench tree's animation
alternating, so that (nearly) every bin changes every frame.

usage:
  damage_exact_bench.py --all OUT.txt [--parent-lib LIB]   every step below as a child process of its own, each under its own time limit,
                                                            nothing started after a failure; writes the report
  damage_exact_bench.py --time CASE                         the four ways alternated in one process, three turns, 200 timed frames after
                                                            20 warm-up frames per turn; one JSON line
  damage_exact_bench.py --trace CASE [--frames N]           N frames, each followed by fdh_read_damage with the mode on (run it under
                                                            rocprofv3 --kernel-trace --stats -f csv); one JSON line"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = {"a": "glyph 4K, one row edited", "c": "bench tree 1080p, one root moved", "s": "S300@4K bench frame, tracking off, animated",
         "t": "S300@4K bench frame, tracking off, static", "h": "bench tree 1080p, the hidden middle root moved by (3, 2)",
         "w": "bench tree 1080p, frames 0 and 40 alternating"}
WAYS = ("raw off", "raw on", "coded off", "coded on")
TILE_BYTES, ENTRY_BYTES = 16384, 24
HBM_PEAK = 8e12  # bytes/s (MI355X_MICROARCH: the specification, not a measurement)

HYPOTHESES = [
    "Hypotheses (stated before the numbers; nothing below had been timed when they were written):",
    "  1. With at most a tenth of the pending bins changed, the exact read is faster than the mode-off read on the same box; at 4K with every",
    "     bin pending by about an order of magnitude: the filter moves at most 3 x 33.4 MB in HBM (~25 us at half of peak) against",
    "     596 - 614 us for 33.4 MB over the link (profiles/damage_readback.txt).  This is the one gate.",
    "  2. When every bin changed, the exact read costs the mode-off read plus the filter and one synchronise; an overhead above a tenth of",
    "     the mode-off read at 4K needs an explanation.",
    "  3. A read of an unchanged, untracked frame costs the filter and nothing else.",
]


def frames_for(case):
    """-> (w, h, tracking, setup(ctx), frame(ctx, i))"""
    from figdraw_amd.scene import rect
    from figdraw_amd.scenes import make_render_tree_100
    none = lambda ctx: None  # noqa: E731
    if case in ("a", "c"):
        import damage_bench
        w, h, setup, frame = damage_bench.frames_for(case, 0)
        return w, h, True, setup, frame
    if case in ("s", "t"):
        w, h = 3840, 2160
        scenes = [make_render_tree_100(float(w), float(h), frame=f, full_frame_blur=True) for f in range(8 if case == "s" else 1)]
        return w, h, False, none, lambda ctx, i: ctx.render_frame(scenes[i % len(scenes)], w, h)
    w, h = 1920, 1080
    if case == "h":
        sc = make_render_tree_100(float(w), float(h), frame=0)
        lst = next(iter(sc.layers.values()))
        root = lst.rootIds[len(lst.rootIds) * 2 // 4]

        def frame(ctx, i):
            x, y, bw, bh = lst.nodes[root].screenBox
            lst.nodes[root].screenBox = rect(x + (3.0 if i % 2 else -3.0), y + (2.0 if i % 2 else -2.0), bw, bh)
            ctx.render_frame(sc, w, h)
        return w, h, True, none, frame
    if case == "w":
        scenes = [make_render_tree_100(float(w), float(h), frame=f) for f in (0, 40)]
        return w, h, True, none, lambda ctx, i: ctx.render_frame(scenes[i % 2], w, h)
    raise SystemExit(f"unknown case {case}")


def _open(case):
    from figdraw_amd.context import HipContext
    w, h, tracking, setup, frame = frames_for(case)
    ctx = HipContext(device=0)
    setup(ctx)
    ctx.set_damage_tracking(tracking)
    ctx.set_damage_readback(True)
    return ctx, w, h, frame


def time_case(case, timed=200, warm=20, turns=3):
    ctx, w, h, frame = _open(case)
    L, hnd = ctx.L, ctx.h
    gx, gy = (w + 63) // 64, (h + 63) // 64
    t_ptr, p_ptr = C.c_void_p(), C.c_void_p()
    n_c, pend_c, nbytes_c = C.c_int(), C.c_int(), C.c_int64()

    def check(rc):
        if rc != 0:
            raise SystemExit(L.fdh_last_error().decode())

    def read(way):
        """-> (tiles, bytes the read hands to whoever sends them on)"""
        if way.startswith("raw"):
            check(L.fdh_read_damage(hnd, C.byref(t_ptr), C.byref(p_ptr), C.byref(n_c), None, None, None))
            return n_c.value, n_c.value * (TILE_BYTES + 16)
        check(L.fdh_read_damage_coded(hnd, C.byref(t_ptr), C.byref(p_ptr), C.byref(n_c), C.byref(nbytes_c), None, None, None))
        return n_c.value, n_c.value * ENTRY_BYTES + nbytes_c.value

    out = {way: {"read_us": [], "total_us": [], "tiles": [], "pending": [], "bytes": []} for way in WAYS}
    i = 0
    for _ in range(turns):
        for way in WAYS:
            on = way.endswith("on")
            ctx.set_damage_exact(on)  # (turning it on makes the next read a fresh one: it is among the warm-up frames)
            reads, totals, tiles, pending, nbytes = [], [], [], [], []
            for k in range(warm + timed):
                t0 = time.perf_counter()
                frame(ctx, i)
                ctx.sync()
                t1 = time.perf_counter()
                n, b = read(way)  # (every read ends in the stream's synchronise and returns with the tiles in page-locked memory)
                t2 = time.perf_counter()
                i += 1
                if k >= warm:
                    if on:
                        check(L.fdh_damage_exact_stats(hnd, C.byref(pend_c), None, None))
                    reads.append((t2 - t1) * 1e6); totals.append((t2 - t0) * 1e6); tiles.append(n); nbytes.append(b)
                    pending.append(pend_c.value if on else n)
            v = out[way]
            v["read_us"].append(round(statistics.median(reads), 1))
            v["total_us"].append(round(statistics.median(totals), 1))
            v["tiles"].append(round(statistics.mean(tiles), 1))
            v["pending"].append(round(statistics.mean(pending), 1))
            v["bytes"].append(round(statistics.mean(nbytes)))
    ctx.close()
    print(json.dumps({"case": case, "w": w, "h": h, "grid": gx * gy, "timed": timed, "warm": warm, "ways": out}))


def trace_case(case, frames):
    ctx, w, h, frame = _open(case)
    ctx.set_damage_exact(True)
    tiles = pending = 0
    for i in range(frames):
        frame(ctx, i)
        t, _, _ = ctx.read_damage()
        tiles += len(t)
        pending += ctx.damage_exact_stats()[0]
    ctx.close()
    print(json.dumps({"case": case, "frames": frames, "tiles": tiles, "pending": pending, "grid": ((w + 63) // 64) * ((h + 63) // 64)}))


def _kernel_stats(d):
    rows = {}
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        for r in csv.DictReader(open(path)):
            name = r["Name"].split("(")[0].replace("void ", "").replace("fdh::", "").split("<")[0]
            calls, total, lo, hi = rows.get(name, (0, 0.0, 1e30, 0.0))
            rows[name] = (calls + int(r.get("Calls") or 0), total + float(r.get("TotalDurationNs") or 0.0) / 1e3, min(lo, float(r.get("MinNs") or 1e30) / 1e3),
                          max(hi, float(r.get("MaxNs") or 0.0) / 1e3))
    return rows


def _step(cmd, limit, env=None):
    """a child process under its own time limit -> its stdout; None (and a line on stderr) when it failed"""
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print(f"step exceeded {limit} s: {' '.join(cmd)}", file=sys.stderr)
        return None
    if r.returncode != 0:
        print(f"step failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", file=sys.stderr)
        return None
    return r.stdout


def run_all(out_path, parent_lib, trace_dir, cases):
    me = [sys.executable, os.path.abspath(__file__)]
    lines = ["tools/damage_exact_bench.py -- a read with exact damage readback off and on, MI355X.  Host clock, profiler off; per case the four",
             "ways alternated in one process (three turns), 200 timed frames after 20 warm-up frames per turn; medians per turn, us.",
             "read = from the frame's fdh_sync to the read's return (tiles in page-locked memory); pending = bins pending before the filter;",
             "tiles = bins the read returned; bytes = what the read hands on per frame (raw: 16 + 16384 a tile; coded: 24 a tile + payload).", ""]
    lines += HYPOTHESES + [""]
    ok = True
    for case in cases:
        got = _step(me + ["--time", case], 560)
        if got is None:
            ok = False
            break
        print(f"timed case ({case})", flush=True)
        r = json.loads(got.strip().splitlines()[-1])
        lines.append(f"({case}) {CASES[case]}: {r['w']} x {r['h']}, {r['grid']} bins")
        for way in WAYS:
            v = r["ways"][way]
            rd = sorted(v["read_us"])
            lines.append(f"    {way:9s}  read {rd[1]:9.1f} (turns {rd[0]:.1f} .. {rd[2]:.1f})   pending {v['pending'][1]:7.1f}   tiles {v['tiles'][1]:7.1f}   bytes {v['bytes'][1]:10d}")
    if ok:
        os.makedirs(trace_dir, exist_ok=True)
        lines += ["", "rocprofv3 --kernel-trace --stats, a run per case, 60 frames each read with fdh_read_damage, the mode on, every bin pending at 4K",
                  "(the first read of a run is the fresh one: k_damage_filter's fill form, which reads the surface and writes the mirror):"]
        for case in ("t", "s"):
            d = os.path.join(trace_dir, case)
            got = _step(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "t", "--"] + me + ["--trace", case, "--frames", "60"], 300)
            if got is None:
                ok = False
                break
            print(f"traced ({case})", flush=True)
            meta = json.loads([ln for ln in got.strip().splitlines() if ln.startswith("{")][-1])
            kern = _kernel_stats(d)
            lines.append(f"  ({case}) {CASES[case]}: {meta['frames']} reads, {meta['pending']} bins pending and {meta['tiles']} tiles in all")
            for name in ("k_damage_filter", "k_damage_pack"):
                if name in kern:
                    calls, us, lo, hi = kern[name]
                    line = f"    {name:16s} {calls:4d} launches, {us / max(calls, 1):8.2f} us per launch (min {lo:.2f}, max {hi:.2f})"
                    if name == "k_damage_filter":
                        # per launch: the surface and the mirror are read for every pending bin, the mirror is written for every tile returned
                        moved = (2 * meta["pending"] + meta["tiles"]) * TILE_BYTES
                        line += f"; {moved / max(calls, 1) / 1e6:.1f} MB per launch, {moved / max(us * 1e-6, 1e-12) / 1e12:.2f} TB/s = {100 * moved / max(us * 1e-6, 1e-12) / HBM_PEAK:.0f} % of the 8 TB/s spec"
                    lines.append(line)
    if ok and parent_lib:
        lines += ["", "bench.py --gpus 1 --steps 200 --warmup 20, same box, alternating (parent library / this one), Mpixels/s:"]
        for turn in (1, 2):
            for name, lib in (("parent", parent_lib), ("new", None)):
                env = dict(os.environ)
                if lib:
                    env["FIGDRAW_HIP_LIB"] = os.path.abspath(lib)
                got = _step([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20"], 420, env)
                if got is None:
                    ok = False
                    break
                print(f"bench.py {name}_{turn}", flush=True)
                r = json.loads([ln for ln in got.strip().splitlines() if ln.startswith("{")][-1])
                lines.append(f"  {name}_{turn} {r['value']} ms/step {r['ms_per_step']}")
            if not ok:
                break
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", metavar="OUT")
    ap.add_argument("--parent-lib")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build", "exact_trace"))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--time", choices=list(CASES))
    ap.add_argument("--trace", choices=list(CASES))
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.all, a.parent_lib, a.trace_dir, a.cases.split(",")))
    elif a.time:
        time_case(a.time)
    elif a.trace:
        trace_case(a.trace, a.frames)
    else:
        ap.error("nothing to do")
