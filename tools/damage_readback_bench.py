#!/usr/bin/env python3
"""Damage readback (include/figdraw_hip_readback.h): what it costs to have a frame's pixels in a host mirror, three ways.

  A  fdh_read_pixels of the whole frame into the mirror                                         (what the library offered before)
  B  fdh_damage_bins, then one fdh_read_pixels per horizontal run of damaged bins, copied in    (the best those entry points allow)
  C  fdh_read_damage_into                                                                        (this header)

Cases: tools/damage_bench.py's (a) - (d), tracking on, and (s) the S300@4K bench frame with tracking off: every read a full one.

usage:
  damage_readback_bench.py --all OUT.txt [--parent-lib LIB]   every step below as a child process of its own, each under its own time
                                                               limit, nothing started after a failure; writes the report
  damage_readback_bench.py --time CASE                         the three ways alternated in one process, three times each, 200 timed
                                                               frames after 20 warm-up frames per turn; one JSON line
  damage_readback_bench.py --trace CASE [--frames N]           N frames, each followed by fdh_read_damage + fdh_apply_damage (run it under
                                                               rocprofv3 --kernel-trace --memory-copy-trace --stats -f csv); one JSON line
  damage_readback_bench.py --summarize DIR                     the per-launch table from DIR/<case>/ (what --all does after the traces)"""
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

CASES = {"a": "glyph 4K, one row edited", "b": "non-clip cells, one fill toggled", "c": "bench tree 1080p, one root moved",
         "d": "bench tree 1080p animated (every bin)", "s": "S300@4K bench frame, tracking off (every read full)"}
WAYS = ("A", "B", "C")
TILE_BYTES = 16384
PCIE_SPEC = 63e9  # bytes/s, PCIe Gen5 x16 (MI355X_MICROARCH: the link's specification, not a measurement)


def frames_for(case):
    """-> (w, h, tracking, setup(ctx), frame(ctx, i))"""
    if case != "s":
        import damage_bench
        w, h, setup, frame = damage_bench.frames_for(case, 0)
        return w, h, True, setup, frame
    from figdraw_amd.scenes import make_render_tree_100
    w, h = 3840, 2160
    scenes = [make_render_tree_100(float(w), float(h), frame=f, full_frame_blur=True) for f in range(8)]
    return w, h, False, lambda ctx: None, lambda ctx, i: ctx.render_frame(scenes[i % 8], w, h)


def _open(case):
    import numpy as np
    from figdraw_amd.context import HipContext
    w, h, tracking, setup, frame = frames_for(case)
    ctx = HipContext(device=0)
    setup(ctx)
    ctx.set_damage_tracking(tracking)
    ctx.set_damage_readback(True)
    return ctx, np.zeros((h, w, 4), np.uint8), frame


def time_case(case, timed=200, warm=20, turns=3):
    import numpy as np
    ctx, mirror, frame = _open(case)
    L, hnd = ctx.L, ctx.h
    h, w = mirror.shape[:2]
    gx, gy = (w + 63) // 64, (h + 63) // 64
    mask = np.zeros((gy, gx), np.uint8)
    scratch = np.zeros(64 * w * 4, np.uint8)
    n_c = C.c_int()

    def way_a():
        if L.fdh_read_pixels(hnd, 0, 0, w, h, mirror.ctypes.data) != 0:
            raise SystemExit(L.fdh_last_error().decode())
        return gx * gy

    def way_b():
        if L.fdh_damage_bins(hnd, mask.ctypes.data, mask.size, None, None, None) != 0:
            raise SystemExit(L.fdh_last_error().decode())
        n = 0
        for by in np.nonzero(mask.any(axis=1))[0].tolist():
            row = mask[by]
            edges = np.flatnonzero(np.diff(np.concatenate(([0], row, [0]))))  # run starts and ends, alternating
            y0, rh = 64 * by, min(64, h - 64 * by)
            for b0, b1 in zip(edges[0::2].tolist(), edges[1::2].tolist()):
                x0, rw = 64 * b0, min(64 * b1, w) - 64 * b0
                if L.fdh_read_pixels(hnd, x0, y0, rw, rh, scratch.ctypes.data) != 0:
                    raise SystemExit(L.fdh_last_error().decode())
                mirror[y0:y0 + rh, x0:x0 + rw] = scratch[:rh * rw * 4].reshape(rh, rw, 4)
                n += b1 - b0
        return n

    def way_c():
        if L.fdh_read_damage_into(hnd, mirror.ctypes.data, 4 * w, w, h, C.byref(n_c)) != 0:
            raise SystemExit(L.fdh_last_error().decode())
        return n_c.value

    fn = {"A": way_a, "B": way_b, "C": way_c}
    out = {way: {"read_us": [], "total_us": [], "bins": []} for way in WAYS}
    i = 0
    for _ in range(turns):
        for way in WAYS:
            reads, totals, bins = [], [], []
            for k in range(warm + timed):
                t0 = time.perf_counter()
                frame(ctx, i)
                ctx.sync()
                t1 = time.perf_counter()
                n = fn[way]()  # (every way ends in the stream's synchronise and returns with the pixels in `mirror`)
                t2 = time.perf_counter()
                i += 1
                if k >= warm:
                    reads.append((t2 - t1) * 1e6); totals.append((t2 - t0) * 1e6); bins.append(n)
            out[way]["read_us"].append(round(statistics.median(reads), 1))
            out[way]["total_us"].append(round(statistics.median(totals), 1))
            out[way]["bins"].append(round(statistics.mean(bins), 1))
        # after a turn the three mirrors' common image is the frame: C's reads lost nothing while A and B had their turns
        want = ctx.read_pixels()
        L.fdh_read_damage_into(hnd, mirror.ctypes.data, 4 * w, w, h, C.byref(n_c))
        if not np.array_equal(mirror, want):
            raise SystemExit(f"case {case}: the mirror differs from fdh_read_pixels")
    ctx.close()
    print(json.dumps({"case": case, "w": w, "h": h, "grid": gx * gy, "timed": timed, "warm": warm, "ways": out}))


def trace_case(case, frames):
    ctx, mirror, frame = _open(case)
    h, w = mirror.shape[:2]
    tiles, first = 0, 0
    for i in range(frames):
        frame(ctx, i)
        t, px, _ = ctx.read_damage()  # (the tiles themselves: fdh_read_damage_into copies the whole frame when most of the grid is pending)
        ctx.apply_damage(mirror, t, px)
        n = len(t)
        tiles += n
        first = n if i == 0 else first
    ctx.close()
    print(json.dumps({"case": case, "frames": frames, "tiles": tiles, "first_tiles": first}))


def _stats(d, pattern):
    rows = {}
    for path in sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True)):
        for r in csv.DictReader(open(path)):
            name = r["Name"].split("(")[0].replace("void ", "").replace("fdh::", "").split("<")[0]
            calls, total, longest = rows.get(name, (0, 0.0, 0.0))
            rows[name] = (calls + int(r.get("Calls") or 0), total + float(r.get("TotalDurationNs") or 0.0) / 1e3, max(longest, float(r.get("MaxNs") or 0.0) / 1e3))
    return rows


def summarize(d, out=sys.stdout):
    for key in sorted(os.listdir(d)):
        meta_path = os.path.join(d, key + ".json")
        if not os.path.isdir(os.path.join(d, key)) or not os.path.exists(meta_path):
            continue
        meta = json.load(open(meta_path))
        kern, copies = _stats(os.path.join(d, key), "*kernel_stats.csv"), _stats(os.path.join(d, key), "*memory_copy_stats.csv")
        print(f"case ({meta['case']}) {CASES[meta['case']]}: {meta['frames']} frames, {meta['tiles']} tiles in all", file=out)
        for name in ("k_damage_accumulate", "k_damage_pack"):
            if name in kern:
                calls, us, longest = kern[name]
                calls = max(calls, 1)
                line = f"  {name:22s} {calls:5d} launches, {us / calls:9.2f} us per launch"
                if name == "k_damage_pack":
                    nbytes = meta["tiles"] * TILE_BYTES
                    rate = nbytes / max(us * 1e-6, 1e-12)
                    line += f"; {nbytes / calls / 1e6:.3f} MB per launch, {rate / 1e9:.1f} GB/s on its own bytes = {100 * rate / PCIE_SPEC:.0f} % of the link's 63 GB/s spec"
                    rest = meta["tiles"] - meta.get("first_tiles", 0)
                    if 0 < rest < meta["tiles"] and calls > 1 and us > longest > 0:  # the partial reads alone: all but the first, full one (the longest launch)
                        r2 = rest * TILE_BYTES / ((us - longest) * 1e-6)
                        line += (f"\n  {'  all but the longest':22s} {calls - 1:5d} launches, {(us - longest) / (calls - 1):9.2f} us per launch; {rest * TILE_BYTES / (calls - 1) / 1e6:.3f} MB per launch, "
                                 f"{r2 / 1e9:.1f} GB/s = {100 * r2 / PCIE_SPEC:.0f} % of spec; the longest (the first read, {meta['first_tiles']} tiles) {longest:.1f} us")
                print(line, file=out)
        for name, (calls, us, _) in sorted(copies.items()):
            print(f"  copy {name:17s} {calls:5d} commands, {us / max(calls, 1):9.2f} us per command", file=out)
        others = ", ".join(f"{k} {v[1] / meta['frames']:.1f}" for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1]) if not k.startswith("k_damage_pack") and k != "k_damage_accumulate")
        print(f"  other kernels, us per frame: {others}", file=out)


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


def run_all(out_path, parent_lib, trace_dir):
    me = [sys.executable, os.path.abspath(__file__)]
    lines = ["tools/damage_readback_bench.py -- a frame's pixels in a host mirror, MI355X.  Host clock, profiler off; per case the three ways",
             "alternated in one process (A, B, C, three turns), 200 timed frames after 20 warm-up frames per turn; medians per turn, us.",
             "read = from the frame's fdh_sync to the pixels being in the mirror; total = the same plus recording, submitting and rendering the",
             "frame (Python's marshalling of the scene included: it is most of the total for (a) and (b)).",
             "  A fdh_read_pixels of the whole frame   B fdh_damage_bins + one fdh_read_pixels per run of damaged bins   C fdh_read_damage_into", ""]
    ok = True
    for case in CASES:
        got = _step(me + ["--time", case], 420)
        if got is None:
            ok = False
            break
        print(f"timed case ({case})", flush=True)
        r = json.loads(got.strip().splitlines()[-1])
        lines.append(f"({case}) {CASES[case]}: {r['w']} x {r['h']}, {r['grid']} bins")
        for way in WAYS:
            v = r["ways"][way]
            rd, tt = sorted(v["read_us"]), sorted(v["total_us"])
            lines.append(f"    {way}  read {rd[1]:9.1f} (turns {rd[0]:.1f} .. {rd[2]:.1f})   total {tt[1]:10.1f} (turns {tt[0]:.1f} .. {tt[2]:.1f})   bins fetched per frame {v['bins'][1]:.1f}")
    if ok:
        os.makedirs(trace_dir, exist_ok=True)
        for case in ("a", "s"):
            got = _step(["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "-f", "csv", "-d", os.path.join(trace_dir, case), "-o", "t", "--"] + me + ["--trace", case, "--frames", "60"], 300)
            if got is None:
                ok = False
                break
            print(f"traced ({case})", flush=True)
            meta = [ln for ln in got.strip().splitlines() if ln.startswith("{")][-1]
            open(os.path.join(trace_dir, case + ".json"), "w").write(meta)
    if ok:
        lines += ["", "rocprofv3 --kernel-trace --memory-copy-trace --stats, a run per case, 60 frames each read with fdh_read_damage + fdh_apply_damage",
                  "(the first read of a run is a full one and is in the totals):"]
        import io
        buf = io.StringIO()
        summarize(trace_dir, buf)
        lines += buf.getvalue().rstrip().splitlines()
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
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build", "readback_trace"))
    ap.add_argument("--time", choices=list(CASES))
    ap.add_argument("--trace", choices=list(CASES))
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.all, a.parent_lib, a.trace_dir))
    elif a.summarize:
        summarize(a.summarize)
    elif a.time:
        time_case(a.time)
    elif a.trace:
        trace_case(a.trace, a.frames)
    else:
        ap.error("nothing to do")
