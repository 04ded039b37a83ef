#!/usr/bin/env python3
"""Coded damage readback (include/figdraw_hip_stream.h): what it costs to have the pending bins on the host, two ways.

  A  fdh_read_damage         raw tiles, 16384 bytes per bin        (k_damage_pack)
  B  fdh_read_damage_coded   directory + coded payloads            (k_damage_encode)

Cases: tools/damage_readback_bench.py's -- tools/damage_bench.py's (a) - (d), tracking on, and (s) the S300@4K bench frame with tracking
off: every read a full one.

usage:
  damage_stream_bench.py --all OUT.txt [--parent-lib LIB]   every step below as a child process of its own, each under its own time limit,
                                                             nothing started after a failure; writes the report
  damage_stream_bench.py --time CASE                         the two ways alternated in one process, three turns, 200 timed frames after 20
                                                             warm-up frames per turn; one JSON line
  damage_stream_bench.py --trace CASE [--frames N]           N frames, each followed by one read of each kind in turn (run it under
                                                             rocprofv3 --kernel-trace --stats -f csv); one JSON line
  damage_stream_bench.py --summarize DIR                     the per-launch table from DIR/<case>/ (what --all does after the traces)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from damage_readback_bench import CASES, _open, _stats, _step  # noqa: E402

WAYS = ("A", "B")
TILE_BYTES, ENTRY_BYTES = 16384, 24
MODES = ("SOLID", "PAL", "RUNS", "RAW")


def time_case(case, timed=200, warm=20, turns=3):
    import numpy as np
    ctx, mirror, frame = _open(case)
    L, hnd = ctx.L, ctx.h
    h, w = mirror.shape[:2]
    t_p, p_p = C.c_void_p(), C.c_void_p()
    n_c, bytes_c = C.c_int(), C.c_int64()
    hist = np.zeros(4, np.int64)

    def way_a():
        if L.fdh_read_damage(hnd, C.byref(t_p), C.byref(p_p), C.byref(n_c), None, None, None) != 0:
            raise SystemExit(L.fdh_last_error().decode())
        return n_c.value, n_c.value * (TILE_BYTES + 16)

    def way_b():
        if L.fdh_read_damage_coded(hnd, C.byref(t_p), C.byref(p_p), C.byref(n_c), C.byref(bytes_c), None, None, None) != 0:
            raise SystemExit(L.fdh_last_error().decode())
        return n_c.value, n_c.value * ENTRY_BYTES + bytes_c.value

    fn = {"A": way_a, "B": way_b}
    out = {way: {"read_us": [], "bins": [], "bytes": []} for way in WAYS}
    i = 0
    for _ in range(turns):
        for way in WAYS:
            reads, bins, nbytes = [], [], []
            for k in range(warm + timed):
                frame(ctx, i)
                ctx.sync()
                t1 = time.perf_counter()
                n, b = fn[way]()  # (both end in the stream's synchronise and return with the bytes in host memory)
                t2 = time.perf_counter()
                i += 1
                if k >= warm:
                    reads.append((t2 - t1) * 1e6); bins.append(n); nbytes.append(b)
                    if way == "B" and n:  # (outside the timed span)
                        d = np.frombuffer(C.string_at(t_p.value, n * ENTRY_BYTES), ctx.CODED_TILE)
                        hist += np.bincount(d["mode"], minlength=4)
            out[way]["read_us"].append(round(statistics.median(reads), 1))
            out[way]["bins"].append(round(statistics.mean(bins), 1))
            out[way]["bytes"].append(round(statistics.mean(nbytes), 1))
        # after a turn: a mirror that takes one coded read of everything is the frame
        want = ctx.read_pixels()
        ctx.set_damage_readback(False); ctx.set_damage_readback(True)
        tiles, payload, full = ctx.read_damage_coded()
        ctx.decode_damage(mirror, tiles, payload)
        if not full or not np.array_equal(mirror, want):
            raise SystemExit(f"case {case}: the decoded mirror differs from fdh_read_pixels")
    ctx.close()
    print(json.dumps({"case": case, "w": w, "h": h, "grid": ((w + 63) // 64) * ((h + 63) // 64), "timed": timed, "warm": warm, "ways": out,
                      "modes": hist.tolist()}))


def trace_case(case, frames):
    ctx, mirror, frame = _open(case)
    tiles = {"A": 0, "B": 0}
    coded = 0
    for i in range(frames):
        frame(ctx, i)
        if i % 2 == 0:
            t, px, _ = ctx.read_damage()
            tiles["A"] += len(t)
        else:
            t, payload, _ = ctx.read_damage_coded()
            tiles["B"] += len(t)
            coded += len(payload) + ENTRY_BYTES * len(t)
    ctx.close()
    print(json.dumps({"case": case, "frames": frames, "tiles": tiles, "coded_bytes": coded}))


def summarize(d, out=sys.stdout):
    for key in sorted(os.listdir(d)):
        meta_path = os.path.join(d, key + ".json")
        if not os.path.isdir(os.path.join(d, key)) or not os.path.exists(meta_path):
            continue
        meta = json.load(open(meta_path))
        kern = _stats(os.path.join(d, key), "*kernel_stats.csv")
        print(f"case ({meta['case']}) {CASES[meta['case']]}: {meta['frames']} frames, reads alternating A / B; tiles {meta['tiles']}, coded bytes {meta['coded_bytes']}", file=out)
        for name in ("k_damage_pack", "k_damage_encode", "k_damage_accumulate"):
            if name in kern:
                calls, us, longest = kern[name]
                line = f"  {name:22s} {calls:5d} launches, {us / max(calls, 1):9.2f} us per launch, the longest {longest:.1f} us"
                if calls > 1 and us > longest > 0:
                    line += f"; all but the longest {(us - longest) / (calls - 1):.2f} us per launch"
                print(line, file=out)
        others = ", ".join(f"{k} {v[1] / meta['frames']:.1f}" for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1]) if not k.startswith("k_damage_"))
        print(f"  other kernels, us per frame: {others}", file=out)


def run_all(out_path, parent_lib, trace_dir):
    me = [sys.executable, os.path.abspath(__file__)]
    lines = ["tools/damage_stream_bench.py -- the pending bins on the host, raw and coded, MI355X.  Host clock, profiler off; per case the two ways",
             "alternated in one process (A, B, three turns), 200 timed frames after 20 warm-up frames per turn; medians per turn, us.",
             "read = from the frame's fdh_sync to the call's return, the bytes being in (page-locked) host memory.",
             "bytes = what reached the host per read: A 16384 + 16 per tile, B 24 per tile + payload_bytes.",
             "  A fdh_read_damage (k_damage_pack)   B fdh_read_damage_coded (k_damage_encode)", "",
             "Hypotheses, stated before the numbers:",
             "  1. B's bytes are the reference encoder's on the same frames (held by tests/test_damage_stream.py, byte for byte); the ratios per case",
             "     are recorded here.",
             "  2. For a partial read -- case (a), 56 bins -- B's read time is within A's: A in the same process, the margin the spread of A's own",
             "     three turns.",
             "  3. For content that does not code -- case (s), the blurred bench frame -- B costs no more than A plus the directory: the link moves",
             "     the same bytes.", ""]
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
            rd = sorted(v["read_us"])
            lines.append(f"    {way}  read {rd[1]:9.1f} (turns {rd[0]:.1f} .. {rd[2]:.1f})   bins per read {v['bins'][1]:.1f}   bytes per read {v['bytes'][1]:.0f}")
        a, b = r["ways"]["A"], r["ways"]["B"]
        total = max(sum(r["modes"]), 1)
        lines.append(f"    bytes A / B = {a['bytes'][1] / max(b['bytes'][1], 1):.1f} x;  B's tiles " + ", ".join(f"{m} {100 * c / total:.1f} %" for m, c in zip(MODES, r["modes"])))
    if ok:
        os.makedirs(trace_dir, exist_ok=True)
        for case in ("a", "s"):
            got = _step(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", os.path.join(trace_dir, case), "-o", "t", "--"] + me + ["--trace", case, "--frames", "60"], 300)
            if got is None:
                ok = False
                break
            print(f"traced ({case})", flush=True)
            meta = [ln for ln in got.strip().splitlines() if ln.startswith("{")][-1]
            open(os.path.join(trace_dir, case + ".json"), "w").write(meta)
    if ok:
        lines += ["", "rocprofv3 --kernel-trace --stats (no counters), a run per case, 60 frames, the reads alternating A / B (30 each; each kind's first",
                  "read of (a) is a large one: frame 0 is full, frame 1's read holds what two frames changed):"]
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
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build", "stream_trace"))
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
