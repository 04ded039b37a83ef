#!/usr/bin/env python3
"""What keeping an atlas's content across a repack or a growth costs with fdh_compact_atlas (include_glyphs/figdraw_hip_atlas.h) against what
an application had to do before it existed -- fdh_reset_atlas and every put again --, on an MI355X -> profiles/atlas_move.txt.

  atlas_move_bench.py OUT [--rounds N] [--warmup W] [--parent-lib LIB] [--trace-dir DIR]
  atlas_move_bench.py --step NAME [--rounds N] [--warmup W]        one leg in this process; one JSON line

The workload: the 376 coverage glyph variants (tests/coverage_cases.py variants()), the 106 font fields (tests/msdf_cases.py inputs()) and one
1024 x 1024 image.  Such an image does not fit a 1024 atlas (the packer keeps a margin), so the sizes are one step up from 1024 and 1024 -> 2048:
(a) compaction at the same size, 2048, and (b) growth 2048 -> 4096.  Legs:
  compact / grow            fdh_compact_atlas(2048) of the compacted 2048 atlas; fdh_compact_atlas(4096) of it (put back to 2048 outside the clock)
  alloc 2048 / alloc 4096   fdh_reset_atlas of that size alone: allocating and clearing the new levels and freeing the old ones, as a check on
                            the call's own split (us_pack, us_alloc, us_tables, us_move of FdhAtlasMoveStats: host clock inside the call)
  rebuild, batches / rebuild, singles    fdh_reset_atlas(size) and every put again, the glyphs through the two batch calls or through single calls,
                            with --parent-lib on the parent commit's library (else on this one: the put paths are the parent's)
A measurement is the host clock around the whole call or calls (each ends in a device synchronise), profiler off, one context per leg, a
process per leg, the legs one after the other, N timed rounds after W warm ones; median (p10 .. p90).  With --trace-dir the kernels of the
compact leg come from a rocprofv3 --kernel-trace --stats run of its own.  Every step is a child process under its own time limit and
nothing is started after a failure.  There is no CPU fallback: without a device the context cannot be made and the tool fails."""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = ["compact", "grow", "alloc 2048", "alloc 4096", "rebuild, batches 2048", "rebuild, singles 2048", "rebuild, batches 4096", "rebuild, singles 4096"]


def workload():
    import numpy as np

    import coverage_cases as CC
    import msdf_cases as MC

    rng = np.random.default_rng(1)
    image = rng.integers(0, 256, size=(1024, 1024, 4), dtype=np.uint8)
    glyphs = [(1000 + i, segs, w, h) for i, (_, segs, w, h) in enumerate(CC.variants())]
    fields = [(5000 + i, segs, w, h, R) for i, (_, segs, w, h, R) in enumerate(MC.inputs())]
    return image, glyphs, fields


def put_all(ctx, load, batched):
    image, glyphs, fields = load
    ctx.put_image(1, image)
    if batched:
        ctx.put_glyph_coverage_batch(glyphs)
        ctx.put_glyph_outlines(fields)
    else:
        for key, segs, w, h in glyphs:
            ctx.put_glyph_outline(key, segs, w, h)
        for key, segs, w, h, R in fields:
            ctx.put_glyph_outline(key, segs, w, h, mtsdf=True, sdf_range=R)


def step(name, rounds, warmup):
    from figdraw_amd.context import HipContext

    load = workload()
    n_keys = 1 + len(load[1]) + len(load[2])
    ctx = HipContext(atlas_size=2048, device=0)
    put_all(ctx, load, True)
    assert ctx.atlas_size() == 2048
    us, stats, split = [], None, {"us_pack": [], "us_alloc": [], "us_tables": [], "us_move": []}
    for k in range(warmup + rounds):
        if name in ("compact", "grow"):
            if ctx.atlas_size() != 2048 or k == 0:
                ctx.compact_atlas(2048)
            ctx.sync()
            t1 = time.perf_counter()
            stats = ctx.compact_atlas(2048 if name == "compact" else 4096)
            t2 = time.perf_counter()
            assert ctx.atlas_usage()["entries"] == n_keys and ctx.has_image(1) and ctx.has_image(5000)
            if k >= warmup:
                for part in split:
                    split[part].append(stats[part])
        elif name.startswith("alloc"):
            ctx.sync()
            t1 = time.perf_counter()
            ctx.reset_atlas(int(name.split()[1]))
            t2 = time.perf_counter()
        else:
            size, batched = int(name.split()[-1]), "batches" in name
            ctx.sync()
            t1 = time.perf_counter()
            ctx.reset_atlas(size)
            put_all(ctx, load, batched)
            t2 = time.perf_counter()
            assert ctx.atlas_size() == size and ctx.has_image(1) and ctx.has_image(5000)
        if k >= warmup:
            us.append((t2 - t1) * 1e6)
    ctx.close()
    us.sort()
    print(json.dumps({"step": name, "us": [statistics.median(us), us[len(us) // 10], us[9 * len(us) // 10]], "stats": stats,
                      "split": {part: statistics.median(v) for part, v in split.items() if v}}))


def run_child(name, rounds, warmup, lib, trace_dir=None, limit=300):
    env = dict(os.environ)
    if lib:
        env["FIGDRAW_HIP_LIB"] = os.path.abspath(lib)
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

    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            rows.append((row["Name"], int(row["Calls"]), float(row["TotalDurationNs"]) / 1e3, float(row["AverageNs"]) / 1e3))
    return rows or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--trace-dir")
    args = ap.parse_args()
    if args.step:
        step(args.step, args.rounds, args.warmup)
        return 0
    if not args.out:
        ap.error("nothing to do")
    fmt = lambda v: f"{v[0]:10.1f} ({v[1]:9.1f} .. {v[2]:9.1f})"  # noqa: E731
    lines = [f"tools/atlas_move_bench.py -- fdh_compact_atlas against fdh_reset_atlas and every put again, MI355X (host {platform.node()}).",
             "376 coverage glyph variants, 106 font fields, one 1024 x 1024 image; whole calls = host clock around the call or calls of a row (each ends",
             f"in a device synchronise), profiler off, a process per row, {args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds.",
             "rebuild rows: " + ("the parent commit's library" if args.parent_lib else "this library (its put paths are the parent's)") + ".", ""]
    got, ok = {}, True
    for name in STEPS:
        lib = args.parent_lib if name.startswith("rebuild") else None
        got[name] = run_child(name, args.rounds, args.warmup, lib) if ok else None
        ok = ok and got[name] is not None
        lines.append(f"{name:28s} " + (fmt(got[name]["us"]) if got[name] else "not measured"))
        print(lines[-1], flush=True)
    if ok:
        for leg, size in (("compact", 2048), ("grow", 4096)):
            st = got[leg]["stats"]
            lines += ["", f"{leg}: {st['entries']} entries, {st['rects_moved']} level rectangles, {st['texels']} texels, {st['tiles']} tiles of k_atlas_move, {st['launches']} launches, "
                          f"packed area {st['packed_before']} -> {st['packed_after']}",
                      f"  the call's own host clock (FdhAtlasMoveStats, medians over the timed rounds, us): compaction order and trial packing {got[leg]['split']['us_pack']:.0f}; allocating "
                      f"and clearing the new levels and freeing the old ones {got[leg]['split']['us_alloc']:.0f} (the alloc row, fdh_reset_atlas({size}) alone: {got[f'alloc {size}']['us'][0]:.1f}); "
                      f"building the tables {got[leg]['split']['us_tables']:.0f}; their upload, the launches and the wait for the stream {got[leg]['split']['us_move']:.0f}",
                      f"  against the rebuild through batches: {got[f'rebuild, batches {size}']['us'][0] / got[leg]['us'][0]:.2f} x; through single calls: "
                      f"{got[f'rebuild, singles {size}']['us'][0] / got[leg]['us'][0]:.2f} x"]
    if ok and args.trace_dir:
        rows = run_child("compact", args.rounds, args.warmup, None, trace_dir=args.trace_dir)
        ok = rows is not None
        lines += ["", f"kernels of the compact row, rocprofv3 --kernel-trace --stats, a run of its own ({args.warmup + args.rounds + 1} compactions and the puts that fill the atlas once):",
                  f"  {'kernel':60s} {'calls':>8s} {'total us':>12s} {'mean us':>10s}"]
        for n, calls, total, mean in sorted(rows or [], key=lambda r: -r[2])[:12]:
            lines.append(f"  {n[:60]:60s} {calls:8d} {total:12.1f} {mean:10.2f}")
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-14:]))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
