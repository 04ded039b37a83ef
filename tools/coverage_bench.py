#!/usr/bin/env python3
"""What filling an atlas with coverage glyphs costs as ONE fdh_put_glyph_coverage_batch (include_glyphs/figdraw_hip_coverage.h) against the same glyphs as
single fdh_put_glyph_outline calls, on an MI355X -> profiles/coverage_batch.txt.

  coverage_bench.py OUT [--rounds N] [--warmup W]

Four lines: the 94 ASCII outlines of the font fixture and the 376 of four sub-pixel variants (x shifted by 0, 0.25, 0.5, 0.75), each without
and with the LCD filter.  A measurement is the host clock around the whole set -- the batch call, or the loop of single calls; both end in a
device synchronise -- on one context in one process, the two alternating, N timed rounds after W (the atlas is reset before every set,
outside the clock).  The single path is what it was before the batch existed.  Before anything is timed, level 0 of a batch-filled atlas
is compared with a singles-filled one at every measured size: faster and different is not faster.  There is no CPU fallback: without a
device the context cannot be made and the tool fails.

  coverage_bench.py --cubic OUT --parent-lib LIB [--passes N]
  coverage_bench.py --time-cubic {batch,singles} [--lcd] | --trace-cubic [--lcd] [--calls N]       one step of --cubic; one JSON line

The cubic leg (include_glyphs/figdraw_hip_cubic_batch.h): the 106 skewed font outlines (tests/msdf_cubic_cases.py skewed()) as ONE
fdh_put_glyph_coverage_batch_cubic of this library against 106 fdh_put_glyph_outline_cubic coverage calls of the parent commit's library
(LIB), plain and LCD-filtered, by the protocol of profiles/msdf.txt section 6: host clock around the set, the legs alternating, each a
process of its own, 200 timed after 20, N passes (default 2); the batch's kernels from a rocprofv3 --kernel-trace --stats run of its
own.  Every step is a child process under its own time limit and nothing is started after a failure."""
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

NEW_KERNELS = ("k_coverage_cells_batch", "k_coverage_sum_batch", "k_lcd_filter_batch")


def sets():
    import coverage_cases as CC

    return {"font, 94 glyphs": CC.font(), "four variants, 376 glyphs": CC.variants()}


def put(ctx, glyphs, lcd, batched):
    if batched:
        ctx.put_glyph_coverage_batch([(1 + i, segs, w, h) for i, (_, segs, w, h) in enumerate(glyphs)], lcd_filter=lcd)
    else:
        for i, (_, segs, w, h) in enumerate(glyphs):
            ctx.put_glyph_outline(1 + i, segs, w, h, lcd_filter=lcd)


def measure(glyphs, lcd, rounds, warmup):
    """-> ({batched: [us]}, the batch's stats, level 0 equal)"""
    import numpy as np
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=2048, device=0)
    level0 = {}
    for batched in (True, False):
        ctx.reset_atlas()
        put(ctx, glyphs, lcd, batched)
        level0[batched] = ctx.debug_read_surface(4)
    equal = bool(np.array_equal(level0[True], level0[False]) and level0[True].any())
    us = {True: [], False: []}
    for k in range(warmup + rounds):
        for batched in (True, False):
            ctx.reset_atlas()
            ctx.sync()
            t1 = time.perf_counter()
            put(ctx, glyphs, lcd, batched)
            t2 = time.perf_counter()
            if k >= warmup:
                us[batched].append((t2 - t1) * 1e6)
    ctx.reset_atlas()
    put(ctx, glyphs, lcd, True)
    stats = ctx.glyph_coverage_batch_stats()
    assert ctx.atlas_size() == 2048
    ctx.close()
    return us, stats, equal


def cubic_puts():
    import msdf_cubic_cases

    return [(segs, w, h) for _, segs, w, h, _ in msdf_cubic_cases.skewed()]


def put_cubic(ctx, puts, first_key, lcd, batched):
    if batched:
        ctx.put_glyph_coverage_batch_cubic([(first_key + i, segs, w, h) for i, (segs, w, h) in enumerate(puts)], lcd_filter=lcd)
    else:
        for i, (segs, w, h) in enumerate(puts):
            ctx.put_glyph_outline_cubic(first_key + i, segs, w, h, lcd_filter=lcd)


def time_cubic(leg, lcd, timed=200, warm=20, trace=False):
    """one leg in this process: the host clock around the 106 glyphs, the 4096 atlas reset before every set outside the clock; one JSON line"""
    from figdraw_amd.context import HipContext

    puts = cubic_puts()
    ctx = HipContext(atlas_size=4096, device=0)
    us = []
    for k in range(warm + timed):
        ctx.reset_atlas()
        ctx.sync()
        t1 = time.perf_counter()
        put_cubic(ctx, puts, 1, lcd, leg == "batch")
        t2 = time.perf_counter()
        if k >= warm:
            us.append((t2 - t1) * 1e6)
    stats = ctx.glyph_coverage_batch_stats() if leg == "batch" else None
    ctx.close()
    out = {"leg": leg, "lcd": lcd, "calls": timed, "batch_stats": stats}
    if not trace:
        out.update(median_us=statistics.median(us), p10_us=sorted(us)[len(us) // 10], p90_us=sorted(us)[9 * len(us) // 10])
    print(json.dumps(out))


CUBIC_HEAD = """tools/coverage_bench.py --cubic -- the 106 skewed font outlines (tests/msdf_cubic_cases.py skewed(): 2 335 segments of 8 floats, 1 782 cubics) as
coverage glyphs: ONE fdh_put_glyph_coverage_batch_cubic of this library against 106 fdh_put_glyph_outline_cubic calls of the parent commit's
library, MI355X, 4096 atlas reset before every set outside the clock.  Host clock around the set, profiler off, 200 timed after 20 per leg;
the legs alternate, each a process of its own, two passes; kernels from a rocprofv3 --kernel-trace --stats run of its own, 60 batches.

Hypotheses, stated before the numbers (nothing about the cubic path had been timed when they were written):
  1. the launches are fdh_put_glyph_coverage_batch's and the lines are of the same order as the quadratic font's (a cubic flattens into
     ceil(sqrt(30 dev)) chords where a quadratic takes ceil(sqrt(10 dev))): the batch costs about what the 94-glyph batch above costs per
     glyph, 0.35 to 0.5 ms, the extra being the host's flattening of 1 782 cubics.
  2. the 106 single calls cost what single coverage puts cost, 5 to 6 ms: the idle device between puts is the same.
  3. the LCD filter is one more launch on the batch's side and 106 more on the singles' side.
"""


def run_cubic(out_path, parent_lib, trace_dir, passes):
    from damage_readback_bench import _stats, _step

    me = [sys.executable, os.path.abspath(__file__)]
    parent_env = dict(os.environ, FIGDRAW_HIP_LIB=os.path.abspath(parent_lib))
    lines = CUBIC_HEAD.splitlines() + [""]
    ok = True
    for lcd in (False, True):
        flag = ["--lcd"] if lcd else []
        med = {"batch": [], "singles": []}
        stats = None
        for _ in range(passes):
            for leg, env in (("batch", None), ("singles", parent_env)):
                got = _step(me + ["--time-cubic", leg] + flag, 300, env) if ok else None
                if got is None:
                    ok = False
                    break
                r = json.loads([ln for ln in got.strip().splitlines() if ln.startswith("{")][-1])
                med[leg].append((r["median_us"], r["p10_us"], r["p90_us"]))
                stats = r.get("batch_stats") or stats
        if not ok:
            break
        d = os.path.join(trace_dir, "cubic_coverage" + ("_lcd" if lcd else ""))
        if _step(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "t", "--"] + me + ["--trace-cubic", "--calls", "60"] + flag, 300) is None:
            ok = False
            break
        kern = _stats(d, "*kernel_stats.csv")
        b, s1 = [m[0] for m in med["batch"]], [m[0] for m in med["singles"]]
        spread = max(max(b) - min(b), max(s1) - min(s1))
        lines.append(f"{'LCD-filtered' if lcd else 'plain'}: batch, median us per pass {', '.join(f'{m[0]:.1f} (p10 {m[1]:.1f}, p90 {m[2]:.1f})' for m in med['batch'])}; "
                     f"106 single calls of the parent, {', '.join(f'{m[0]:.1f} (p10 {m[1]:.1f}, p90 {m[2]:.1f})' for m in med['singles'])}")
        lines.append(f"    ratio of the means of the passes' medians {sum(s1) / sum(b):.1f} x; singles - batch {sum(s1) / len(s1) - sum(b) / len(b):.1f} us, "
                     f"the larger spread between a leg's own passes {spread:.1f} us: {'the batch wins by more than the spread' if min(s1) - max(b) > spread else 'NOT beyond the spread'}")
        lines.append(f"    the batch: {stats}")
        lines.append("    kernels, us per launch (launches per batch): " + ", ".join(f"{k} {v[1] / max(v[0], 1):.2f} ({v[0] / 60:.0f}), the longest {v[2]:.1f}"
                                                                                   for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1])))
        print("\n".join(lines[-4:]), flush=True)
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--cubic", metavar="OUT", help="the skewed font set as one cubic coverage batch against single cubic calls of --parent-lib")
    ap.add_argument("--parent-lib")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--time-cubic", choices=["batch", "singles"])
    ap.add_argument("--trace-cubic", action="store_true")
    ap.add_argument("--lcd", action="store_true")
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build", "coverage_trace"))
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.time_cubic:
        time_cubic(args.time_cubic, args.lcd)
        return 0
    if args.trace_cubic:
        time_cubic("batch", args.lcd, timed=args.calls, warm=0, trace=True)
        return 0
    if args.cubic:
        if not args.parent_lib:
            ap.error("--cubic needs --parent-lib")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        return run_cubic(args.cubic, args.parent_lib, args.trace_dir, max(args.passes, 2))
    if not args.out:
        ap.error("nothing to do")
    q = lambda v, f: sorted(v)[int(f * (len(v) - 1))]  # noqa: E731
    lines = [f"tools/coverage_bench.py -- coverage glyphs as one fdh_put_glyph_coverage_batch against single fdh_put_glyph_outline calls, MI355X.",
             f"whole set = host clock around the batch call / around the loop of single calls (each ends in a device synchronise), profiler off, one context",
             f"(atlas 2048, reset before every set outside the clock), batch and singles alternating, {args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds.",
             "level 0 = the atlas after the batch against the atlas after the single calls, compared before the timing.", ""]
    lines.append(f"{'set':28s} {'LCD':4s} {'singles us':>30s} {'batch us':>30s} {'singles / batch':>16s}  {'launches':>8s} {'tiles':>6s} {'lines':>6s} {'bytes copied':>12s}  level 0")
    ok = True
    for name, glyphs in sets().items():
        for lcd in (False, True):
            us, st, equal = measure(glyphs, lcd, args.rounds, args.warmup)
            ok = ok and equal
            fmt = lambda v: f"{statistics.median(v):9.1f} ({q(v, 0.1):8.1f} .. {q(v, 0.9):8.1f})"  # noqa: E731
            lines.append(f"{name:28s} {'yes' if lcd else 'no':4s} {fmt(us[False]):>30s} {fmt(us[True]):>30s} {statistics.median(us[False]) / statistics.median(us[True]):15.1f}x"
                         f"  {st['launches']:8d} {st['tiles']:6d} {st['edges']:6d} {st['bytes_copied']:12d}  {'equal' if equal else 'DIFFERENT'}")
            print(lines[-1], flush=True)
    lines += ["", "single calls per set: one copy, k_rasterize_lines, k_lcd_filter with the filter, a blit and a minify per level of the glyph's chain, and a",
              "synchronise, per glyph.  The batch: two copies, the launches above, one synchronise.", "",
              "registers of the new kernels (tools/kernel_regs.py):"]
    regs = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py")], capture_output=True, text=True).stdout
    lines += [ln for ln in regs.splitlines() if any(k in ln for k in NEW_KERNELS)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
