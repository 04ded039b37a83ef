#!/usr/bin/env python3
"""What filling an atlas with coverage glyphs costs as ONE fdh_put_glyph_coverage_batch (include_glyphs/figdraw_hip_coverage.h) against the same glyphs as
single fdh_put_glyph_outline calls, on an MI355X -> profiles/coverage_batch.txt.

  coverage_bench.py OUT [--rounds N] [--warmup W]

Four lines: the 94 ASCII outlines of the font fixture and the 376 of four sub-pixel variants (x shifted by 0, 0.25, 0.5, 0.75), each without
and with the LCD filter.  A measurement is the host clock around the whole set -- the batch call, or the loop of single calls; both end in a
device synchronise -- on one context in one process, the two alternating, N timed rounds after W (the atlas is reset before every set,
outside the clock).  The single path is what it was before the batch existed.  Before anything is timed, level 0 of a batch-filled atlas
is compared with a singles-filled one at every measured size: faster and different is not faster.  There is no CPU fallback: without a
device the context cannot be made and the tool fails."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
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
