#!/usr/bin/env python3
"""What a distance-field put costs (fdh_put_glyph_outline with FDH_GLYPH_MTSDF, k_msdf_generate, with FDH_GLYPH_MTSDF_CORRECT
k_msdf_correct, and with FDH_GLYPH_MTSDF_OVERLAP k_msdf_generate_union), on an MI355X -> profiles/msdf.txt.

  msdf_bench.py --all OUT [--nocull-lib LIB] [--parent-lib LIB] [--passes N]
                                               every step as a child process under its own time limit, in turn, nothing started after a
                                               failure; writes the report: per case the call without and with the correction pass, with
                                               the overlap flag, then the other libraries without either, N times over in that order
                                               (libraries alternate).
                                               --nocull-lib: the library built with -DFDH_MSDF_NO_CULL=1
                                               (make -C figdraw_amd/csrc variant NAME=msdf_nocull DEFS=-DFDH_MSDF_NO_CULL=1);
                                               --parent-lib: the parent commit's library, for "the flag-off call is unchanged"
  msdf_bench.py --batch OUT --parent-lib LIB [--passes N]
                                               the font set as ONE fdh_put_glyph_outlines (include_glyphs/figdraw_hip_glyphs.h) against 106 single puts
                                               of the parent commit's library, per flag combination, alternating, N passes each (default 2);
                                               then the batch's kernels from a rocprofv3 run of its own; writes section 6's table
  msdf_bench.py --cubic-batch OUT --parent-lib LIB [--passes N]
                                               the 106 skewed font outlines (tests/msdf_cubic_cases.py skewed()) as ONE fdh_put_glyph_outlines_cubic
                                               (include_glyphs/figdraw_hip_cubic_batch.h) against 106 fdh_put_glyph_outline_cubic calls of the parent
                                               commit's library, plain and with the correction, --batch's protocol; writes section 8's table
  msdf_bench.py --cubic OUT [--passes N]      the font set with every quadratic skewed into a cubic (tests/msdf_cubic_cases.py), three ways: native
                                               through fdh_put_glyph_outline_cubic; (a) each cubic cut into four quadratics; (b) each cubic
                                               flattened to lines at 0.025 px, both through fdh_put_glyph_outline.  Per leg the host clock around
                                               the set, the generator's device time from a rocprofv3 run of its own, and the largest texel
                                               difference from the float64 cubic reference; writes section 7's table
  msdf_bench.py --time-cubic LEG | --trace-cubic LEG | --error-cubic LEG     one step of --cubic (LEG: native, quadratics, lines); one JSON line
  msdf_bench.py --time CASE [--correct] [--overlap] [--batched]    the whole call on the host clock, profiler off: 200 timed calls after 20; one JSON line
  msdf_bench.py --trace CASE [--correct] [--overlap] [--batched] [--calls N]   N calls (run it under rocprofv3 --kernel-trace --stats -f csv); one JSON line
                                               --batched: a call is one fdh_put_glyph_outlines of the case's puts

Cases: small = one glyph outline ('g' of the fixture, scaled to a 32 x 32 field, range 4); large = six glyph outlines scaled and laid side by
side in a 256 x 256 field (about 200 segments); font = the 106 inputs of tests/msdf_cases.py, one put each (a "call" is all 106); many =
16 383 copies of one square, as many contours, in a 16 x 16 field (40 timed calls after 5); cubicfont (--time / --trace only) = the 106 skewed
font outlines, segments of 8 floats, one fdh_put_glyph_outline_cubic each or with --batched one fdh_put_glyph_outlines_cubic."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from damage_readback_bench import _stats, _step  # noqa: E402

CASES = {"small": "32 x 32, one glyph", "large": "256 x 256, six glyphs side by side", "font": "the 106 font inputs, one put each",
         "many": "16 x 16, 16383 squares"}
TIMED_CASES = dict(CASES, cubicfont="the 106 skewed font outlines (cubic segments), one put each")  # --time / --trace; --all runs CASES
ROUNDS = {"many": (40, 5)}  # (timed, warm-up) where 200 after 20 would take too long


def outlines(case):
    """-> [(segs float32 (n, 6), w, h, range)]: the puts of one call"""
    import numpy as np

    if case == "font":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import msdf_cases

        return [(segs, w, h, R) for _, segs, w, h, R in msdf_cases.inputs()]
    if case == "cubicfont":  # segments of 8 floats: put_all takes the cubic calls
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import msdf_cubic_cases

        return [(segs, w, h, R) for _, segs, w, h, R in msdf_cubic_cases.skewed()]
    if case == "many":
        a, b, c, d = (2.0, 2.0), (10.0, 2.0), (10.0, 9.0), (2.0, 9.0)
        nan = float("nan")
        square = np.array([[p[0], p[1], nan, nan, q[0], q[1]] for p, q in ((a, b), (b, c), (c, d), (d, a))], np.float32)
        return [(np.tile(square, (16383, 1)), 16, 16, 4)]
    return [outline(case) + (4,)]


def outline(case):
    """-> (segs float32 (n, 6), w, h)"""
    import numpy as np

    z = np.load(os.path.join(ROOT, "tests", "golden", "outlines_ubuntu20.npz"))
    if case == "small":
        segs, (w, h) = z["segs_103"].astype(np.float32), z["size_103"]
        s = np.float32(24.0 / max(int(w), int(h)))
        return segs * s + np.float32(4), 32, 32
    parts = []
    for i, code in enumerate((66, 82, 103, 109, 56, 38)):  # 3 columns x 2 rows of 85 x 128 cells
        segs, (w, h) = z[f"segs_{code}"].astype(np.float32), z[f"size_{code}"]
        s = np.float32(76.0 / max(int(w), int(h)))
        part = segs * s
        part[:, 0::2] += np.float32(6 + 85 * (i % 3))
        part[:, 1::2] += np.float32(20 + 128 * (i // 3))
        parts.append(part)
    return np.concatenate(parts).astype(np.float32), 256, 256


CORRECT = {False: {}, True: {"correct": True}}  # (a library from before the flag is driven without the keyword's bit)
OVERLAP = {False: {}, True: {"overlap": True}}


def _context():
    from figdraw_amd.context import HipContext

    return HipContext(atlas_size=4096, device=0)


def put_all(ctx, puts, first_key, correct, overlap, batched):
    if puts[0][0].shape[1] == 8:  # cubic outlines (no overlap flag there)
        if batched:
            ctx.put_glyph_outlines_cubic([(first_key + i, segs, w, h, R) for i, (segs, w, h, R) in enumerate(puts)], correct=correct)
            return
        for i, (segs, w, h, R) in enumerate(puts):
            ctx.put_glyph_outline_cubic(first_key + i, segs, w, h, mtsdf=True, sdf_range=R, **CORRECT[correct])
        return
    if batched:
        ctx.put_glyph_outlines([(first_key + i, segs, w, h, R) for i, (segs, w, h, R) in enumerate(puts)], correct=correct, overlap=overlap)
        return
    for i, (segs, w, h, R) in enumerate(puts):
        ctx.put_glyph_outline(first_key + i, segs, w, h, mtsdf=True, sdf_range=R, **CORRECT[correct], **OVERLAP[overlap])


def time_case(case, correct=False, overlap=False, batched=False):
    puts = outlines(case)
    timed, warm = ROUNDS.get(case, (200, 20))
    ctx = _context()
    us = []
    for k in range(warm + timed):
        if k % (100 // len(puts) or 1) == 0:
            ctx.reset_atlas()  # (the packer's search grows with what is packed; every call packs a new rectangle)
        t1 = time.perf_counter()
        put_all(ctx, puts, 1 + k * len(puts), correct, overlap, batched)
        t2 = time.perf_counter()
        if k >= warm:
            us.append((t2 - t1) * 1e6)
    stats = ctx.glyph_batch_stats() if batched else None
    ctx.close()
    print(json.dumps({"case": case, "correct": correct, "overlap": overlap, "batched": batched, "batch_stats": stats, "segments": sum(len(p[0]) for p in puts), "calls": timed, "median_us": statistics.median(us),
                      "p10_us": sorted(us)[len(us) // 10], "p90_us": sorted(us)[9 * len(us) // 10]}))


def trace_case(case, calls, correct=False, overlap=False, batched=False):
    puts = outlines(case)
    ctx = _context()
    for k in range(calls):
        if k % (100 // len(puts) or 1) == 0:
            ctx.reset_atlas()
        put_all(ctx, puts, 1 + k * len(puts), correct, overlap, batched)
    ctx.close()
    print(json.dumps({"case": case, "correct": correct, "overlap": overlap, "batched": batched, "segments": sum(len(p[0]) for p in puts), "calls": calls}))


HEAD = """tools/msdf_bench.py -- a distance-field put (fdh_put_glyph_outline with FDH_GLYPH_MTSDF), MI355X.
whole call = host clock around the call, profiler off, 200 timed calls after 20 (it packs, builds the edge records, copies them, launches
k_msdf_generate, with FDH_GLYPH_MTSDF_CORRECT k_msdf_correct, and the level chain's blits and minifies, and synchronises); kernel =
k_msdf_generate and k_msdf_correct alone from a rocprofv3 --kernel-trace --stats run of its own, 60 calls.  this / corrected: the product
library without / with FDH_GLYPH_MTSDF_CORRECT; overlap: the product library with FDH_GLYPH_MTSDF_OVERLAP (k_msdf_generate_union in
k_msdf_generate's place); no cull: the -DFDH_MSDF_NO_CULL=1 build; parent: the parent commit's library.  font: a call is 106 puts, a
launch one of them; many: 40 timed calls after 5, 12 traced.

Hypotheses, stated before the numbers (nothing had been timed when they were written):
  1. small (32 x 32, one glyph): the whole call is launch plus synchronise latency -- the kernel is a few microseconds of a call of
     many tens, and culling changes nothing that can be seen in the call.
  2. large (256 x 256, about 200 segments): the kernel is VALU-bound on the cubic solve (1024 waves x 200 edges x ~300 VALU
     instructions per quadratic without culling); culling removes most edges per 8 x 8 tile and the kernel's time with it.
  3. the flag-off call is what the parent commit's was: same launches, and k_msdf_generate's arithmetic is the parent's instruction for
     instruction (its per-edge body moved into an inline function; 53 VGPRs before and after).
  4. the corrected call costs one more launch: on small that is launch latency plus one wave's walk over the 34 edges for each round of
     the few tiles that hold a candidate (no culling there), a fraction of the generator's 50 us; on large, where most of the 1024 tiles
     leave after phase 1, it is the phase-2 rounds of the few tiles with candidates, each walking all 254 edges: a latency chain of one
     wave, tens of microseconds, beside the generator's 190.
  5. the union generator does k_msdf_generate's work per edge and adds one tail and one ranking per contour: on the font set, 1 to 3
     contours a glyph, a few per cent of the kernel and nothing that shows in the call; on many (16 383 contours of 4 edges) the tail
     is a quarter of the work and the cull's bound is taken per contour: the kernel may cost up to twice the plain one.
"""


def run_all(out_path, nocull_lib, trace_dir, parent_lib=None, passes=1, cases=tuple(CASES)):
    me = [sys.executable, os.path.abspath(__file__)]
    lines = HEAD.splitlines() + [""]
    libs = [("this", None, False, False), ("corrected", None, True, False), ("overlap", None, False, True)]
    libs += [("no cull", os.path.abspath(nocull_lib), False, False)] if nocull_lib else []
    libs += [("parent", os.path.abspath(parent_lib), False, False)] if parent_lib else []
    ok = True
    for case in cases:
        for turn, (tag, lib, correct, overlap) in enumerate(libs * passes):
            env = dict(os.environ)
            if lib:
                env["FIGDRAW_HIP_LIB"] = lib
            flag = (["--correct"] if correct else []) + (["--overlap"] if overlap else [])
            n_calls = 12 if case == "many" else 60
            got = _step(me + ["--time", case] + flag, 300, env)
            if got is None:
                ok = False
                break
            r = json.loads([ln for ln in got.strip().splitlines() if ln.startswith("{")][-1])
            d = os.path.join(trace_dir, f"{case}_{tag.replace(' ', '')}_{turn}")
            got = _step(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "t", "--"] + me + ["--trace", case, "--calls", str(n_calls)] + flag, 300, env)
            if got is None:
                ok = False
                break
            kern = _stats(d, "*kernel_stats.csv")
            gen = "k_msdf_generate_union" if overlap else "k_msdf_generate"
            calls, us, longest = kern.get(gen, (0, 0.0, 0.0))
            ccalls, cus, clongest = kern.get("k_msdf_correct", (0, 0.0, 0.0))
            others = ", ".join(f"{k} {v[1] / n_calls:.1f}" for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1]) if k not in (gen, "k_msdf_correct"))
            lines.append(f"{case} ({CASES[case]}, {r['segments']} segments), {tag}: whole call median {r['median_us']:.1f} us (p10 {r['p10_us']:.1f}, p90 {r['p90_us']:.1f}); "
                         f"{gen} {us / max(calls, 1):.2f} us per launch over {calls} launches, the longest {longest:.1f}"
                         + (f"; k_msdf_correct {cus / ccalls:.2f} us per launch over {ccalls} launches, the longest {clongest:.1f}" if ccalls else ""))
            lines.append(f"    other kernels of the call, us per call: {others}")
            print(lines[-2], flush=True)
        if not ok:
            break
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


# ---------------------------------------------------------------------------------------------------- cubic outlines
CUBIC_LEGS = ("native", "quadratics", "lines")


def _split_cubic(P, t):
    """de Casteljau at t -> the two halves, (4, 2) each"""
    a, b, c = P[0] + (P[1] - P[0]) * t, P[1] + (P[2] - P[1]) * t, P[2] + (P[3] - P[2]) * t
    d, e = a + (b - a) * t, b + (c - b) * t
    m = d + (e - d) * t
    return [P[0], a, d, m], [m, e, c, P[3]]


def cubic_puts(leg):
    """-> [(segs, w, h, R)] of the skewed font set: 8-float outlines for `native`; 6-float outlines for `quadratics` (each cubic cut at 1/4,
    1/2, 3/4 and each part replaced by the quadratic with control point (3 (Q1 + Q2) - (Q0 + Q3)) / 4, the midpoint approximation) and for
    `lines` (each cubic in the coverage path's chords of 0.025 px)"""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import msdf_cubic_cases as CC

    out = []
    nan = float("nan")
    for _, segs, w, h, R in CC.skewed():
        if leg == "native":
            out.append((segs, w, h, R))
            continue
        rows = []
        for q in segs.astype(np.float64):
            if np.isnan(q[2]) or np.isnan(q[4]):
                rows.append([q[0], q[1], q[2], q[3], q[6], q[7]])
            elif leg == "lines":
                rows += [[x0, y0, nan, nan, x1, y1] for x0, y0, x1, y1 in CC.flatten_lines(q.astype(np.float32)[None])]
            else:
                P = [np.array(q[2 * k:2 * k + 2]) for k in range(4)]
                left, right = _split_cubic(P, 0.5)
                parts = _split_cubic(left, 0.5) + _split_cubic(right, 0.5)
                ends = [np.float32(parts[0][0])] + [np.float32(Q[3]) for Q in parts]  # rounded once, so that the parts meet
                ends[-1] = np.float32(P[3])
                for k, Q in enumerate(parts):
                    c = (3.0 * (Q[1] + Q[2]) - (Q[0] + Q[3])) / 4.0
                    rows.append([ends[k][0], ends[k][1], c[0], c[1], ends[k + 1][0], ends[k + 1][1]])
        out.append((np.array(rows, np.float32), w, h, R))
    return out


def _put_cubic_set(ctx, leg, puts, first_key):
    rects = []
    for i, (segs, w, h, R) in enumerate(puts):
        if leg == "native":
            rects.append(ctx.put_glyph_outline_cubic(first_key + i, segs, w, h, mtsdf=True, sdf_range=R))
        else:
            rects.append(ctx.put_glyph_outline(first_key + i, segs, w, h, mtsdf=True, sdf_range=R))
    return rects


def time_cubic(leg, timed=100, warm=10):
    puts = cubic_puts(leg)
    ctx = _context()
    us = []
    for k in range(warm + timed):
        ctx.reset_atlas()
        t1 = time.perf_counter()
        _put_cubic_set(ctx, leg, puts, 1)
        t2 = time.perf_counter()
        if k >= warm:
            us.append((t2 - t1) * 1e6)
    ctx.close()
    print(json.dumps({"leg": leg, "segments": sum(len(p[0]) for p in puts), "calls": timed, "median_us": statistics.median(us),
                      "p10_us": sorted(us)[len(us) // 10], "p90_us": sorted(us)[9 * len(us) // 10]}))


def trace_cubic(leg, calls):
    puts = cubic_puts(leg)
    ctx = _context()
    for _ in range(calls):
        ctx.reset_atlas()
        _put_cubic_set(ctx, leg, puts, 1)
    ctx.close()
    print(json.dumps({"leg": leg, "calls": calls}))


def error_cubic(leg):
    """the device's texels of the leg against the float64 reference of the cubic outlines"""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import msdf_cubic_cases as CC
    import msdf_cubic_ref as R

    puts = cubic_puts(leg)
    ctx = _context()
    rects = _put_cubic_set(ctx, leg, puts, 1)
    atlas = ctx.debug_read_surface(4)
    ctx.close()
    worst, beyond, images = 0, 0, 0
    for (x, y, w, h), (_, segs, _, _, Rr) in zip(rects, CC.skewed()):
        d = np.abs(atlas[y:y + h, x:x + w].astype(int) - R.generate(segs, w, h, Rr).astype(int)).max(axis=2)
        worst, beyond, images = max(worst, int(d.max())), beyond + int((d > 1).sum()), images + int((d > 1).sum() > 2)
    print(json.dumps({"leg": leg, "max_lsb": worst, "texels_beyond_1_lsb": beyond, "images_beyond_the_cap": images}))


CUBIC_HEAD = """tools/msdf_bench.py --cubic -- the 106 font inputs with every quadratic skewed into a genuine cubic (tests/msdf_cubic_cases.py skewed()),
as distance fields, three ways, MI355X: native = fdh_put_glyph_outline_cubic on the cubics; quadratics = each cubic cut into four quadratics
on the host (midpoint approximation), fdh_put_glyph_outline; lines = each cubic flattened to lines at 0.025 px, fdh_put_glyph_outline.  Host
clock around the 106 puts, profiler off, 100 timed sets after 10, the legs alternating, each a process of its own; the generator's device
time from a rocprofv3 --kernel-trace --stats run of its own, 20 sets; the field error is the device's texels against the float64 reference
of the CUBIC outlines (tests/msdf_cubic_ref.py), over all 106 images.

Hypothesis, stated before the numbers (nothing had been timed when it was written): a native cubic costs several times a quadratic per
edge and texel (K + 1 = 9 to 33 evaluations of g and four refinements of six Newton steps against one closed-form solve and four Newton
steps), but the native call walks a quarter of leg (a)'s curved edges and a smaller fraction still of leg (b)'s lines, which are cheap per
edge; the three generators come out within a small factor of one another, native the slowest per launch or close to it, and the whole
call, which is launch latency and the level chain, shows no difference beyond its spread.  What the native call buys is the field error:
legs (a) and (b) leave texels several LSB from the cubic reference, the native call none beyond the tolerance.
"""


def run_cubic(out_path, trace_dir, passes=2):
    me = [sys.executable, os.path.abspath(__file__)]
    lines = CUBIC_HEAD.splitlines() + [""]
    med = {leg: [] for leg in CUBIC_LEGS}
    seg = {}
    ok = True
    for _ in range(passes):
        for leg in CUBIC_LEGS:
            got = _step(me + ["--time-cubic", leg], 300) if ok else None
            if got is None:
                ok = False
                break
            r = json.loads([ln for ln in got.strip().splitlines() if ln.startswith("{")][-1])
            med[leg].append((r["median_us"], r["p10_us"], r["p90_us"]))
            seg[leg] = r["segments"]
    for leg in CUBIC_LEGS:
        if not ok:
            break
        d = os.path.join(trace_dir, "cubic_" + leg)
        got = _step(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "t", "--"] + me + ["--trace-cubic", leg, "--calls", "20"], 300)
        err = _step(me + ["--error-cubic", leg], 300) if got is not None else None
        if got is None or err is None:
            ok = False
            break
        kern = _stats(d, "*kernel_stats.csv")
        gen = "k_msdf_generate_cubic" if leg == "native" else "k_msdf_generate"
        calls, us, longest = kern.get(gen, (0, 0.0, 0.0))
        e = json.loads([ln for ln in err.strip().splitlines() if ln.startswith("{")][-1])
        lines.append(f"{leg} ({seg[leg]} segments): the 106 puts, median us per pass {', '.join(f'{m[0]:.1f} (p10 {m[1]:.1f}, p90 {m[2]:.1f})' for m in med[leg])}; "
                     f"{gen} {us / max(calls, 1):.2f} us per launch over {calls} launches, {us / 20:.1f} us per set, the longest {longest:.1f}")
        lines.append(f"    against the cubic reference: largest difference {e['max_lsb']} LSB, {e['texels_beyond_1_lsb']} texels beyond 1 LSB, {e['images_beyond_the_cap']} images beyond the cap of 2 texels")
        print("\n".join(lines[-2:]), flush=True)
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


BATCH_HEAD = """tools/msdf_bench.py --batch -- the 106 font inputs as ONE fdh_put_glyph_outlines against 106 single fdh_put_glyph_outline calls of the
parent commit's library, MI355X.  Host clock around the 106 glyphs, profiler off, 200 timed after 20 per leg; the two legs alternate, each
leg a process of its own, `passes` times per flag combination.  Kernels: a rocprofv3 --kernel-trace --stats run of its own, 60 batches.

Hypotheses, stated before the numbers (nothing had been timed when they were written):
  1. the batched generate launch (about 2 100 waves) takes about as long as the single launch of its slowest glyph: tens of microseconds,
     where the 106 single launches add up to milliseconds.
  2. the call is then dominated by the host -- build_shape and the edge records of 106 outlines, the packer -- and by the level chain's
     launches: 2 x 12 - 1 of them on a 4096 atlas, most with nothing to do below level 5.
"""


CUBIC_BATCH_HEAD = """tools/msdf_bench.py --cubic-batch -- the 106 skewed font outlines (tests/msdf_cubic_cases.py skewed(): 2 335 segments of 8 floats, 1 782 of them
cubics) as ONE fdh_put_glyph_outlines_cubic of this library against 106 fdh_put_glyph_outline_cubic calls of the parent commit's library,
MI355X, 4096 atlas reset before every call outside the clock.  Section 6's protocol: host clock around the 106 glyphs, profiler off, 200 timed
after 20 per leg; the legs alternate, each a process of its own, two passes per flag combination; kernels from a rocprofv3 --kernel-trace
--stats run of its own, 60 batches.

Hypotheses, stated before the numbers (nothing about the cubic path had been timed when they were written):
  1. the batched cubic generator is several times section 6's 85 us -- a cubic edge costs 9 to 33 evaluations of the quintic and four
     refinements of six Newton steps where a quadratic costs one closed-form solve -- but stays well under a millisecond: about 2 500 waves
     with culling, over 256 CUs.
  2. the 106 single cubic calls cost what section 6's single calls cost plus the heavier launches, 8 ms or more, because the idle device
     between puts is the same; so the batch wins by about the same difference, and by a smaller ratio than 11.9 x only in so far as the
     host's share (cubic build_shape, 36-float records: 336 KB instead of 224 KB) and the generator grew.
  3. the correction is one more launch of the generator's order (no culling, but only the tiles with candidates walk the edges).
"""


def run_batch(out_path, parent_lib, trace_dir, passes=2, case="font", head=None, combos=((False, False), (False, True), (True, False), (True, True))):
    me = [sys.executable, os.path.abspath(__file__)]
    lines = (head or BATCH_HEAD).splitlines() + [""]
    parent_env = dict(os.environ, FIGDRAW_HIP_LIB=os.path.abspath(parent_lib))
    ok = True
    for correct, overlap in combos:
        flag = (["--correct"] if correct else []) + (["--overlap"] if overlap else [])
        name = " | ".join(["MTSDF"] + (["CORRECT"] if correct else []) + (["OVERLAP"] if overlap else []))
        med = {"batch": [], "singles": []}
        stats = None
        for _ in range(passes):
            for leg, cmd, env in (("batch", ["--batched"], None), ("singles", [], parent_env)):
                got = _step(me + ["--time", case] + flag + cmd, 300, env) if ok else None
                if got is None:
                    ok = False
                    break
                r = json.loads([ln for ln in got.strip().splitlines() if ln.startswith("{")][-1])
                med[leg].append((r["median_us"], r["p10_us"], r["p90_us"]))
                stats = r.get("batch_stats") or stats
        if not ok:
            break
        d = os.path.join(trace_dir, "batch_" + "_".join([case] + [f.strip("-") for f in flag]))
        got = _step(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "t", "--"] + me + ["--trace", case, "--batched", "--calls", "60"] + flag, 300)
        if got is None:
            ok = False
            break
        kern = _stats(d, "*kernel_stats.csv")
        b, s1 = [m[0] for m in med["batch"]], [m[0] for m in med["singles"]]
        spread = max(max(b) - min(b), max(s1) - min(s1))
        lines.append(f"{name}: batch, median us per pass {', '.join(f'{m[0]:.1f} (p10 {m[1]:.1f}, p90 {m[2]:.1f})' for m in med['batch'])}; "
                     f"106 single calls of the parent, {', '.join(f'{m[0]:.1f} (p10 {m[1]:.1f}, p90 {m[2]:.1f})' for m in med['singles'])}")
        lines.append(f"    ratio of the means of the passes' medians {sum(s1) / sum(b):.1f} x; singles - batch {sum(s1) / len(s1) - sum(b) / len(b):.1f} us, "
                     f"the larger spread between a leg's own passes {spread:.1f} us: {'the batch wins by more than the spread' if min(s1) - max(b) > spread else 'NOT beyond the spread'}")
        lines.append(f"    the batch: {stats}")
        lines.append("    kernels, us per launch (launches per batch): " + ", ".join(f"{k} {v[1] / max(v[0], 1):.2f} ({v[0] / 60:.0f}), the longest {v[2]:.1f}"
                                                                                   for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1])))
        lines.append(f"    kernels, us per batch in all: {sum(v[1] for v in kern.values()) / 60:.1f}")
        print("\n".join(lines[-5:]), flush=True)
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", metavar="OUT")
    ap.add_argument("--batch", metavar="OUT", help="the font set as one batch against single calls of --parent-lib")
    ap.add_argument("--cubic-batch", metavar="OUT", help="the skewed font set as one cubic batch against single cubic calls of --parent-lib")
    ap.add_argument("--cubic", metavar="OUT", help="cubic outlines natively against four quadratics per cubic and against lines")
    ap.add_argument("--time-cubic", choices=list(CUBIC_LEGS))
    ap.add_argument("--trace-cubic", choices=list(CUBIC_LEGS))
    ap.add_argument("--error-cubic", choices=list(CUBIC_LEGS))
    ap.add_argument("--batched", action="store_true", help="with --time / --trace: one fdh_put_glyph_outlines per call")
    ap.add_argument("--nocull-lib")
    ap.add_argument("--parent-lib")
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--correct", action="store_true", help="with --time / --trace: put with FDH_GLYPH_MTSDF_CORRECT")
    ap.add_argument("--overlap", action="store_true", help="with --time / --trace: put with FDH_GLYPH_MTSDF_OVERLAP")
    ap.add_argument("--cases", default=",".join(CASES), help="with --all: the cases to run, comma-separated")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build", "msdf_trace"))
    ap.add_argument("--time", choices=list(TIMED_CASES))
    ap.add_argument("--trace", choices=list(TIMED_CASES))
    ap.add_argument("--calls", type=int, default=60)
    a = ap.parse_args()
    unknown = [c for c in a.cases.split(",") if c not in CASES]
    if unknown:
        ap.error(f"--cases: unknown case(s) {', '.join(unknown)}; the cases are {', '.join(CASES)}")
    if a.cubic:
        sys.exit(run_cubic(a.cubic, a.trace_dir, max(a.passes, 2)))
    elif a.time_cubic:
        time_cubic(a.time_cubic)
    elif a.trace_cubic:
        trace_cubic(a.trace_cubic, a.calls if a.calls != 60 else 20)
    elif a.error_cubic:
        error_cubic(a.error_cubic)
    elif a.cubic_batch:
        if not a.parent_lib:
            ap.error("--cubic-batch needs --parent-lib")
        sys.exit(run_batch(a.cubic_batch, a.parent_lib, a.trace_dir, max(a.passes, 2), "cubicfont", CUBIC_BATCH_HEAD, ((False, False), (True, False))))
    elif a.batch:
        if not a.parent_lib:
            ap.error("--batch needs --parent-lib")
        sys.exit(run_batch(a.batch, a.parent_lib, a.trace_dir, max(a.passes, 2)))
    elif a.all:
        sys.exit(run_all(a.all, a.nocull_lib, a.trace_dir, a.parent_lib, a.passes, a.cases.split(",")))
    elif a.time:
        time_case(a.time, a.correct, a.overlap, a.batched)
    elif a.trace:
        trace_case(a.trace, a.calls, a.correct, a.overlap, a.batched)
    else:
        ap.error("nothing to do")
