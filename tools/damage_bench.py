#!/usr/bin/env python3
"""Damage tracking (include/figdraw_hip_damage.h): per-frame GPU time with tracking off against on, for frames a UI produces.

  (a) glyph  the 10k-glyph frame at 4K (BASELINE config 4) with one glyph row edited per frame
  (b) cells  make_non_clip_benchmark with one cell's fill toggled per frame
  (c) tree   the 1080p bench tree (no full-frame blur) with one root moved per frame
  (d) anim   the animated 1080p bench tree without the full-frame blur: every bin changes (the overhead case)

usage:
  damage_bench.py --case a --mode on [--frames 60]    renders the frames (run it under rocprofv3 --kernel-trace --stats for the per-kernel
                                                       split); prints one JSON line: wall ms per frame and fdh_damage_bins' mean count
  damage_bench.py --summarize DIR                      the table from DIR/<case>_<mode>/*kernel_stats.csv (one rocprofv3 run per case and
                                                       mode): GPU us per frame = all kernels' total duration / frames rendered"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"a": "glyph 4K, one row edited", "b": "non-clip cells, one fill toggled", "c": "bench tree 1080p, one root moved",
         "d": "bench tree 1080p animated (every bin)"}


def frames_for(case, n):
    """-> (w, h, setup(ctx), frame(ctx, i))"""
    from figdraw_amd import scenes as SC
    from figdraw_amd.scene import fill, rect, rgba

    if case == "a":
        images = SC.load_glyph_fixture(os.path.join(ROOT, "tests", "golden", "glyphs_ubuntu20.npz"))
        w, h = 3840, 2160
        sc = SC.make_glyph_scene(float(w), float(h), images)
        lst = next(iter(sc.layers.values()))
        from figdraw_amd.scene import FigKind
        texts = [i for i, nd in enumerate(lst.nodes) if nd.kind == FigKind.nkText]
        row = [texts[len(texts) // 2]]  # one row's glyph run, moved by a pixel per frame

        def setup(ctx):
            for k, img in images.items():
                ctx.put_image(k, img)

        def frame(ctx, i):
            for j in row:
                x, y, bw, bh = lst.nodes[j].screenBox
                lst.nodes[j].screenBox = rect(x + (1.0 if i % 2 else -1.0), y, bw, bh)
            ctx.render_frame(sc, w, h)
        return w, h, setup, frame
    if case == "b":
        sc = SC.make_non_clip_benchmark()
        lst = next(iter(sc.layers.values()))

        def frame(ctx, i):
            lst.nodes[7].fill = fill(rgba(255, 0, 0, 255) if i % 2 else rgba(0, 0, 255, 255))
            ctx.render_frame(sc, 1200, 800)
        return 1200, 800, lambda ctx: None, frame
    if case == "c":
        w, h = 1920, 1080
        sc = SC.make_render_tree_100(float(w), float(h), frame=0)
        lst = next(iter(sc.layers.values()))
        root = lst.rootIds[len(lst.rootIds) // 2]

        def frame(ctx, i):
            x, y, bw, bh = lst.nodes[root].screenBox
            lst.nodes[root].screenBox = rect(x + (3.0 if i % 2 else -3.0), y, bw, bh)
            ctx.render_frame(sc, w, h)
        return w, h, lambda ctx: None, frame
    if case == "d":
        w, h = 1920, 1080
        return w, h, lambda ctx: None, lambda ctx, i: ctx.render_frame(SC.make_render_tree_100(float(w), float(h), frame=i), w, h)
    raise SystemExit(f"unknown case {case}")


def run(case, mode, n):
    import numpy as np
    from figdraw_amd.context import HipContext

    w, h, setup, frame = frames_for(case, n)
    ctx = HipContext(device=0)
    setup(ctx)
    ctx.set_damage_tracking(mode == "on")
    frame(ctx, 0)  # (the first tracked frame is a full one: it is in the kernel totals, 1 frame of n + 1)
    ctx.sync()
    t0 = time.perf_counter()
    damaged = []
    for i in range(1, 1 + n):
        frame(ctx, i)
        ctx.sync()
        damaged.append(int(ctx.damage_bins().sum()))
    wall = (time.perf_counter() - t0) * 1e3 / n
    bins = int(np.prod(ctx.damage_bins().shape))
    ctx.close()
    print(json.dumps({"case": case, "mode": mode, "frames": n + 1, "wall_ms_per_frame": round(wall, 3),
                      "damaged_bins_mean": round(sum(damaged) / len(damaged), 1), "bins": bins}))


def summarize(d):
    rows = {}
    for path in sorted(glob.glob(os.path.join(d, "*_*", "**", "*kernel_stats.csv"), recursive=True)):
        key = os.path.relpath(path, d).split(os.sep)[0]
        case, mode = key.split("_", 1)
        meta = json.load(open(os.path.join(d, key + ".json")))
        per = {}
        for r in csv.DictReader(open(path)):
            name = r["Name"].split("(")[0].replace("void ", "").replace("fdh::", "")
            name = name.split("<")[0]
            per[name] = per.get(name, 0.0) + float(r["TotalDurationNs"]) / 1e3 / meta["frames"]
        rows[(case, mode)] = (sum(per.values()), per, meta)
    print(f"{'case':38s} {'off us/frame':>13s} {'on us/frame':>12s} {'on/off':>7s} {'bins on':>12s}")
    for c in "abcd":
        if (c, "off") not in rows or (c, "on") not in rows:
            continue
        off, on = rows[(c, "off")], rows[(c, "on")]
        print(f"{'(' + c + ') ' + CASES[c]:38s} {off[0]:13.1f} {on[0]:12.1f} {on[0] / off[0]:7.3f} {on[2]['damaged_bins_mean']:6.1f}/{on[2]['bins']}")
    print("\nper kernel, us per frame (off -> on):")
    for c in "abcd":
        if (c, "off") not in rows or (c, "on") not in rows:
            continue
        off, on = rows[(c, "off")][1], rows[(c, "on")][1]
        parts = ", ".join(f"{k} {off.get(k, 0):.1f} -> {on.get(k, 0):.1f}" for k in sorted(set(off) | set(on), key=lambda k: -max(off.get(k, 0), on.get(k, 0))))
        print(f"  ({c}) {parts}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=list(CASES))
    ap.add_argument("--mode", choices=["on", "off"])
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        run(a.case, a.mode, a.frames)
