#!/usr/bin/env python3
"""Picking (include/figdraw_hip_pick.h): what a pick costs, next to what a frame costs, on the frames bench.py and BASELINE config 4 render.

  pick_bench.py                 (GPU) one JSON line per measurement:
    frame     the bench frame (300-rect tree + full-frame blur, 3840x2160): one frame at a time as bench.py's one_frame_at_a_time leg times
              it (its animation frames through fdh_render_frame from tools/call_player.c on one context, picking off: median of 5 batches of
              200), and the host time of fdh_render_frame with picking off and on (fdh_get_frame_stats' ms_host_record: the calling thread's
              recording, median of 100 frames, off / on alternated twice)
    points    fdh_pick_points wall-clock -- the wait for the frame, the copies and the launch included -- for 64 seeded points, max_hits = 1:
              median and 90th percentile of 200 calls; bench frame and config 4 (10 001 glyph quads)
    region    a full-frame fdh_pick_region (3840x2160), wall-clock, median of 5; and its ratio to the frame's phase-0 compositor time
  pick_bench.py --frame-only    (GPU) the one-frame-at-a-time figure alone -- it runs on a library without picking (FIGDRAW_HIP_LIB=the
                                parent's): the point-query bar is that figure, on the same box
  pick_bench.py --bands         (CPU) the oracle's 1-LSB band shares of tests/test_pick.py's scenes: the pixels its exactness check leaves
                                out, against the caps it asserts"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 3840, 2160


def _timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def _frames():
    from figdraw_amd import scenes as SC

    images = SC.load_glyph_fixture(os.path.join(ROOT, "tests", "golden", "glyphs_ubuntu20.npz"))
    return {"bench": (SC.make_render_tree_100(float(W), float(H), frame=0, full_frame_blur=True), {}),
            "config4": (SC.make_glyph_scene(float(W), float(H), images), images)}


def one_frame_at_a_time():
    """us per frame, frames strictly one after another on one context (bench.py's one_frame_at_a_time leg: its 8 animation frames)"""
    from figdraw_amd import call_stream as CS
    from figdraw_amd import scenes as SC
    from figdraw_amd.context import HipContext

    cscenes = [SC.make_render_tree_100(float(W), float(H), frame=f, full_frame_blur=True).to_c() for f in range(8)]
    ctx = HipContext(device=0)
    player = CS.Player()
    player.play_scenes([ctx], cscenes, 20, W, H)
    ctx.sync()
    batches = []
    for _ in range(5):
        t0 = time.perf_counter()
        player.play_scenes([ctx], cscenes, 200, W, H)
        ctx.sync()
        batches.append((time.perf_counter() - t0) * 1e6 / 200)
    ctx.close()
    return statistics.median(batches), batches


def gpu():
    from figdraw_amd.context import HipContext

    frames = _frames()
    rng = np.random.default_rng(64)
    pts = rng.uniform((0.0, 0.0), (float(W), float(H)), size=(64, 2)).astype(np.float32)
    one_frame_us, batches = one_frame_at_a_time()
    # the host time of fdh_render_frame with picking off / on
    sc, _ = frames["bench"]
    ctx = HipContext(device=0)
    host = {}
    for on in (False, True, False, True):
        ctx.set_pick(on)
        ms = []
        for _ in range(100):
            ctx.render_frame(sc, W, H)
            ms.append(ctx.frame_stats().ms_host_record)
        host.setdefault("on" if on else "off", []).append(statistics.median(ms) * 1e3)
    ctx.close()
    print(json.dumps({"what": "frame", "frame": "bench", "one_frame_at_a_time_us": round(one_frame_us, 1), "batches_us": [round(b, 1) for b in batches],
                      "host_record_us_pick_off": [round(v, 1) for v in host["off"]], "host_record_us_pick_on": [round(v, 1) for v in host["on"]]}), flush=True)
    for name, (sc, images) in frames.items():
        ctx = HipContext(device=0)
        for k, img in images.items():
            ctx.put_image(k, img)
        ctx.set_pick(True)
        ctx.render_frame(sc, W, H)
        ctx.profile(5)
        composite_main_us = ctx.frame_stats().ms_composite_main * 1e3
        ctx.render_frame(sc, W, H)
        ctx.sync()
        st = ctx.frame_stats()
        for _ in range(10):
            ctx.pick_points(pts, threshold=128, max_hits=1)
        t = _timed(lambda: ctx.pick_points(pts, threshold=128, max_hits=1), 200)
        hits, counts = ctx.pick_points(pts, threshold=128, max_hits=1)
        print(json.dumps({"what": "points", "frame": name, "n_draws": st.n_draws, "points": len(pts), "max_hits": 1,
                          "us_median": round(statistics.median(t), 1), "us_p90": round(float(np.percentile(t, 90)), 1),
                          "points_hit": int((counts > 0).sum())}), flush=True)
        ctx.pick_region(threshold=128)
        t = _timed(lambda: ctx.pick_region(threshold=128), 5)
        print(json.dumps({"what": "region", "frame": name, "pixels": W * H, "us_median": round(statistics.median(t), 1),
                          "composite_main_us": round(composite_main_us, 1),
                          "ratio_to_composite_main": round(statistics.median(t) / max(composite_main_us, 1e-3), 2)}), flush=True)
        ctx.close()


def bands():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_pick as T

    print(f"{'scene':28s} {'draws':>5s}  top@128  top@64  list@64  list@128  (caps: top {100 * T.TOP_CAP:.1f} %, list {100 * T.LIST_CAP:.1f} %)")
    for name in T.SCENES:
        sc, w, h, used, calls = T.scene_stream(name)
        draws, _ = T.draw_records(calls)
        A = T.oracle_alphas(calls, w, h, used)
        s = [100 * T.band_shares(A, draws, 128)[0], 100 * T.band_shares(A, draws, 64)[0], 100 * T.band_shares(A, draws, 64)[1],
             100 * T.band_shares(A, draws, 128)[1]]
        print(f"{name:28s} {len(draws):5d}  " + "  ".join(f"{v:6.3f}%" for v in s), flush=True)
    sc, w, h, used, calls = T.scene_stream("random_scene_3")
    draws, _ = T.draw_records(calls)
    A = T.oracle_alphas(calls, w, h, used)
    print(f"{'random_scene_3, shadows':28s} {len(draws):5d}  {100 * T.band_shares(A, draws, 128, True)[0]:6.3f}%  "
          f"{100 * T.band_shares(A, draws, 64, True)[0]:6.3f}%  {100 * T.band_shares(A, draws, 64, True)[1]:6.3f}%")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--bands", action="store_true")
    ap.add_argument("--frame-only", action="store_true")
    a = ap.parse_args()
    if a.bands:
        bands()
    elif a.frame_only:
        us, batches = one_frame_at_a_time()
        print(json.dumps({"what": "frame", "frame": "bench", "library": os.environ.get("FIGDRAW_HIP_LIB", "this tree's"),
                          "one_frame_at_a_time_us": round(us, 1), "batches_us": [round(b, 1) for b in batches]}), flush=True)
    else:
        gpu()
