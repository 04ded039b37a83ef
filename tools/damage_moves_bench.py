#!/usr/bin/env python3
"""Moved damage readback (include_readback/figdraw_hip_moves.h): what a scroll costs on the wire and on the GPU, with and without COPY tiles.

Cases: (p17) a 4K page of text rows and image cards scrolled by 17 pixels a frame; (p120) the same page scrolled by 120; (b) the bench
frame (the bench tree at 1080p) with one panel -- a root and its subtree -- moved by (6, 4) a frame.

  coded   fdh_read_damage_coded, exact damage readback on          moved   fdh_find_damage_moves (its first two candidates; (b): the
                                                                           panel's move as the application knows it) + fdh_read_damage_moved

usage:
  damage_moves_bench.py --bytes                       no GPU: the page painted in numpy (the bench frame by the CPU oracle), coded by
                                                      tests/tilemove_ref.py with and without moves; prints the report's byte lines
  damage_moves_bench.py --time CASE [--ways coded]    7 batches of 12 timed reads after 4 warm-up reads, the two ways alternated batch by
                                                      batch (or one way only: what a parent library can run); one JSON line
  damage_moves_bench.py --all OUT.txt [--parent-lib LIB] [--bytes-file F]   the steps above as child processes, each under its own time limit, nothing
                                                      started after a failure; writes the report"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"p17": "4K page of text rows and image cards, scrolled by 17 pixels a frame", "p120": "the same page, scrolled by 120 pixels a frame",
         "b": "bench tree 1080p, one panel moved by (6, 4) a frame"}
GROUND = (244, 244, 240, 255)
INK = (24, 26, 32)
ROW, CARD_W, CARD_H = 24, 384, 216

HYPOTHESES = [
    "Hypotheses (stated before any timing; the byte counts below are arithmetic and were known):",
    "  1. On the scrolled page nearly every tile whose source is inside the frame is a COPY: the wire bytes fall by more than an order of",
    "     magnitude (p17), less at p120 where two bin rows of new content scroll in.",
    "  2. The moved read costs the coded exact read plus k_damage_move_match: per pending bin and move that survives the first four rows,",
    "     16 KB of surface and 16 KB of mirror -- at most 2 x 33.4 MB a move at 4K, ~20 - 40 us at a few TB/s; the encoder does less work",
    "     (a COPY tile stores 24 bytes).  Expected: within +-10 % of the coded read on the GPU side, faster end to end once the bytes are sent on.",
    "  3. The mover reads ~270 KB of mirror per probing bin at max_shift 256 (~550 MB at 4K, cache-resident): 100 - 300 us; at max_shift 128 half.",
]


# ------------------------------------------------------------------------------------------------------------------ the page
def _page(w, h):
    """the page's items in page coordinates, far taller than the frame: ("text", x, y, glyph id) and ("card", x, y, key)"""
    from figdraw_amd.scenes import load_glyph_fixture
    images = load_glyph_fixture(os.path.join(ROOT, "tests", "golden", "glyphs_ubuntu20.npz"))
    glyphs = {k: images[k] for k in range(1033, 1127)}
    rng = np.random.RandomState(12)
    cards = {}
    for k in range(4):  # a photo-like card: smooth shading and grain
        yy, xx = np.mgrid[0:CARD_H, 0:CARD_W]
        img = np.stack([(xx * (k + 1) // 3 + rng.randint(0, 24, xx.shape)) & 255, (yy * 2 + rng.randint(0, 24, xx.shape)) & 255,
                        ((xx + yy) // 2 + rng.randint(0, 24, xx.shape)) & 255, np.full(xx.shape, 255)], axis=2).astype(np.uint8)
        cards[5000 + k] = img
    items = []
    y = -400
    while y < h + 800:
        if (y // ROW) % 14 == 0:
            for x in range(40, w - CARD_W, CARD_W + 120):
                items.append(("card", x, y, 5000 + int(rng.randint(0, 4))))
            y += CARD_H + ROW - (CARD_H % ROW)
            continue
        x = 40
        while x < w - 60:
            code = 1033 + int(rng.randint(0, 94))
            if rng.rand() < 0.15:
                x += 10  # a space
                continue
            items.append(("text", x, y + 20 - glyphs[code].shape[0], code))
            x += glyphs[code].shape[1] + 2
        y += ROW
    return items, glyphs, cards


def _paint(w, h, items, glyphs, cards, sy):
    """the frame in numpy: ink through the glyph's coverage over the ground, cards opaque"""
    px = np.empty((h, w, 4), np.float32)
    px[:] = GROUND
    for kind, x, y, key in items:
        y -= sy
        img = glyphs[key] if kind == "text" else cards[key]
        ih, iw = img.shape[:2]
        if y + ih <= 0 or y >= h:
            continue
        y0, y1 = max(y, 0), min(y + ih, h)
        src = img[y0 - y:y1 - y]
        if kind == "card":
            px[y0:y1, x:x + iw] = src
        else:
            cov = src[..., 3:4].astype(np.float32) / 255.0
            px[y0:y1, x:x + iw, :3] = px[y0:y1, x:x + iw, :3] * (1.0 - cov) + np.array(INK, np.float32) * cov
    return np.clip(px + 0.5, 0, 255).astype(np.uint8)


def _draw(ctx, w, h, items, glyphs, cards, sy):
    white = [(255, 255, 255, 255)] * 4
    ink = [INK + (255,)] * 4
    ctx.begin_frame(w, h, True, tuple(v / 255.0 for v in GROUND))
    for kind, x, y, key in items:
        y -= sy
        img = glyphs[key] if kind == "text" else cards[key]
        if y + img.shape[0] <= 0 or y >= h:
            continue
        ctx.draw_image(key, (float(x), float(y)), ink if kind == "text" else white, (float(img.shape[1]), float(img.shape[0])))
    ctx.end_frame()


def _bench_tree(k):
    from figdraw_amd.scene import rect
    from figdraw_amd.scenes import make_render_tree_100
    w, h = 1920, 1080
    sc = make_render_tree_100(float(w), float(h), frame=0)
    lst = next(iter(sc.layers.values()))
    root = lst.rootIds[len(lst.rootIds) // 4]

    def shift(idx, dx, dy):
        x, y, bw, bh = lst.nodes[idx].screenBox
        lst.nodes[idx].screenBox = rect(x + dx, y + dy, bw, bh)
        for c in lst.child_indices(idx):
            shift(c, dx, dy)
    shift(root, 6.0 * k, 4.0 * k)
    return sc, w, h


# ------------------------------------------------------------------------------------------------------------------ bytes, on the CPU
def _wire(old, new, moves):
    import tilecode_ref as T
    import tilemove_ref as M
    h, w = new.shape[:2]
    differs = [(x, y, tw, th) for x, y, tw, th in T.tiles_of(w, h) if (old[y:y + th, x:x + tw] != new[y:y + th, x:x + tw]).any()]
    d1, _ = T.encode_frame(new, differs)
    d2, _, copied = M.encode_frame_moved(old, new, moves, differs)
    return len(differs), T.wire_bytes(d1), T.wire_bytes(d2), copied


def bytes_report():
    lines = ["Coded bytes of one frame's read, directory and payload (24 bytes a tile + each payload rounded up to 16), from the reference coder",
             "(tests/tilemove_ref.py) on frames made on the CPU -- the page painted in numpy, the bench tree by the CPU oracle.  Arithmetic:"]
    w, h = 3840, 2160
    items, glyphs, cards = _page(w, h)
    for case, step in (("p17", 17), ("p120", 120)):
        old, new = _paint(w, h, items, glyphs, cards, 0), _paint(w, h, items, glyphs, cards, step)
        n, plain, moved, copied = _wire(old, new, [(0, step)])
        lines.append(f"  ({case}) {CASES[case]}: {n} of {((w + 63) // 64) * ((h + 63) // 64)} tiles changed; coded {plain} bytes; moved {moved} bytes "
                     f"({copied} COPY tiles): {plain / max(moved, 1):.1f} x fewer; the raw frame is {4 * w * h}")
    from oracle import oracle as O
    frames = []
    for k in (0, 1):
        sc, w, h = _bench_tree(k)
        ref = O.Oracle(threads=8)
        ref.render_frame(sc, w, h)
        frames.append(ref.read_pixels())
    n, plain, moved, copied = _wire(frames[0], frames[1], [(-6, -4)])
    lines.append(f"  (b) {CASES['b']}: {n} of {((w + 63) // 64) * ((h + 63) // 64)} tiles changed; coded {plain} bytes; moved {moved} bytes ({copied} COPY tiles): "
                 f"{plain / max(moved, 1):.1f} x fewer")
    return lines


# ------------------------------------------------------------------------------------------------------------------ times, on the GPU
def time_case(case, ways, batches=7, timed=12, warm=4):
    from figdraw_amd.context import HipContext
    ctx = HipContext(device=0)
    L, hnd = ctx.L, ctx.h
    if case == "b":
        scenes = [_bench_tree(k) for k in range(2)]
        w, h = scenes[0][1], scenes[0][2]
        frame = lambda i: ctx.render_frame(scenes[i % 2][0], w, h)  # noqa: E731
        known = lambda i: [(-6, -4)] if i % 2 else [(6, 4)]  # noqa: E731
    else:
        w, h = 3840, 2160
        step = 17 if case == "p17" else 120
        items, glyphs, cards = _page(w, h)
        for k, v in list(glyphs.items()) + list(cards.items()):
            ctx.put_image(k, v)
        frame = lambda i: _draw(ctx, w, h, items, glyphs, cards, (i % 16) * step)  # noqa: E731  (15 scrolls forward, then a jump back)
        known = None
    ctx.set_damage_tracking(True)
    ctx.set_damage_readback(True)
    ctx.set_damage_exact(True)
    t_ptr, p_ptr = C.c_void_p(), C.c_void_p()
    n_c, cp_c, nb_c, no_c = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
    mv = np.zeros((2, 2), np.int16)
    votes = np.zeros(2, np.int32)
    has_moves = hasattr(L, "fdh_read_damage_moved")

    def check(rc):
        if rc != 0:
            raise SystemExit(L.fdh_last_error().decode())

    out = {way: {"read_us": [], "find_us": [], "tiles": [], "copied": [], "bytes": []} for way in ways}
    i = 0
    for b in range(batches):
        for way in ways:
            if way == "moved" and not has_moves:
                raise SystemExit("this library has no fdh_read_damage_moved")
            reads, finds, tiles, copied, nbytes = [], [], [], [], []
            for k in range(warm + timed):
                frame(i)
                ctx.sync()
                t0 = time.perf_counter()
                n_mv = 0
                if way == "moved":
                    if known is None:
                        check(L.fdh_find_damage_moves(hnd, 128, mv.ctypes.data, votes.ctypes.data, 2, C.byref(no_c)))
                        n_mv = no_c.value
                    else:
                        mv[0] = known(i)[0]
                        n_mv = 1
                t1 = time.perf_counter()
                if way == "moved":
                    check(L.fdh_read_damage_moved(hnd, mv.ctypes.data, n_mv, C.byref(t_ptr), C.byref(p_ptr), C.byref(n_c), C.byref(nb_c), None, None, None, C.byref(cp_c)))
                else:
                    check(L.fdh_read_damage_coded(hnd, C.byref(t_ptr), C.byref(p_ptr), C.byref(n_c), C.byref(nb_c), None, None, None))
                    cp_c.value = 0
                t2 = time.perf_counter()
                i += 1
                if k >= warm:
                    reads.append((t2 - t1) * 1e6); finds.append((t1 - t0) * 1e6); tiles.append(n_c.value); copied.append(cp_c.value)
                    nbytes.append(24 * n_c.value + nb_c.value)
            v = out[way]
            v["read_us"].append(round(statistics.median(reads), 1)); v["find_us"].append(round(statistics.median(finds), 1))
            v["tiles"].append(round(statistics.mean(tiles), 1)); v["copied"].append(round(statistics.mean(copied), 1)); v["bytes"].append(round(statistics.mean(nbytes)))
    ctx.close()
    print(json.dumps({"case": case, "w": w, "h": h, "batches": batches, "timed": timed, "ways": out}))


def _step(cmd, limit, env=None):
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print(f"step exceeded {limit} s: {' '.join(cmd)}", file=sys.stderr)
        return None
    if r.returncode != 0:
        print(f"step failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", file=sys.stderr)
        return None
    return r.stdout


def _summary(v, key):
    s = sorted(v[key])
    return f"{statistics.median(s):9.1f} (batches {s[0]:.1f} .. {s[-1]:.1f})"


def run_all(out_path, parent_lib, cases, bytes_file):
    me = [sys.executable, os.path.abspath(__file__)]
    lines = ["tools/damage_moves_bench.py -- a scroll read with and without COPY tiles.", ""] + HYPOTHESES + [""]
    got = open(bytes_file).read() if bytes_file else _step(me + ["--bytes"], 900)  # (the byte lines need no GPU: they may come from an earlier --bytes)
    ok = got is not None
    if ok:
        lines += got.strip().splitlines() + [""]
        lines += ["Times, MI355X.  Host clock, profiler off; per case 7 batches of 12 timed reads after 4 warm-up reads, the ways alternated batch by",
                  "batch in one process; the median of the batch medians, us, and the spread between batches, which is the noise floor.",
                  "read = from the frame's fdh_sync (and the mover's return) to the read's return; find = fdh_find_damage_moves (max_shift 128, 2 candidates);",
                  "bytes = 24 a tile + payload, as the GPU coded them."]
    for case in cases if ok else []:
        runs = [("this library", None, ["coded", "moved"])] + ([("parent library", parent_lib, ["coded"])] if parent_lib else [])
        lines.append(f"({case}) {CASES[case]}")
        for name, lib, ways in runs:
            env = dict(os.environ)
            if lib:
                env["FIGDRAW_HIP_LIB"] = os.path.abspath(lib)
            got = _step(me + ["--time", case, "--ways", ",".join(ways)], 400, env)
            if got is None:
                ok = False
                break
            print(f"timed ({case}) {name}", flush=True)
            r = json.loads([ln for ln in got.strip().splitlines() if ln.startswith("{")][-1])
            for way in ways:
                v = r["ways"][way]
                line = f"    {name:14s} {way:6s} read {_summary(v, 'read_us')}   tiles {statistics.mean(v['tiles']):7.1f}   COPY {statistics.mean(v['copied']):7.1f}   bytes {round(statistics.mean(v['bytes'])):9d}"
                if way == "moved":
                    line += f"   find {_summary(v, 'find_us')}"
                lines.append(line)
        if not ok:
            break
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it.  What is not listed above was not measured."]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", metavar="OUT")
    ap.add_argument("--parent-lib")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--bytes", action="store_true")
    ap.add_argument("--bytes-file")
    ap.add_argument("--time", choices=list(CASES))
    ap.add_argument("--ways", default="coded,moved")
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.all, a.parent_lib, a.cases.split(","), a.bytes_file))
    elif a.bytes:
        print("\n".join(bytes_report()))
    elif a.time:
        time_case(a.time, a.ways.split(","))
    else:
        ap.error("nothing to do")
