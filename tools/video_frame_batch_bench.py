#!/usr/bin/env python3
"""What a batch of decoded video frames costs (fdh_put_video_frames, fdh_update_video_frames; include_glyphs/figdraw_hip_video_frames.h) on
an MI355X, against the single calls it replaces -> profiles/video_frame_batch.txt.

  video_frame_batch_bench.py OUT --parent-lib LIB [--rounds N] [--warmup W]
  video_frame_batch_bench.py --step SHAPE:OP:SIDE [--rounds N] [--warmup W]      one step in this process; one JSON line

The protocol is tools/device_image_bench.py --batch's: a measurement is the host clock around ONE batch call of n frames on this tree's
library, or around n single calls of the same frames on --parent-lib, the parent commit's library -- every call ends in a device
synchronise --, on one context, N timed rounds after W, median (p10 .. p90).  A row is a shape and an operation (update, put); each side of
a row is a process of its own, the two alternating their order from row to row; the n of a shape alternate inside a process.  Shapes:
thumbs -- n = 1, 4, 16, 64 frames of 320 x 180 NV12; hd -- 16 frames of 1280 x 720 NV12; wall -- 9 frames of 1920 x 1080, NV12, P010 and
BGRA8 by turns.  The frames of a shape share one source per format.  For a put the atlas is reset before every round outside the clock; an
update goes to entries a put made once.  Every step is a child process under its own time limit, nothing is started after a failure, and
what was not reached is written down as "not measured".  There is no CPU fallback: without a device the context cannot be made and the
step fails."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = ("update", "put")
NV12, P010, BGRA8 = 1, 2, 0
SHAPES = {  # name -> (width, height, the formats by turns, the n, the atlas)
    "thumbs": (320, 180, (NV12,), (1, 4, 16, 64), 4096),
    "hd": (1280, 720, (NV12,), (16,), 8192),
    "wall": (1920, 1080, (NV12, P010, BGRA8), (9,), 8192),
}
HEAD = """tools/video_frame_batch_bench.py -- n decoded video frames as ONE fdh_put_video_frames / fdh_update_video_frames (this tree's library)
against n single fdh_put_video_frame / fdh_update_video_frame calls of the PARENT commit's library, MI355X.

Hypotheses, written before the first number:
1. The launch count does not depend on n: a group of the batch is one launch whatever it holds, so the thumbs rows report the same
   `launches` for n = 1, 4, 16 and 64 (one group; 320 x 180 ends its chain at level 7, so the tails add one: 2).
2. A single call is a launch or two plus a synchronise, 20 - 30 us whatever the frame up to 256 x 256 (profiles/video_frame.txt), and n
   single calls cost n times that.  A batch pays one copy of its tables, its launches and one synchronise, plus the host's work per frame
   (validation, two pointer attributes, placement, the tables) and the device's work per tile.  So from some n on the batch beats the n
   single calls of the parent by more than the parent's own run-to-run spread (p90 - p10 of that row); expected: from n = 4.  The ratio
   grows with n until the tiles' device time dominates: 16 frames of 1280 x 720 are 14 720 tiles, 9 of 1920 x 1080 are 18 360, where the
   conversion itself is most of either side and the ratio falls towards 1.
3. A batch of ONE is slower than the single call by about what the image batch's was, 7 - 11 us (profiles/device_image_batch.txt): the
   table copy and the tables' making.
What would refute 2: a batch of 4 no faster than 4 single calls, or a per-frame host cost near a single call's (hipPointerGetAttributes,
twice per frame, is the suspect).
"""


def step(shape, op, side, rounds, warmup):
    """one shape and operation on one side: "batch" -- one call of n frames -- or "single" -- n calls; the n alternate"""
    import numpy as np
    from figdraw_amd.context import HipContext

    w, h, formats, counts, atlas = SHAPES[shape]
    rng = np.random.default_rng(w)
    ctx = HipContext(atlas_size=atlas, device=0)
    hip = C.CDLL("libamdhip64.so")

    def device(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0  # (a bare int would travel as 32 bits)
        return p.value

    cw, ch = (w + 1) // 2, (h + 1) // 2
    sources = {}  # format -> (y_ptr, uv_ptr, w, h, pitch_y, pitch_uv, format, matrix, range, flags)
    for fmt in formats:
        if fmt == BGRA8:
            sources[fmt] = (device(rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)), 0, w, h, 4 * w, 0, BGRA8, 0, 0, 0)
        else:
            dt, es = (np.uint8, 1) if fmt == NV12 else (np.uint16, 2)
            top = 256 if fmt == NV12 else 65536
            sources[fmt] = (device(rng.integers(0, top, size=(h, w)).astype(dt)), device(rng.integers(0, top, size=(ch, cw, 2)).astype(dt)), w, h, w * es, 2 * cw * es, fmt, 1, 0, 0)
    legs = {}
    for n in counts:
        items = [(k + 1,) + sources[formats[k % len(formats)]] for k in range(n)]
        if side == "batch":
            legs[str(n)] = (lambda items=items: ctx.put_video_frames(items)) if op == "put" else (lambda items=items: ctx.update_video_frames(items))
        else:
            call = ctx.put_video_frame if op == "put" else ctx.update_video_frame
            legs[str(n)] = lambda items=items, call=call: [call(*it[:7], format=it[7], matrix=it[8], range=it[9], flags=it[10]) for it in items]
    us = {leg: [] for leg in legs}
    launches = {}
    if op == "update":
        for k in range(max(counts)):
            it = (k + 1,) + sources[formats[k % len(formats)]]
            ctx.put_video_frame(*it[:7], format=it[7], matrix=it[8], range=it[9], flags=it[10])
    for k in range(warmup + rounds):
        for leg, f in legs.items():
            if op == "put":
                ctx.reset_atlas()
            ctx.sync()
            t1 = time.perf_counter()
            f()
            t2 = time.perf_counter()
            if k >= warmup:
                us[leg].append((t2 - t1) * 1e6)
            if side == "batch":
                launches[leg] = ctx.video_batch_stats()["launches"]
    ctx.close()
    q = lambda v, f: sorted(v)[int(f * (len(v) - 1))]  # noqa: E731
    print(json.dumps({"step": f"{shape}:{op}:{side}", "launches": launches, **{leg: [statistics.median(v), q(v, 0.1), q(v, 0.9)] for leg, v in us.items()}}))


def run_child(name, rounds, warmup, lib, limit=300):
    """one step as a process of its own -> its JSON line; None: it failed"""
    env = dict(os.environ, FIGDRAW_HIP_LIB=os.path.abspath(lib)) if lib else None
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--rounds", str(rounds), "--warmup", str(warmup)]
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        print(f"step {name!r} failed with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-4000:]}", flush=True)
        return None
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--step")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib")
    args = ap.parse_args()
    if args.step:
        shape, op, side = args.step.split(":")
        step(shape, op, side, args.rounds, args.warmup)
        return 0
    if not args.out or not args.parent_lib:
        ap.error("OUT and --parent-lib")
    fmt = lambda v: f"{v[0]:9.1f} ({v[1]:8.1f} .. {v[2]:8.1f})"  # noqa: E731
    lines = [HEAD, "whole calls = host clock around the call or the n calls (each call ends in a device synchronise), profiler off, one context; a put's atlas is",
             f"reset before every round outside the clock; {args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds.", ""]
    ok, findings, first_win = True, [], {}
    for row, (shape, op) in enumerate((s, o) for o in OPS for s in SHAPES):
        order = ("batch", "single") if row % 2 == 0 else ("single", "batch")
        got = {}
        for side in order:
            got[side] = run_child(f"{shape}:{op}:{side}", args.rounds, args.warmup, args.parent_lib if side == "single" else None) if ok else None
            ok = ok and got[side] is not None
        w, h, formats, _, _ = SHAPES[shape]
        lines.append(f"{shape}: {w} x {h}, {len(formats)} format{'s' if len(formats) > 1 else ''}, {op}   ({order[0]} first)")
        if not ok:
            lines.append("    not measured")
            continue
        for leg, b in got["batch"].items():
            if leg in ("step", "launches"):
                continue
            s1 = got["single"][leg]
            n = int(leg)
            spread = s1[2] - s1[1]
            note = ""
            if n >= 4 and not b[0] < s1[0] - spread:
                note = "   FINDING: not faster than the single calls by more than their spread"
            if n == 1 and b[0] > s1[0] + spread:
                note = "   FINDING: slower than the single call beyond its spread"
            if note:
                findings.append(f"{shape} {op} n = {n}")
            if b[0] < s1[0] - spread and (shape, op) not in first_win:
                first_win[(shape, op)] = n
            lines.append(f"    n = {n:3d}   batch {fmt(b)}   {n:3d} single calls, parent {fmt(s1)}   single / batch = {s1[0] / b[0]:6.2f}   batch - single = {b[0] - s1[0]:9.1f}   launches {got['batch']['launches'][leg]}{note}")
        print("\n".join(lines[-6:]), flush=True)
    lines += ["", "the least n of a row's shape at which the batch beats the parent's n single calls by more than their p90 - p10: "
              + (", ".join(f"{s} {o}: {n}" for (s, o), n in first_win.items()) if first_win else "none")]
    lines += ["rows that miss their condition (n >= 4: faster than the parent's n single calls by more than that row's p90 - p10; n = 1: no slower beyond it): "
              + (", ".join(findings) if findings else "none")]
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
