#!/usr/bin/env python3
"""What video with an alpha plane costs on its way into the atlas and out of the frame (fdh_update_video_alpha, fdh_read_video_alpha;
include_video/figdraw_hip_video_alpha.h) on an MI355X, against its siblings without the plane -> profiles/video_alpha.txt.

  video_alpha_bench.py OUT --parent-lib LIB [--rounds N] [--warmup W]
  video_alpha_bench.py --step WxH:in|out[:siblings] [--rounds N] [--warmup W]      one step in this process; one JSON line

The protocol is that of tools/video_422_bench.py: a measurement is the host clock around whole calls -- every call ends in a device
synchronise -- on one context (atlas 4096 for the way in; one rendered frame over a transparent clear for the way out), N timed rounds
after W, median (p10 .. p90), the legs of a step alternating round by round in one process, at 1920 x 1080 and 3840 x 2160, planes
tightly packed in device memory.  The legs:
  the measuring stick: the sibling calls -- fdh_update_video_planes / fdh_read_video_planes for I420, I444, I410, fdh_update_video_422 /
      fdh_read_video_422 for UYVY -- in a process of their own (`:siblings`) on the PARENT commit's library (--parent-lib, through
      FIGDRAW_HIP_LIB), and once more beside the new calls on this tree's library as a control; on the way out also
      fdh_read_video_frame BGRA8 of the same frame;
  the new calls: A420, A444, A410, UYVA, each premultiplied and with FDH_VIDEO_STRAIGHT_ALPHA (`s`).
Every step is a child process under its own time limit, nothing is started after a failure, and what was not reached is written down
as "not measured".  There is no CPU fallback.

The hypotheses, stated before measuring:
  1. a premultiplied export costs its sibling's time times the ratio of the bytes moved -- the surface's 4 bytes a texel plus the planes'
     -- with the alpha plane and without: A420 6.5 / 5.5, A444 8 / 7, A410 12 / 10, UYVA 7 / 6; the margin is the spread (p90 - p10) of the
     sibling's own leg;
  2. the same for the imports (the atlas's level 0 takes the surface's place; the chain's bytes are the same on both sides);
  3. what the straight builds cost over the premultiplied ones is unknown -- three integer divisions a texel may well dominate: the
     ratio is reported, and a straight export at 3840 x 2160 that is slower than the BGRA8 export of the same frame is a lead, not a
     failure.
Whatever comes out is written down; nothing here gates a test."""
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

SIZES = ((1920, 1080), (3840, 2160))
STRAIGHT = 2
# leg -> (the call's family, format, bit depth, chroma: 0 = 4:2:0, 2 = 4:4:4, 3 = a UYVY plane, flags)
SIBLINGS = {"i420": ("planes", 3, 8, 0, 0), "i444": ("planes", 5, 8, 2, 0), "i410": ("planes", 6, 10, 2, 0), "uyvy": ("422", 10, 8, 3, 0)}
ALPHA = {"a420": ("alpha", 11, 8, 0, 0), "a420s": ("alpha", 11, 8, 0, STRAIGHT), "a444": ("alpha", 12, 8, 2, 0), "a444s": ("alpha", 12, 8, 2, STRAIGHT),
         "a410": ("alpha", 13, 10, 2, 0), "a410s": ("alpha", 13, 10, 2, STRAIGHT), "uyva": ("alpha", 14, 8, 3, 0), "uyvas": ("alpha", 14, 8, 3, STRAIGHT)}
# (the new leg, its sibling, bytes moved a texel with the alpha plane / without)
PAIRS = (("a420", "i420", 6.5 / 5.5), ("a444", "i444", 8 / 7), ("a410", "i410", 12 / 10), ("uyva", "uyvy", 7 / 6))


def step(w, h, side, siblings_only, rounds, warmup):
    import numpy as np
    from figdraw_amd.context import HipContext

    hip = C.CDLL("libamdhip64.so")

    def device(n, data=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
        if data is not None:
            assert hip.hipMemcpy(p, C.c_void_p(data.ctypes.data), C.c_size_t(n), 1) == 0
        return p.value

    ctx = HipContext(atlas_size=4096 if side == "in" else 512, device=0)
    assert w % 16 == 0 and h % 2 == 0
    rng = np.random.default_rng(w)
    legs = {}
    if side == "in":
        ctx.put_image(1, np.zeros((h, w, 4), np.uint8))  # one entry, key 1: every leg is an update of it
    else:
        img = rng.integers(0, 256, size=(256, 256, 4)).astype(np.uint16)  # premultiplied noise with every alpha over a transparent clear
        img[..., :3] = img[..., :3] * img[..., 3:] // 255
        ctx.put_image(1, img.astype(np.uint8))
        ctx.begin_frame(w, h, True, (0.0, 0.0, 0.0, 0.0))
        ctx.draw_rect((0.0, 0.0, w * 0.6, h * 0.5), (200, 40, 90, 255))
        for y in range(0, h, 256):
            for x in range(0, w, 256):
                ctx.draw_image(1, (float(x), float(y)), [(255, 255, 255, 255)] * 4, (256.0, 256.0))
        ctx.end_frame()
        ctx.sync()
        if not siblings_only:
            bgra = device(w * h * 4)
            legs["bgra8"] = lambda: ctx.read_video_frame(bgra, 0, 4 * w, 0, format=0, matrix=0, range=0)
    for name, (family, fmt, bits, chroma, flags) in {**SIBLINGS, **({} if siblings_only else ALPHA)}.items():
        es, dt = (1, np.uint8) if bits == 8 else (2, np.uint16)
        if chroma == 3:
            shapes, pitches = [(h, 2 * w)], [2 * w, 0, 0]
        else:
            cw, ch = (w, h) if chroma == 2 else (w // 2, h // 2)
            shapes, pitches = [(h, w), (ch, cw), (ch, cw)], [w * es, cw * es, cw * es]
        top = 256 if chroma == 3 else 1 << bits
        mk = (lambda s, es=es, dt=dt, top=top: device(int(np.prod(s)) * es, rng.integers(0, top, size=s).astype(dt))) if side == "in" else (lambda s, es=es: device(int(np.prod(s)) * es))
        ptrs = [mk(s) for s in shapes] + [0] * (3 - len(shapes))
        if family == "alpha":
            es_a = 2 if bits == 10 else 1
            a = device(w * h * es_a, rng.integers(0, 1 << bits, size=(h, w)).astype(dt)) if side == "in" else device(w * h * es_a)
            ptrs, pitches = ptrs + [a], pitches + [w * es_a]
        if side == "in":
            call = {"alpha": ctx.update_video_alpha, "422": ctx.update_video_422, "planes": ctx.update_video_planes}[family]
            legs[name] = lambda call=call, ptrs=ptrs, pitches=pitches, fmt=fmt, flags=flags: call(1, ptrs, w, h, pitches, format=fmt, flags=flags)
        else:
            call = {"alpha": ctx.read_video_alpha, "422": ctx.read_video_422, "planes": ctx.read_video_planes}[family]
            legs[name] = lambda call=call, ptrs=ptrs, pitches=pitches, fmt=fmt, flags=flags: call(ptrs, pitches, format=fmt, flags=flags)
    us = {leg: [] for leg in legs}
    for k in range(warmup + rounds):
        for leg, f in legs.items():
            ctx.sync()
            t1 = time.perf_counter()
            f()
            t2 = time.perf_counter()
            if k >= warmup:
                us[leg].append((t2 - t1) * 1e6)
    ctx.close()
    q = lambda v, f: sorted(v)[int(f * (len(v) - 1))]  # noqa: E731
    print(json.dumps({"step": f"{w}x{h}:{side}", **{leg: [statistics.median(v), q(v, 0.1), q(v, 0.9)] for leg, v in us.items()}}))


def run_child(name, rounds, warmup, lib=None, limit=240):
    """one step as a process of its own -> its JSON line; None: it failed.  lib: the library it loads (FIGDRAW_HIP_LIB)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--rounds", str(rounds), "--warmup", str(warmup)]
    env = dict(os.environ, **({"FIGDRAW_HIP_LIB": os.path.abspath(lib)} if lib else {}))
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        print(f"step {name!r} failed with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-4000:]}", flush=True)
        return None
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--step")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.step:
        size, side, *rest = args.step.split(":")
        w, h = (int(v) for v in size.split("x"))
        step(w, h, side, rest == ["siblings"], args.rounds, args.warmup)
        return 0
    if not args.out or not args.parent_lib:
        ap.error("OUT and --parent-lib")
    fmt = lambda v: f"{v[0]:9.1f} ({v[1]:8.1f} .. {v[2]:8.1f})"  # noqa: E731
    lines = ["tools/video_alpha_bench.py -- video with an alpha plane in (k_video_alpha_import, k_image_import_tail) and out (k_video_alpha_export), MI355X.",
             "whole calls = host clock around the call (each ends in a device synchronise), profiler off, one context; the way in: fdh_update_* of an",
             "entry in an atlas of 4096; the way out: one rendered frame, premultiplied noise with every alpha over a transparent clear; planes tightly",
             f"packed in device memory; {args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds; the legs of a step alternate round by round",
             "in one process.  `parent`: the sibling calls on the parent commit's library, a process of their own; `this tree`: the same calls as a",
             "control, bgra8 (fdh_read_video_frame), and the new calls, premultiplied and with FDH_VIDEO_STRAIGHT_ALPHA (s).",
             "hypotheses, stated before measuring:",
             "  1. a premultiplied export costs its sibling's (parent) time times the bytes moved with the alpha plane over those without -- a420 6.5 / 5.5,",
             "     a444 8 / 7, a410 12 / 10, uyva 7 / 6 -- within the spread (p90 - p10) of the sibling's own leg;",
             "  2. the same for the imports;",
             "  3. the straight builds' cost over the premultiplied ones is unknown (three integer divisions a texel may well dominate): the ratio is",
             "     reported; a straight export at 3840 x 2160 slower than bgra8 of the same frame is a lead (DESIGN.md section 8), not a failure.", ""]
    ok, verdicts = True, []
    for (w, h) in SIZES:
        for side in ("in", "out"):
            parent = run_child(f"{w}x{h}:{side}:siblings", args.rounds, args.warmup, lib=args.parent_lib) if ok else None
            ok = ok and parent is not None
            got = run_child(f"{w}x{h}:{side}", args.rounds, args.warmup) if ok else None
            ok = ok and got is not None
            lines.append(f"{w} x {h}, the way {side}" + ("" if got else ": not measured"))
            if not got:
                continue
            for where, legs in (("parent", parent), ("this tree", got)):
                for leg, v in legs.items():
                    if leg != "step":
                        lines.append(f"    {where:10s} {leg:8s} {fmt(v)}")
            for mine, sib, ratio in PAIRS:
                m, s = got[mine], parent[sib]
                allowed = s[0] * ratio + (s[2] - s[1])
                verdicts.append(f"{w} x {h} {side} {mine}: {m[0]:.1f} us against {sib} (parent) {s[0]:.1f} x {ratio:.3f} + spread {s[2] - s[1]:.1f} = {allowed:.1f}: hypothesis {1 if side == 'out' else 2} "
                                f"{'HOLDS' if m[0] <= allowed else 'FAILS'}; {mine} / {sib} = {m[0] / s[0]:.2f}")
                st = got[mine + "s"]
                verdicts.append(f"{w} x {h} {side} {mine}s: {st[0]:.1f} us, straight / premultiplied = {st[0] / m[0]:.2f}"
                                + (f"; against bgra8 {got['bgra8'][0]:.1f}: {'SLOWER, a lead' if st[0] > got['bgra8'][0] else 'not slower'}" if side == "out" else ""))
            print("\n".join(lines[-22:]), flush=True)
    lines += ["", "verdicts:"] + (["    " + v for v in verdicts] or ["    not measured"])
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
