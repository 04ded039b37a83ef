#!/usr/bin/env python3
"""What three-plane video costs on its way into the atlas and out of the frame (fdh_update_video_planes, fdh_read_video_planes;
include_video/figdraw_hip_video_planar.h) on an MI355X, against the semi-planar calls and against what an application does without the
planar ones -> profiles/video_planar.txt.

  video_planar_bench.py OUT [--rounds N] [--warmup W] [--trace-dir DIR]
  video_planar_bench.py --step WxH:in|out [--rounds N] [--warmup W]      one step in this process; one JSON line

The protocol is that of tools/video_frame_bench.py and tools/video_out_bench.py: a measurement is the host clock around whole calls --
every call ends in a device synchronise -- on one context (atlas 4096 for the way in; one rendered frame for the way out), N timed rounds
after W, median (p10 .. p90), the legs of a step alternating round by round in one process, at 1920 x 1080 and 3840 x 2160.  The legs:
  (a) the semi-planar calls as the parent commit has them (their translation units are untouched here): NV12 and P010;
  (b) the planar calls: I420, I010, I444, I410;
  (c) what an application does today: tools/microbench/planar_repack.hip -- one launch of its own on the context's stream that interleaves
      the two chroma planes (10 bit: and shifts every word, the luma plane's too) in front of (a)'s update, or splits (a)'s export
      behind it, the clock around both.
Before timing, a step checks that (b) and (c) leave the same bytes (level 0 of the atlas; the three planes).  --trace-dir: every step once
more under rocprofv3 --kernel-trace --stats, runs of their own, for the kernels' own times.  Every step is a child process under its own
time limit, nothing is started after a failure, and what was not reached is written down as "not measured".  There is no CPU fallback.

The hypothesis, stated before measuring: for 4:2:0, (b) beats (c) in both directions and at both sizes beyond the spread -- (c) reads and
writes the chroma planes (10 bit: the whole frame) once more and pays a second launch; and (b) lies within the spread of (a), which moves
the same bytes.  profiles/video_frame.txt records that the NV12 import is slower than the BGRA8 import although it reads fewer bytes; if
the planar import inherits that it shows as (b) = (a) > bgra8's figure there.  Whatever comes out is written down; nothing here gates a test."""
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
KERNELS = ("k_video_planar_import<", "k_video_planar_export<", "k_video_import<", "k_video_export<", "k_interleave<", "k_split<", "k_image_import_tail")
REPACK_SRC = os.path.join(ROOT, "tools", "microbench", "planar_repack.hip")
REPACK_LIB = os.path.join(ROOT, "build", "libplanar_repack.so")


def build_repack():
    if not os.path.exists(REPACK_LIB) or os.path.getmtime(REPACK_LIB) < os.path.getmtime(REPACK_SRC):
        os.makedirs(os.path.dirname(REPACK_LIB), exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", REPACK_SRC, "-o", REPACK_LIB])
    return REPACK_LIB


def step(w, h, side, rounds, warmup):
    import numpy as np
    from figdraw_amd.context import HipContext

    hip = C.CDLL("libamdhip64.so")
    repack = C.CDLL(build_repack())
    for f in (repack.planar_repack_interleave, repack.planar_repack_split):
        f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_long, C.c_long]

    def device(n, data=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
        if data is not None:
            assert hip.hipMemcpy(p, C.c_void_p(data.ctypes.data), C.c_size_t(n), 1) == 0
        return p.value

    def download(ptr, n):
        out = np.empty(n, np.uint8)
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(n), 2) == 0
        return out

    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    ctx = HipContext(atlas_size=4096 if side == "in" else 512, device=0)
    ctx.set_stream(stream.value)
    cw, ch = w // 2, h // 2
    assert w % 16 == 0 and h % 2 == 0
    rng = np.random.default_rng(w)
    legs = {}
    # per bit depth: Y, Cb, Cr planes, the semi-planar pair (luma, chroma) and the repack's scratch luma, all tightly packed in device memory
    bufs = {}
    for ten in (0, 1):
        es, dt = (2, np.uint16) if ten else (1, np.uint8)
        top = 1024 if ten else 256  # (clean 10-bit words: the repack kernel and the calls then agree on every bit)
        mk = (lambda shape: device(int(np.prod(shape)) * es, rng.integers(0, top, size=shape).astype(dt))) if side == "in" else (lambda shape: device(int(np.prod(shape)) * es))
        bufs[ten] = dict(y=mk((h, w)), cb=mk((ch, cw)), cr=mk((ch, cw)), cb4=mk((h, w)), cr4=mk((h, w)), luma=device(w * h * es), pairs=device(cw * ch * 2 * es), es=es)
    if side == "in":
        # one entry, key 1: every leg is an update of it (an update may change the format, not the size)
        ctx.put_video_planes(1, (bufs[0]["y"], bufs[0]["cb"], bufs[0]["cr"]), w, h, (w, cw, cw), format=3)
        rect = ctx.image_rect(1)
        entry = lambda: ctx.read_atlas_level(0)[rect[1]:rect[1] + h, rect[0]:rect[0] + w].copy()  # noqa: E731
        for ten, (sib, planar, full) in enumerate(((1, 3, 5), (2, 4, 6))):
            b, es = bufs[ten], bufs[ten]["es"]
            name = ("nv12", "i420", "i444") if not ten else ("p010", "i010", "i410")

            def a(b=b, es=es, sib=sib, ten=ten):
                ctx.update_video_frame(1, b["luma"] if ten else b["y"], b["pairs"], w, h, w * es, cw * 2 * es, format=sib)

            def c(b=b, ten=ten, a=a):
                assert repack.planar_repack_interleave(stream, ten, b["y"], b["luma"], b["cb"], b["cr"], b["pairs"], cw * ch, w * h) == 0
                a()

            def bb(b=b, es=es, planar=planar):
                ctx.update_video_planes(1, (b["y"], b["cb"], b["cr"]), w, h, (w * es, cw * es, cw * es), format=planar)

            c()
            want = entry()
            ctx.update_video_planes(1, (b["y"], b["cb4"], b["cr4"]), w, h, (w * es,) * 3, format=full)
            assert not np.array_equal(entry(), want)
            bb()
            assert np.array_equal(entry(), want), "(b) and (c) differ"
            legs[f"(a) {name[0]}"] = a
            legs[f"(b) {name[1]}"] = bb
            legs[f"(c) interleave + {name[0]}"] = c
            legs[f"(b) {name[2]}"] = lambda b=b, es=es, full=full: ctx.update_video_planes(1, (b["y"], b["cb4"], b["cr4"]), w, h, (w * es,) * 3, format=full)
    else:
        ctx.put_image(1, rng.integers(0, 256, size=(256, 256, 4)).astype(np.uint8))
        ctx.begin_frame(w, h, True, (0.1, 0.2, 0.3, 1.0))
        ctx.draw_rect((0.0, 0.0, w * 0.6, h * 0.5), (200, 40, 90, 255))
        for y in range(0, h, 256):
            for x in range(0, w, 256):
                ctx.draw_image(1, (float(x), float(y)), [(255, 255, 255, 255)] * 4, (256.0, 256.0))
        ctx.end_frame()
        ctx.sync()
        for ten, (sib, planar, full) in enumerate(((1, 3, 5), (2, 4, 6))):
            b, es = bufs[ten], bufs[ten]["es"]
            name = ("nv12", "i420", "i444") if not ten else ("p010", "i010", "i410")

            def a(b=b, es=es, sib=sib):
                ctx.read_video_frame(b["luma"], b["pairs"], w * es, cw * 2 * es, format=sib)

            def c(b=b, ten=ten, a=a):
                a()
                assert repack.planar_repack_split(stream, ten, b["luma"], b["y"], b["pairs"], b["cb"], b["cr"], cw * ch, w * h) == 0
                assert hip.hipStreamSynchronize(stream) == 0

            def bb(b=b, es=es, planar=planar):
                ctx.read_video_planes((b["y"], b["cb"], b["cr"]), (w * es, cw * es, cw * es), format=planar)

            c()
            want = [download(b["cb"], cw * ch * es), download(b["cr"], cw * ch * es)] + ([download(b["y"], w * h * es)] if ten else [])
            hip.hipMemset(C.c_void_p(b["cb"]), 0, C.c_size_t(cw * ch * es))
            bb()
            got = [download(b["cb"], cw * ch * es), download(b["cr"], cw * ch * es)] + ([download(b["y"], w * h * es)] if ten else [])
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), "(b) and (c) differ"
            legs[f"(a) {name[0]}"] = a
            legs[f"(b) {name[1]}"] = bb
            legs[f"(c) {name[0]} + split"] = c
            legs[f"(b) {name[2]}"] = lambda b=b, es=es, full=full: ctx.read_video_planes((b["y"], b["cb4"], b["cr4"]), (w * es,) * 3, format=full)
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


def run_child(name, rounds, warmup, limit=240, trace_dir=None):
    """one step as a process of its own -> its JSON line; under the profiler: {kernel: (launches, mean, least, most)} in us; None: it failed"""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--rounds", str(rounds), "--warmup", str(warmup)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", trace_dir, "-o", "t", "--"] + cmd
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print(f"step {name!r} failed with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-4000:]}", flush=True)
        return None
    if not trace_dir:
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    import csv
    import glob

    found = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if any(kernel in row["Name"] for kernel in KERNELS):
                found[row["Name"].split("(")[0]] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3)
    return found or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--step")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-dir")
    args = ap.parse_args()
    if args.step:
        size, side = args.step.split(":")
        w, h = (int(v) for v in size.split("x"))
        step(w, h, side, args.rounds, args.warmup)
        return 0
    if not args.out:
        ap.error("OUT")
    build_repack()
    fmt = lambda v: f"{v[0]:9.1f} ({v[1]:8.1f} .. {v[2]:8.1f})"  # noqa: E731
    lines = ["tools/video_planar_bench.py -- three-plane video in (k_video_planar_import, k_image_import_tail) and out (k_video_planar_export), MI355X.",
             "whole calls = host clock around the call (each ends in a device synchronise), profiler off, one context; the way in: fdh_update_* of an",
             "entry in an atlas of 4096; the way out: one rendered frame; planes tightly packed in device memory;",
             f"{args.rounds} timed rounds after {args.warmup}; median (p10 .. p90) in microseconds; the legs of a step alternate round by round in one process.",
             "(a) the semi-planar calls as the parent commit has them (their translation units are untouched); (b) the planar calls; (c) what an",
             "application does without them: tools/microbench/planar_repack.hip, one launch of its own that interleaves / splits the chroma planes",
             "(10 bit: and shifts the whole frame), in front of / behind (a)'s call, the clock around both.  (b) and (c) left the same bytes.",
             "hypothesis, stated before measuring: for 4:2:0, (b) beats (c) both ways at both sizes beyond the spread -- (c) moves the chroma planes",
             "(10 bit: the frame) once more and pays a second launch -- and (b) lies within the spread of (a).", ""]
    ok, verdicts = True, []
    for (w, h) in SIZES:
        for side in ("in", "out"):
            got = run_child(f"{w}x{h}:{side}", args.rounds, args.warmup) if ok else None
            ok = ok and got is not None
            lines.append(f"{w} x {h}, the way {side}" + ("" if got else ": not measured"))
            if not got:
                continue
            legs = {k: v for k, v in got.items() if k != "step"}
            for leg, v in legs.items():
                lines.append(f"    {leg:28s} {fmt(v)}")
            for b, c, a in (("(b) i420", "nv12", "(a) nv12"), ("(b) i010", "p010", "(a) p010")):
                cv = next(v for k, v in legs.items() if k.startswith("(c)") and c in k)
                bv, av = legs[b], legs[a]
                wins = bv[2] < cv[1]
                verdicts.append(f"{w} x {h} {side} {b[4:]}: (c) / (b) = {cv[0] / bv[0]:.2f}, (b) {'beats (c) beyond the spread (p90 of b < p10 of c)' if wins else 'does NOT beat (c) beyond the spread'}; (b) / (a) = {bv[0] / av[0]:.2f}")
            print("\n".join(lines[-7:]), flush=True)
    lines += ["", "the kernels alone, us per launch: mean (least .. most), rocprofv3 --kernel-trace --stats, a run of its own per step"]
    for (w, h) in SIZES:
        for side in ("in", "out"):
            got = run_child(f"{w}x{h}:{side}", args.rounds, args.warmup, trace_dir=os.path.join(args.trace_dir, f"{w}_{side}")) if ok and args.trace_dir else None
            ok = ok and (got is not None or not args.trace_dir)
            lines.append(f"{w} x {h}, the way {side}" + ("" if got else ": not measured"))
            for kernel, v in sorted((got or {}).items()):
                lines.append(f"    {kernel:64s} {v[1]:9.1f} ({v[2]:8.1f} .. {v[3]:8.1f}) over {v[0]} launches")
    lines += ["", "verdict on the hypothesis:"] + (["    " + v for v in verdicts] or ["    not measured"])
    if not ok:
        lines += ["", "INCOMPLETE: a step failed; nothing was started after it"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
