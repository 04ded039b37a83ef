#!/usr/bin/env python3
"""bench.py -- BASELINE.json's headline metric on MI355X.

  metric   Mpixels/s composited @3840x2160 with the 300-rect scene (+ % of the HBM roofline)
  workload BASELINE.json configs[2]: examples/renderlist_100_common.nim restated at 3840x2160
           (300 shadowed SDF rects: 304 nodes -> ~700 draws) plus one full-frame nkBackdropBlur(18)
           ahead of the demo's own 360x240 blur node and overlay (SURVEY.md 8d "S300@4K")
  step     one frame through fdh_render_frame: the scene tree goes in, the RGBA8 surface comes out (C++ tree walk,
           draw records, 90 KB upload, binning, tile compositing, both blurs), as the reference's benchmark times
           renderFrame per frame (examples/windy_non_clip_benchmark.nim:113-147); frames_in_flight contexts per GPU.
  plain    `bench.py --gpus 1 --steps N --warmup W`: set up, pick the host-thread mode on short untimed batches, W frames of
           warm-up, ONE timed batch of exactly N frames, the headline line (`value`, `ms_per_step`, ...), nothing else.
           --dump-outputs DIR writes the frame of the last timed step.
  --full   everything else: the median of --repeats (default 7) batches and, measured after them, the in-flight and oracle
           checks, the same frames through the ~710-call BackendContext seam (`per_call_path`), the GPU work alone from
           resident records (`replay_resident_records`), one frame at a time, per-kernel times, rooflines, the retained
           path, the CPU baseline and, on N > 1 ranks, the gather legs

N > 1 (launched by torch.distributed.run, one rank per GPU), two ways to shard:
  --mode frames   (default) frames are independent, so rank r renders its own frames with no data-path collective --
                  weak scaling.  With --full, after the timed region the ranks' final frames are gathered to rank 0 with ONE RCCL
                  gather over xGMI; its time is reported separately and is not part of `value`.
  --mode stripes  BASELINE.json configs[4] (run it with --width 7680 --height 4320): a batch of 8 frames (frame = 0..7 in
                  rotation), every rank renders rows stripe_rows(H, N, r) of EVERY frame (with its redundant blur halo) and
                  the stripes of each frame are gathered into rank 0's image INSIDE the timed region (grouped RCCL send /
                  recv, pipelined one frame behind the rendering).  `value` = W*H*frames / wall including the gathers --
                  strong scaling; `gather_ms` is the part of the wall time rank 0 spent in them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s spec
# VALU issue peak: 256 CUs x 4 SIMDs, one wave64 VALU instruction per SIMD every 2 cycles (SIMD-32; tools/microbench/
# valu_rate.hip, raw output profiles/r02_valu_rate.txt: v_fma / v_add / v_rndne / v_cvt 0.99 ns = 2 cycles at the ~2.0 GHz the
# chip sustains under that load, v_exp / v_rcp / v_sqrt 3.4 ns = 4 slots, v_pk_fma_f32 2.0 ns = 2 slots, i.e. no gain over
# two plain FMAs) at the 2.4 GHz maximum clock.  Transcendentals count as one instruction and cost four slots, so a kernel
# full of them (this one: sqrt, exp, rcp per edge pixel) cannot reach frac = 1.
VALU_PEAK_GINST = 256 * 4 * 2.4 / 2.0
# FP32 vector peak (/opt/skills/guides/MI355X_MICROARCH.md): 256 CUs x 4 SIMDs x 64 lanes x 2 flops (FMA) per 2 cycles x 2.4 GHz
VALU_PEAK_TFLOPS = 157.3
# The host-thread calibration times batches of --steps frames, at most this many (~0.1 s at 4K): enough to rank the candidates,
# and the calibration stays within seconds whatever --steps is.
CALIBRATION_FRAMES = 2000


def frame_tensor(ctx):
    """Zero-copy torch view of the context's RGBA8 surface (H, W, 4) uint8."""
    import torch

    ptr, w, h, pitch = ctx.frame_device_ptr()

    class _Surf:
        __cuda_array_interface__ = {"shape": (h, w, 4), "typestr": "|u1", "data": (ptr, False), "version": 2,
                                    "strides": (pitch, 4, 1)}

    return torch.as_tensor(_Surf(), device=f"cuda:{ctx.device}")


DUMP_SAMPLE_PIXELS = 1 << 20  # 16 MB of float32 RGBA + 8 MB of float64 indices: a dump stays within 64 MB at any frame size


def dump_frame(out_dir, frame):
    """--dump-outputs: the (h, w, 4) RGBA8 frame the last timed step produced, as .npy files that the same command on another build
    can be compared with file for file (a 4K frame as float32 would be 133 MB, so the pixels are a fixed sample):
      frame_sample.npy        (n, 4) float32: RGBA of a seeded sample of n = min(h * w, DUMP_SAMPLE_PIXELS) pixels, in index order
      frame_sample_index.npy  (n,) float64: their flat indices y * w + x
      frame_row_sums.npy      (h, 4) float64: every row's channel sums over all of its pixels (exact)"""
    os.makedirs(out_dir, exist_ok=True)
    h, w = frame.shape[:2]
    n = min(h * w, DUMP_SAMPLE_PIXELS)
    idx = np.arange(h * w) if n == h * w else np.sort(np.random.default_rng(12345).choice(h * w, size=n, replace=False))
    np.save(os.path.join(out_dir, "frame_sample.npy"), frame.reshape(h * w, 4)[idx].astype(np.float32))
    np.save(os.path.join(out_dir, "frame_sample_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, "frame_row_sums.npy"), frame.sum(axis=1, dtype=np.float64))


def setup_comm(ctxs, dist, rank, world):
    """One RCCL communicator per process through the library's own C ABI (fdh_comm_*): rank 0 makes the id, torch.distributed
    carries the 128 bytes, the first context owns the communicator and the others borrow it."""
    from figdraw_amd.context import HipContext

    box = [HipContext.comm_unique_id() if rank == 0 else None]
    if dist is not None:
        dist.broadcast_object_list(box, src=0)
    ctxs[0].comm_init(box[0], rank, world)
    for c in ctxs[1:]:
        c.comm_share(ctxs[0])


def run_stripes(args, dist, rank, local_rank, world, on_host, gather):
    """BASELINE config 5: an 8-frame batch, each frame row-striped over the ranks, stripes gathered to rank 0 per frame.
    Every rank renders rows fdh_stripe_rows(H, world, rank) of EVERY frame through fdh_render_frame (tree in, rows out; the
    vertical blur halo is re-rendered, so nothing is exchanged while a frame renders) on frames_in_flight contexts, and each
    frame's stripes are gathered into rank 0's surface INSIDE the timed region:
      --gather c_abi (default with RCCL): fdh_gather_stripes -- grouped ncclSend / ncclRecv issued by the library on the context's
                     stream behind the frame's kernels, received in place into rank 0's own surface: no host synchronisation
                     per frame, no staging copy
      --gather torch (gloo self-test, or on request): torch.distributed grouped isend / irecv with a host sync per frame"""
    import torch

    from figdraw_amd import call_stream as CS  # noqa: F401  (the C player is not used here: per-frame gathers sit between the frames)
    from figdraw_amd import context as C_
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import make_render_tree_100
    from figdraw_amd.sharding import stripe_rows

    w, h = args.width, args.height
    NS = 8
    F = max(1, min(args.frames_in_flight, args.steps))
    y0, y1 = stripe_rows(h, world, rank)
    rows = [stripe_rows(h, world, r) for r in range(world)]
    scenes = [make_render_tree_100(w, h, frame=f, full_frame_blur=True) for f in range(NS)]
    cs = [sc.to_c() for sc in scenes]
    col = C_._F4(1.0, 1.0, 1.0, 1.0)
    ctxs = []
    for i in range(F):
        c = HipContext(device=local_rank)
        c.set_stripe(y0, y1)
        c.render_frame(scenes[i % NS], w, h)
        ctxs.append(c)
    for c in ctxs:
        c.sync()
    # (under gloo the library's gather only runs when a transport is named explicitly: FDH_RCCL_LIB -- the tests' stand-in for RCCL, which
    # refuses two ranks on one device)
    use_c_abi = gather == "c_abi" and (not on_host or bool(os.environ.get("FDH_RCCL_LIB")))
    use_host = gather == "host"
    dev = "cpu" if on_host else f"cuda:{local_rank}"
    gather_s = [0.0]
    ranks_seen = None
    if use_c_abi:
        setup_comm(ctxs, dist, rank, world)
        ranks_seen = ctxs[0].comm_info()[1]  # the communicator's size as fdh_comm_init left it: a SCALE record proves RCCL saw N ranks
    elif use_host:
        # the consumer is the host: every rank reads its own rows back over its own PCIe link (8 links in parallel on a node, no xGMI
        # fan-in into one GPU); pinned destination, one buffer per context
        stripe_host = [torch.empty((max(y1 - y0, 1), w, 4), dtype=torch.uint8).pin_memory() for _ in range(F)]
    else:
        full = [torch.zeros((h, w, 4), dtype=torch.uint8, device=dev) for _ in range(F)] if rank == 0 else None

    def gather_torch(i):
        """stripe of context i from every rank into rank 0's image: grouped send / recv (ncclGroupStart .. End under RCCL)"""
        t0 = time.perf_counter()
        ctxs[i].sync()
        mine = frame_tensor(ctxs[i])[y0:y1]  # (asked again per frame: a context alternates between two surfaces)
        if on_host:
            mine = mine.cpu()
        if rank == 0:
            full[i][y0:y1].copy_(mine, non_blocking=True)
            ops = [dist.P2POp(dist.irecv, full[i][a:b], r) for r, (a, b) in enumerate(rows) if r != 0 and b > a] if dist is not None else []
        else:
            ops = [dist.P2POp(dist.isend, mine, 0)] if y1 > y0 else []
        if ops:
            for req in dist.batch_isend_irecv(ops):
                req.wait()
        if not on_host:
            torch.cuda.current_stream().synchronize()
        gather_s[0] += time.perf_counter() - t0

    def run(n):
        pending = None
        for k in range(n):
            i = k % F
            c = ctxs[i]
            if not use_c_abi and pending is not None and pending == i:
                gather_torch(pending)  # (the surface is about to be overwritten)
                pending = None
            if use_host and k >= F and y1 > y0:  # the frame this context rendered F frames ago goes to the host before its surface is reused
                t0 = time.perf_counter()
                c._ck(c.L.fdh_read_pixels(c.h, 0, y0, w, y1 - y0, stripe_host[i].data_ptr()))
                gather_s[0] += time.perf_counter() - t0
            c._ck(c.L.fdh_render_frame(c.h, cs[k % NS].byref(), float(w), float(h), 1, col))
            if use_host:
                continue
            if use_c_abi:
                t0 = time.perf_counter()
                c.gather_stripes(0, None)  # queued on the context's stream behind the frame; rank 0 receives in place
                gather_s[0] += time.perf_counter() - t0
            else:
                if pending is not None:
                    gather_torch(pending)
                pending = i
        if pending is not None:
            gather_torch(pending)
        if use_host and y1 > y0:  # the last F frames' stripes
            t0 = time.perf_counter()
            for i in range(min(F, n)):
                ctxs[i]._ck(ctxs[i].L.fdh_read_pixels(ctxs[i].h, 0, y0, w, y1 - y0, stripe_host[i].data_ptr()))
            gather_s[0] += time.perf_counter() - t0

    def barrier():
        if dist is not None:
            dist.barrier()
        for c in ctxs:
            c.sync()
        torch.cuda.synchronize()

    def timed(steps):
        barrier()
        gather_s[0] = 0.0
        t0 = time.perf_counter()
        run(steps)
        for c in ctxs:
            c.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dist is not None:
            dist.barrier()
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt, gather_s[0]

    run(args.warmup)
    res = sorted(timed(args.steps) for _ in range(args.repeats))
    elapsed, gather_host = res[len(res) // 2]
    if rank != 0:
        for c in ctxs:
            c.close()
        return None
    last_k = args.steps - 1
    last_i = last_k % F
    # rank 0's image of the last frame: read back only for --full's checks and --dump-outputs
    got = None
    if use_host:
        got = stripe_host[last_i].numpy()[: y1 - y0]  # (every rank holds its own rows: rank 0's stripe is what it computed)
    elif args.full or args.dump_outputs:
        if use_c_abi:
            ctxs[last_i].W, ctxs[last_i].H = w, h
            got = ctxs[last_i].read_pixels()
        else:
            got = full[last_i].cpu().numpy()
        if args.full:
            assert int(got[..., 3].min()) == 255, "the gathered frame has unwritten pixels"
    if args.dump_outputs:
        dump_frame(args.dump_outputs, got)
    check = None
    if args.full and not args.no_cpu_baseline:  # the last frame against the oracle (outside the timed region)
        from oracle import oracle as O

        orc = O.Oracle(threads=min(os.cpu_count() or 1, 16))
        orc.render_frame(scenes[last_k % NS], w, h)
        if use_host:
            d = np.abs(got.astype(int) - orc.read_pixels()[y0:y1].astype(int))
            check = {"frame": last_k % NS, "rows_checked": [y0, y1], "parity_max_lsb": int(d.max()), "parity_pixels_differing": int((d.max(axis=2) > 0).sum())}
            if check["parity_max_lsb"] > 1:
                print(json.dumps({"error": "rank 0's stripe (read back by the host) disagrees with the oracle", "check": check}))
                sys.exit(1)
        else:
            d = np.abs(got.astype(int) - orc.read_pixels().astype(int))
            check = {"frame": last_k % NS, "parity_max_lsb": int(d.max()), "parity_pixels_differing": int((d.max(axis=2) > 0).sum())}
            if check["parity_max_lsb"] > 1:
                print(json.dumps({"error": "gathered frame disagrees with the oracle", "check": check}))
                sys.exit(1)
    st = ctxs[0].frame_stats()
    ms_step = 1e3 * elapsed / args.steps
    out = {
        "metric": f"Mpixels/s composited @{w}x{h}, 300 SDF rects+shadows, row-striped (BASELINE.json configs[4]; the headline metric is quoted at 3840x2160)",
        "value": round(w * h * args.steps / elapsed / 1e6, 1), "unit": "Mpixels/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 4), "repeats": args.repeats, "batches_ms": [round(1e3 * t, 4) for t, _ in res],
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"S300@8Kx8 (BASELINE.json configs[4]): 8-frame batch of the renderlist_100 scene at {w}x{h} with the full-frame blur, "
                               f"row-striped over {world} rank(s), every frame through fdh_render_frame, stripes gathered to rank 0 per frame inside the timed region",
                   "mode": "stripes", "draws": st.n_draws, "rows_per_rank": [b - a for a, b in rows], "frames_in_flight_per_gpu": F,
                   "gather": "fdh_gather_stripes (C ABI: grouped ncclSend / ncclRecv on the context's stream, received in place)" if use_c_abi
                             else "none: every rank reads its stripe back to pinned host memory over its own PCIe link (fdh_read_pixels); the consumer is the host" if use_host
                             else "torch.distributed batch_isend_irecv with a host sync per frame",
                   "rccl_ranks_seen": ranks_seen,
                   "parallelism": f"row stripes x{world}" if world > 1 else "single GPU (one stripe = the frame)"},
        "gather_ms": round(1e3 * gather_host / args.steps, 4),
        "gather_note": "per frame, this rank's HOST time inside the gather calls (c_abi: enqueue only -- the transfer runs on the stream; torch: includes "
                       "waiting for the stripe and the transfer; host: the blocking readback of the stripe rendered frames_in_flight frames earlier); "
                       "part of `value`'s wall time",
        "gathered_frame_check": check,
        "roofline": None, "cpu_baseline": None,
    }
    for c in ctxs:
        c.close()
    return out


class Watchdog:
    """A collective that never completes (a rank lost, a link down, a first-ever ncclSend / ncclRecv pair that hangs) must not take the
    figures measured before it along: after `seconds` every rank leaves with exit code 3, rank 0 printing `line()` first."""

    def __init__(self, seconds, rank, line):
        import threading

        def fire():
            if rank == 0:
                print(json.dumps(line()), flush=True)
            os._exit(3)

        self.t = threading.Timer(seconds, fire)
        self.t.daemon = True

    def __enter__(self):
        self.t.start()
        return self

    def __exit__(self, *exc):
        self.t.cancel()
        return False


def write_provisional(out):
    """rank 0, before the C-ABI gather leg: the line as it stands, where the launcher (self_launch) finds it if the ranks die in that leg"""
    try:
        os.makedirs(os.path.dirname(PROVISIONAL), exist_ok=True)
        json.dump(out, open(PROVISIONAL, "w"))
    except OSError:
        pass


def stripes_main(args, dist, rank, local_rank, world, on_host):
    """--mode stripes: one leg per gather.  With --gather both (the default on several ranks) the torch.distributed leg runs first and
    owns `value`; with --full the library's fdh_gather_stripes leg follows under the watchdog and is reported as `c_abi_gather`."""
    first = "torch" if args.gather == "both" else args.gather
    out = run_stripes(args, dist, rank, local_rank, world, on_host, first)
    if rank == 0:
        out["torch_world_size"] = dist.get_world_size() if dist is not None else 1
    if args.full and args.gather == "both" and world > 1:
        can = not on_host or bool(os.environ.get("FDH_RCCL_LIB"))
        if not can:
            if rank == 0:
                out["c_abi_gather"] = {"skipped": "gloo run with no stand-in transport named (FDH_RCCL_LIB): the library's gather needs RCCL, one GPU per rank"}
        else:
            if rank == 0:
                write_provisional(out)

            def late():
                return dict(out, c_abi_gather={"error": f"the fdh_gather_stripes leg did not complete within {args.gather_timeout} s; `value` (torch.distributed gather) was measured before it"})

            with Watchdog(args.gather_timeout, rank, late):
                try:
                    # (--dump-outputs holds the frame of the leg that owns `value`)
                    leg = run_stripes(argparse.Namespace(**dict(vars(args), dump_outputs=None)), dist, rank, local_rank, world, on_host, "c_abi")
                    if rank == 0:
                        out["c_abi_gather"] = {"value": leg["value"], "unit": leg["unit"], "ms_per_step": leg["ms_per_step"], "batches_ms": leg["batches_ms"],
                                               "gather_ms": leg["gather_ms"], "gather": leg["config"]["gather"], "rccl_ranks_seen": leg["config"]["rccl_ranks_seen"],
                                               "gathered_frame_check": leg["gathered_frame_check"]}
                        out["config"]["rccl_ranks_seen"] = leg["config"]["rccl_ranks_seen"]
                except Exception as e:  # (reported; `value` was measured through the other gather)
                    if rank == 0:
                        out["c_abi_gather"] = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0:
        print(json.dumps(out), flush=True)




def free_port():
    import socket

    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


PROVISIONAL = os.path.join(ROOT, "gpurun_out", "bench_provisional_line.json")


def self_launch(args, argv):
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment: start the N ranks as a CHILD (python -m torch.distributed.run,
    one rank per GPU) before this process has made any GPU call -- it never makes one --, relay rank 0's JSON line and the child's
    exit code.  Refuses (rc 4) a line whose n_gpus is not the N that was asked for."""
    import subprocess

    port = os.environ.get("MASTER_PORT") or str(free_port())
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.pop("MASTER_PORT", None)
    try:
        os.remove(PROVISIONAL)
    except OSError:
        pass
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.abspath(__file__)] + argv
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    rc = r.returncode
    if not lines and os.path.exists(PROVISIONAL):
        # the ranks died inside the C-ABI gather leg (after `value` and the torch gather were measured and written down)
        d = json.load(open(PROVISIONAL))
        d["c_abi_gather"] = {"error": f"the ranks exited with code {rc} inside the fdh_gather_* leg; `value` and the torch.distributed gather were measured before it"}
        lines = [json.dumps(d)]
        rc = rc or 3
    if not lines:
        sys.stderr.write(r.stdout[-4000:])
        sys.exit(rc or 1)
    line = lines[-1]
    try:
        n = json.loads(line).get("n_gpus")
    except ValueError:
        n = None
    print(line, flush=True)
    if n != args.gpus:
        sys.stderr.write(f"bench.py: asked for --gpus {args.gpus}, the line says n_gpus = {n}\n")
        sys.exit(rc or 4)
    sys.exit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks (one per GPU).  With no WORLD_SIZE in the environment and N > 1 this process starts them itself (a torch.distributed.run "
                         "child); under a launcher it must equal WORLD_SIZE")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=None,
                    help="timed batches of --steps frames each; the median batch is reported (default: 1, with --full 7)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the median of --repeats batches, the in-flight and oracle checks, the per-call, "
                         "resident-record and one-frame-at-a-time legs, per-kernel times, rooflines, the CPU baseline and the gather legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the frame the last timed step produced to DIR/*.npy (a seeded sample of its pixels, "
                         "float32, their indices and every row's channel sums)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for the 1-GPU self-test)")
    ap.add_argument("--all-ranks-on-device0", action="store_true", help="self-test of the N>1 code path on a 1-GPU box")
    ap.add_argument("--frames-in-flight", type=int, default=4,
                    help="independent render contexts per GPU (own stream + surfaces) whose frames overlap; 1 = strictly one frame at a time")
    ap.add_argument("--host-threads", type=int, default=0,
                    help="host threads driving the contexts of `value` (0 = one calling thread or one per context, whichever an untimed calibration "
                         "finds faster)")
    ap.add_argument("--gather", choices=["c_abi", "torch", "host", "both"], default=None,
                    help="who moves the finished rows / frames to rank 0: c_abi = the library's own fdh_gather_* (RCCL through the C ABI, stream-ordered, "
                         "north_star's single RCCL gather); torch = torch.distributed; host (--mode stripes) = no gather: every rank reads its stripe back "
                         "over its OWN PCIe link (fdh_read_pixels) -- the consumer is the host; both = the torch leg first (its figures are `value` / "
                         "`gather_ms`), then with --full the c_abi leg under a watchdog, reported beside it.  Default: c_abi on one rank, both on several")
    ap.add_argument("--gather-timeout", type=float, default=180.0, help="seconds the gather legs of an N > 1 run may take before they are given up")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--mode", choices=["frames", "stripes"], default=None,
                    help="frames: every rank renders whole frames (weak scaling); stripes: every rank renders its row stripe of every frame of an "
                         "8-frame batch and the stripes are gathered to rank 0 inside the timed region (BASELINE config 5, strong scaling)")
    ap.add_argument("--config", type=int, choices=[3, 5], default=3,
                    help="BASELINE.json configs by their 1-based number: 3 = the headline (S300@4K, frames mode); 5 = configs[4], S300@8Kx8: "
                         "--mode stripes --width 7680 --height 4320 --steps 8")
    ap.add_argument("--launch-check", action="store_true",
                    help="only prove the launch: the ranks meet (all-reduce of ones over --backend) and rank 0 prints n_gpus; no GPU call, no rendering")
    argv = sys.argv[1:]
    args = ap.parse_args()
    if args.config == 5:
        args.mode = args.mode or "stripes"
        args.width, args.height = args.width or 7680, args.height or 4320
        args.steps = args.steps or 8
    args.mode = args.mode or "frames"
    args.width, args.height = args.width or W, args.height or H
    args.steps = args.steps or 200
    args.repeats = args.repeats or (7 if args.full else 1)

    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus is None:
        args.gpus = int(env_world or "1")
    if env_world is None and args.gpus > 1:
        return self_launch(args, argv)  # (nothing above this line touches the GPU or imports torch)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(env_world or "1")
    if world != args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} under a launcher with WORLD_SIZE = {world}: refusing to print a line for the wrong N\n")
        sys.exit(4)
    if args.gather is None:
        args.gather = "c_abi" if world == 1 else os.environ.get("FDH_BENCH_GATHER", "both")
    if args.launch_check:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        seen = 1
        if world > 1:
            import torch

            dist.init_process_group("gloo" if args.backend != "nccl" else "nccl", rank=rank, world_size=world)
            t = torch.ones(1, dtype=torch.int64, device="cpu" if args.backend != "nccl" else f"cuda:{local_rank}")
            dist.all_reduce(t)
            seen = int(t.item())
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": world, "ranks_reduced": seen, "backend": args.backend}), flush=True)
        return
    import torch

    dist = None
    if args.all_ranks_on_device0:
        local_rank = 0
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(local_rank)
    on_host = dist is not None and args.backend != "nccl"  # gloo moves tensors through host memory
    if args.mode == "stripes":
        return stripes_main(args, dist, rank, local_rank, world, on_host)

    from figdraw_amd import call_stream as CS
    from figdraw_amd import context as C_mod
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import make_render_tree_100

    w, h = args.width, args.height
    # F contexts per GPU, each with its own stream, surfaces and submit thread: frames are independent, and one frame at a time
    # leaves the machine idle in every kernel's ramp and tail and in the small dependent launches that end a frame.
    F = max(1, min(args.frames_in_flight, args.steps))
    NS = 8  # distinct frames of the animation in rotation (rank r: frame = r + world * i)
    scenes = [make_render_tree_100(w, h, frame=rank + world * i, full_frame_blur=True) for i in range(NS)]
    cscenes = [sc.to_c() for sc in scenes]  # marshalled once: the timed loop hands the library FdhScene pointers
    scene = scenes[0]
    ctxs = [HipContext(device=local_rank) for _ in range(F)]
    ctx = ctxs[0]
    t_host0 = time.perf_counter()
    ctx.render_frame(scene, w, h)  # decomposition + upload + first GPU pass
    ctx.sync()
    t_host1 = time.perf_counter()
    for i, c in enumerate(ctxs[1:], 1):
        c.render_frame(scenes[i % NS], w, h)
        c.sync()
    player = CS.Player()  # tools/call_player.c: the frame loop in C, no Python between the library calls

    def sync_all():
        for c in ctxs:
            c.sync()
        torch.cuda.synchronize()

    def barrier():
        if dist is not None:
            dist.barrier()
        sync_all()

    def timed(fn, steps):
        """barrier + synchronize, `steps` frames, synchronize; MAX over ranks.  Seconds."""
        barrier()
        t0 = time.perf_counter()
        fn(steps)
        sync_all()
        dt = time.perf_counter() - t0
        if dist is not None:
            dist.barrier()
            tt = torch.tensor([dt], dtype=torch.float64, device="cpu" if on_host else f"cuda:{local_rank}")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt

    def batches(fn, steps, repeats):
        """`repeats` timed batches of exactly `steps` frames each; (median seconds, all of them in ms).  A 20-frame batch is a
        1.2 ms timed region: one of them says little, the median of five is stable."""
        ts = sorted(timed(fn, steps) for _ in range(repeats))
        return ts[len(ts) // 2], [round(1e3 * t, 4) for t in ts]

    # ---- THE PATH (`value`): scene tree in -> pixels out, every frame: fdh_render_frame = C++ tree walk + draw-record build +
    # upload + binning + both blurs + compositing, frame k of the animation on context k % F.  What the reference's benchmark
    # times per frame (examples/windy_non_clip_benchmark.nim:113-147: renderFrame(renders, frameSize)).
    # Who drives the contexts.  One calling thread walking every context's trees in turn (the reference's render loop, once per
    # window) or one host thread per context (an application with several windows): on a quiet host the single thread's even
    # round-robin interleaves the contexts' kernels slightly better, on a busy one its ~50 us of tree walk per frame fall behind
    # the GPU's rate and a thread per context is faster (profiles/README.md).  --host-threads 0 (default) tries both on untimed
    # batches and times the run with the faster; the line says which (`host_threads_per_gpu`, `host_threads_calibration`).
    def make_run(threads):
        def run(n):
            player.play_scenes(ctxs, cscenes, n, w, h, threads=threads)
        return run

    # ... and who walks the trees: the calling thread with the library's walk pool beside it (fdh_set_walk_threads, the default) or
    # the calling thread alone.  The bench frame is GPU-bound either way (host 25 - 30 us against 51 us per frame, GPU ~57): what
    # differs is how the four contexts' kernels interleave -- a host that is only just faster than the GPU keeps the queues short
    # and the frames staggered (docs/HISTORY.md section 4a) -- so the calibration tries both and says which it took (`walk_pool_threads`).
    calibration = None
    pool_default = ctx.walk_stats()[0]
    pool = pool_default
    if args.host_threads > 0:
        T = max(1, min(args.host_threads, F))
    else:
        calibration = {}
        n_cal = min(args.steps, CALIBRATION_FRAMES)
        for cand, pool_n in [(1, pool_default), (F, pool_default), (1, 0)]:
            key = f"{cand}" if pool_n == pool_default else f"{cand}, walk pool off"
            if key in calibration:
                continue
            for c in ctxs:
                c.set_walk_threads(pool_n)
            fn = make_run(cand)
            fn(min(max(args.warmup, args.steps), CALIBRATION_FRAMES))  # (a whole batch untimed first: a candidate's first batches carry its one-offs -- pool threads' first wake-up, staging growth)
            # (five batches: with two, one late wake-up of a pool thread in both 1.3-ms batches of the driver's command once put the
            # run on the slowest candidate -- 116.7 Gpixel/s where the runs before and after it measured 134 - 139.  And their MEDIAN,
            # round 5: a thread per context has the occasional fast batch and a slow typical one -- its best of five beat the single
            # thread's by 0.7 % in one driver-style run, which then measured 131.8 Gpixel/s against 144.8 - 148.9 on the same box)
            ts5 = sorted(timed(fn, n_cal) for _ in range(5))  # (max over ranks inside timed)
            calibration[key] = round(1e3 * ts5[2], 4)
        # the first candidate (one calling thread, the walk pool beside it: the library's default) unless another is clearly faster
        default_key = next(iter(calibration))
        best = min(calibration, key=lambda k: calibration[k])
        if calibration[best] > 0.98 * calibration[default_key]:
            best = default_key
        if best != default_key:
            # a second opinion before leaving the library's default (round 6: one driver-style run measured the default at 4.7 ms per batch
            # in calibration -- three of its five batches hit by something on the shared host --, took a thread per context and ran at
            # 146 Gpixel/s where the runs beside it, on the default, read 160 - 163): the default is measured again, and so is the winner
            for key, (cand, pool_n) in (("1", (1, pool_default)), (best, (int(best.split(",")[0]), 0 if "off" in best else pool_default))):
                for c in ctxs:
                    c.set_walk_threads(pool_n)
                fn = make_run(cand)
                fn(n_cal)
                again = sorted(timed(fn, n_cal) for _ in range(5))[2]
                calibration[key + ", second run"] = round(1e3 * again, 4)
                calibration[key] = min(calibration[key], round(1e3 * again, 4))
            if calibration[best] > 0.98 * calibration[default_key]:
                best = default_key
        T = int(best.split(",")[0])
        pool = 0 if "off" in best else pool_default
    for c in ctxs:
        c.set_walk_threads(pool)
    run_dynamic = make_run(T)
    run_dynamic(args.warmup)
    elapsed, batch_ms = batches(run_dynamic, args.steps, args.repeats)
    mpix = world * w * h * args.steps / elapsed / 1e6
    ms_step = 1e3 * elapsed / args.steps
    if args.dump_outputs and rank == 0:
        dump_frame(args.dump_outputs, ctxs[(args.steps - 1) % F].read_pixels())  # (the last timed step: frame steps - 1 on its context)

    def headline(st):
        """the fields of the line that every run prints: the figure, how it was timed, the workload"""
        return {
            "metric": "Mpixels/s composited @3840x2160, 300 SDF rects+shadows; % HBM roofline",
            "value": round(mpix, 1),
            "unit": "Mpixels/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_step, 4),
            "repeats": args.repeats,
            "batches_ms": batch_ms,
            "timing": (f"median of {args.repeats} timed batches of exactly {args.steps} frames each" if args.repeats > 1 else
                       f"one timed batch of exactly {args.steps} frames") + ", every batch bracketed by barrier + synchronize "
                      "(`batches_ms`: all of them, sorted); `value` = pixels of one batch / the median batch's wall time",
            "step": "one frame through fdh_render_frame: scene tree in -> RGBA8 surface out (C++ tree walk, draw records, upload, binning, both blurs, "
                    "compositing), frame k of the animation on context k % frames_in_flight; the loop is C (tools/call_player.c), on one calling thread or "
                    "one host thread per context, " + ("whichever an untimed calibration found faster on this host" if calibration is not None else
                                                       "as --host-threads sets it") + " (config.host_threads_per_gpu)",
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32 (blur taps: u8 x f16 -> f32 MFMA)",
            "data": "synthetic",
            "config": {"workload": f"S300@4K: renderlist_100 scene at {w}x{h}, 300 shadowed SDF rects + full-frame and 360x240 "
                                   f"2-pass Gaussian backdrop blur(18) (BASELINE.json configs[2])",
                       "draws": st.n_draws, "phases": st.n_phases, "blur_nodes": st.n_blurs, "fragments": int(st.fragments),
                       "parallelism": f"frame-parallel x{world}" if world > 1 else "single GPU", "frames_in_flight_per_gpu": F, "host_threads_per_gpu": T,
                       "walk_pool_threads": pool, "walk_pool_threads_default": pool_default},
            "host_threads_calibration": calibration,
        }

    if not args.full:  # a plain run stops here: everything below is --full's
        if rank == 0:
            print(json.dumps(headline(ctx.frame_stats())), flush=True)
        return
    # Integrity of the frames-in-flight mode (outside the timed region): every context must hold exactly the frame it
    # renders with the GPU to itself.  (Wrong pixels once came from a packed-FP32 misread beside another context's MFMAs:
    # DESIGN.md section 4.)  Context i rendered frame (last k with k % F == i) of the batch.
    in_flight_differing = 0
    in_flight_frames, in_flight_scene = [], []
    for i, c in enumerate(ctxs):
        k_last = max(k for k in range(max(args.steps - F, 0), args.steps) if k % F == i) if args.steps > i else None
        got_in_flight = c.read_pixels()
        in_flight_frames.append(got_in_flight)
        si = (k_last % NS) if k_last is not None else (i % NS)
        in_flight_scene.append(si)
        c.render_frame(scenes[si], w, h)
        c.sync()
        in_flight_differing += int((got_in_flight != c.read_pixels()).any(axis=2).sum())
    in_flight_vs_oracle = None
    for c in ctxs:
        c.set_walk_threads(-1)  # (the legs below run with the library's default)

    # ---- the same frames through the PER-CALL seam: ~710 fdh_draw_* calls between fdh_begin_frame / fdh_end_frame per frame,
    # issued from C (what a Nim HipContext shim behind figrender.nim would do: figbackend.nim:468-634)
    rec = HipContext(record_only=True)
    streams = []
    for sc in scenes:
        rec.record_begin()
        rec.render_frame(sc, w, h)
        calls = rec.record_calls()
        streams.append(CS.pack(calls))
    calls_per_frame = len(calls)
    rec.close()

    def run_calls(n):
        player.play_frames(ctxs, streams, n, w, h)

    run_calls(args.warmup)
    pc_elapsed, pc_batch_ms = batches(run_calls, args.steps, args.repeats)
    per_call_differing = 0
    for i, c in enumerate(ctxs):  # the per-call frames are the same frames: same pixels
        k_last = max(k for k in range(max(args.steps - F, 0), args.steps) if k % F == i) if args.steps > i else None
        if k_last is not None:
            got = c.read_pixels()
            c.render_frame(scenes[k_last % NS], w, h)
            c.sync()
            per_call_differing += int((got != c.read_pixels()).any(axis=2).sum())
    per_call = {"value": round(world * w * h * args.steps / pc_elapsed / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(1e3 * pc_elapsed / args.steps, 4),
                "batches_ms": pc_batch_ms, "calls_per_frame": calls_per_frame,
                "pixels_differing_from_fdh_render_frame": per_call_differing,
                "note": "the reference's plug-in seam: every BackendContext call of the frame (figbackend.nim:468-634) as one C-ABI call from "
                        "tools/call_player.c, fdh_begin_frame .. fdh_end_frame per frame, same contexts in flight"}
    st0 = ctx.frame_stats()

    # ---- resident records: the GPU side alone (binning + blurs + compositing of a frame whose records stay in HBM; no tree walk,
    # no upload).  Round 1 / 2's headline; here the ceiling the dynamic path is measured against.
    def run_replay(total):
        left = [total // F + (1 if i < total % F else 0) for i in range(F)]
        while any(left):
            for i, c in enumerate(ctxs):
                n = min(left[i], 4)
                if n:
                    c.replay_async(n)
                    left[i] -= n

    # (a short batch with all contexts in flight leaves each context's resident job as the dynamic leg's frames were recorded)
    run_dynamic(2 * F)
    sync_all()
    run_replay(args.warmup)
    rp_elapsed, rp_batch_ms = batches(run_replay, args.steps, args.repeats)
    replay = {"value": round(world * w * h * args.steps / rp_elapsed / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(1e3 * rp_elapsed / args.steps, 4),
              "batches_ms": rp_batch_ms, "note": "fdh_replay_async: the frame's GPU work from records already resident in HBM (no tree walk, no upload)"}

    # ---- strictly one frame at a time (the latency figures; also what the per-kernel numbers below refer to)
    def run_single_dynamic(n):
        player.play_scenes(ctxs[:1], cscenes, n, w, h)

    run_single_dynamic(args.warmup)
    sd_elapsed, sd_batch_ms = batches(run_single_dynamic, args.steps, args.repeats)
    # where the calling thread's time goes (one context, frames back to back): fdh_debug_host_times per frame, averaged
    acc = {}
    n_ht = min(args.steps, 100)
    for k in range(n_ht):
        ctx._ck(ctx.L.fdh_render_frame(ctx.h, cscenes[k % NS].byref(), float(w), float(h), 1, C_mod._F4(1.0, 1.0, 1.0, 1.0)))
        for name, v in ctx.host_times().items():
            acc[name] = acc.get(name, 0) + v
    ctx.sync()
    host_times_us = {name: round(v / n_ht / 1e3, 1) for name, v in acc.items()}
    ctx.render_frame(scene, w, h)
    ctx.replay(args.warmup)
    barrier()
    ts0 = time.perf_counter()
    ctx.replay(args.steps)
    ctx.sync()
    single_elapsed = time.perf_counter() - ts0
    st_batch = ctx.frame_stats()

    # per-frame distribution (SURVEY.md 8d timing protocol): one event between consecutive frames
    ft = ctx.replay_timed(min(args.steps, 120))
    frame_dist = {"n": int(len(ft)), "min": round(float(ft.min()), 4), "p50": round(float(np.percentile(ft, 50)), 4),
                  "p95": round(float(np.percentile(ft, 95)), 4), "max": round(float(ft.max()), 4)}
    # per-kernel durations, HIP events on the context's stream stamped by each launch itself (same frames, same records); the
    # full-frame blur node on both of its routes (same pixels): the fused kernel (the default) and two passes
    ctx.set_blur_route(1)
    ctx.render_frame(scene, w, h)
    ctx.replay(5)
    ctx.profile(min(args.steps, 50))
    st_fx = ctx.frame_stats()
    ctx.set_blur_route(0)
    ctx.render_frame(scene, w, h)
    ctx.replay(5)
    ctx.profile(min(args.steps, 50))
    st = ctx.frame_stats()
    ctx.set_blur_route(-1)

    dynamic = None
    if rank == 0:
        # the RETAINED path (fdh_scene_*): the tree lives in the context, one rectangle moves per frame, only its root
        # (and the two roots holding blur nodes) is decomposed again, every other root's records are spliced from the cache
        n_dyn = min(args.steps, 100)
        sc_r = make_render_tree_100(w, h, frame=0, full_frame_blur=True)
        ctx.scene_retain(sc_r, w, h)
        lst = next(iter(sc_r.layers.values()))
        moved = []
        for i in range(8):
            nd = lst.nodes[17]
            x0, y0, bw, bh = nd.screenBox
            nd.screenBox = (x0 + 3.0 * (i + 1), y0 + 2.0, bw, bh)
            moved.append(ctx._marshal_nodes([nd]))
            nd.screenBox = (x0, y0, bw, bh)
        for i in range(8):
            ctx._ck(ctx.L.fdh_scene_update_nodes(ctx.h, 0, 17, 1, moved[i & 7][1], moved[i & 7][3]))
            ctx._ck(ctx.L.fdh_scene_render(ctx.h))
        ctx.sync()
        tr = time.perf_counter()
        for i in range(n_dyn):
            ctx._ck(ctx.L.fdh_scene_update_nodes(ctx.h, 0, 17, 1, moved[i & 7][1], moved[i & 7][3]))
            ctx._ck(ctx.L.fdh_scene_render(ctx.h))
        ctx.sync()
        tr = time.perf_counter() - tr
        sr = ctx.frame_stats()
        walked, reused = ctx.scene_stats()
        dynamic = {"one_context": {"ms_per_frame": round(1e3 * sd_elapsed / args.steps, 4), "mpixels_per_s": round(w * h * args.steps / sd_elapsed / 1e6, 1), "batches_ms": sd_batch_ms},
                   "host_record_us": round(host_times_us["begin_frame"] - host_times_us["wait_upload"] + host_times_us["walk"] + host_times_us["end"], 1),
                   "host_prepare_us": host_times_us["prepare"],
                   "host_issue_us": round(1e3 * st0.ms_host_launch, 1), "host_times_us": host_times_us,
                   "note": "`value` IS this path with frames_in_flight contexts; host_*: per frame, the calling thread records (tree walk, large sibling "
                           "groups on the walk pool: config.walk_pool_threads) and prepares (layout, run table), the context's submit thread issues (upload "
                           "kernel + launches); host_record_us excludes what begin_frame waits for the GPU (host_times_us.wait_upload: back-pressure "
                           "when the host runs ahead); host_times_us: fdh_debug_host_times averaged over a batch of one-at-a-time frames",
                   "retained": {"ms_per_frame": round(1e3 * tr / n_dyn, 4), "mpixels_per_s": round(w * h * n_dyn / tr / 1e6, 1),
                                "host_record_us": round(1e3 * sr.ms_host_record, 1), "host_issue_us": round(1e3 * sr.ms_host_launch, 1),
                                "roots_walked": walked, "roots_reused": reused, "uploaded_bytes_per_frame": ctx.last_upload_bytes(),
                                "note": "one context: fdh_scene_update_nodes (one of 304 roots moves) + fdh_scene_render per frame: the edited root is decomposed again, "
                                        "the others' draw records come from the per-root cache; only the 256-byte chunks of the record block that changed are uploaded"}}
        ctx.render_frame(scene, w, h)  # back to the benchmark frame for the gather / parity legs below
        ctx.sync()

    # ---- the one collective of the path: the gather of finished frames to rank 0.  Frames are independent, so
    # `value` above holds no data-path collective (weak scaling); here (a) one gather of every rank's final frame, timed on its
    # own, and (b) the same K-frame batch with EVERY frame gathered to rank 0 inside the timed region, reported beside `value`.
    gather_ms, gather_how, gather_error = None, None, None
    if dist is not None and args.gather in ("torch", "both"):
        # (a) through torch.distributed -- the leg whose every call has run on real hardware before; measured FIRST
        def torch_leg_timed_out():
            return {"metric": "Mpixels/s composited @3840x2160, 300 SDF rects+shadows; % HBM roofline",
                    "value": round(world * w * h * args.steps / elapsed / 1e6, 1), "unit": "Mpixels/s", "n_gpus": world,
                    "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 4), "repeats": args.repeats,
                    "batches_ms": batch_ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                    "config": {"workload": f"S300@4K: renderlist_100 scene at {w}x{h} (BASELINE.json configs[2])",
                               "parallelism": f"frame-parallel x{world}", "frames_in_flight_per_gpu": F},
                    "gather": {"error": f"torch.distributed.gather of the frames to rank 0 did not complete within {args.gather_timeout} s; `value` (no collective "
                                        "on the data path) was measured before it"}}

        with Watchdog(args.gather_timeout, rank, torch_leg_timed_out):
            try:
                mine = frame_tensor(ctx).contiguous()
                if on_host:
                    mine = mine.cpu()
                outs = [torch.empty_like(mine) for _ in range(world)] if rank == 0 else None
                barrier()
                g0 = time.perf_counter()
                dist.gather(mine, outs, dst=0)
                torch.cuda.synchronize()
                gather_ms = 1e3 * (time.perf_counter() - g0)
                gather_how = f"torch.distributed.gather ({args.backend})"
                if rank == 0:
                    assert all(int(o[..., 3].min()) == 255 for o in outs), "a gathered frame has unwritten pixels"
                del outs
            except Exception as e:  # (reported, not fatal: `value` holds no collective)
                gather_error = f"{type(e).__name__}: {e}"

    def c_abi_leg():
        """(b) the library's own gather (fdh_gather_frames: grouped ncclSend / ncclRecv on the context's stream): one gather of every rank's
        final frame timed on its own, then the same K-frame batch with EVERY frame gathered to rank 0 inside the timed region."""
        setup_comm(ctxs, dist, rank, world)
        seen = ctxs[0].comm_info()[1]
        col = C_mod._F4(1.0, 1.0, 1.0, 1.0)
        dev = f"cuda:{local_rank}"
        slots = [[torch.empty((h, w, 4), dtype=torch.uint8, device=dev) for _ in range(world)] for _ in range(F)] if rank == 0 else None
        ptrs = [[t.data_ptr() for t in sl] for sl in slots] if rank == 0 else [None] * F
        ctx.render_frame(scene, w, h)
        barrier()
        g0 = time.perf_counter()
        ctx.gather_frames(0, ptrs[0])
        ctx.sync()
        ms = 1e3 * (time.perf_counter() - g0)
        if rank == 0:
            assert all(int(o[..., 3].min()) == 255 for o in slots[0]), "a gathered frame has unwritten pixels"
            # rank 0's own frame comes back through the gather as it sits in its surface
            assert bool((slots[0][0] == frame_tensor(ctx)).all()), "rank 0's own frame changed on its way through fdh_gather_frames"

        def run_with_gather(n):
            for k in range(n):
                c = ctxs[k % F]
                c._ck(c.L.fdh_render_frame(c.h, cscenes[k % NS].byref(), float(w), float(h), 1, col))
                c.gather_frames(0, ptrs[k % F])  # behind the frame on the context's stream: no host synchronisation

        run_with_gather(args.warmup)
        wg_elapsed, wg_batch_ms = batches(run_with_gather, args.steps, args.repeats)
        ctx.render_frame(scene, w, h)
        ctx.sync()
        return {"gather_ms": round(ms, 3), "gather": "fdh_gather_frames (C ABI: grouped ncclSend / ncclRecv on the context's stream)",
                "rccl_ranks_seen": seen,
                "with_gather_every_frame": {"value": round(world * w * h * args.steps / wg_elapsed / 1e6, 1), "unit": "Mpixels/s",
                                            "ms_per_step": round(1e3 * wg_elapsed / args.steps, 4), "batches_ms": wg_batch_ms,
                                            "note": "the same batch with every frame of every rank gathered to rank 0 (fdh_gather_frames) inside the timed region: "
                                                    f"rank 0 takes in {world - 1} x {w * h * 4 / 1e6:.1f} MB per round of frames over its xGMI links"}}

    c_abi_wanted = dist is not None and args.gather in ("c_abi", "both")
    c_abi_can = c_abi_wanted and (not on_host or bool(os.environ.get("FDH_RCCL_LIB")))
    if rank != 0:
        if c_abi_can:
            with Watchdog(args.gather_timeout, rank, dict):
                try:
                    c_abi_leg()
                except Exception:
                    pass  # (rank 0 reports its own side; a rank that failed here leaves rank 0 to the watchdog)
        return

    def hbm(bytes_, ms):
        gbs = bytes_ / (ms * 1e-3) / 1e9
        return {"achieved": round(gbs, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 5)}

    # Counters that cannot be collected inside this process (HBM bytes, instruction counts) come from the newest committed
    # rocprofv3 --pmc passes over this very command (tools/pmc_traffic.sh -> profiles/r*_pmc_traffic.json, corrected as
    # MI355X_MICROARCH.md prescribes) and are attached only when the workload is the one those passes profiled.
    pmc, pmc_src = {}, None
    try:
        import glob
        import hashlib

        from figdraw_amd import context as C_

        f = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))[-1]
        j = json.load(open(f))
        if (w, h) == (W, H) and 700 <= st.n_draws <= 715:
            pmc = j["kernels"]
            lib = os.environ.get("FIGDRAW_HIP_LIB", C_.LIB_PATH)
            sha = hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16]
            pmc_src = {"file": os.path.relpath(f, ROOT), "profiled_library_sha16": j.get("library_sha16"), "this_library_sha16": sha,
                       "same_build": j.get("library_sha16") == sha,
                       "note": "counters from the committed rocprofv3 --pmc passes, not measured in this run"}
    except Exception:
        pass

    # Dominant launch = k_composite_tiles, phase 0.  It is VALU-issue bound (it moves 4 B per pixel whatever the overdraw):
    # achieved = wave-level VALU instructions per launch (SQ_INSTS_VALU, PMC pass) / the launch's duration in THIS run.
    roofline = None
    if st.ms_composite_main > 0:
        k = pmc.get("k_composite_tiles.phase0", {})
        insts = k.get("SQ_INSTS_VALU")
        sec = st.ms_composite_main * 1e-3
        fm = list(st.fragments_main_by_mode)
        tflops = st.flops_composite_main / sec / 1e12
        # ALGORITHMIC figure first (flops per covered fragment by mode x the fragments this launch covers, over the
        # launch's duration measured in this run, against the FP32 vector peak); the instruction ISSUE rate beside it
        roofline = {"kernel": "k_composite_tiles<4, true>: the launch that starts a frame (every bin, from the clear colour; the build for phases "
                              "without clip operations) -- a row of its own in profiles/*_kernel_stats*.csv",
                    "ms_per_launch": round(st.ms_composite_main, 4),
                    "bound": "valu", "unit": "TFLOP/s", "peak": VALU_PEAK_TFLOPS, "achieved": round(tflops, 2), "frac": round(tflops / VALU_PEAK_TFLOPS, 4),
                    "algorithmic": {"flops_per_launch": int(st.flops_composite_main),
                                    "fragments_by_mode": {"ClipAA(3)": fm[0], "DropShadow(7)": fm[1], "InsetShadow(9)": fm[2], "AnnularAA(12)": fm[3],
                                                          "other": int(st.fragments_main_other), "of_which_elliptical_corners": int(st.fragments_main_elliptical)},
                                    "flops_per_fragment": {"ClipAA(3)": 25, "DropShadow(7)": 36, "InsetShadow(9)": 71, "AnnularAA(12)": 28, "other": 25,
                                                           "elliptical_corners": 30, "blend_and_requantise": 16},
                                    "note": "SURVEY.md 8(d) per-fragment flop counts (35 + exp, 70 + exp with exp as 1) x sum of quad areas per mode"},
                    "issue_rate": {"unit": "G wave-instructions/s", "peak": round(VALU_PEAK_GINST, 1),
                                   "achieved": round(insts / sec / 1e9, 1) if insts else None,
                                   "frac": round(insts / sec / 1e9 / VALU_PEAK_GINST, 4) if insts else None,
                                   "valu_instructions_per_launch": insts, "salu_instructions_per_launch": k.get("SQ_INSTS_SALU"),
                                   "issued_lane_ops_per_algorithmic_flop": round(insts * 64 / st.flops_composite_main, 3) if insts and st.flops_composite_main else None,
                                   "note": "SQ_INSTS_VALU per launch (PMC pass) / this run's launch time against one wave64 VALU instruction per SIMD per 2 cycles "
                                           "(1024 SIMDs x 2.4 GHz / 2); an issue rate, not an algorithmic fraction: more instructions would raise it"},
                    "traffic": k.get("hbm_bytes"), "traffic_source": pmc_src,
                    "hbm": dict(hbm(st.bytes_composite_main, st.ms_composite_main), algorithmic_bytes_per_launch=int(st.bytes_composite_main)),
                    "note": "fused tile compositor: VALU-bound (it moves 4 B/pixel out + 128 B/draw in by construction, `hbm`: ~0.1 of the HBM peak says nothing "
                            "about the kernel); the HBM-side launches are the blur passes (roofline, roofline_blur)"}
    # The HBM-bound launches: the two passes of the frame's largest blur node (full frame here), each against its own bytes
    roofline_blur = None
    if st.ms_blur_big_h > 0 and st.ms_blur_big_v > 0:
        bh, bv = int(st.bytes_blur_big_h), int(st.bytes_blur_big_v)
        both = hbm(bh + bv, st.ms_blur_big_h + st.ms_blur_big_v)
        th, tv = pmc.get("k_blur_mx.h", {}).get("hbm_bytes"), pmc.get("k_blur_mx.v", {}).get("hbm_bytes")
        roofline_blur = dict(both, bound="hbm", kernel="k_blur_mx<NK, false> + k_blur_mx<NK, true>: horizontal and vertical pass of the full-frame blur node (matrix pipe) -- the TWO-PASS route "
                                    "(fdh_set_blur_route(0)), profiled on its own; the frames of `value` take the one-kernel route, `fused_route` below",
                             ms_per_frame=round(st.ms_blur_big_h + st.ms_blur_big_v, 4), algorithmic_bytes_per_frame=bh + bv,
                             traffic=(th + tv) if th and tv else None, traffic_source=pmc_src,
                             passes={"horizontal": dict(hbm(bh, st.ms_blur_big_h), ms=round(st.ms_blur_big_h, 4), algorithmic_bytes=bh, traffic=th),
                                     "vertical": dict(hbm(bv, st.ms_blur_big_v), ms=round(st.ms_blur_big_v, 4), algorithmic_bytes=bv, traffic=tv)},
                             all_blur_launches_ms=round(st.ms_blur_h + st.ms_blur_v, 4),
                             arithmetic="v_mfma_f32_32x32x16_f16, f32 accumulate: RGBA8 texels as exact f16 subnormals x the taps as one f16 each at scale 2^10 "
                                        "(rounded from the centre tap outwards, the error carried from tap to tap; rounds 2 - 4: two halves, 22 bits, twice the MFMAs), "
                                        "every product exact; <= 1 LSB from the f32 FIR at ~0.1 % of a UI frame's pixels (DESIGN.md section 4)",
                             bytes_note="H: region + halo rows read and written; V: those rows read, the region written; the fused composite reads the "
                                        "surface only where it has to blend (the cleared opaque surface of this frame: nowhere but the quad's border blocks)")
    if roofline_blur is not None and st_fx.ms_blur_fused > 0:
        bfx = int(st_fx.bytes_blur_fused)
        roofline_blur["fused_route"] = dict(hbm(bfx, st_fx.ms_blur_fused), ms=round(st_fx.ms_blur_fused, 4), algorithmic_bytes=bfx,
                                            kernel="k_blur_fx<NKH, NKV>: both passes in one out-of-place kernel, the RGBA8 intermediate in LDS",
                                            traffic=pmc.get("k_blur_fx", {}).get("hbm_bytes"),
                                            survey_8d_bytes=dict(hbm(bh + bv, st_fx.ms_blur_fused), algorithmic_bytes=bh + bv,
                                                                 note="SURVEY.md 8(d) counts a blur node as H read + H write + V read + V write; this kernel "
                                                                      "produces that result without the intermediate's round trip through memory"),
                                            headline_route=True,
                                            note="the route every frame takes by default since the end of round 4 (fdh_set_blur_route(-1 | 1)): faster than the two "
                                                 "passes alone AND with four contexts in flight (tools/ab_routes.sh); `algorithmic_bytes` / `frac` are against "
                                                 "what IT must move (region read once + written once), half the two-pass figure; same pixels bit for bit")
    # `roofline` = the LONGEST launch of the route the frames of `value` take.  Since the end of round 4 that is the fused full-frame blur
    # (k_blur_fx), an HBM-side kernel: achieved = the bytes IT must move (the region read once + written once; SURVEY.md 8d's per-node figure
    # minus the intermediate's round trip, which this kernel does not make) / its launch duration measured in this run.  The compositor
    # -- the longest launch until then, VALU-bound -- stays beside it as `roofline_compositor`.
    roofline_main = roofline
    if roofline_blur is not None and "fused_route" in roofline_blur and st_fx.ms_blur_fused >= st.ms_composite_main:
        fr = roofline_blur["fused_route"]
        kfx = pmc.get("k_blur_fx", {})
        roofline_main = {"kernel": "k_blur_fx<NKH, NKV>: the fused full-frame backdrop blur (both separable passes in one out-of-place kernel, the RGBA8 intermediate "
                                   "in registers) -- the longest launch of a frame; a row of its own in profiles/*_kernel_stats*.csv",
                         "ms_per_launch": fr["ms"], "bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS, "achieved": fr["achieved"], "frac": fr["frac"],
                         "algorithmic_bytes_per_launch": fr["algorithmic_bytes"],
                         "algorithmic_note": "4 B x region pixels read + 4 B x region pixels written (one launch = one full-frame blur node of one frame)",
                         "traffic": fr.get("traffic"), "traffic_source": pmc_src,
                         "survey_8d_bytes": fr.get("survey_8d_bytes"),
                         "instruction_side": {"valu_instructions_per_launch": kfx.get("SQ_INSTS_VALU"), "mfma_busy_cycles_per_launch": kfx.get("SQ_VALU_MFMA_BUSY_CYCLES"),
                                              "note": "the kernel is not limited by HBM: its SIMDs' cycles go to the two matrix-pipe products (40 v_mfma_f32_32x32x16_f16 per "
                                                      "32 x 32 block since the end of round 5, 80 before) and the operand / pack VALU work around them (DESIGN.md section 4)"},
                         "second_longest": {"kernel": "k_composite_tiles<4, true>", "ms_per_launch": round(st.ms_composite_main, 4), "see": "roofline_compositor"}}
    elif roofline_blur is not None and "fused_route" in roofline_blur:
        # (end of round 5: with one MFMA per operand the fused blur is the SHORTER of the two large launches again; the compositor -- VALU-bound, the
        # FP32 vector peak its roofline -- is the longest and `roofline` is its; the blur stays in view here and in `roofline_blur.fused_route`)
        fr = roofline_blur["fused_route"]
        roofline_main = dict(roofline, second_longest={"kernel": "k_blur_fx<NKH, NKV>: the fused full-frame backdrop blur", "ms_per_launch": fr["ms"], "bound": "hbm",
                                                       "unit": "GB/s", "peak": HBM_PEAK_GBS, "achieved": fr["achieved"], "frac": fr["frac"],
                                                       "algorithmic_bytes_per_launch": fr["algorithmic_bytes"], "traffic": fr.get("traffic"), "see": "roofline_blur.fused_route"})
    # how the matrix-pipe blur kernels hold a tap: asked of the library itself (the lo halves of its weight fragments are zero in the one-f16 build)
    import ctypes as C

    _dense, _bits, _reach, _nk = (C.c_float * 160)(), (C.c_uint16 * (11 * 2 * 64 * 8))(), C.c_int(), C.c_int()
    ctx.L.fdh_blur_weight_fragments.argtypes = [C.c_float, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    weights_bits = None
    if ctx.L.fdh_blur_weight_fragments(18.0, 0, _dense, _bits, C.byref(_reach), C.byref(_nk)) == 0:
        fr_bits = np.frombuffer(_bits, dtype=np.uint16)[: _nk.value * 2 * 64 * 8].reshape(_nk.value, 2, 64, 8)
        weights_bits = 22 if fr_bits[:, 1].any() else 11
    if roofline_blur is not None:
        roofline_blur["weights_bits"] = weights_bits
        roofline_blur["weights"] = ("each tap ONE f16 at scale 2^10, rounding error carried to the next tap out; products u8 (as f16 subnormal) x f16 -> f32 accumulators on the "
                                    "matrix pipe; blur.frag computes in f32.  Worst case 255 sum|w - w^| = 0.09 LSB per pass before the RGBA8 rounding "
                                    "(tests/test_abi_and_sharding.py); on white noise / a 1-px checkerboard vs blur.frag on SwiftShader: profiles/r06_blur_weights_pin.txt")
    frame_gbs = st.bytes_algorithmic / (ms_step * 1e-3) / 1e9
    single_dyn_ms = 1e3 * sd_elapsed / args.steps
    single_gbs = st.bytes_algorithmic / (single_dyn_ms * 1e-3) / 1e9

    cpu_baseline = None
    if world == 1 and not args.no_cpu_baseline:
        from oracle import oracle as O

        # the oracle parallelises each draw over rows; beyond ~16 threads the per-draw fork/join dominates
        cores = min(os.cpu_count() or 1, 16)
        orc = O.Oracle(threads=cores)
        c0 = time.perf_counter()
        n_frames = 0
        while True:  # bounded sample: whole frames of the same workload until >= 12 s of CPU work
            orc.render_frame(scene if n_frames == 0 else make_render_tree_100(w, h, frame=n_frames, full_frame_blur=True), w, h)
            n_frames += 1
            dt = time.perf_counter() - c0
            if dt >= 12.0 or n_frames >= 64:
                break
        cpu_baseline = {"value": round(n_frames * w * h / dt / 1e6, 3), "unit": "Mpixels/s", "cores": cores, "kind": "port", "threads_cap": 16,
                        "threads_cap_reason": "the oracle is GL-structured on purpose (one full pass over the quad per draw, rows split over threads, a join per draw: "
                                              "it is the checker and mirrors the reference's draw-by-draw blending); past ~16 threads the 700 fork/joins per frame cost "
                                              f"more than the rows they save.  Host has {os.cpu_count()} hardware threads",
                        "sample": f"{n_frames} frames (frame = 0..{n_frames - 1}) of the same {w}x{h} scene ({st.n_draws} draws each), "
                                  f"oracle/figdraw_oracle.c, OpenMP over rows, {dt:.1f} s"}
        if n_frames > 1:  # parity check below compares frame 0
            orc.render_frame(scene, w, h)

        got = ctx.read_pixels()
        d = np.abs(got.astype(int) - orc.read_pixels().astype(int))
        cpu_baseline["parity_max_lsb"] = int(d.max())
        cpu_baseline["parity_pixels_differing"] = int((d.max(axis=2) > 0).sum())
        if F > 1:  # one of the frames that were rendered IN FLIGHT (kept from before the re-render above) against the oracle
            orc.render_frame(scenes[in_flight_scene[F - 1]], w, h)
            d = np.abs(in_flight_frames[F - 1].astype(int) - orc.read_pixels().astype(int))
            in_flight_vs_oracle = {"context": F - 1, "animation_frame": rank + world * in_flight_scene[F - 1], "parity_max_lsb": int(d.max()),
                                   "parity_pixels_differing": int((d.max(axis=2) > 0).sum())}

    out = dict(headline(st), **{
        "frames_in_flight_check": {"contexts": F, "identical_to_each_frame_rendered_alone": in_flight_differing == 0,
                                   "pixels_differing": in_flight_differing, "in_flight_frame_vs_oracle": in_flight_vs_oracle},
        "per_call_path": per_call,
        "replay_resident_records": replay,
        "one_frame_at_a_time": {"value": round(w * h * args.steps / sd_elapsed / 1e6, 1), "unit": "Mpixels/s (this rank)",
                                "ms_per_step": round(single_dyn_ms, 4), "batches_ms": sd_batch_ms,
                                "replay_resident_records": {"value": round(w * h * args.steps / single_elapsed / 1e6, 1), "ms_per_step": round(1e3 * single_elapsed / args.steps, 4)},
                                "note": "one context: fdh_render_frame per frame (the submit thread still overlaps frame n's launches with frame n + 1's tree walk)"},
        "roofline": roofline_main,
        "roofline_compositor": roofline,
        "roofline_blur": roofline_blur,
        "frame": {"algorithmic_bytes": int(st.bytes_algorithmic), "achieved_GBs": round(frame_gbs, 1),
                  "frac_of_hbm_peak": round(frame_gbs / HBM_PEAK_GBS, 5),
                  "one_frame_at_a_time": {"achieved_GBs": round(single_gbs, 1), "frac_of_hbm_peak": round(single_gbs / HBM_PEAK_GBS, 5)},
                  "gfragments_per_s": round(world * st.fragments * args.steps / elapsed / 1e9, 2),
                  "ms_event_timed": round(st_batch.ms_total, 4), "ms_per_frame_dist": frame_dist,
                  "gl_equivalent_bytes": int(8 * st.fragments),  # 8 B x fragments: what a GL rasteriser's blend RMW moves; context only

                  "kernel_ms": {"bin": round(st.ms_bin, 4), "composite_all": round(st.ms_composite, 4),
                                "composite_main": round(st.ms_composite_main, 4), "blur_h": round(st.ms_blur_h, 4),
                                "blur_v": round(st.ms_blur_v, 4)},
                  "host_decompose_upload_first_frame_ms": round(1e3 * (t_host1 - t_host0), 2)},
        "dynamic_path": dynamic,
        "cpu_baseline": cpu_baseline,
    })
    if gather_ms is not None:
        out["gather_ms"] = round(gather_ms, 3)
        out["gather"] = gather_how
    if gather_error is not None:
        out["gather_error"] = gather_error
    if world > 1:
        out["torch_world_size"] = dist.get_world_size()
        out["rccl_ranks_seen"] = None  # the communicator size fdh_comm_init reports (null: no fdh_gather_* leg ran)
    # a frame that came out differently in flight than alone (or off the oracle) voids the throughput figure
    bad = in_flight_differing != 0 or per_call_differing != 0 or (in_flight_vs_oracle is not None and in_flight_vs_oracle["parity_max_lsb"] > 1) or \
        (cpu_baseline is not None and cpu_baseline["parity_max_lsb"] > 1)
    if bad:
        out["value"] = None
        out["error"] = "frames rendered in flight differ from the same frames rendered alone, or from the oracle"
    if c_abi_wanted and not c_abi_can:
        out["c_abi_gather"] = {"skipped": "gloo run with no stand-in transport named (FDH_RCCL_LIB): the library's gather needs RCCL, one GPU per rank"}
    elif c_abi_can:
        # everything above is measured and written down before the first fdh_gather_* call between ranks
        write_provisional(out)

        def late():
            return dict(out, c_abi_gather={"error": f"the fdh_gather_frames leg did not complete within {args.gather_timeout} s; `value` (no collective on the "
                                                    "data path) and the torch.distributed gather were measured before it"})

        with Watchdog(args.gather_timeout, rank, late):
            try:
                leg = c_abi_leg()
                out["c_abi_gather"] = leg
                out["rccl_ranks_seen"] = leg["rccl_ranks_seen"]
                if gather_ms is None:  # (--gather c_abi: the library's gather is the only one)
                    out["gather_ms"], out["gather"] = leg["gather_ms"], leg["gather"]
                out["with_gather_every_frame"] = leg["with_gather_every_frame"]
            except Exception as e:
                out["c_abi_gather"] = {"error": f"{type(e).__name__}: {e}"}
    print(json.dumps(out), flush=True)
    if bad:
        sys.exit(1)


if __name__ == "__main__":
    main()
