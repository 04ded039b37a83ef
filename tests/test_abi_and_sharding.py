"""CPU suite, part 2: the C-ABI library loads and exports every symbol include/figdraw_hip.h declares (no compute
calls without a GPU), fails loudly without a device, and the N>1 sharding path works over gloo (world_size 2)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "figdraw_hip.h")).read()
    return sorted(set(re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    from figdraw_amd import context

    context.build()
    lib = C.CDLL(context.LIB_PATH)
    names = _declared_symbols()
    assert len(names) >= 45
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    lib.fdh_version.restype = C.c_char_p
    assert b"gfx950" in lib.fdh_version()


def _header_param_counts():
    hdr = open(os.path.join(ROOT, "include", "figdraw_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for m in re.finditer(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_nim_shim_binds_what_it_calls():
    """INTEGRATION.md's Nim shim cannot be compiled here (no Nim toolchain).  What can be checked is: every fdh_* function it
    calls is declared with importc, and every importc declaration has as many parameters as the C declaration."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    shim = text[text.index("```nim") + 6:]
    shim = shim[:shim.index("```")]
    counts = _header_param_counts()
    declared = {}
    for m in re.finditer(r"proc (fdh_\w+)\((.*?)\): c(?:int|string) \{\.importc, cdecl\.\}", shim, flags=re.S):
        n = 0
        for group in m.group(2).split(";"):
            group = group.strip()
            if group:
                n += group.split(":")[0].count(",") + 1
        declared[m.group(1)] = n
    assert len(declared) >= 40
    for name, n in declared.items():
        assert name in counts, f"the shim imports {name}, which include/figdraw_hip.h does not declare"
        assert counts[name] == n, f"{name}: the shim's importc has {n} parameters, the header {counts[name]}"
    called = set(re.findall(r"\b(fdh_\w+)\(", shim))
    assert not (called - set(declared)), f"called without an importc declaration: {sorted(called - set(declared))}"
    # the BackendContext methods of SURVEY.md 8(b) the shim must override
    for method in ("beginFrame", "endFrame", "drawRoundedRectSdf", "drawImage", "drawMsdfImage", "drawMtsdfImage", "drawBackdropBlur", "beginMask",
                   "endMask", "popMask", "beginRectMask", "popRectMask", "readPixels", "putImage", "updateImage", "removeImage", "resetImageAtlas",
                   "translate", "rotate", "scale", "applyTransform", "saveTransform", "restoreTransform", "transformMirrorsY", "drawRect",
                   "drawFilledQuad", "drawQuadraticBezierSdf", "setTextSubpixelShift", "atlasPackedArea", "drawImageAdj",
                   "setTextLcdFilteringEnabled", "textLcdFilteringEnabled"):
        assert re.search(r"method %s\*\(ctx: HipContext" % method, shim), method


def test_abi_smoke_in_c99(tmp_path):
    """tests/abi_smoke.c: every entry point include/figdraw_hip.h declares, called from C99 on a FDH_CREATE_RECORD_ONLY context
    (no GPU needed).  A signature that drifts between header and library fails to compile or fails its checks here."""
    from figdraw_amd import context

    context.build()
    exe = tmp_path / "abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so", "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "img1.flippy")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "abi_smoke: OK" in r.stdout
    # the C file must mention every declared symbol
    src = open(os.path.join(ROOT, "tests", "abi_smoke.c")).read()
    missing = [n for n in _declared_symbols() if not re.search(r"\b%s\b" % n, src)]
    assert not missing, f"tests/abi_smoke.c does not call {missing}"


def test_call_player_builds_as_c99_and_rejects_bad_streams():
    """tools/call_player.c -- the C driver bench.py times -- compiles as strict C99 against the installed header (no GPU needed) and
    its stream reader refuses what it cannot parse instead of reading past the end."""
    import ctypes as C

    import numpy as np

    from figdraw_amd import call_stream as CS
    from figdraw_amd.context import HipContext

    lib = C.CDLL(CS.build_player(force=True))
    for name in ("fdh_play_calls", "fdh_play_frames", "fdh_play_scenes", "fdh_play_scenes_threads"):
        assert hasattr(lib, name), name
    rec = HipContext(record_only=True)
    player = CS.Player()
    rec.record_begin()
    ok = np.array([CS.OPS["begin_frame"], 1, 0x3F800000, 0x3F800000, 0x3F800000, 0x3F800000, CS.OPS["save_transform"], CS.OPS["restore_transform"],
                   CS.OPS["end_frame"]], dtype=np.uint32)
    player.play(rec, ok, 64, 48)
    assert [c[0] for c in rec.record_calls()] == ["begin_frame", "save_transform", "restore_transform", "end_frame"]
    for bad in (np.array([999], dtype=np.uint32),                                   # unknown op
                np.array([CS.OPS["draw_rect"], 0, 0], dtype=np.uint32)):            # arguments cut short
        assert player.P.fdh_play_calls(rec.h, bad.ctypes.data, bad.size, 64, 48) != 0
    rec.close()


def test_corrupt_flippy_files_are_refused_not_crashed():
    """fdh_put_flippy parses a file format (header, per-mip sizes, snappy streams: common/formatflippy.nim:77-149): flipped bytes,
    truncations and absurd lengths must come back as an error code or as an image -- never a read outside the buffer."""
    import random

    from figdraw_amd.context import FigdrawHipError, HipContext

    data = open(os.path.join(ROOT, "tests", "golden", "img1.flippy"), "rb").read()
    rnd = random.Random(1)
    ctx = HipContext(record_only=True, atlas_size=1024)
    ok = refused = 0
    for it in range(800):
        b = bytearray(data)
        mode = rnd.randrange(4)
        if mode == 0:
            for _ in range(rnd.randrange(1, 8)):
                b[rnd.randrange(len(b))] = rnd.randrange(256)
        elif mode == 1:
            b = b[:rnd.randrange(0, len(b))]
        elif mode == 2:
            b[rnd.randrange(0, 64)] = rnd.randrange(256)
        else:
            pos = rnd.randrange(len(b) - 4)
            b[pos:pos + 4] = bytes([255, 255, 255, 127])
        try:
            ctx.put_flippy(5000 + it % 7, bytes(b))
            ok += 1
        except FigdrawHipError:
            refused += 1
        if it % 200 == 199:  # (a fresh atlas now and then: accepted images fill it)
            ctx.close()
            ctx = HipContext(record_only=True, atlas_size=1024)
    ctx.close()
    assert ok > 50 and refused > 50


def test_built_code_object_passes_the_isa_lint():
    """Two properties of the gfx950 code inside the library that the parity tests can only catch by luck:
    no packed-FP32 instruction (misread on MI355X beside another wave's MFMAs), and no exec-mask write inside the draw loops of
    the compositor builds that are compiled with -structurizecfg-skip-uniform-regions.  csrc/Makefile runs the same check after
    every link; here it guards a library that was built some other way."""
    from figdraw_amd import context

    context.build()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_isa.py"), context.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "packed-FP32 instructions: 0" in r.stdout
    # (every instantiation: builds <0|2|4>, first launch of a frame or not, with or without the direct entries -- and the deep strips' launch)
    for build in [f"k_composite_tiles<{p}, {f}, {d}>" for p in (0, 2, 4) for f in ("true", "false") for d in ("true", "false")] + ["k_composite_deep<1>"]:
        assert f"{build}: no exec-mask write inside the draw loop nest" in r.stdout, r.stdout


def test_struct_layouts_match_python_mirror():
    from figdraw_amd import context, scene

    lib = context.load()
    assert lib.fdh_sizeof_fig() == C.sizeof(scene.CFig)
    assert lib.fdh_sizeof_glyph() == C.sizeof(scene.CGlyph)
    from oracle import oracle as O

    assert O.lib().fo_sizeof_fig() == C.sizeof(scene.CFig)


def test_no_cpu_fallback_without_a_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from figdraw_amd.context import FigdrawHipError, HipContext

    with pytest.raises(FigdrawHipError) as e:
        HipContext()
    assert e.value.code == -2  # FDH_ERR_NO_DEVICE


def test_null_handle_is_rejected_not_crashed():
    from figdraw_amd import context

    lib = context.load()
    assert lib.fdh_end_frame(None) == -1
    assert b"null" in lib.fdh_last_error()


def test_stripe_partition_properties():
    from figdraw_amd.sharding import frame_of_rank, stripe_rows

    for h in (1, 7, 8, 160, 375, 1080, 2160, 4320):
        for world in (1, 2, 3, 4, 8):
            rows = [stripe_rows(h, world, r) for r in range(world)]
            assert rows[0][0] == 0 and rows[-1][1] == h
            for (a0, b0), (a1, b1) in zip(rows, rows[1:]):
                assert b0 == a1 and a0 <= b0
            assert all(a % 8 == 0 or a == h for a, _ in rows)
    assert [frame_of_rank(s, 4, r) for s in range(2) for r in range(4)] == list(range(8))
    # the C ABI's partition rule (what a Nim host calls) is the same rule
    from figdraw_amd import context

    L = context.load()
    for h in (1, 7, 8, 160, 375, 1080, 2160, 4320):
        for world in (1, 2, 3, 4, 8):
            for r in range(world):
                y0, y1 = C.c_int(), C.c_int()
                assert L.fdh_stripe_rows(h, world, r, C.byref(y0), C.byref(y1)) == 0
                assert (y0.value, y1.value) == stripe_rows(h, world, r)


_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, torch, torch.distributed as dist
import ref_scenes as RS
from figdraw_amd.sharding import stripe_rows, gather_stripes
from oracle import oracle as O
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
w, h = 320, 240
o = O.Oracle(); o.render_frame(RS.backdrop_blur(float(w), float(h)), w, h)
full = o.read_pixels()
y0, y1 = stripe_rows(h, world, rank)
frame = gather_stripes(torch.from_numpy(full[y0:y1].copy()), h, dst=0)
if rank == 0:
    assert frame.shape == (h, w, 4)
    assert (frame.numpy() == full).all()
    print("GATHER_OK")
dist.destroy_process_group()
"""


def test_two_rank_gloo_stripe_gather(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29517", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "GATHER_OK" in outs[0]


def test_saturated_core_is_conservative_against_the_oracle():
    """Host logic, no GPU: the pixel rectangle the submission path marks as a draw's saturated core (fdh_saturated_core)
    must hold what the kernels assume there -- coverage exactly 1 for fills / drop-shadow bodies, exactly no effect for
    strokes and inner shadows -- checked on the oracle's pixels for random shapes with circular and elliptical corners at
    fractional positions."""
    import ctypes as C
    import random

    import numpy as np

    from figdraw_amd import context
    from oracle import oracle as O

    L = context.load()
    F4, F2, I4 = C.c_float * 4, C.c_float * 2, C.c_int * 4
    L.fdh_saturated_core.argtypes = [F4, F4, F4, C.c_int, C.c_float, C.c_float, F2, C.c_float, I4]
    rnd = random.Random(5)
    W, H, aa = 160, 120, 1.2
    bg = (0.2, 0.4, 0.6, 1.0)
    bg8 = np.array([51, 102, 153, 255], np.uint8)
    col = (250, 10, 30, 255)
    found = 0
    for it in range(120):
        w, h = rnd.uniform(20, 130), rnd.uniform(20, 100)
        x, y = rnd.uniform(2, W - w - 2), rnd.uniform(2, H - h - 2)
        m = min(w, h) / 2
        rx = [rnd.uniform(0, m) if rnd.random() < 0.7 else 0.0 for _ in range(4)]
        ry = list(rx) if rnd.random() < 0.6 else [rnd.uniform(0, m) for _ in range(4)]
        mode = rnd.choice([3, 3, 12, 11, 9, 7])
        factor = {3: 4.0, 12: rnd.choice([1.5, 4.0, 9.0]), 11: 3.0, 9: rnd.uniform(1, 12), 7: rnd.uniform(2, 16)}[mode]
        spread = rnd.uniform(0, 6) if mode in (7, 9) else 0.0
        rect, shape = (x, y, w, h), (0.0, 0.0)
        if mode == 7:  # drop shadow: padded quad around the shape (figrender.nim:654-689)
            pad = 1.5 * factor + spread + 1.0
            rect, shape = (x - pad, y - pad, w + 2 * pad, h + 2 * pad), (w, h)
        if mode == 9:
            shape = (rnd.uniform(-5, 5), rnd.uniform(-5, 5))  # inset: the shadow offset travels in shapeSize
        out = I4()
        assert L.fdh_saturated_core(F4(*rect), F4(*rx), F4(*ry), mode, factor, spread, F2(*shape), aa, out) == 0
        x0, y0, x1, y1 = out
        if x1 <= x0 or y1 <= y0:
            continue
        found += 1
        o = O.Oracle(threads=2)
        o.set_aa_factor(aa)
        o.begin_frame(W, H, True, bg)
        o.draw_rounded_rect_sdf(rect, [col] * 4, rx, ry, mode, factor, spread, shape)
        o.end_frame()
        core = o.read_pixels()[max(y0, 0):y1, max(x0, 0):x1]
        want = np.array(col, np.uint8) if mode in (3, 7) else bg8
        assert (core == want).all(), (it, mode, rect, rx, ry, factor, spread, shape, tuple(out))
    assert found > 60


def _krow(g, t, vertical):
    """row of a 16-texel k-step that element t of lane group g carries (mx_krow, figdraw_amd/csrc/fdh_types.h)"""
    return (t & 3) + 8 * (t >> 2) + 4 * g if vertical else 8 * g + t


def test_blur_weight_fragments_reproduce_the_fir():
    """Host logic, no GPU: the weight fragments of the matrix-pipe blur passes (fdh_blur_weight_fragments) are the banded
    Toeplitz form of the merged FIR: lane (j, g) of k-step m holds, for window texels 16 m + krow(g, t), the tap that texel
    meets at output j as ONE f16 at scale 2^10 (round 5; the second half's slot is zero): within half a step of the tap + what
    its inner neighbour carried over (the rounding error travels from the centre tap outwards), symmetric, zeros outside the
    band, and every output's weights sum to 2^10 x the taps' sum up to the outermost taps' (tiny) steps.  krow: 8 g + t for the horizontal pass; for the vertical one the order in which a 32 x 32
    accumulator tile holds its rows, (t & 3) + 8 (t >> 2) + 4 g (mx_krow, fdh_types.h: the fused kernel's horizontal product
    feeds the vertical one from registers) -- every row of a k-step exactly once either way."""
    import ctypes as C

    from figdraw_amd import context as ctx_mod

    L = ctx_mod.load()
    L.fdh_blur_weight_fragments.argtypes = [C.c_float, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    worst_bound = [0.0]
    for radius in (0.8, 3.0, 9.0, 18.0, 27.5, 40.0, 64.0, 100.0):
        for vertical in (0, 1):
            dense = (C.c_float * 160)()
            bits = (C.c_uint16 * (11 * 2 * 64 * 8))()
            reach, nk = C.c_int(), C.c_int()
            assert L.fdh_blur_weight_fragments(radius, vertical, dense, bits, C.byref(reach), C.byref(nk)) == 0
            r, n = reach.value, nk.value
            taps = np.array(dense[: 2 * r + 1], dtype=np.float64)
            assert abs(taps.sum() - 1.0) < 1e-5 and (taps >= 0).all() and np.allclose(taps, taps[::-1], atol=1e-7)
            delta = 0 if vertical else (-r) % 4
            assert 16 * n >= 32 + 2 * r + delta and n <= 11
            frag = np.frombuffer(bits, dtype=np.float16)[: n * 2 * 64 * 8].astype(np.float64).reshape(n, 2, 64, 8)
            assert (frag[:, 1] == 0).all()
            w = frag[:, 0]  # [k-step][lane][t]
            step = lambda v: 2.0 ** (np.floor(np.log2(max(v, 2.0 ** -14))) - 10)  # one f16 step at v
            per_output = np.zeros(32)
            abs_err = np.zeros(32)  # sum over an output's taps of |weight as multiplied - exact tap|, in units of 2^-10
            for m in range(n):
                for lane in range(64):
                    j, g = lane & 31, lane >> 5
                    for t in range(8):
                        k = 16 * m + _krow(g, t, vertical) - delta - j
                        want = taps[k] * 1024.0 if 0 <= k <= 2 * r else 0.0
                        # (its own rounding, half a step, + the error carried over from the tap inside it: at most half a step of the largest tap)
                        carried = 0.0 if k == r else 0.501 * step(1024.0 * taps.max())
                        assert abs(w[m, lane, t] - want) <= (0.501 * step(want) + carried if want else 0.0), (radius, vertical, m, lane, t, w[m, lane, t], want)
                        per_output[j] += w[m, lane, t]
                        abs_err[j] += abs(w[m, lane, t] - want)
            assert np.allclose(per_output, 1024.0 * taps.sum(), atol=2e-2), (radius, vertical, per_output[0])
            # The analytic worst case of one pass: a texel is at most 255, so an output's sum is off by at most 255 sum |w - w^| of a level
            # BEFORE it is rounded to RGBA8 -- whatever the content (noise, a checkerboard).  An eighth of a level per pass (measured: 0.092): the pass can
            # move a texel by one LSB only where the exact sum lies within that of a rounding tie, never by two; after two passes the
            # frame stays within 1 LSB of the float FIR's (the second pass smooths the first one's +-1 steps: sum w |e| <= 1, + 0.25),
            # which is what the GPU suite measures on hostile content (test_matrix_pipe_blur_on_hostile_content_matches_blur_frag).
            bound = 255.0 * abs_err.max() / 1024.0
            assert bound <= 0.125, (radius, vertical, bound)
            worst_bound[0] = max(worst_bound[0], bound)
            assert sorted(_krow(g, t, vertical) for g in range(2) for t in range(8)) == list(range(16))
    print(f"worst 255 sum|w - w^| over the radii: {worst_bound[0]:.4f} LSB per pass")


@pytest.mark.parametrize("radius", [1.0, 5.0, 18.0, 64.0])
def test_blur_weight_fragments_blur_like_the_reference(radius):
    """Host logic, no GPU: a numpy restatement of what the matrix-pipe passes compute -- weight * texel products summed,
    scaled by 2^-10, rounded to nearest even, RGBA8 between the passes, clamp-to-edge taps -- with the weight fragments the
    library builds, against the oracle's blur (max 1 LSB) and the reference's blur.frag on SwiftShader (max 2 LSB)."""
    import ctypes as C

    from conftest import diff_stats, load_png
    from figdraw_amd import context as ctx_mod
    from oracle import oracle as O

    L = ctx_mod.load()
    L.fdh_blur_weight_fragments.argtypes = [C.c_float, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    src = load_png("blur_src.png")
    img = src.astype(np.float64)
    for vertical in (0, 1):
        dense = (C.c_float * 160)()
        bits = (C.c_uint16 * (11 * 2 * 64 * 8))()
        reach, nk = C.c_int(), C.c_int()
        assert L.fdh_blur_weight_fragments(radius, vertical, dense, bits, C.byref(reach), C.byref(nk)) == 0
        r, n = reach.value, nk.value
        frag = np.frombuffer(bits, dtype=np.float16)[: n * 2 * 64 * 8].astype(np.float64).reshape(n, 2, 64, 8)
        delta = 0 if vertical else (-r) % 4
        # output 0 of a block (lane j = 0) meets window texel 16 m + 8 g + t with tap k = that - delta
        taps = np.zeros(2 * r + 1)
        for m in range(n):
            for g in range(2):
                for t in range(8):
                    k = 16 * m + _krow(g, t, vertical) - delta
                    if 0 <= k <= 2 * r:
                        taps[k] = frag[m, 0, 32 * g, t] + frag[m, 1, 32 * g, t]
        axis = 0 if vertical else 1
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        ext = np.pad(img, pad, mode="edge")
        acc = np.zeros_like(img)
        for k in range(2 * r + 1):
            sl = [slice(None)] * 3
            sl[axis] = slice(k, k + img.shape[axis])
            acc += taps[k] * ext[tuple(sl)]
        img = np.rint(acc / 1024.0)  # numpy rounds half to even, like v_cvt_pk_u8_f32
    got = img.astype(np.uint8)
    mx, n0, n1 = diff_stats(got, O.blur_image(src, radius))
    # (blur_src.png is noise -- mean second difference 150 levels -- the content on which the one-f16 weights' error pattern does NOT
    # cancel: 1.5 - 2.6 % of its pixels move, by one LSB; the scene tests, whose content is a UI's, keep the suite's 0.5 % bar)
    assert mx <= 1 and n0 <= 0.04 * src.shape[0] * src.shape[1], (radius, "vs oracle", mx, n0)
    mx, n0, n1 = diff_stats(got, load_png(f"ss_blur_r{radius:g}.png"))
    assert mx <= 2, (radius, "vs blur.frag on SwiftShader", mx, n0)


def _run_bench_two_ranks(extra, port):
    """bench.py's N > 1 path on a one-GPU box: two ranks on device 0, gloo for the process group (tensors go through host
    memory; RCCL needs one GPU per rank).  With --full: the checks and gather legs the callers read are --full's."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--all-ranks-on-device0", "--backend", "gloo", "--full"] + extra
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(2)]
    outs = [p.communicate(timeout=900) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1].decode()[-2000:] for o in outs]
    import json

    return json.loads([ln for ln in outs[0][0].decode().splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_stripes_mode_two_ranks_gathers_the_frame():
    """BASELINE config 5's run mode (row stripes + gather inside the timed region) through bench.py itself: the image rank 0
    assembles from the two ranks' stripes must be the oracle's frame."""
    d = _run_bench_two_ranks(["--mode", "stripes", "--width", "1920", "--height", "1080", "--steps", "9", "--warmup", "2"], 29531)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["mode"] == "stripes"
    assert sum(d["config"]["rows_per_rank"]) == 1080
    assert d["gathered_frame_check"]["parity_max_lsb"] <= 1 and d["gathered_frame_check"]["parity_pixels_differing"] < 0.005 * 1920 * 1080
    assert d["value"] > 0 and d["gather_ms"] > 0


def _mock_rccl():
    """tests/mock/mock_rccl.c -> build/libmock_rccl.so: the stand-in transport for the RCCL entry points fdh_comm.cpp binds"""
    out = os.path.join(ROOT, "build", "libmock_rccl.so")
    src = os.path.join(ROOT, "tests", "mock", "mock_rccl.c")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", src, "-o", out, "-L/opt/rocm/lib", "-lamdhip64",
                               "-lrt", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_stand_in_transport_exports_what_the_library_binds():
    """tests/mock/mock_rccl.c (CPU suite: it builds here, and offers every entry point fdh_comm.cpp looks up with dlsym)"""
    lib = C.CDLL(_mock_rccl())
    src = open(os.path.join(ROOT, "figdraw_amd", "csrc", "fdh_comm.cpp")).read()
    wanted = sorted(set(re.findall(r'sym\("(nccl[A-Za-z]+)"\)', src)))
    assert len(wanted) >= 10, wanted
    for name in wanted:
        assert hasattr(lib, name), name


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["stripes", "frames"])
def test_the_librarys_gather_between_two_ranks_over_a_stand_in_transport(mode):
    """The N > 1 branch of fdh_gather_stripes / fdh_gather_frames EXECUTED: two processes on device 0 (RCCL itself refuses that:
    "Duplicate GPU detected", tools/rccl_probe.py), the library bound to tests/mock/mock_rccl.c through FDH_RCCL_LIB -- sends are
    device-to-host copies into shared-memory mailboxes, receives the copies out.  What this proves is the library's side: which
    rows each rank sends, the in-place receives into rank 0's surface, four contexts per rank sharing one communicator (the lock,
    the issue order), fdh_comm_info reporting the communicator's own size.  It says nothing about RCCL or xGMI.  bench.py checks
    the assembled frame against the oracle (stripes) / every gathered frame for unwritten pixels (frames)."""
    env_lib = {"FDH_RCCL_LIB": _mock_rccl()}
    old = {k: os.environ.get(k) for k in env_lib}
    os.environ.update(env_lib)
    try:
        if mode == "stripes":
            d = _run_bench_two_ranks(["--mode", "stripes", "--gather", "c_abi", "--width", "1920", "--height", "1080", "--steps", "9", "--warmup", "2"], 29541)
            assert d["n_gpus"] == 2 and "fdh_gather_stripes" in d["config"]["gather"] and d["config"]["rccl_ranks_seen"] == 2
            assert sum(d["config"]["rows_per_rank"]) == 1080
            assert d["gathered_frame_check"]["parity_max_lsb"] <= 1 and d["gathered_frame_check"]["parity_pixels_differing"] < 0.005 * 1920 * 1080
        else:
            d = _run_bench_two_ranks(["--gather", "c_abi", "--width", "1280", "--height", "720", "--steps", "8", "--warmup", "2", "--no-cpu-baseline"], 29543)
            assert d["n_gpus"] == 2 and "fdh_gather_frames" in json.dumps(d) and d["frames_in_flight_check"]["pixels_differing"] == 0
        assert d["value"] > 0 and d["gather_ms"] > 0
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
def test_bench_stripes_mode_one_rank_gathers_through_the_c_abi():
    """the same run mode on ONE rank with the default gather: bench.py creates the RCCL communicator through fdh_comm_init
    (rank 0 of 1 -- what a 1-GPU box can execute of it) and issues fdh_gather_stripes behind every frame on the context's
    stream, no host synchronisation per frame; the frame left in rank 0's surface must be the oracle's."""
    import json

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "stripes", "--width", "1920", "--height", "1080", "--steps", "9",
                        "--warmup", "2", "--repeats", "2", "--full"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 1 and "fdh_gather_stripes" in d["config"]["gather"] and d["config"]["rows_per_rank"] == [1080]
    assert d["gathered_frame_check"]["parity_max_lsb"] <= 1 and d["value"] > 0
    assert "1920x1080" in d["metric"]


@pytest.mark.gpu
def test_bench_stripes_mode_with_the_host_as_consumer():
    """--gather host: no gather -- every rank reads its own stripe back to pinned host memory over its own PCIe link
    (fdh_read_pixels), the mode for a consumer that is the host.  One rank and two ranks (gloo carries only the barriers):
    rank 0's rows must be the oracle's, rccl_ranks_seen stays null (no communicator)."""
    import json

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "stripes", "--gather", "host", "--width", "1920", "--height", "1080",
                        "--steps", "9", "--warmup", "2", "--repeats", "2", "--full"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 1 and "own PCIe link" in d["config"]["gather"] and d["config"]["rccl_ranks_seen"] is None
    assert d["gathered_frame_check"]["parity_max_lsb"] <= 1 and d["gathered_frame_check"]["rows_checked"] == [0, 1080] and d["value"] > 0
    d = _run_bench_two_ranks(["--mode", "stripes", "--gather", "host", "--width", "1920", "--height", "1080", "--steps", "9", "--warmup", "2"], 29537)
    assert d["n_gpus"] == 2 and sum(d["config"]["rows_per_rank"]) == 1080
    assert d["gathered_frame_check"]["parity_max_lsb"] <= 1 and d["gathered_frame_check"]["rows_checked"][0] == 0


@pytest.mark.gpu
def test_bench_frames_mode_two_ranks():
    """bench.py's default N > 1 mode (frame-parallel, weak scaling) on two ranks."""
    d = _run_bench_two_ranks(["--width", "1280", "--height", "720", "--steps", "8", "--warmup", "2", "--no-cpu-baseline"], 29533)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert d["frames_in_flight_check"]["pixels_differing"] == 0
    assert d["value"] > 0 and d["gather_ms"] > 0


@pytest.mark.gpu
def test_c_abi_gather_on_one_rank():
    """fdh_comm_* / fdh_gather_*: what a 1-GPU box can execute of the RCCL path -- librccl loads, a one-rank communicator is
    created on the context's device, a second context borrows it, and both gathers deliver the destination rank's own rows /
    frame into a separate device image behind the frame's kernels (no host synchronisation in between)."""
    import ref_scenes as RS
    from figdraw_amd.context import HipContext

    w, h = 640, 360
    src, src2, dst = HipContext(device=0), HipContext(device=0), HipContext(device=0)
    dst.begin_frame(w, h, True, (0.0, 0.0, 0.0, 0.0))
    dst.end_frame()
    dst.sync()
    dptr = dst.frame_device_ptr()[0]
    uid = HipContext.comm_unique_id()
    assert len(uid) == 128 and any(uid)
    src.comm_init(uid, 0, 1)
    src2.comm_share(src)
    sc = RS.backdrop_blur(float(w), float(h))
    src.render_frame(sc, w, h)
    src.gather_stripes(0, dptr)  # queued behind the frame on src's stream
    src.sync()
    assert (dst.read_pixels() == src.read_pixels()).all()
    src2.render_frame(RS.nested_clips(float(w), float(h)), w, h)
    src2.gather_frames(0, [dptr])
    src2.sync()
    assert (dst.read_pixels() == src2.read_pixels()).all()
    # the communicator belongs to whoever still holds it: the context that created it may go first
    src.close()
    src2.render_frame(sc, w, h)
    src2.gather_frames(0, [dptr])
    src2.sync()
    assert (dst.read_pixels() == src2.read_pixels()).all()
    src2.close()
    dst.close()


def _bench(args, env=None, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout,
                       env={k: v for k, v in dict(os.environ, **(env or {})).items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


def test_bench_gpus_n_starts_n_ranks_itself():
    """`python bench.py --gpus 2` with no launcher around it (the driver's command form): bench.py starts the two ranks itself as a
    torch.distributed.run child before touching any GPU, relays rank 0's line and the child's exit code.  --launch-check stops after
    the ranks have met (all-reduce of ones over gloo): no GPU needed, so this runs in the CPU suite."""
    r, d = _bench(["--gpus", "2", "--backend", "gloo", "--launch-check"], timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert d == {"launch_check": True, "n_gpus": 2, "ranks_reduced": 2, "backend": "gloo"}
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("{")]) == 1  # ONE line
    # under somebody else's launcher --gpus must be the launcher's world size: a line for the wrong N is refused
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--launch-check"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode == 4 and "refusing" in r.stderr and not r.stdout.strip()
    # and with no --gpus at all a launcher's WORLD_SIZE is taken as it is (torch.distributed.run bench.py)
    r, d = _bench(["--launch-check"], timeout=120)
    assert r.returncode == 0 and d["n_gpus"] == 1


def test_bench_config_5_selects_the_baseline_stripes_run():
    """--config 5 = BASELINE.json configs[4] (S300@8Kx8): stripes mode, 7680x4320, 8 steps -- read off the parser (no GPU)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'args.width, args.height = args.width or 7680, args.height or 4320' in src and 'args.mode = args.mode or "stripes"' in src
    assert 'args.steps = args.steps or 8' in src


def test_bench_dump_of_a_4k_frame_is_a_fixed_sample_within_64_mb(tmp_path):
    """--dump-outputs (no GPU): a frame too large to write whole as float32 is written as the same seeded pixel sample every time,
    float32 / float64 only, at most 64 MB, plus row sums over every pixel; a frame that fits is written pixel for pixel."""
    sys.path.insert(0, ROOT)
    import bench

    h, w = 2160, 3840
    frame = np.random.default_rng(1).integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    for d in ("a", "b"):
        bench.dump_frame(str(tmp_path / d), frame)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["frame_row_sums.npy", "frame_sample.npy", "frame_sample_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert got[f].dtype in (np.float32, np.float64), f
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f)), f  # (the same sample on every run)
    idx = got["frame_sample_index.npy"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE_PIXELS and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < h * w
    assert np.array_equal(got["frame_sample.npy"], frame.reshape(-1, 4)[idx].astype(np.float32))
    assert np.array_equal(got["frame_row_sums.npy"], frame.astype(np.float64).sum(axis=1))
    small = frame[:360, :640]
    bench.dump_frame(str(tmp_path / "s"), small)
    assert np.array_equal(np.load(tmp_path / "s" / "frame_sample_index.npy"), np.arange(360 * 640))
    assert np.array_equal(np.load(tmp_path / "s" / "frame_sample.npy"), small.reshape(-1, 4).astype(np.float32))


@pytest.mark.gpu
def test_bench_plain_run_times_its_steps_and_dumps_the_last_frame(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W`: one timed batch of exactly N frames and the headline line only (what --full adds
    is absent); --dump-outputs holds the frame of the last timed step -- the same pixels a --full run dumps, and the oracle's."""
    from figdraw_amd.scenes import make_render_tree_100
    from oracle import oracle as O

    w, h, steps = 1280, 720, 6
    common = ["--gpus", "1", "--steps", str(steps), "--warmup", "2", "--width", str(w), "--height", str(h)]
    r, d = _bench(common + ["--dump-outputs", str(tmp_path / "plain")], timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == steps and d["repeats"] == 1 and len(d["batches_ms"]) == 1
    assert abs(d["batches_ms"][0] / steps - d["ms_per_step"]) < 1e-3
    for k in ("frames_in_flight_check", "per_call_path", "roofline", "cpu_baseline"):
        assert k not in d, k
    r, f = _bench(common + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f["repeats"] == 7 and f["frames_in_flight_check"]["pixels_differing"] == 0 and "per_call_path" in f
    names = ("frame_sample.npy", "frame_sample_index.npy", "frame_row_sums.npy")
    dump = {n: np.load(tmp_path / "plain" / n) for n in names}
    for n in names:
        assert np.array_equal(dump[n], np.load(tmp_path / "full" / n)), n
    # the last timed step is frame steps - 1 of the animation (rank 0 of 1); at 1280x720 the sample is every pixel
    orc = O.Oracle(threads=8)
    orc.render_frame(make_render_tree_100(w, h, frame=steps - 1, full_frame_blur=True), w, h)
    want = orc.read_pixels().reshape(-1, 4).astype(np.float32)
    assert np.array_equal(dump["frame_sample_index.npy"], np.arange(w * h))
    diff = np.abs(dump["frame_sample.npy"] - want)
    assert diff.max() <= 1 and (diff.max(axis=1) > 0).sum() <= 0.005 * w * h, (diff.max(), (diff.max(axis=1) > 0).sum())
    assert np.abs(dump["frame_row_sums.npy"] - want.reshape(h, w, 4).sum(axis=1)).max() <= w


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["frames", "config5"])
def test_bench_self_launch_runs_both_gather_legs(mode):
    """The command form the driver uses for a SCALE point -- `python bench.py --gpus 2 ...`, nothing around it -- on a one-GPU box: two
    ranks on device 0 over gloo, the library's gather bound to the stand-in transport.  One invocation, one line: n_gpus = 2, the
    torch.distributed gather leg (owns `value` / `gather_ms`), then the fdh_gather_* leg (`c_abi_gather`) with the communicator's own
    size next to torch's."""
    env = {"FDH_RCCL_LIB": _mock_rccl(), "MASTER_PORT": "29551" if mode == "frames" else "29553"}
    if mode == "frames":
        r, d = _bench(["--gpus", "2", "--backend", "gloo", "--all-ranks-on-device0", "--width", "1280", "--height", "720", "--steps", "8", "--warmup", "2",
                       "--repeats", "3", "--no-cpu-baseline", "--full"], env)
        assert r.returncode == 0, (r.stderr[-2000:], r.stdout[-2000:])
        assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["torch_world_size"] == 2 and d["rccl_ranks_seen"] == 2
        assert "torch.distributed.gather" in d["gather"] and d["gather_ms"] > 0
        leg = d["c_abi_gather"]
        assert "fdh_gather_frames" in leg["gather"] and leg["gather_ms"] > 0 and leg["with_gather_every_frame"]["value"] > 0
        assert d["frames_in_flight_check"]["pixels_differing"] == 0
    else:
        r, d = _bench(["--gpus", "2", "--backend", "gloo", "--all-ranks-on-device0", "--config", "5", "--width", "1920", "--height", "1080", "--warmup", "2",
                       "--repeats", "3", "--full"], env)
        assert r.returncode == 0, (r.stderr[-2000:], r.stdout[-2000:])
        assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 8 and d["config"]["mode"] == "stripes"
        assert d["torch_world_size"] == 2 and d["config"]["rccl_ranks_seen"] == 2
        assert "torch.distributed" in d["config"]["gather"] and d["gathered_frame_check"]["parity_max_lsb"] <= 1
        leg = d["c_abi_gather"]
        assert "fdh_gather_stripes" in leg["gather"] and leg["value"] > 0 and leg["gathered_frame_check"]["parity_max_lsb"] <= 1
    assert d["value"] > 0
