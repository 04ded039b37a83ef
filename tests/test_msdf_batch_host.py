"""A batch of distance-field glyphs in one call (fdh_put_glyph_outlines, include_glyphs/figdraw_hip_glyphs.h), what a CPU can check: the header and the
C ABI; on record-only contexts the packing, the validation of the whole batch before anything is placed and the growth of the atlas, each
against single calls of fdh_put_glyph_outline; and the source of the four batched kernels of k_msdf.hip under the sequential host shim of
tests/emu (tests/msdf_batch_emu) against the single launchers of the same file.  Everything here is equality."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import emu_build
import msdf_cases as MC
import msdf_overlap_cases as OC
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, GlyphOutline, HipContext

ROOT = MC.ROOT
HEADER = os.path.join(ROOT, "include_glyphs", "figdraw_hip_glyphs.h")
NEW_API = ("fdh_put_glyph_outlines", "fdh_glyph_batch_stats", "fdh_sizeof_glyph_outline")
INVALID = -1
LCD_FILTER, LCD_CONTEXT, MTSDF, CORRECT, OVERLAP = 1, 2, 4, 8, 32
SQUARE = MC.poly([(2, 2), (10, 2), (10, 9), (2, 9)])
TRIANGLE = MC.poly([(2, 2), (10, 2), (6, 9)])
NONE = np.zeros((0, 6), np.float32)


def square(w, h):
    """a square with a margin of 1/4 of the image, at least 0.25: it fits a 1 x 1 image too, mostly outside it"""
    mx, my = max(w / 4.0, 0.25), max(h / 4.0, 0.25)
    return MC.poly([(mx, my), (w - mx, my), (w - mx, h - my), (mx, h - my)])


def small_shapes():
    """the sizes at which the tile table, a partial tile and the level-0 rule for 1-texel fields can go wrong, a 0-segment glyph between them"""
    out = []
    for w, h in ((1, 1), (9, 1), (1, 9), (8, 8), (7, 9), (17, 23)):
        out += [(f"{w} x {h}", square(w, h), w, h, 2), (f"0 segments after {w} x {h}", NONE, 5, 3, 4)]
    return out[:-1]


# ------------------------------------------------------------------------------------------------------------------ header and ABI
def test_header_declares_and_library_exports_the_batch_api():
    src = open(HEADER).read()
    assert re.search(r'#include "(\.\./include/)?figdraw_hip\.h"', src)
    assert "figdraw_hip_glyphs.h" not in os.listdir(os.path.join(ROOT, "include"))  # include/ keeps the headers it had
    declared = re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", src)
    assert sorted(declared) == sorted(NEW_API)
    L = context.load()
    for name in NEW_API:
        assert hasattr(L, name), name
    assert L.fdh_sizeof_glyph_outline() == C.sizeof(GlyphOutline) == 32
    main = open(os.path.join(ROOT, "include", "figdraw_hip.h")).read()
    assert not any(re.search(r"\b%s\b" % n, main) for n in NEW_API[1:]) and not re.search(r"FDH_API[^;]*fdh_put_glyph_outlines", main)
    assert "figdraw_hip_glyphs.h" in main and "it would be a new entry point" not in main  # the specification points to the new header


def test_glyphs_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "glyphs_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "glyphs_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "glyphs_abi_smoke: OK" in r.stdout
    src = open(os.path.join(ROOT, "tests", "glyphs_abi_smoke.c")).read()
    assert all(re.search(r"\b%s\b" % n, src) for n in NEW_API)


# ------------------------------------------------------------------------------------------------------------------ record-only contexts
def packed_area(ctx):
    area = C.c_int64(-1)
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def state(ctx, keys):
    return ctx.atlas_size(), packed_area(ctx), [ctx.has_image(k) for k in keys]


def test_record_only_packing_of_the_font_set():
    """the 106 font inputs as one batch, R = 4 and R = 2 through the per-glyph range, against 106 single calls"""
    inputs = MC.inputs()
    assert len(inputs) == 106 and {c[4] for c in inputs} == {2, 4}
    a, b = HipContext(record_only=True), HipContext(record_only=True)
    keys = [5000 + i for i in range(len(inputs))]
    rects = a.put_glyph_outlines([(k, segs, w, h, R) for k, (_, segs, w, h, R) in zip(keys, inputs)], sdf_range=8)
    singles = [b.put_glyph_outline(k, segs, w, h, mtsdf=True, sdf_range=R) for k, (_, segs, w, h, R) in zip(keys, inputs)]
    assert rects == singles
    assert state(a, keys) == state(b, keys) and all(state(a, keys)[2])
    st = a.glyph_batch_stats()
    assert st["glyphs"] == 106 and st["written"] == 106 and st["dropped_by_growth"] == 0 and st["launches"] == 0 and st["bytes_copied"] == 0
    a.close()
    b.close()


def _rc(ctx, glyphs, flags, null=False):
    """the C call itself -> status; glyphs: [(key, segs or None, n_segs or None, w, h, range)]"""
    arr = (GlyphOutline * max(len(glyphs), 1))()
    keep = []
    for g, (key, segs, n, w, h, R) in zip(arr, glyphs):
        segs = None if segs is None else np.ascontiguousarray(segs, np.float32).reshape(-1, 6)
        keep.append(segs)
        g.key, g.segs, g.width, g.height, g.sdf_range = key, (segs.ctypes.data if segs is not None and len(segs) else None), w, h, R
        g.n_segs = n if n is not None else len(segs)
    out = ((C.c_int * 4) * max(len(glyphs), 1))()
    return ctx.L.fdh_put_glyph_outlines(ctx.h, None if null else C.addressof(arr), len(glyphs), flags, C.addressof(out))


def test_validation_refuses_the_whole_batch():
    ctx = HipContext(record_only=True)
    ctx.put_glyph_outlines([(1, SQUARE, 12, 11)])
    keys = [1] + list(range(100, 140))
    before = state(ctx, keys)
    assert before[2] == [True] + [False] * 40
    good = lambda k: (k, SQUARE, None, 12, 11, 0)  # noqa: E731
    many = np.tile(TRIANGLE, (21845, 1))  # 65535 segments, the most one glyph takes
    assert len(many) == 65535
    refused = {
        "an open contour in the middle": ([good(100), (101, SQUARE[:3], None, 12, 11, 0), good(102)], MTSDF),
        "a range of 65": ([good(100), (101, SQUARE, None, 12, 11, 65), good(102)], MTSDF),
        "a range of 65 in the flags": ([good(100)], MTSDF | 65 << 8),
        "an LCD flag": ([good(100)], MTSDF | LCD_FILTER),
        "the other LCD flag": ([good(100)], MTSDF | LCD_CONTEXT),
        "no FDH_GLYPH_MTSDF": ([good(100)], 0),
        "a range alone": ([good(100)], 4 << 8),
        "FDH_GLYPH_MTSDF_CORRECT alone": ([good(100)], CORRECT),
        "FDH_GLYPH_MTSDF_OVERLAP alone": ([good(100)], OVERLAP),
        "an unknown flag": ([good(100)], MTSDF | 16),
        "a 4097-wide glyph": ([good(100), (101, SQUARE, None, 4097, 11, 0)], MTSDF),
        "a 0-high glyph": ([good(100), (101, SQUARE, None, 12, 0, 0)], MTSDF),
        "65536 segments in one glyph": ([good(100), (101, np.tile(SQUARE, (16384, 1)), None, 12, 11, 0)], MTSDF),
        "segments without a pointer": ([good(100), (101, None, 4, 12, 11, 0)], MTSDF),
        "a negative segment count": ([good(100), (101, None, -1, 12, 11, 0)], MTSDF),
        "2^24 + 1 texels": ([(100 + i, NONE, None, 2048, 2048, 0) for i in range(4)] + [(104, NONE, None, 1, 1, 0)], MTSDF),
        "2^20 + 1 segments": ([(100 + i, many, None, 12, 11, 0) for i in range(16)] + [(116, np.concatenate([TRIANGLE] * 3 + [SQUARE] * 2), None, 12, 11, 0)], MTSDF),
    }
    assert sum(len(g[1]) if g[1] is not None else 0 for g in refused["2^20 + 1 segments"][0]) == 2 ** 20 + 1
    for what, (glyphs, flags) in refused.items():
        assert _rc(ctx, glyphs, flags) == INVALID, what
        assert state(ctx, keys) == before, f"{what}: the context changed"
    assert _rc(ctx, [good(100)], MTSDF, null=True) == INVALID and state(ctx, keys) == before
    assert ctx.glyph_batch_stats()["glyphs"] == 1  # a refused call leaves the figures of the call before it
    with pytest.raises(FigdrawHipError) as e:
        ctx.put_glyph_outlines([(100, SQUARE, 12, 11), (101, SQUARE[:3], 12, 11)])
    assert e.value.code == INVALID and "put_glyph_outlines" in str(e.value)
    # n_glyphs = 0 is OK and changes nothing
    assert _rc(ctx, [], MTSDF) == 0 and _rc(ctx, [], MTSDF, null=True) == 0 and ctx.put_glyph_outlines([]) == []
    assert state(ctx, keys) == before and ctx.glyph_batch_stats()["glyphs"] == 0
    # at the limits, not over them: accepted (a second context: four 2048 x 2048 rectangles make the atlas grow)
    big = HipContext(record_only=True)
    assert _rc(big, [(100 + i, NONE, None, 2048, 2048, 0) for i in range(4)], MTSDF) == 0
    assert _rc(big, [(200 + i, many, None, 12, 11, 0) for i in range(16)] + [(216, np.tile(SQUARE, (4, 1)), None, 12, 11, 0)], MTSDF | CORRECT | OVERLAP) == 0
    assert big.has_image(216) and big.glyph_batch_stats()["glyphs"] == 17
    big.close()
    ctx.close()


def test_growth_is_what_single_calls_leave():
    """atlas size 64 and twelve 40 x 40 squares: every other placement grows the atlas and drops what was there"""
    a, b = HipContext(atlas_size=64, record_only=True), HipContext(atlas_size=64, record_only=True)
    keys = list(range(300, 312))
    rects = a.put_glyph_outlines([(k, square(40, 40), 40, 40) for k in keys], correct=True)
    singles = [b.put_glyph_outline(k, square(40, 40), 40, 40, mtsdf=True, correct=True) for k in keys]
    assert rects == singles and state(a, keys) == state(b, keys)
    lost = sum(not b.has_image(k) for k in keys)
    st = a.glyph_batch_stats()
    assert a.atlas_size() > 64 and 0 < lost < 12
    assert st["dropped_by_growth"] == lost and st["written"] == 12 - lost and st["glyphs"] == 12
    # a key put twice in one batch: two rectangles, the entry is the later one's
    r2 = a.put_glyph_outlines([(400, SQUARE, 12, 11), (400, SQUARE, 12, 11)])
    s2 = [b.put_glyph_outline(400, SQUARE, 12, 11, mtsdf=True) for _ in range(2)]
    assert r2 == s2 and r2[0] != r2[1] and state(a, keys + [400]) == state(b, keys + [400])
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------ the kernels' source on a CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_msdf.hip + fdh_msdf_host.h compiled as plain C++ with tests/msdf_batch_emu/emu.cpp under the sequential shim of tests/emu (64 lanes of
    a wave together, with the ballot) -> the directory of `wave` and of `wave_san`, the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "msdf_batch_emu", ("k_msdf.hip", "fdh_msdf_host.h"), {"wave": (), "wave_san": emu_build.SAN})


def batches():
    """-> {name: [(name, segs, w, h, R)]}: the 16 overlapping outlines; the 71 hostile ones and the small shapes"""
    return {"overlapping": [(n, s, w, h, 4) for n, s, w, h in OC.inputs()],
            "hostile and small": [c[:5] for c in MC.hostile_inputs()] + small_shapes()}


@pytest.mark.parametrize("exe", ["wave", "wave_san"])
@pytest.mark.parametrize("batch", ["overlapping", "hostile and small"])
def test_the_batched_kernels_under_a_host_shim(shim, exe, batch):
    """all four flag combinations: every glyph's bytes are the single launcher's, no pad between the fields is written, the correction's input is not"""
    glyphs = batches()[batch]
    assert len(glyphs) == {"overlapping": 16, "hostile and small": 71 + 11}[batch]
    with open(shim / f"{exe}.raw", "wb") as f:
        f.write(struct.pack("<i", len(glyphs)))
        for _, segs, w, h, R in glyphs:
            segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 6)
            f.write(struct.pack("<4i", w, h, R, len(segs)))
            f.write(segs.tobytes())
    r = subprocess.run(["./" + exe, f"{exe}.raw"], cwd=shim, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, f"{r.returncode} {r.stdout}{r.stderr}"
    for overlap in (0, 1):
        assert f"overlap {overlap}: generate: 0 of {len(glyphs)} glyphs differ; correct: 0 differ\n" in r.stdout
    tiles = sum(((w + 7) // 8) * ((h + 7) // 8) for _, _, w, h, _ in glyphs)
    assert re.search(r"glyphs %d tiles %d edges \d+" % (len(glyphs), tiles), r.stdout)
