"""The two batches for outlines with cubic segments (fdh_put_glyph_outlines_cubic, fdh_put_glyph_coverage_batch_cubic;
include_glyphs/figdraw_hip_cubic_batch.h), what a CPU can check: the header and the C ABI; on record-only contexts the packing, the validation of
the whole batch before anything is placed, the growth of the atlas and a full atlas, each against single calls of
fdh_put_glyph_outline_cubic; and the source of the two batched kernels of k_msdf_cubic.hip under the sequential host shim of tests/emu
(tests/msdf_cubic_batch_emu) against the single launchers of the same file and of k_msdf.hip.  Everything here is equality."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import emu_build
import msdf_cases as MC
import msdf_cubic_cases as CC
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, GlyphOutline, HipContext

ROOT = MC.ROOT
HEADER = os.path.join(ROOT, "include_glyphs", "figdraw_hip_cubic_batch.h")
NEW_API = ("fdh_put_glyph_outlines_cubic", "fdh_put_glyph_coverage_batch_cubic")
INVALID, ATLAS_FULL = -1, -4
LCD_FILTER, LCD_CONTEXT, MTSDF, CORRECT, OVERLAP = 1, 2, 4, 8, 32
BOX = CC.cpath((2, 4), (4, -2, 8, 8, 10, 4), (10, 9), (2, 9), (2, 4))  # in 12 x 11: a box whose top side is a cubic
SQUARE6 = MC.poly([(2, 2), (10, 2), (10, 9), (2, 9)])
TRIANGLE6 = MC.poly([(2, 2), (10, 2), (6, 9)])
SQUARE, TRIANGLE = CC.lift(SQUARE6), CC.lift(TRIANGLE6)                # the 8-float format, no cubic
NONE = np.zeros((0, 8), np.float32)
SMALL = CC.cpath((1, 1), (5, -2, 10, 4, 8, 8), (1, 8), (1, 1))
DEVICE_ONLY = [("1 x 9", SMALL, 1, 9, 2), ("9 x 1", SMALL, 9, 1, 2), ("17 x 9", SMALL, 17, 9, 2), ("0 segments", NONE, 12, 11, 4)]  # test_msdf_cubic.py's


def cubic_square(w, h):
    """a closed shape of four cubics with a margin of 1/4 of the image"""
    mx, my = w / 4.0, h / 4.0
    return CC.circle(w / 2.0, h / 2.0, min(w / 2.0 - mx, h / 2.0 - my))


def mixed():
    """-> [(name, segs8, w, h, R)]: cubic glyphs of the skewed font set interleaved with cubic-free ones, per-glyph ranges 1, 2, 4, 64"""
    out = []
    for i, ((name, s8, w, h, _), (_, s6, w6, h6, _)) in enumerate(zip(CC.skewed()[3::9], MC.inputs()[4::9])):
        out += [(name, s8, w, h, (1, 2, 4, 64)[i % 4]), (name + " lifted", CC.lift(s6), w6, h6, (64, 4, 2, 1)[i % 4])]
    return out


# ------------------------------------------------------------------------------------------------------------------ header and ABI
def test_header_declares_and_library_exports_the_cubic_batches():
    src = open(HEADER).read()
    assert '#include "figdraw_hip_coverage.h"' in src and '#include "figdraw_hip_cubic.h"' in src
    assert "figdraw_hip_cubic_batch.h" not in os.listdir(os.path.join(ROOT, "include"))  # include/ keeps the headers it had
    declared = re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", src)
    assert sorted(declared) == sorted(NEW_API)
    assert "fdh_glyph_batch_stats" in src and "fdh_glyph_coverage_batch_stats" in src and "either" in src.lower()  # the stats calls report either format
    L = context.load()
    for name in NEW_API:
        assert hasattr(L, name), name
    main = open(os.path.join(ROOT, "include", "figdraw_hip.h")).read()
    assert not any(re.search(r"\b%s\b" % n, main) for n in NEW_API) and "figdraw_hip_cubic_batch.h" in main
    single = open(os.path.join(ROOT, "include_glyphs", "figdraw_hip_cubic.h")).read()
    assert "figdraw_hip_cubic_batch.h" in single and "both batches take the 6-float format only" not in single


def test_cubic_batch_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "cubic_batch_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "cubic_batch_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cubic_batch_abi_smoke: OK" in r.stdout
    src = open(os.path.join(ROOT, "tests", "cubic_batch_abi_smoke.c")).read()
    assert all(re.search(r"\b%s\b" % n, src) for n in NEW_API + ("fdh_glyph_batch_stats", "fdh_glyph_coverage_batch_stats"))


# ------------------------------------------------------------------------------------------------------------------ record-only contexts
def packed_area(ctx):
    area = C.c_int64(-1)
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def state(ctx, keys):
    return ctx.atlas_size(), packed_area(ctx), [ctx.has_image(k) for k in keys]


@pytest.mark.parametrize("which", ["the skewed font set", "a mixed list"])
def test_record_only_packing_is_the_single_calls(which):
    """both calls: rectangles, has_image, atlas_size and atlas_packed_area equal those of the single cubic calls in order; per-glyph ranges"""
    glyphs = CC.skewed() if which == "the skewed font set" else mixed()
    assert len(glyphs) == (106 if which == "the skewed font set" else 24)
    keys = [5000 + i for i in range(len(glyphs))]
    a, b = HipContext(record_only=True), HipContext(record_only=True)
    rects = a.put_glyph_outlines_cubic([(k, segs, w, h, R) for k, (_, segs, w, h, R) in zip(keys, glyphs)], sdf_range=8, correct=True)
    singles = [b.put_glyph_outline_cubic(k, segs, w, h, mtsdf=True, sdf_range=R, correct=True) for k, (_, segs, w, h, R) in zip(keys, glyphs)]
    assert rects == singles and state(a, keys) == state(b, keys) and all(state(a, keys)[2])
    st = a.glyph_batch_stats()
    assert st["glyphs"] == len(glyphs) and st["written"] == len(glyphs) and st["dropped_by_growth"] == 0 and st["launches"] == 0 and st["bytes_copied"] == 0
    assert a.glyph_coverage_batch_stats()["glyphs"] == 0  # figures of its own
    keys2 = [7000 + i for i in range(len(glyphs))]
    rects = a.put_glyph_coverage_batch_cubic([(k, segs, w, h) for k, (_, segs, w, h, _) in zip(keys2, glyphs)], lcd_filter=True)
    singles = [b.put_glyph_outline_cubic(k, segs, w, h, lcd_filter=True) for k, (_, segs, w, h, _) in zip(keys2, glyphs)]
    assert rects == singles and state(a, keys + keys2) == state(b, keys + keys2) and all(state(a, keys2)[2])
    st = a.glyph_coverage_batch_stats()
    assert st["glyphs"] == len(glyphs) and st["written"] == len(glyphs) and st["dropped_by_growth"] == 0 and st["launches"] == 0 and st["bytes_copied"] == 0
    assert a.glyph_batch_stats()["glyphs"] == len(glyphs)
    a.close()
    b.close()


UNTOUCHED = -7  # what a rectangle holds that the call did not fill


def _rc(ctx, fn, glyphs, flags, null=False, n=None, floats=8, rects=False):
    """the C call itself -> status, or with `rects` (status, the out_rects array as tuples, UNTOUCHED where the call wrote nothing);
    glyphs: [(key, segs or None, n_segs or None, w, h, range)]"""
    arr = (GlyphOutline * max(len(glyphs), 1))()
    keep = []
    for g, (key, segs, ns, w, h, R) in zip(arr, glyphs):
        segs = None if segs is None else np.ascontiguousarray(segs, np.float32).reshape(-1, floats)
        keep.append(segs)
        g.key, g.segs, g.width, g.height, g.sdf_range = key, (segs.ctypes.data if segs is not None and len(segs) else None), w, h, R
        g.n_segs = ns if ns is not None else len(segs)
    out = ((C.c_int * 4) * max(len(glyphs), 1))(*([(UNTOUCHED,) * 4] * max(len(glyphs), 1)))
    rc = getattr(ctx.L, fn)(ctx.h, None if null else C.addressof(arr), len(glyphs) if n is None else n, flags, C.addressof(out))
    return (rc, [tuple(r) for r in out][:len(glyphs)]) if rects else rc


FIELDS, COVERAGE = "fdh_put_glyph_outlines_cubic", "fdh_put_glyph_coverage_batch_cubic"


def test_validation_refuses_the_whole_batch():
    """each refusal: FDH_ERR_INVALID, no entry, the packed area and the figures of both stats calls as before"""
    ctx = HipContext(record_only=True)
    ctx.put_glyph_outlines_cubic([(1, BOX, 12, 11)])
    ctx.put_glyph_coverage_batch_cubic([(2, BOX, 12, 11), (3, SQUARE, 12, 11)])
    keys = [1, 2, 3] + list(range(100, 140))
    before = state(ctx, keys)
    assert before[2] == [True] * 3 + [False] * 40
    good = lambda k: (k, BOX, None, 12, 11, 0)  # noqa: E731
    valid = [good(100), good(101), (102, SQUARE, None, 12, 11, 0)]
    many = np.tile(CC.lift(TRIANGLE6), (21845, 1))  # 65535 segments, the most one field glyph takes
    cubics = np.tile(BOX, (16384, 1))               # 65536 segments; 16384 of them cubics
    steep = np.tile(np.array([[0, 0, 3000, 0, 0, 3000, 0, 0]], np.float32), (16384, 1))  # closed lobes of 256 chords each: 2^22 lines
    assert len(CC.flatten_lines(steep[:1])) == 256
    over_segments = lambda n8: [(100 + i, many, None, 12, 11, 0) for i in range(16)] + [(116, n8, None, 12, 11, 0)]  # noqa: E731
    seventeen = np.concatenate([TRIANGLE] * 3 + [SQUARE] * 2)
    assert 16 * len(many) + len(seventeen) == 2 ** 20 + 1
    refused = {
        "an unknown flag": (FIELDS, valid, MTSDF | 16, {}),
        "an unknown flag, coverage": (COVERAGE, valid, 16, {}),
        "an LCD flag on the field call": (FIELDS, valid, MTSDF | LCD_FILTER, {}),
        "the other LCD flag on the field call": (FIELDS, valid, MTSDF | LCD_CONTEXT, {}),
        "no FDH_GLYPH_MTSDF on the field call": (FIELDS, valid, 0, {}),
        "FDH_GLYPH_MTSDF on the coverage call": (COVERAGE, valid, MTSDF, {}),
        "a range in the flags of the coverage call": (COVERAGE, valid, 4 << 8, {}),
        "a range of 65 in the flags": (FIELDS, valid, MTSDF | 65 << 8, {}),
        "a range of 65 in a glyph": (FIELDS, valid + [(103, BOX, None, 12, 11, 65)], MTSDF, {}),
        "sdf_range on the coverage call": (COVERAGE, valid + [(103, BOX, None, 12, 11, 4)], 0, {}),
        "a 0-wide glyph": (FIELDS, valid + [(103, BOX, None, 0, 11, 0)], MTSDF, {}),
        "a 4097-high glyph": (FIELDS, valid + [(103, BOX, None, 12, 4097, 0)], MTSDF, {}),
        "a 0-high glyph, coverage": (COVERAGE, valid + [(103, BOX, None, 12, 0, 0)], 0, {}),
        "a 4097-wide glyph, coverage": (COVERAGE, valid + [(103, BOX, None, 4097, 11, 0)], 0, {}),
        "a negative segment count": (FIELDS, valid + [(103, None, -1, 12, 11, 0)], MTSDF, {}),
        "a negative segment count, coverage": (COVERAGE, valid + [(103, None, -1, 12, 11, 0)], 0, {}),
        "segments without a pointer": (FIELDS, valid + [(103, None, 4, 12, 11, 0)], MTSDF, {}),
        "segments without a pointer, coverage": (COVERAGE, valid + [(103, None, 4, 12, 11, 0)], 0, {}),
        "an open contour in the last glyph": (FIELDS, valid + [(103, BOX[:3], None, 12, 11, 0)], MTSDF, {}),
        "an open contour in the last glyph, of lines": (FIELDS, valid + [(103, SQUARE[:3], None, 12, 11, 0)], MTSDF | CORRECT, {}),
        "65536 segments in one glyph": (FIELDS, valid + [(103, cubics, None, 12, 11, 0)], MTSDF, {}),
        "n = -1": (FIELDS, valid, MTSDF, {"n": -1}),
        "n = -1, coverage": (COVERAGE, valid, 0, {"n": -1}),
        "no array": (FIELDS, valid, MTSDF, {"null": True}),
        "no array, coverage": (COVERAGE, valid, 0, {"null": True}),
        "65536 glyphs": (FIELDS, [(1000 + i, NONE, None, 1, 1, 0) for i in range(65536)], MTSDF, {}),
        "65536 glyphs, coverage": (COVERAGE, [(1000 + i, NONE, None, 1, 1, 0) for i in range(65536)], 0, {}),
        "2^24 + 1 texels": (FIELDS, [(100 + i, BOX, None, 2048, 2048, 0) for i in range(4)] + [(104, NONE, None, 1, 1, 0)], MTSDF, {}),
        "2^24 + 1 texels, coverage": (COVERAGE, [(100 + i, BOX, None, 2048, 2048, 0) for i in range(4)] + [(104, NONE, None, 1, 1, 0)], 0, {}),
        "2^20 + 1 segments, no cubic": (FIELDS, over_segments(seventeen), MTSDF, {}),
        "2^20 + 1 segments, a cubic among them": (FIELDS, over_segments(np.concatenate([TRIANGLE] * 3 + [BOX] * 2)), MTSDF, {}),
        "2^20 + 1 segments, coverage": (COVERAGE, over_segments(np.concatenate([TRIANGLE] * 3 + [BOX] * 2)), 0, {}),
        "2^22 + 1 flattened lines": (COVERAGE, [(100, steep, None, 12, 11, 0), (101, TRIANGLE[:1], None, 12, 11, 0)], 0, {}),
        "FDH_GLYPH_MTSDF_OVERLAP with a cubic in the last glyph": (FIELDS, [(100, SQUARE, None, 12, 11, 0), (101, TRIANGLE, None, 12, 11, 0), good(102)], MTSDF | OVERLAP, {}),
    }
    for what, (fn, glyphs, flags, kw) in refused.items():
        assert _rc(ctx, fn, glyphs, flags, **kw) == INVALID, what
        assert state(ctx, keys) == before and not ctx.has_image(1000), f"{what}: the context changed"
        assert ctx.glyph_batch_stats()["glyphs"] == 1 and ctx.glyph_coverage_batch_stats()["glyphs"] == 2, f"{what}: the figures changed"
    with pytest.raises(FigdrawHipError) as e:
        ctx.put_glyph_outlines_cubic([(100, BOX, 12, 11), (101, BOX[:3], 12, 11)])
    assert e.value.code == INVALID and "put_glyph_outlines_cubic" in str(e.value) and "closed contours" in str(e.value)
    # n_glyphs = 0 is OK and changes nothing but the figures
    assert _rc(ctx, FIELDS, [], MTSDF) == 0 and _rc(ctx, FIELDS, [], MTSDF, null=True) == 0 and ctx.put_glyph_outlines_cubic([]) == []
    assert _rc(ctx, COVERAGE, [], 0) == 0 and _rc(ctx, COVERAGE, [], LCD_FILTER, null=True) == 0 and ctx.put_glyph_coverage_batch_cubic([]) == []
    assert state(ctx, keys) == before and ctx.glyph_batch_stats()["glyphs"] == 0 and ctx.glyph_coverage_batch_stats()["glyphs"] == 0
    # at the limits, not over them: accepted
    big = HipContext(record_only=True)
    assert _rc(big, FIELDS, [(100 + i, BOX, None, 2048, 2048, 0) for i in range(4)], MTSDF) == 0
    assert _rc(big, FIELDS, over_segments(np.concatenate([TRIANGLE] * 4 + [BOX])), MTSDF | CORRECT) == 0 and big.glyph_batch_stats()["glyphs"] == 17
    assert _rc(big, COVERAGE, [(300, steep, None, 12, 11, 0)], LCD_FILTER) == 0 and big.has_image(300)
    assert _rc(big, COVERAGE, [(2000 + i, NONE, None, 1, 1, 0) for i in range(65535)], 0) == 0 and big.has_image(2000 + 65534)
    big.close()
    ctx.close()


def test_a_batch_without_a_cubic_is_the_six_float_batch():
    """equal status, rectangles and entries for every flag fdh_put_glyph_outlines takes, FDH_GLYPH_MTSDF_OVERLAP among them, and its refusals"""
    six = [(2, SQUARE6, None, 12, 11, 0), (3, TRIANGLE6, None, 12, 11, 2), (4, np.zeros((0, 6), np.float32), None, 5, 3, 0)]
    eight = [(k, CC.lift(s), n, w, h, R) for k, s, n, w, h, R in six]
    open6 = six[:2] + [(4, SQUARE6[:3], None, 12, 11, 0)]
    open8 = [(k, CC.lift(s), n, w, h, R) for k, s, n, w, h, R in open6]
    accepted = 0
    for flags in (MTSDF, MTSDF | OVERLAP, MTSDF | OVERLAP | CORRECT | 8 << 8, MTSDF | CORRECT, MTSDF | LCD_FILTER, 0, OVERLAP, 4 << 8, MTSDF | 65 << 8, MTSDF | 16):
        for g6, g8 in ((six, eight), (open6, open8)):
            got = []
            for fn, glyphs, floats in (("fdh_put_glyph_outlines", g6, 6), (FIELDS, g8, 8)):
                ctx = HipContext(record_only=True)
                ctx.put_image(1, np.zeros((5, 7, 4), np.uint8))
                got.append(_rc(ctx, fn, glyphs, flags, floats=floats, rects=True) + (state(ctx, [1, 2, 3, 4]), ctx.glyph_batch_stats()))
                ctx.close()
            assert got[0] == got[1], flags
            rc, rects = got[1][:2]
            if rc == 0:  # the delegating call filled the caller's out_rects: every glyph's own size at a place of its own
                accepted += 1
                assert [r[2:] for r in rects] == [(g[3], g[4]) for g in g8] and len({r[:2] for r in rects}) == 3 and min(min(r) for r in rects) >= 0, flags
            else:
                assert rects == [(UNTOUCHED,) * 4] * 3, flags
    assert accepted == 4


@pytest.mark.parametrize("overlap", [False, True], ids=["plain", "overlap"])
def test_a_batch_without_a_cubic_against_single_cubic_calls(overlap):
    """the delegating path (no cubic in any glyph) through the binding: rectangles, entries and packer equal single fdh_put_glyph_outline_cubic
    calls in order, with per-glyph ranges, the correction and FDH_GLYPH_MTSDF_OVERLAP (which the single call takes on a cubic-free outline)"""
    glyphs = [(name, CC.lift(segs), w, h, (1, 2, 4, 64)[i % 4]) for i, (name, segs, w, h, _) in enumerate(MC.inputs()[2::8])] + [("0 segments", NONE, 5, 3, 0)]
    assert len(glyphs) == 14
    keys = [600 + i for i in range(len(glyphs))]
    a, b = HipContext(record_only=True), HipContext(record_only=True)
    rects = a.put_glyph_outlines_cubic([(k, segs, w, h, R) for k, (_, segs, w, h, R) in zip(keys, glyphs)], correct=True, overlap=overlap)
    singles = []
    for k, (_, segs, w, h, R) in zip(keys, glyphs):
        out = (C.c_int * 4)()
        assert b.L.fdh_put_glyph_outline_cubic(b.h, k, w, h, segs.ctypes.data if len(segs) else None, len(segs), MTSDF | CORRECT | (OVERLAP if overlap else 0) | R << 8, out) == 0
        singles.append(tuple(out))
    assert rects == singles and [r[2:] for r in rects] == [g[2:4] for g in glyphs] and state(a, keys) == state(b, keys) and all(state(a, keys)[2])
    assert a.glyph_batch_stats()["glyphs"] == a.glyph_batch_stats()["written"] == 14
    a.close()
    b.close()


def test_growth_is_what_single_calls_leave():
    """atlas size 64 and twelve 40 x 40 glyphs, cubic and cubic-free in turn: every other placement grows the atlas and drops what was there"""
    shape = lambda i: cubic_square(40, 40) if i % 2 == 0 else CC.lift(MC.poly([(10, 10), (30, 10), (30, 30), (10, 30)]))  # noqa: E731
    keys = list(range(300, 312))
    for coverage in (False, True):
        a, b = HipContext(atlas_size=64, record_only=True), HipContext(atlas_size=64, record_only=True)
        if coverage:
            rects = a.put_glyph_coverage_batch_cubic([(k, shape(i), 40, 40) for i, k in enumerate(keys)], lcd_filter=True)
            singles = [b.put_glyph_outline_cubic(k, shape(i), 40, 40, lcd_filter=True) for i, k in enumerate(keys)]
        else:
            rects = a.put_glyph_outlines_cubic([(k, shape(i), 40, 40) for i, k in enumerate(keys)], correct=True)
            singles = [b.put_glyph_outline_cubic(k, shape(i), 40, 40, mtsdf=True, correct=True) for i, k in enumerate(keys)]
        assert rects == singles and state(a, keys) == state(b, keys)
        lost = sum(not b.has_image(k) for k in keys)
        st = a.glyph_coverage_batch_stats() if coverage else a.glyph_batch_stats()
        assert a.atlas_size() > 64 and 0 < lost < 12
        assert st["dropped_by_growth"] == lost and st["written"] == 12 - lost and st["glyphs"] == 12
        # a key put twice in one batch: two rectangles, the entry is the later one's
        if coverage:
            r2 = a.put_glyph_coverage_batch_cubic([(400, BOX, 12, 11), (400, TRIANGLE, 9, 7)])
            s2 = [b.put_glyph_outline_cubic(400, BOX, 12, 11), b.put_glyph_outline_cubic(400, TRIANGLE, 9, 7)]
        else:
            r2 = a.put_glyph_outlines_cubic([(400, BOX, 12, 11), (400, BOX, 12, 11)])
            s2 = [b.put_glyph_outline_cubic(400, BOX, 12, 11, mtsdf=True) for _ in range(2)]
        assert r2 == s2 and r2[0] != r2[1] and state(a, keys + [400]) == state(b, keys + [400])
        a.close()
        b.close()


def full_atlas(**kw):
    """a 16384 atlas, the largest, with nine 4096 x 4096 rectangles in it: what is left takes small glyphs and no 4096 x 4090"""
    ctx = HipContext(atlas_size=16384, **kw)
    for i in range(9):
        ctx.put_glyph_outline(900 + i, np.zeros((0, 6), np.float32), 4096, 4096)
    return ctx


FULL_BATCH = [(10, BOX, 12, 11), (11, TRIANGLE, 12, 11), (12, NONE, 4096, 4090), (13, BOX, 12, 11)]


@pytest.mark.parametrize("coverage", [False, True])
def test_atlas_full_in_the_middle(coverage):
    a, b = full_atlas(record_only=True), full_atlas(record_only=True)
    batch = a.put_glyph_coverage_batch_cubic if coverage else a.put_glyph_outlines_cubic
    single = (lambda k, s, w, h: b.put_glyph_outline_cubic(k, s, w, h)) if coverage else (lambda k, s, w, h: b.put_glyph_outline_cubic(k, s, w, h, mtsdf=True))
    with pytest.raises(FigdrawHipError) as e:
        batch(FULL_BATCH)
    assert e.value.code == ATLAS_FULL
    singles = [single(*g) for g in FULL_BATCH[:2]]
    with pytest.raises(FigdrawHipError) as e:
        single(*FULL_BATCH[2])
    assert e.value.code == ATLAS_FULL
    keys = [900 + i for i in range(9)] + [10, 11, 12, 13]
    assert state(a, keys) == state(b, keys) and state(a, keys)[2] == [True] * 11 + [False] * 2 and a.atlas_size() == 16384
    st = a.glyph_coverage_batch_stats() if coverage else a.glyph_batch_stats()
    assert st["glyphs"] == 4 and st["written"] == 2 and st["dropped_by_growth"] == 0
    assert batch(FULL_BATCH[3:]) == [single(*FULL_BATCH[3])] and len(singles) == 2
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------ the kernels' source on a CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_msdf_cubic.hip + fdh_msdf_cubic_host.h + k_msdf.hip + fdh_msdf_host.h compiled as plain C++ with tests/msdf_cubic_batch_emu/emu.cpp under the
    sequential shim of tests/emu (64 lanes of a wave together, with the ballot) -> the directory of `wave` and of `wave_san`, the same stand-alone
    program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "msdf_cubic_batch_emu", ("k_msdf_cubic.hip", "fdh_msdf_cubic_host.h", "k_msdf.hip", "fdh_msdf_host.h"),
                           {"wave": (), "wave_san": emu_build.SAN})


def emulated_batch():
    """-> [(name, segs8, w, h, R)], 74 glyphs: 27 of the skewed font set (every fourth), the 31 hostile outlines no wider and no higher than 64, the 2 analytic
    shapes, the 4 device-only shapes of test_msdf_cubic.py and 10 cubic-free outlines (every tenth font input but the last, lifted)"""
    lifted = [(name + " lifted", CC.lift(segs), w, h, R) for name, segs, w, h, R in MC.inputs()[::10][:10]]
    return CC.skewed()[::4] + [c[:5] for c in CC.hostile() if c[2] <= 64 and c[3] <= 64] + [c[:5] for c in CC.analytic()] + DEVICE_ONLY + lifted


def _write(path, glyphs):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(glyphs)))
        for _, segs, w, h, R in glyphs:
            segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 8)
            f.write(struct.pack("<4i", w, h, R, len(segs)))
            f.write(segs.tobytes())


RUNS = {"in order": ("wave", False, 0), "reversed": ("wave", True, 0), "cut in the middle": ("wave", False, 37), "in order, under sanitizers": ("wave_san", False, 0)}


@pytest.mark.parametrize("run", list(RUNS))
def test_the_batched_kernels_under_a_host_shim(shim, run):
    """every glyph's slice of the batched output, generated and corrected, is the single launchers' output; a cubic-free glyph's is also
    k_msdf_generate's and k_msdf_correct's; no 0xEE pad around the fields is written, the correction's input is not.  `cut`: the tables of
    glyphs 37 .. 73 with edge_off rebased, as after a growth at glyph 37."""
    exe, reverse, first = RUNS[run]
    glyphs = emulated_batch()
    assert len(glyphs) == 27 + 31 + 2 + 4 + 10
    if reverse:
        glyphs = glyphs[::-1]
    name = run.replace(" ", "_").replace(",", "") + ".raw"
    _write(shim / name, glyphs)
    r = subprocess.run(["./" + exe, name] + ([str(first)] if first else []), cwd=shim, capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, f"{r.returncode} {r.stdout}{r.stderr}"
    m = len(glyphs) - first
    lifted = sum(len(c[1]) == 0 or bool(np.isnan(np.asarray(c[1])[:, 2:6]).any(axis=1).all()) for c in glyphs[first:])
    assert f"generate: 0 of {m} glyphs differ; correct: 0 differ; cubic-free: {lifted} glyphs, 0 differ from k_msdf.hip\n" in r.stdout
    tiles = sum(((w + 7) // 8) * ((h + 7) // 8) for _, _, w, h, _ in glyphs[first:])
    assert re.search(r"glyphs %d tiles %d edges \d+ cubics [1-9]\d+" % (m, tiles), r.stdout)
