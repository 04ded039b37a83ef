"""A batch of coverage glyphs in one call (fdh_put_glyph_coverage_batch, include_glyphs/figdraw_hip_coverage.h), what a CPU can check: the header and the
C ABI; on record-only contexts the packing, the validation of the whole batch before anything is placed, the growth of the atlas and a full
atlas, each against single calls of fdh_put_glyph_outline; and the source of the three batched kernels of k_atlas_upload.hip under the host
shim of tests/emu (tests/coverage_batch_emu) against the single launchers of the same file and against the oracle.  Everything here is equality."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import coverage_cases as CC
import emu_build
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, GlyphOutline, HipContext
from oracle import oracle as O

ROOT = CC.ROOT
HEADER = os.path.join(ROOT, "include_glyphs", "figdraw_hip_coverage.h")
NEW_API = ("fdh_put_glyph_coverage_batch", "fdh_glyph_coverage_batch_stats")
INVALID, ATLAS_FULL = -1, -4
LCD_FILTER, LCD_CONTEXT, MTSDF, CORRECT, OVERLAP = 1, 2, 4, 8, 32
SQUARE = CC.poly([(2, 2), (10, 2), (10, 9), (2, 9)])
TRIANGLE = CC.poly([(2, 2), (10, 2), (6, 9)])
NONE = CC.NONE


# ------------------------------------------------------------------------------------------------------------------ header and ABI
def test_header_declares_and_library_exports_the_coverage_batch():
    src = open(HEADER).read()
    assert re.search(r'#include "figdraw_hip_glyphs\.h"', src)
    assert "figdraw_hip_coverage.h" not in os.listdir(os.path.join(ROOT, "include"))  # include/ keeps the headers it had
    declared = re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", src)
    assert sorted(declared) == sorted(NEW_API)
    L = context.load()
    for name in NEW_API:
        assert hasattr(L, name), name
    main = open(os.path.join(ROOT, "include", "figdraw_hip.h")).read()
    assert not any(re.search(r"\b%s\b" % n, main) for n in NEW_API)  # no declaration there ...
    assert "figdraw_hip_coverage.h" in main                          # ... the coverage comment points to the new header


def test_coverage_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "coverage_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "coverage_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "coverage_abi_smoke: OK" in r.stdout
    src = open(os.path.join(ROOT, "tests", "coverage_abi_smoke.c")).read()
    assert all(re.search(r"\b%s\b" % n, src) for n in NEW_API)


# ------------------------------------------------------------------------------------------------------------------ record-only contexts
def packed_area(ctx):
    area = C.c_int64(-1)
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def state(ctx, keys):
    return ctx.atlas_size(), packed_area(ctx), [ctx.has_image(k) for k in keys]


@pytest.mark.parametrize("which", ["font", "variants"])
def test_record_only_packing(which):
    """the 94 font outlines, and the 376 of four sub-pixel variants, as one batch against single calls"""
    glyphs = CC.font() if which == "font" else CC.variants()
    assert len(glyphs) == {"font": 94, "variants": 376}[which]
    a, b = HipContext(record_only=True), HipContext(record_only=True)
    keys = [5000 + i for i in range(len(glyphs))]
    rects = a.put_glyph_coverage_batch([(k, segs, w, h) for k, (_, segs, w, h) in zip(keys, glyphs)], lcd_filter=which == "variants")
    singles = [b.put_glyph_outline(k, segs, w, h, lcd_filter=which == "variants") for k, (_, segs, w, h) in zip(keys, glyphs)]
    assert rects == singles
    assert state(a, keys) == state(b, keys) and all(state(a, keys)[2])
    st = a.glyph_coverage_batch_stats()
    assert st["glyphs"] == len(glyphs) == st["written"] and st["dropped_by_growth"] == 0 and st["launches"] == 0 and st["bytes_copied"] == 0
    assert a.glyph_batch_stats()["glyphs"] == 0  # the distance-field batch's figures are its own
    a.close()
    b.close()


def _rc(ctx, glyphs, flags, null=False, n=None):
    """the C call itself -> status; glyphs: [(key, segs or None, n_segs or None, w, h, range)]"""
    arr = (GlyphOutline * max(len(glyphs), 1))()
    keep = []
    for g, (key, segs, ns, w, h, R) in zip(arr, glyphs):
        segs = None if segs is None else np.ascontiguousarray(segs, np.float32).reshape(-1, 6)
        keep.append(segs)
        g.key, g.segs, g.width, g.height, g.sdf_range = key, (segs.ctypes.data if segs is not None and len(segs) else None), w, h, R
        g.n_segs = ns if ns is not None else len(segs)
    out = ((C.c_int * 4) * max(len(glyphs), 1))()
    return ctx.L.fdh_put_glyph_coverage_batch(ctx.h, None if null else C.addressof(arr), len(glyphs) if n is None else n, flags, C.addressof(out))


def test_validation_refuses_the_whole_batch():
    ctx = HipContext(record_only=True)
    ctx.put_glyph_coverage_batch([(1, SQUARE, 12, 11), (2, TRIANGLE, 12, 11)])
    ctx.put_glyph_outlines([(3, SQUARE, 12, 11)])
    keys = [1, 2, 3] + list(range(100, 140))
    before = state(ctx, keys), ctx.glyph_coverage_batch_stats(), ctx.glyph_batch_stats()
    assert before[0][2] == [True] * 3 + [False] * 40 and before[1]["glyphs"] == 2 and before[2]["glyphs"] == 1
    good = lambda k: (k, SQUARE, None, 12, 11, 0)  # noqa: E731
    lines_2_20 = np.tile(TRIANGLE, (2 ** 20 // 3 + 1, 1))[:2 ** 20]  # 2^20 straight segments: the most a batch takes
    curve = np.array([[0, 0, 2000, 4000, 4000, 0]], np.float32)      # a curve of 64 chords, the most one takes
    curves_2_22 = np.tile(curve, (2 ** 16, 1))                       # 2^22 flattened lines: the most a batch takes
    assert len(CC.flatten(O, curve)) == 64
    refused = {
        "FDH_GLYPH_MTSDF": ([good(100)], MTSDF),
        "FDH_GLYPH_MTSDF with an LCD flag": ([good(100)], MTSDF | LCD_FILTER),
        "FDH_GLYPH_MTSDF_CORRECT": ([good(100)], CORRECT),
        "FDH_GLYPH_MTSDF_OVERLAP": ([good(100)], LCD_FILTER | OVERLAP),
        "a range in the flags": ([good(100)], 4 << 8),
        "an unknown flag": ([good(100)], 16),
        "another unknown flag": ([good(100)], LCD_CONTEXT | 1 << 16),
        "a glyph with a range": ([good(100), (101, SQUARE, None, 12, 11, 4), good(102)], 0),
        "a 4097-wide glyph": ([good(100), (101, SQUARE, None, 4097, 11, 0)], LCD_FILTER),
        "a 4097-high glyph": ([good(100), (101, SQUARE, None, 12, 4097, 0)], 0),
        "a 0-high glyph": ([good(100), (101, SQUARE, None, 12, 0, 0)], 0),
        "segments without a pointer": ([good(100), (101, None, 4, 12, 11, 0)], 0),
        "a negative segment count": ([good(100), (101, None, -1, 12, 11, 0)], 0),
        "2^24 + 1 texels": ([(100 + i, NONE, None, 2048, 2048, 0) for i in range(4)] + [(104, NONE, None, 1, 1, 0)], 0),
        "2^20 + 1 segments": ([(100, lines_2_20, None, 12, 11, 0), (101, TRIANGLE[:1], None, 12, 11, 0)], 0),
        "2^22 + 1 flattened lines": ([(100, curves_2_22, None, 12, 11, 0), (101, TRIANGLE[:1], None, 12, 11, 0)], 0),
    }
    for what, (glyphs, flags) in refused.items():
        assert _rc(ctx, glyphs, flags) == INVALID, what
        assert (state(ctx, keys), ctx.glyph_coverage_batch_stats(), ctx.glyph_batch_stats()) == before, f"{what}: the context changed"
    assert _rc(ctx, [good(100)], 0, null=True) == INVALID and _rc(ctx, [good(100)], 0, n=-1) == INVALID and _rc(ctx, [good(100)], 0, n=65536) == INVALID
    assert (state(ctx, keys), ctx.glyph_coverage_batch_stats(), ctx.glyph_batch_stats()) == before
    with pytest.raises(FigdrawHipError) as e:
        ctx.put_glyph_coverage_batch([(100, SQUARE, 12, 11), (101, SQUARE, 4097, 11)])
    assert e.value.code == INVALID and "put_glyph_coverage_batch" in str(e.value)
    # n_glyphs = 0 is OK and places nothing
    assert _rc(ctx, [], 0) == 0 and _rc(ctx, [], LCD_FILTER, null=True) == 0 and ctx.put_glyph_coverage_batch([]) == []
    assert state(ctx, keys) == before[0] and ctx.glyph_coverage_batch_stats()["glyphs"] == 0 and ctx.glyph_batch_stats() == before[2]
    # at the limits, not over them: accepted (contexts of their own: four 2048 x 2048 rectangles make the atlas grow)
    big = HipContext(record_only=True)
    assert _rc(big, [(100 + i, NONE, None, 2048, 2048, 0) for i in range(4)], 0) == 0
    assert _rc(big, [(200, lines_2_20, None, 12, 11, 0)], LCD_CONTEXT) == 0
    assert _rc(big, [(201, curves_2_22, None, 4096, 1, 0), (202, NONE, None, 1, 4096, 0)], LCD_FILTER) == 0
    assert big.has_image(200) and big.has_image(202) and big.glyph_coverage_batch_stats()["glyphs"] == 2
    big.close()
    many = HipContext(record_only=True)
    assert _rc(many, [(1000 + i, NONE, None, 1, 1, 0) for i in range(65535)], 0) == 0
    assert many.glyph_coverage_batch_stats()["glyphs"] == 65535 and many.has_image(1000 + 65534)
    many.close()
    ctx.close()


def test_growth_is_what_single_calls_leave():
    """atlas size 64 and twelve 40 x 40 squares: every other placement grows the atlas and drops what was there"""
    a, b = HipContext(atlas_size=64, record_only=True), HipContext(atlas_size=64, record_only=True)
    keys = list(range(300, 312))
    rects = a.put_glyph_coverage_batch([(k, CC.square(40, 40), 40, 40) for k in keys], lcd_filter=True)
    singles = [b.put_glyph_outline(k, CC.square(40, 40), 40, 40, lcd_filter=True) for k in keys]
    assert rects == singles and state(a, keys) == state(b, keys)
    lost = sum(not b.has_image(k) for k in keys)
    st = a.glyph_coverage_batch_stats()
    assert a.atlas_size() > 64 and 0 < lost < 12
    assert st["dropped_by_growth"] == lost and st["written"] == 12 - lost and st["glyphs"] == 12
    # a key put twice in one batch: two rectangles, the entry is the later one's
    r2 = a.put_glyph_coverage_batch([(400, SQUARE, 12, 11), (400, TRIANGLE, 9, 7)])
    s2 = [b.put_glyph_outline(400, SQUARE, 12, 11), b.put_glyph_outline(400, TRIANGLE, 9, 7)]
    assert r2 == s2 and r2[0] != r2[1] and state(a, keys + [400]) == state(b, keys + [400])
    a.close()
    b.close()


def full_atlas(**kw):
    """a 16384 atlas, the largest, with nine 4096 x 4096 rectangles in it: what is left takes small glyphs and no 4096 x 4090"""
    ctx = HipContext(atlas_size=16384, **kw)
    for i in range(9):
        ctx.put_glyph_outline(900 + i, NONE, 4096, 4096)
    return ctx


FULL_BATCH = [(10, SQUARE, 12, 11), (11, TRIANGLE, 12, 11), (12, NONE, 4096, 4090), (13, SQUARE, 12, 11)]


def test_atlas_full_in_the_middle():
    a, b = full_atlas(record_only=True), full_atlas(record_only=True)
    with pytest.raises(FigdrawHipError) as e:
        a.put_glyph_coverage_batch(FULL_BATCH)
    assert e.value.code == ATLAS_FULL
    singles = [b.put_glyph_outline(k, segs, w, h) for k, segs, w, h in FULL_BATCH[:2]]
    with pytest.raises(FigdrawHipError) as e:
        b.put_glyph_outline(*FULL_BATCH[2])
    assert e.value.code == ATLAS_FULL
    keys = [900 + i for i in range(9)] + [10, 11, 12, 13]
    assert state(a, keys) == state(b, keys) and state(a, keys)[2] == [True] * 11 + [False] * 2 and a.atlas_size() == 16384
    st = a.glyph_coverage_batch_stats()
    assert st["glyphs"] == 4 and st["written"] == 2 and st["dropped_by_growth"] == 0
    assert a.put_glyph_coverage_batch(FULL_BATCH[3:]) == [b.put_glyph_outline(*FULL_BATCH[3])] and len(singles) == 2
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------ the kernels' source on a CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_atlas_upload.hip + fdh_msdf_host.h compiled as plain C++ with tests/coverage_batch_emu/emu.cpp under the sequential shim of tests/emu ->
    the directory of `wave` and of `wave_san`, the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "coverage_batch_emu", ("k_atlas_upload.hip", "fdh_msdf_host.h"), {"wave": (), "wave_san": emu_build.SAN},
                           flags=("-ffp-contract=off",))


def batches():
    """-> {name: [(name, segs, w, h)]}"""
    import coverage_hostile_cases as H

    # the families of coverage_hostile_cases.py that the second batch does not hold already (test_coverage_exact_host.py holds the oracle to
    # exact areas on them); an outline with cubics goes in as the straight lines the cubic call makes of it
    hostile = [(f"{family}: {name}", H.as6(segs), w, h) for family, name, segs, w, h in H.cases() if family not in ("font outlines scaled 3.7 x", "shapes")]
    return {"font and variants": CC.variants(), "leaving the image and shapes": CC.scaled() + CC.shapes(), "hostile": hostile}


@pytest.fixture(scope="module")
def oracle_images():
    """{batch: [(unfiltered, filtered)]} by the oracle, once for both programs"""
    return {name: [(CC.oracle_image(O, segs, w, h, False), CC.oracle_image(O, segs, w, h, True)) for _, segs, w, h in glyphs] for name, glyphs in batches().items()}


@pytest.mark.parametrize("exe", ["wave", "wave_san"])
@pytest.mark.parametrize("batch", ["font and variants", "leaving the image and shapes", "hostile"])
def test_the_batched_kernels_under_a_host_shim(shim, oracle_images, exe, batch):
    """every glyph's bytes are the single launcher's and the oracle's, unfiltered and filtered; no pad between the images is written, no input is"""
    glyphs = batches()[batch]
    assert len(glyphs) == {"font and variants": 376, "leaving the image and shapes": 94 + 18, "hostile": 64 + 80 + 4 + 2 + 8 + 8 + 6 + 3 + 4 + 4}[batch]
    n_lines = 0
    with open(shim / f"{exe}.raw", "wb") as f:
        f.write(struct.pack("<i", len(glyphs)))
        for _, segs, w, h in glyphs:
            lines = CC.flatten(O, segs)
            n_lines += len(lines)
            f.write(struct.pack("<3i", w, h, len(lines)))
            f.write(lines.tobytes())
    r = subprocess.run(["./" + exe, f"{exe}.raw", f"{exe}.out"], cwd=shim, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, f"{r.returncode} {r.stdout}{r.stderr}"
    assert f"coverage: 0 of {len(glyphs)} glyphs differ; lcd: 0 differ\n" in r.stdout
    tiles = sum(((w + 7) // 8) * ((h + 7) // 8) for _, _, w, h in glyphs if w > 1 and h > 1)
    assert f"glyphs {len(glyphs)} tiles {tiles} lines {n_lines}\n" in r.stdout
    out = np.fromfile(shim / f"{exe}.out", np.uint8)
    at = 0
    for (name, _, w, h), (plain, lcd) in zip(glyphs, oracle_images[batch]):
        got = out[at:at + 8 * w * h].reshape(2, h, w, 4)
        at += 8 * w * h
        if w > 1 and h > 1:
            assert np.array_equal(got[0], plain) and np.array_equal(got[1], lcd), name
        else:  # no tiles: nothing written
            assert (got == 0xEE).all(), name
    assert at == len(out)
