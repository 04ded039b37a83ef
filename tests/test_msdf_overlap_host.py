"""Overlapping contours in distance-field generation (fdh_put_glyph_outline with FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_OVERLAP, step 6 of the
specification in include/figdraw_hip.h), what a CPU can check: the flag on a record-only context; the reference tests/msdf_overlap_ref.py
itself -- its sign against non-zero winding on the 16 overlapping outlines of msdf_overlap_cases.py, against msdf_ref on the font set, on
single contours, under another contour order, in float32 against float64 --; and the source of k_msdf_generate_union and
k_msdf_correct_union with fdh_msdf_host.h under the sequential host shim of tests/emu, with a wave's ballot and with waves of one lane
(tests/msdf_overlap_emu), against that reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emu_build
import msdf_cases as MC
import msdf_correct_ref as CR
import msdf_overlap_cases as OC
import msdf_overlap_ref as OR
import msdf_ref as M
from figdraw_amd.context import HipContext

ROOT = MC.ROOT
INVALID = -1
LCD_FILTER, LCD_CONTEXT, MTSDF, CORRECT, OVERLAP = 1, 2, 4, 8, 32
CORRECT_CAP = 1  # step 5's own cap (test_msdf_correct_host.py): a verdict may flip where |d(q)| is within rounding of R / 255
SQUARE = MC.poly([(2, 2), (10, 2), (10, 9), (2, 9)])


def RANGE(r):
    return r << 8


def differing(a, b):
    return int((a != b).any(axis=2).sum())


# ------------------------------------------------------------------------------------------------------------------ 1. the flag
def test_flag_on_a_record_only_context():
    src = open(os.path.join(ROOT, "include", "figdraw_hip.h")).read()
    assert re.search(r"\bFDH_GLYPH_MTSDF_OVERLAP\s*=\s*32\b", src)
    ctx = HipContext(record_only=True)
    rect = ctx.put_glyph_outline(71, SQUARE, 12, 11, mtsdf=True, sdf_range=4, overlap=True)  # accepted, and the rectangle is packed
    assert rect[2:] == (12, 11) and rect[0] >= 0 and rect[1] >= 0 and ctx.has_image(71)
    assert ctx.put_glyph_outline(72, SQUARE, 12, 11, mtsdf=True, correct=True, overlap=True)[2:] == (12, 11)  # range 0 = 4

    def rc(flags, segs=SQUARE, key=80):
        segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 6)
        out = (C.c_int * 4)()
        return ctx.L.fdh_put_glyph_outline(ctx.h, key, 12, 11, segs.ctypes.data, len(segs), flags, out)

    assert rc(MTSDF | OVERLAP) == 0 and rc(MTSDF | OVERLAP | RANGE(1)) == 0 and rc(MTSDF | OVERLAP | RANGE(64)) == 0
    assert rc(MTSDF | OVERLAP | CORRECT) == 0 and rc(MTSDF | OVERLAP | CORRECT | RANGE(8)) == 0
    assert rc(MTSDF) == 0 and rc(MTSDF | CORRECT) == 0 and rc(0) == 0  # without the flag: as before
    assert rc(OVERLAP, key=84) == INVALID and not ctx.has_image(84)  # alone: refused before anything is packed
    assert rc(OVERLAP | RANGE(4)) == INVALID and rc(OVERLAP | CORRECT) == INVALID
    assert rc(OVERLAP | LCD_FILTER) == INVALID and rc(OVERLAP | LCD_CONTEXT) == INVALID
    assert rc(MTSDF | OVERLAP | LCD_FILTER, key=85) == INVALID and rc(MTSDF | OVERLAP | LCD_CONTEXT, key=85) == INVALID and not ctx.has_image(85)
    assert rc(MTSDF | OVERLAP | RANGE(65)) == INVALID
    assert rc(MTSDF | OVERLAP | 16) == INVALID and rc(MTSDF | OVERLAP | 64) == INVALID and rc(MTSDF | OVERLAP | 1 << 16) == INVALID  # bits that are still unknown
    assert rc(MTSDF | OVERLAP, SQUARE[:3], key=81) == INVALID and not ctx.has_image(81)  # an open contour
    assert rc(MTSDF | OVERLAP, np.zeros((0, 6), np.float32), key=82) == 0 and ctx.has_image(82)  # an outline without edges is no error
    img = np.zeros((11, 12, 4), np.uint8)
    out = (C.c_int * 4)()
    for flags in (OVERLAP, OVERLAP | LCD_FILTER, OVERLAP | MTSDF, OVERLAP | MTSDF | CORRECT):  # fdh_put_glyph_image does not know the flag
        assert ctx.L.fdh_put_glyph_image(ctx.h, 83, 12, 11, img.ctypes.data, flags, out) == INVALID
    assert not ctx.has_image(83)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the reference
@pytest.fixture(scope="module")
def overlapping():
    """the 16 outlines through the float64 reference, once -> {name: (distances (h, w, 4), winding != 0)}"""
    return {name: (OR.distances(segs, w, h), MC.winding(segs, w, h) != 0) for name, segs, w, h in OC.inputs()}


def test_reference_contours_and_classes():
    cs, o = OR.contours(OC.RING)
    assert o == 1.0 and [a for _, a in cs] == [576.0, -11.5 * 11.5]
    cs, o = OR.contours(OC.reverse(OC.RING))  # the contours swap places and both run the other way
    assert o == -1.0 and [a for _, a in cs] == [11.5 * 11.5, -576.0]
    shapes, filled = OR._classes(OC.FIVE_AND_A_HOLE)
    assert filled == [True] * 5 + [False] and all(s.orient == 1.0 for s in shapes)
    shapes, filled = OR._classes(OC.reverse(OC.FIVE_AND_A_HOLE))
    assert filled == [False] + [True] * 5 and all(s.orient == -1.0 for s in shapes)
    # a known answer: (9.5, 12.5) is 3.5 inside the first of two 12 x 12 squares and 0.5 outside the second; step 4 alone says 0.5 outside
    two = OC.join(OC.rect(4, 4, 16, 16), OC.rect(10, 10, 22, 22))
    assert OR.distances(two, 26, 26)[12, 9, 3] == 3.5 and M.distances(M.build_shape(two), 26, 26)[12, 9, 3] == -0.5
    # ring plus bar: in the hole but in the bar, inside; in the hole beside the bar, outside by the distance to the bar
    ring_bar = OC.join(OC.RING, OC.rect(1.75, 13.75, 30.25, 18.25))
    d = OR.distances(ring_bar, 32, 32)[..., 3]
    assert d[16, 16] == 1.75 and d[13, 16] == -0.25 and d[11, 16] == -1.25  # (the last: nearer to the hole's border than to the bar)


def test_reference_sign_on_the_overlapping_outlines(overlapping):
    """msdf_cases.check_sign with `true` = the new A, at R = 2, 4 and 8: median and alpha agree with non-zero winding on every texel farther
    than R / 255 from the outline.  Plain step 4 fails the same test on all but the doubled square (measured: 15 of 16)."""
    plain_fails = []
    for name, segs, w, h in OC.inputs():
        d, inside = overlapping[name]
        for R in (2, 4, 8):
            assert OC.check_sign(f"{name}, R = {R}", M.encode(d, R), segs, w, h, R, d[..., 3], inside) > 0.6 * w * h
        try:
            OC.check_sign(name, M.generate(segs, w, h, 4), segs, w, h, 4, d[..., 3], inside)
        except AssertionError:
            plain_fails.append(name)
    print(f"plain step 4 fails the sign test on {len(plain_fails)} of 16")
    assert len(plain_fails) >= 14 and "a square twice" not in plain_fails


def test_reference_float32_stays_inside_the_cap(overlapping):
    """the cap is a condition on the inputs: the float32 form of the reference against float64 (the issue's prototype: 0 texels on each)"""
    over = {}
    for name, segs, w, h in OC.inputs():
        n = MC.over_tolerance(OR.generate(segs, w, h, 4, np.float32), M.encode(overlapping[name][0], 4))
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels of the float32 reference are more than 1 LSB from the float64 reference"
    print(f"float32 reference against float64, texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")


@pytest.fixture(scope="module")
def font_reference():
    """the 106 font inputs through step 6 in float64, once -> {name: image}"""
    return {name: OR.generate(segs, w, h, R) for name, segs, w, h, R in MC.inputs()}


def test_reference_on_the_font_set(font_reference):
    """contours that do not overlap: A is step 4's byte for byte, the median within 1 LSB of it, the sign test passes; channels may differ
    (all four now come from one contour)"""
    differ = texels = 0
    for name, segs, w, h, R in MC.inputs():
        got, plain = font_reference[name], M.generate(segs, w, h, R)
        assert np.array_equal(got[..., 3], plain[..., 3]), f"{name}: A"
        assert np.abs(MC.median3(got) - MC.median3(plain)).max() <= 1, f"{name}: the median"
        MC.check_sign(name, got, segs, w, h, R)
        differ, texels = differ + differing(got, plain), texels + w * h
    print(f"{differ} of {texels} texels differ from plain mode in some channel")
    assert texels == 133509


def test_reference_single_contour_is_step_4():
    singles = [(n, s, w, h, R) for n, s, w, h, R, _ in MC.hostile_inputs() if len(OR.contours(s)[0]) == 1][:24]
    singles += [("circle16 reversed", OC.reverse(MC.circle16()), 28, 24, 4)]
    assert len(singles) == 25
    for name, segs, w, h, R in singles:
        assert np.array_equal(OR.generate(segs, w, h, R), M.generate(segs, w, h, R)), name


def test_reference_is_independent_of_contour_order(overlapping):
    """A is the same on every texel whatever the order; so are R, G and B wherever no two contours have the very same A (there the header's
    tie rule, contour order, names the contour: several of these outlines are symmetric and put texel centres on such ties on purpose)"""
    rng = np.random.RandomState(6)
    for name, segs, w, h in OC.inputs():
        cs = [rows for rows, _ in OR.contours(segs)[0]]
        shapes, _ = OR._classes(segs)
        a = np.stack([M.distances(s, w, h)[..., 3] for s in shapes])
        tie = np.zeros((h, w), bool)
        for i in range(len(a)):
            for j in range(i + 1, len(a)):
                tie |= a[i] == a[j]
        assert name == "a square twice" or tie.sum() <= 0.08 * w * h
        for order in (list(range(len(cs)))[::-1], list(rng.permutation(len(cs)))):
            got = OR.distances(OC.join(*(cs[k] for k in order)), w, h)
            assert np.array_equal(got[..., 3], overlapping[name][0][..., 3]), f"{name}: A under contour order {order}"
            assert np.array_equal(got[~tie], overlapping[name][0][~tie]), f"{name}: contour order {order}"


def test_what_step_6_does_not_cover():
    """recorded, not asserted: the header lists both as not covered"""
    for name, segs, w, h in OC.out_of_scope_inputs():
        d = OR.distances(segs, w, h)
        inside = MC.winding(segs, w, h) != 0
        far = np.abs(d[..., 3]) > 4 / 255.0
        print(f"{name}: {int(((d[..., 3] > 0) != inside)[far].sum())} of {w * h} texels have another sign than non-zero winding gives")
        assert d.shape == (h, w, 4) and np.isfinite(d).all()


# ------------------------------------------------------------------------------------------------------------------ 3. the kernels' source on a CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_msdf.hip + fdh_msdf_host.h compiled as plain C++ with tests/msdf_overlap_emu/emu.cpp under the sequential shim of tests/emu ->
    {program: its directory}: `wave` with the ballot (and `wave_san`: the same stand-alone program under AddressSanitizer and UBSan), `lane`
    and `lane_nocull` with waves of one lane (-DEMU_LANES_ALONE: the generators only)"""
    csrc = ("k_msdf.hip", "fdh_msdf_host.h")
    wave = emu_build.build(tmp_path_factory, "msdf_overlap_emu", csrc, {"wave": (), "wave_san": emu_build.SAN})
    lane = emu_build.build(tmp_path_factory, "msdf_overlap_emu", csrc, {"lane": (), "lane_nocull": ("-DFDH_MSDF_NO_CULL=1",)}, flags=("-DEMU_LANES_ALONE", "-DEMU_GENERATE_ONLY"))
    return {"wave": wave, "wave_san": wave, "lane": lane, "lane_nocull": lane}


def _through_the_shim(shim, exe, name, segs, w, h, R):
    """-> {"plain", "union"[, "corrected"]: texels, "contours": (contours, holes)}"""
    tmp = shim[exe]
    np.ascontiguousarray(segs, np.float32).tofile(tmp / "segs.raw")
    r = subprocess.run(["./" + exe, str(w), str(h), str(R), "segs.raw"], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name}: {r.returncode} {r.stdout}{r.stderr}"
    out = {k: np.fromfile(tmp / f"{k}.raw", np.uint8).reshape(h, w, 4) for k in (("plain", "union") if exe.startswith("lane") else ("plain", "union", "corrected"))}
    out["contours"] = tuple(int(v) for v in re.match(r"contours (\d+) holes (\d+)", r.stdout).groups())
    return out


def all_inputs():
    """the 16 overlapping outlines and the 2 of msdf_overlap_cases.tie_inputs(), the 106 font inputs and the 71 hostile ones -> [(name, segs, w, h, R)]"""
    return [(n, s, w, h, 4) for n, s, w, h in OC.inputs() + OC.tie_inputs()] + MC.inputs() + [("hostile: " + c[0],) + c[1:5] for c in MC.hostile_inputs()]


@pytest.fixture(scope="module")
def emulated(shim):
    return {name: _through_the_shim(shim, "wave", name, segs, w, h, R) for name, segs, w, h, R in all_inputs()}


@pytest.fixture(scope="module")
def wanted(overlapping, font_reference):
    """the reference's image of every input (those of the fixtures above are not made twice)"""
    out = {name: M.encode(overlapping[name][0], 4) for name, _, _, _ in OC.inputs()}
    out.update(font_reference)
    for name, segs, w, h in OC.tie_inputs():
        out[name] = OR.generate(segs, w, h, 4)
    for name, segs, w, h, R, _ in MC.hostile_inputs():
        out["hostile: " + name] = OR.generate(segs, w, h, R)
    return out


def test_the_generator_source_under_a_host_shim(emulated, wanted, overlapping):
    over = {}
    for name, segs, w, h, R in all_inputs():
        n = MC.over_tolerance(emulated[name]["union"], wanted[name])
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels are more than 1 LSB from the reference"
        cs, o = OR.contours(segs)
        assert emulated[name]["contours"] == (len(cs), sum(o * a < 0.0 for _, a in cs)), f"{name}: the host's contours and holes"
        if len(cs) <= 1:
            assert np.array_equal(emulated[name]["union"], emulated[name]["plain"]), f"{name}: a single contour is step 4's"
    print(f"texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")
    assert len(emulated) == 16 + 2 + 106 + 71
    for name, segs, w, h in OC.inputs():  # the sign test on the shim's texels
        d, inside = overlapping[name]
        OC.check_sign(name, emulated[name]["union"], segs, w, h, 4, d[..., 3], inside)
    for name, segs, w, h, R in MC.inputs():
        MC.check_sign(name, emulated[name]["union"], segs, w, h, R)


def test_the_generator_source_under_permuted_contours(shim, emulated, overlapping):
    """the kernel's source, not only the reference, under another contour order: every outline of two or more contours reversed and once
    permuted, through the shim, against the reference of the permuted outline under the cap; A byte-equal to the shim's own A in the
    original order.  And the tie outline: float32 against float64 of the reference is 0 there, so it is on no tie in float32's sense."""
    rng = np.random.RandomState(7)
    for name, segs, w, h in OC.inputs() + OC.tie_inputs():
        cs = [rows for rows, _ in OR.contours(segs)[0]]
        if name == "a square twice":
            continue
        for order in (list(range(len(cs)))[::-1], list(rng.permutation(len(cs)))):
            permuted = OC.join(*(cs[k] for k in order))
            got = _through_the_shim(shim, "wave", f"{name} {order}", permuted, w, h, 4)["union"]
            assert MC.over_tolerance(got, OR.generate(permuted, w, h, 4)) <= MC.CAP, f"{name}: contour order {order}"
            assert np.array_equal(got[..., 3], emulated[name]["union"][..., 3]), f"{name}: A under contour order {order}"
    for name, segs, w, h in OC.tie_inputs():
        assert MC.over_tolerance(OR.generate(segs, w, h, 4, np.float32), OR.generate(segs, w, h, 4)) == 0


def test_culling_off_gives_identical_texels(shim, emulated):
    for name, segs, w, h, R in all_inputs():
        off = _through_the_shim(shim, "lane_nocull", name, segs, w, h, R)
        assert np.array_equal(off["union"], emulated[name]["union"]), f"{name}: k_msdf_generate_union with and without culling"
        assert np.array_equal(off["plain"], emulated[name]["plain"]), f"{name}: k_msdf_generate with and without culling"


def test_16383_contours(shim):
    """the most whole squares the call accepts, each a contour of its own: as many filled contours with equal A, the same texels as one"""
    many = np.tile(SQUARE, (16383, 1))
    want = M.generate(SQUARE, 16, 16, 4)
    for exe in ("lane", "lane_nocull"):
        got = _through_the_shim(shim, exe, "16383 squares", many, 16, 16, 4)
        assert got["contours"] == (16383, 0)
        assert MC.over_tolerance(got["union"], want) <= MC.CAP and MC.over_tolerance(got["plain"], want) <= MC.CAP
        assert np.array_equal(got["union"], _through_the_shim(shim, exe, "one square", SQUARE, 16, 16, 4)["union"])


def test_the_correction_with_both_flags(emulated):
    """k_msdf_correct_union on the shim's own union field: step 5's invariants exactly (m and A unchanged, only marked texels differ, and
    those have R = G = B), and the bytes of msdf_overlap_ref.correct on the same field but for step 5's cap of 1 texel per image"""
    over, changed = {}, 0
    for name, segs, w, h, R in all_inputs():
        F, G = emulated[name]["union"], emulated[name]["corrected"]
        want, marked, _ = OR.correct(F, segs, R)
        n = differing(G, want)
        if n:
            over[name] = n
        assert n <= CORRECT_CAP, f"{name}: {n} texels differ from the reference's correction of the same field"
        got_marked = (G != F).any(axis=2)
        assert int((got_marked != marked).sum()) <= CORRECT_CAP, f"{name}: the marked set"
        assert np.array_equal(G[..., 3], F[..., 3]) and np.array_equal(MC.median3(G), MC.median3(F)), f"{name}: alpha or a median moved"
        gm = G[got_marked]
        assert (gm[:, 0] == gm[:, 1]).all() and (gm[:, 1] == gm[:, 2]).all(), f"{name}: a marked texel's channels disagree"
        changed += int(got_marked.sum())
    print(f"texels that differ from correct(F_shim) per image (cap {CORRECT_CAP}): {over or 'none in any image'}; {changed} texels changed in all")
    assert changed > 0
    # the verdict distance is step 6's: in one square and just outside the other step 4's distance is negative, and a candidate there whose
    # interpolated median is outside would go free
    two = OC.join(OC.rect(4, 4, 16, 16), OC.rect(10, 10, 22, 22))
    q = (np.array([9.5], np.float32), np.array([12.5], np.float32))
    assert OR.true_distance(two, *q)[0] == 3.5 and CR.true_distance(M.build_shape(two), *q)[0] == -0.5


def test_the_shim_under_sanitizers(shim, emulated):
    """the same stand-alone program built with -fsanitize=address,undefined, run directly: holes and filled contours, 17 x 9 (a tile edge one
    texel inside the image), 9 x 1, and an outline without edges; same bytes as the plain build"""
    cases = [c for c in all_inputs() if c[0] in ("round ring plus diagonal bar, reversed", "five nested squares plus one hole", "a square twice", "* x2")]
    cases += [("17 x 9", OC.join(OC.rect(2.25, 1.75, 11, 7.25), OC.rect(8.25, 3.25, 15.5, 8.5)), 17, 9, 2), ("9 x 1", OC.join(MC.poly([(1, -3), (8, 0.5), (2, 4)]), OC.rect(0.25, -1, 4.25, 2)), 9, 1, 2),
              ("0 segments", np.zeros((0, 6), np.float32), 12, 11, 4)]
    assert len(cases) == 7
    for name, segs, w, h, R in cases:
        san = _through_the_shim(shim, "wave_san", name, segs, w, h, R)
        plain = emulated[name] if name in emulated else _through_the_shim(shim, "wave", name, segs, w, h, R)
        for k in ("plain", "union", "corrected"):
            assert np.array_equal(san[k], plain[k]), f"{name}: {k}"
        if name == "0 segments":
            assert not san["union"].any() and not san["corrected"].any()
        elif name not in emulated:
            assert MC.over_tolerance(san["union"], OR.generate(segs, w, h, R)) <= MC.CAP
