"""Glyph outlines with cubic segments (fdh_put_glyph_outline_cubic, include_glyphs/figdraw_hip_cubic.h), what a CPU can check: the call's
rules on a record-only context and through C99; known answers for the reference tests/msdf_cubic_ref.py itself; the inputs of
msdf_cubic_cases.py against the cap (the float32 reference against the float64 one); the source of k_msdf_cubic.hip and
fdh_msdf_cubic_host.h under the host shim of tests/emu (tests/msdf_cubic_emu) against that reference; and the host's flattening for the coverage path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emu_build
import msdf_cases as MC
import msdf_cubic_cases as CC
import msdf_cubic_ref as R
import msdf_ref as M
from figdraw_amd import context
from figdraw_amd.context import HipContext

ROOT = MC.ROOT
INVALID = -1
LCD_FILTER, LCD_CONTEXT, MTSDF, CORRECT, OVERLAP = 1, 2, 4, 8, 32
CORRECT_CAP = 1  # test_msdf_correct_host.py's: a verdict may flip where |d(q)| is within rounding of R / 255


def RANGE(r):
    return r << 8


def all_inputs():
    """-> [(name, segs8, w, h, R, simple)]: the 106 skewed font outlines, the hostile set, the analytic shapes"""
    return [c + (True,) for c in CC.skewed()] + CC.hostile() + [c[:5] + (True,) for c in CC.analytic()]


BOX = CC.cpath((2, 4), (4, -2, 8, 8, 10, 4), (10, 9), (2, 9), (2, 4))  # in 12 x 11: a box whose top side is a cubic
QUAD_BOX = MC.path((2, 4), (6, 0, 10, 4), (10, 9), (2, 9), (2, 4))      # the 6-float format


# ------------------------------------------------------------------------------------------------------------------ 1. the call
def test_rules_on_a_record_only_context():
    src = open(os.path.join(ROOT, "include_glyphs", "figdraw_hip_cubic.h")).read()
    assert "fdh_put_glyph_outline_cubic" in src and '#include "../include/figdraw_hip.h"' in src
    assert "figdraw_hip_cubic.h" in open(os.path.join(ROOT, "include", "figdraw_hip.h")).read()
    ctx = HipContext(record_only=True)
    rect = ctx.put_glyph_outline_cubic(71, BOX, 12, 11, mtsdf=True, sdf_range=4, correct=True)
    assert rect[2:] == (12, 11) and rect[0] >= 0 and rect[1] >= 0 and ctx.has_image(71)
    assert ctx.put_glyph_outline_cubic(72, BOX, 12, 11)[2:] == (12, 11)  # coverage
    assert ctx.put_glyph_outline_cubic(73, BOX, 12, 11, lcd_filter=True)[2:] == (12, 11) and ctx.put_glyph_outline_cubic(74, BOX, 12, 11, lcd_filter="context")[2:] == (12, 11)

    def rc(flags, segs=BOX, key=80, w=12, h=11, n=None, null=False):
        segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 8)
        out = (C.c_int * 4)()
        return ctx.L.fdh_put_glyph_outline_cubic(ctx.h, key, w, h, None if null else segs.ctypes.data, len(segs) if n is None else n, flags, out)

    key = 100

    def refused(*a, **k):
        nonlocal key
        key += 1
        return rc(*a, key=key, **k) == INVALID and not ctx.has_image(key)

    assert rc(MTSDF) == 0 and rc(MTSDF | RANGE(1)) == 0 and rc(MTSDF | RANGE(64) | CORRECT) == 0 and rc(0) == 0
    assert refused(MTSDF | OVERLAP) and refused(MTSDF | OVERLAP | CORRECT)          # with a cubic in the outline
    assert refused(OVERLAP)
    assert refused(MTSDF | RANGE(65)) and refused(RANGE(4)) and refused(CORRECT) and refused(CORRECT | LCD_FILTER)
    assert refused(MTSDF | LCD_FILTER) and refused(MTSDF | LCD_CONTEXT)
    assert refused(MTSDF | 16) and refused(MTSDF | 1 << 16) and refused(64)
    assert refused(MTSDF, w=0) and refused(MTSDF, h=4097) and refused(0, w=4097)
    assert refused(MTSDF, BOX[:3])                                                  # an open contour
    assert refused(MTSDF, n=-1) and refused(MTSDF, null=True)
    assert rc(MTSDF, np.zeros((0, 8), np.float32), key=90, null=True) == 0 and ctx.has_image(90)  # n_segs = 0 with a NULL pointer
    assert rc(0, np.zeros((0, 8), np.float32), key=91, null=True) == 0 and ctx.has_image(91)
    many = np.tile(BOX, (16384, 1))  # 65536 segments
    assert refused(MTSDF, many) and rc(MTSDF, many[:65535 - 3], key=92) == 0        # 65532 = whole boxes; one more segment would open a contour
    assert refused(MTSDF, many[:65535]) is True                                     # 65535 segments pass the limit and fail as an open contour ...
    assert "closed contours" in ctx.L.fdh_last_error().decode()
    assert refused(MTSDF, many[:65536]) and "65535" in ctx.L.fdh_last_error().decode()  # ... 65536 fail at the limit
    assert rc(0, many, key=93) == 0                                                 # coverage has no such limit
    ctx.close()


def test_a_cubic_free_outline_is_the_old_call_on_a_record_only_context():
    """equal rectangles and equal refusals, every flag the old call takes"""
    eight = CC.lift(QUAD_BOX)
    for flags in (0, LCD_FILTER, LCD_CONTEXT, MTSDF, MTSDF | CORRECT | RANGE(8), MTSDF | OVERLAP, MTSDF | LCD_FILTER, OVERLAP, RANGE(4), MTSDF | RANGE(65), 16):
        got = []
        for cubic in (False, True):
            ctx = HipContext(record_only=True)
            ctx.put_image(1, np.zeros((5, 7, 4), np.uint8))
            out = (C.c_int * 4)()
            segs = eight if cubic else QUAD_BOX
            f = ctx.L.fdh_put_glyph_outline_cubic if cubic else ctx.L.fdh_put_glyph_outline
            got.append((f(ctx.h, 2, 12, 11, segs.ctypes.data, len(segs), flags, out), tuple(out), ctx.has_image(2)))
            ctx.close()
        assert got[0] == got[1], flags


def test_cubic_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "cubic_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "cubic_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cubic_abi_smoke: OK" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ 2. the reference
def test_reference_step_1_and_2():
    kinds = {name: [e.kind for e in R.build_shape(segs).edges] for name, segs, *_ in CC.hostile()}
    assert kinds["S-curve with an inflection"][0] == R.CUBIC
    for name in ("P1 = P0 and P2 = P3", "collinear, controls inside the chord", "collinear, controls beyond the ends"):
        assert kinds[name] == [R.LINE] * 4, name
    assert kinds["P1 = P0 only"][0] == R.CUBIC and kinds["P2 = P3 only"][0] == R.CUBIC
    assert kinds["third difference just above the threshold"][0] == R.CUBIC and kinds["third difference just below the threshold"][0] == R.QUADRATIC
    assert kinds["self-touching lobe"] == [R.CUBIC] * 3                              # one edge, one corner, m < 3: thirds
    assert kinds["one-corner contour of one cubic and a line"] == [R.CUBIC, R.LINE]  # two corners: no split
    point = np.array([[3, 3, 3, 3, 3, 3, 3, 3]], np.float32)
    assert not R.build_shape(point).edges                                            # all four equal: dropped
    back = np.array([[3, 3, 9, 9, 5, 5, 3, 3]], np.float32)
    assert not R.build_shape(back).edges                                             # P0 = P3, controls on one line through it: out and back
    with pytest.raises(R.OpenContour):
        R.build_shape(BOX[:3])
    # the thirds keep the original ends and meet bit for bit
    lobe = R.build_shape(CC.hostile()[12][1]).edges
    assert CC.hostile()[12][0] == "self-touching lobe"
    assert (lobe[0].p[0] == lobe[2].p[3]).all() and (lobe[0].p[3] == lobe[1].p[0]).all() and (lobe[1].p[3] == lobe[2].p[0]).all()
    assert [e.colour for e in lobe] == [M.MAGENTA, M.YELLOW, M.CYAN]
    # step 2 against a dense polygon
    e = R.Edge([[1, 2], [5, -3], [9, 8], [4, 4]], R.CUBIC)
    t = np.linspace(0, 1, 200001)[:, None]
    B = (1 - t) ** 3 * e.p[0] + 3 * (1 - t) ** 2 * t * e.p[1] + 3 * (1 - t) * t * t * e.p[2] + t ** 3 * e.p[3]
    assert abs(R.edge_area(e) - 0.5 * np.sum(B[:-1, 0] * B[1:, 1] - B[1:, 0] * B[:-1, 1])) < 1e-8
    assert R.build_shape(CC.circle()).orient == 1.0 and R.build_shape(reverse(CC.circle())).orient == -1.0


def reverse(segs8):
    """every contour run the other way: the segments in reverse order, each one's points reversed (whole outline: for one contour)"""
    s = np.asarray(segs8, np.float32).reshape(-1, 8)[::-1].copy()
    out = s[:, [6, 7, 4, 5, 2, 3, 0, 1]].copy()
    quad = np.isnan(s[:, 4]) & ~np.isnan(s[:, 2])
    out[quad, 2:4], out[quad, 4:6] = s[quad, 2:4], np.nan
    line = np.isnan(s[:, 2])
    out[line, 2:6] = np.nan
    return out


def test_reference_on_the_analytic_shapes():
    """alpha within one quantisation step plus 0.003 texel of the exact distance: the arcs' radial error is 2.7e-4 r = 0.0022 at r = 8"""
    for name, segs, w, h, Rr, exact in CC.analytic():
        img = R.generate(segs, w, h, Rr)
        ys, xs = np.mgrid[0:h, 0:w]
        want = np.clip(exact(xs + 0.5, ys + 0.5), -Rr / 2, Rr / 2)
        err = np.abs(M.decode(img[..., 3], Rr) - want).max()
        print(f"{name}: max |alpha - exact| = {err:.5f} texels")
        assert err <= Rr / 255.0 + 0.003, name
        assert [e.colour for e in R.build_shape(segs).edges] == [M.WHITE] * len(segs)  # no corner anywhere


@pytest.fixture(scope="module")
def reference():
    """every input through the float64 reference once -> {name: (distances, texels)}"""
    out = {}
    for name, segs, w, h, Rr, _ in all_inputs():
        d = R.distances(R.build_shape(segs), w, h)
        out[name] = (d, M.encode(d, Rr))
    return out


def test_colours_of_the_skewed_font_set_are_the_quadratic_outlines():
    n_cubic = 0
    for (name, segs8, w, h, Rr), (_, segs6, _, _, _) in zip(CC.skewed(), MC.inputs()):
        a, b = R.build_shape(segs8), M.build_shape(segs6)
        assert [e.colour for e in a.edges] == b.colours() and a.contour == b.contour and a.orient == b.orient, name
        n_cubic += sum(e.kind == R.CUBIC for e in a.edges)
    assert n_cubic > 1000


def test_degree_elevated_quadratics_give_the_quadratic_field():
    """s = 0: step 1 turns every cubic back into a quadratic (its control point rounded to float32 once more), and the image is within 1 LSB
    of msdf_ref's on the original outline"""
    for (name, segs8, w, h, Rr), (_, segs6, _, _, _) in list(zip(CC.skewed(0.0), MC.inputs()))[::4]:
        shape = R.build_shape(segs8)
        assert not any(e.kind == R.CUBIC for e in shape.edges), name
        assert MC.over_tolerance(M.encode(R.distances(shape, w, h), Rr), M.generate(segs6, w, h, Rr)) == 0, name


def test_reversing_every_contour_leaves_alpha(reference):
    """one-contour outlines of the hostile set and the analytic shapes, run the other way: the orientation flips, alpha's bytes do not"""
    n = 0
    for name, segs, w, h, Rr, _ in CC.hostile() + [c[:5] + (True,) for c in CC.analytic()]:
        if len(set(R.build_shape(segs).contour)) != 1:
            continue
        rev = R.generate(reverse(segs), w, h, Rr)
        assert np.array_equal(rev[..., 3], reference[name][1][..., 3]), name
        n += 1
    assert n >= 30


def test_the_reference_in_float32_stays_inside_the_cap(reference):
    """the cap of msdf_cases.CAP texels per image is a condition on the inputs, checked first"""
    over = {}
    for name, segs, w, h, Rr, _ in all_inputs():
        n = MC.over_tolerance(R.generate(segs, w, h, Rr, np.float32), reference[name][1])
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels of the float32 reference are more than 1 LSB from the float64 reference"
    print(f"float32 reference against float64, texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")
    assert len(reference) == 106 + len(CC.hostile()) + 2


# ------------------------------------------------------------------------------------------------------------------ 3. the kernels' source on a CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_msdf_cubic.hip + fdh_msdf_cubic_host.h (and k_msdf.hip + fdh_msdf_host.h) compiled as plain C++ under the sequential shim of tests/emu
    with the driver of tests/msdf_cubic_emu -> the directory of ./emu, ./emu_nocull (every tile walks every edge) and ./emu_san: the same
    stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "msdf_cubic_emu", ("k_msdf_cubic.hip", "fdh_msdf_cubic_host.h", "k_msdf.hip", "fdh_msdf_host.h"),
                           {"emu": (), "emu_nocull": ("-DFDH_MSDF_NO_CULL=1",), "emu_san": emu_build.SAN})


def _through_the_shim(tmp, name, segs, w, h, Rr, exe="./emu"):
    """-> (uncorrected texels, corrected texels, k_msdf_generate's texels or None, {workgroups, with_rounds, rounds, lines, quadratics, cubics})"""
    np.ascontiguousarray(segs, np.float32).tofile(tmp / "segs.raw")
    if os.path.exists(tmp / "plain.raw"):
        os.remove(tmp / "plain.raw")
    r = subprocess.run([exe, str(w), str(h), str(Rr), "segs.raw"], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name}: {r.returncode} {r.stdout}{r.stderr}"
    stats = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", r.stdout)}
    read = lambda f: np.fromfile(tmp / f, np.uint8).reshape(h, w, 4)
    return read("texels.raw"), read("corrected.raw"), read("plain.raw") if os.path.exists(tmp / "plain.raw") else None, stats


@pytest.fixture(scope="module")
def emulated(shim):
    return {name: _through_the_shim(shim, name, segs, w, h, Rr) for name, segs, w, h, Rr, _ in all_inputs()}


def test_the_kernel_source_against_the_reference(emulated, reference):
    over, cubics = {}, 0
    for name, segs, w, h, Rr, _ in all_inputs():
        n = MC.over_tolerance(emulated[name][0], reference[name][1])
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels are more than 1 LSB from the reference"
        cubics += emulated[name][3]["cubics"]
    print(f"texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}; {cubics} cubic edges in all")
    assert cubics > 1000


def test_the_correction_source_against_the_reference(emulated):
    """correct(F_shim, float64) against the shim's corrected texels, and step 5's invariants exactly"""
    over, rounds = {}, 0
    for name, segs, w, h, Rr, _ in all_inputs():
        F, G, _, stats = emulated[name]
        want, marked, _ = R.correct(F, segs, Rr)
        n = int((G != want).any(axis=2).sum())
        if n:
            over[name] = n
        assert n <= CORRECT_CAP, f"{name}: {n} texels differ from the reference's correction of the same field"
        got_marked = (G != F).any(axis=2)
        assert np.array_equal(G[..., 3], F[..., 3]) and np.array_equal(MC.median3(G), MC.median3(F)), f"{name}: alpha or a median moved"
        assert np.array_equal(G[~got_marked], F[~got_marked])
        gm = G[got_marked]
        assert (gm[:, 0] == gm[:, 1]).all() and (gm[:, 1] == gm[:, 2]).all(), name
        rounds += stats["rounds"]
    print(f"texels that differ from correct(F_shim) per image (cap {CORRECT_CAP}): {over or 'none in any image'}; {rounds} rounds in all")
    assert rounds > 0


def test_culling_changes_no_texel(shim, emulated):
    for name, segs, w, h, Rr, _ in all_inputs()[::3] + CC.hostile():
        F, G, _, _ = _through_the_shim(shim, name, segs, w, h, Rr, exe="./emu_nocull")
        assert np.array_equal(F, emulated[name][0]) and np.array_equal(G, emulated[name][1]), name


def test_sign_of_the_emulated_texels(emulated, reference):
    checked = 0
    for name, segs, w, h, Rr, simple in all_inputs():
        if simple:
            inside = MC.winding(R.flatten(segs), w, h) != 0
            checked += MC.check_sign(name, emulated[name][0], None, w, h, Rr, reference[name][0][..., 3], inside)
    assert checked > 100000


def test_a_cubic_free_outline_gets_the_bytes_of_k_msdf_generate(shim):
    """lines and quadratics forced through k_msdf_generate_cubic's records and kernel against k_msdf_generate in the same emulator"""
    cases = [c[:5] for c in MC.inputs()[::5]] + [c[:5] for c in MC.hostile_inputs() if c[2] * c[3] <= 64 * 64]
    for name, segs6, w, h, Rr in cases:
        F, _, plain, stats = _through_the_shim(shim, name, CC.lift(segs6), w, h, Rr)
        assert plain is not None and stats["cubics"] == 0 and np.array_equal(F, plain), name
    assert len(cases) > 60


def test_the_shim_under_sanitizers(shim, emulated):
    """the stand-alone program built with -fsanitize=address,undefined, run directly: partial tiles, 1-texel images, every kind of edge"""
    names = ("S-curve with an inflection", "self-touching lobe", "cubic, quadratic and lines in one contour", "9 x 9 image", "cusp", "* x2")
    cases = [c for c in all_inputs() if c[0] in names]
    assert len(cases) == len(names)
    for name, segs, w, h, Rr, _ in cases:
        F, G, _, _ = _through_the_shim(shim, name, segs, w, h, Rr, exe="./emu_san")
        assert np.array_equal(F, emulated[name][0]) and np.array_equal(G, emulated[name][1]), name
    for w, h in ((1, 9), (9, 1), (17, 9)):
        segs = CC.cpath((1, 1), (5, -2, 10, 4, 8, 8), (1, 8), (1, 1))
        F, G, _, _ = _through_the_shim(shim, f"{w} x {h}", segs, w, h, 2, exe="./emu_san")
        assert MC.over_tolerance(F, R.generate(segs, w, h, 2)) <= MC.CAP
    F, G, plain, _ = _through_the_shim(shim, "0 segments", np.zeros((0, 8), np.float32), 9, 9, 4, exe="./emu_san")
    assert not F.any() and not G.any() and not plain.any()


# ------------------------------------------------------------------------------------------------------------------ 4. the coverage path
def test_flattening_for_the_coverage_path(shim):
    """the host's lines for a cubic outline: connected, ends kept, the chord count the header's formula, and every chord within 0.025 px of
    the curve (a dense evaluation in float64); lines and quadratics as fdh_put_glyph_outline flattens them (the oracle's formula)"""
    from oracle import oracle as O

    worst = 0.0
    cases = [c[:2] for c in CC.skewed()[::6]] + [c[:2] for c in CC.hostile()]
    for name, segs in cases:
        np.ascontiguousarray(segs, np.float32).tofile(shim / "segs.raw")
        subprocess.check_call(["./emu", "flatten", "segs.raw"], cwd=shim)
        lines = np.fromfile(shim / "lines.raw", np.float32).reshape(-1, 4)
        at = 0
        for q in np.asarray(segs, np.float32).reshape(-1, 8):
            if np.isnan(q[2]):
                k = 1
            elif np.isnan(q[4]):
                k = int(min(max(np.ceil(np.sqrt(np.float32(10) * np.sqrt(np.sum((q[0:2] - 2 * q[2:4] + q[6:8]) ** 2, dtype=np.float32)))), 1), 64))
            else:
                dev = np.sqrt(max(np.sum((q[0:2] - 2 * q[2:4] + q[4:6]) ** 2, dtype=np.float32), np.sum((q[2:4] - 2 * q[4:6] + q[6:8]) ** 2, dtype=np.float32)))
                k = int(min(max(np.ceil(np.sqrt(np.float32(30) * dev)), 1), 256))
            part = lines[at:at + k]
            at += k
            assert (part[0, :2] == q[0:2]).all() and (part[-1, 2:] == q[6:8]).all() and (part[1:, :2] == part[:-1, 2:]).all(), name
            if np.isnan(q[2]) or np.isnan(q[4]):
                continue
            P = q.astype(np.float64).reshape(4, 2)
            for j in range(k):  # the chord against the curve over its interval
                t = np.linspace(j / k, (j + 1) / k, 33)[:, None]
                B = (1 - t) ** 3 * P[0] + 3 * (1 - t) ** 2 * t * P[1] + 3 * (1 - t) * t * t * P[2] + t ** 3 * P[3]
                a, b = part[j, :2].astype(np.float64), part[j, 2:].astype(np.float64)
                d = b - a
                L = np.hypot(*d)
                dist = np.abs((B[:, 0] - a[0]) * d[1] - (B[:, 1] - a[1]) * d[0]) / L if L > 0 else np.hypot(*(B - a).T)
                worst = max(worst, float(dist.max()))
        assert at == len(lines), name
    print(f"largest distance of a cubic from its chord: {worst:.4f} px")
    assert 0.0 < worst <= 0.025
    # a cubic-free outline: the lines of the 6-float outline as the oracle flattens it, so the rasteriser sees what it saw
    name, segs6, w, h, _ = MC.inputs()[ord("g") - 33]
    CC.lift(segs6).tofile(shim / "segs.raw")
    subprocess.check_call(["./emu", "flatten", "segs.raw"], cwd=shim)
    got = np.fromfile(shim / "lines.raw", np.float32).reshape(-1, 4)
    L = O.lib()
    L.fo_flatten_outline.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    want = np.zeros((len(got) + 8, 4), np.float32)
    assert L.fo_flatten_outline(segs6.ctypes.data, len(segs6), want.ctypes.data, len(want)) == len(got)
    assert np.array_equal(got, want[:len(got)])


def test_the_python_restatement_of_the_flattening(shim):
    """msdf_cubic_cases.flatten_lines, which the device test feeds to the oracle's rasteriser, is the host's flattening bit for bit"""
    for name, segs in [c[:2] for c in CC.skewed()[::9]] + [c[:2] for c in CC.hostile()]:
        np.ascontiguousarray(segs, np.float32).tofile(shim / "segs.raw")
        subprocess.check_call(["./emu", "flatten", "segs.raw"], cwd=shim)
        assert np.array_equal(np.fromfile(shim / "lines.raw", np.float32).reshape(-1, 4), CC.flatten_lines(segs)), name
