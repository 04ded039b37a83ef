"""Distance-field generation (fdh_put_glyph_outline with FDH_GLYPH_MTSDF), what a CPU can check: the flag on a record-only context, known
answers for the reference tests/msdf_ref.py itself, the source of k_msdf_generate and fdh_msdf_host.h under the host shim of
tests/emu (tests/msdf_emu) against that reference on all 94 + 12 inputs, the sign of the field against the winding test, the same on the hostile
outlines of msdf_cases.hostile_inputs(), and how well the field reconstructs coverage through the oracle's draw_msdf (measured:
profiles/msdf.txt)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emu_build
import msdf_cases as MC
import msdf_ref as M
from figdraw_amd.context import HipContext

ROOT = MC.ROOT
INVALID = -1
MTSDF, LCD_FILTER, LCD_CONTEXT = 4, 1, 2


def RANGE(r):
    return r << 8


# ------------------------------------------------------------------------------------------------------------------ 1. the flag
def test_flag_on_a_record_only_context():
    src = open(os.path.join(ROOT, "include", "figdraw_hip.h")).read()
    assert re.search(r"\bFDH_GLYPH_MTSDF\s*=\s*4\b", src)
    assert re.search(r"#define\s+FDH_GLYPH_SDF_RANGE\(r\)\s+\(\(uint32_t\)\(r\)\s*<<\s*8\)", src)
    ctx = HipContext(record_only=True)
    square = MC.poly([(2, 2), (10, 2), (10, 9), (2, 9)])
    rect = ctx.put_glyph_outline(71, square, 12, 11, mtsdf=True, sdf_range=4)
    assert rect[2:] == (12, 11) and rect[0] >= 0 and rect[1] >= 0
    assert ctx.has_image(71)
    assert ctx.put_glyph_outline(72, square, 12, 11, mtsdf=True)[2:] == (12, 11)  # range 0 = 4
    assert ctx.put_glyph_outline(73, square, 12, 11)[2:] == (12, 11)  # without the flag: as before

    def rc(flags, segs=square, key=80):
        segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 6)
        out = (C.c_int * 4)()
        return ctx.L.fdh_put_glyph_outline(ctx.h, key, 12, 11, segs.ctypes.data, len(segs), flags, out)

    assert rc(MTSDF | RANGE(64)) == 0 and rc(MTSDF | RANGE(1)) == 0
    assert rc(MTSDF | LCD_FILTER) == INVALID
    assert rc(MTSDF | LCD_CONTEXT) == INVALID
    assert rc(MTSDF | RANGE(4) | LCD_FILTER) == INVALID
    assert rc(RANGE(4)) == INVALID                # a range without the flag
    assert rc(LCD_FILTER | RANGE(2)) == INVALID
    assert rc(MTSDF | RANGE(65)) == INVALID       # above 64
    assert rc(MTSDF | RANGE(255)) == INVALID
    assert rc(8) == INVALID and rc(MTSDF | 1 << 16) == INVALID  # bits that are still unknown
    many = np.tile(square, (16384, 1))            # 65536 segments
    assert rc(MTSDF, many) == INVALID
    assert rc(MTSDF, many[:65532]) == 0           # 65532 segments (16383 squares): the most whole squares under the limit
    assert rc(0, many) == 0                       # coverage has no such limit
    assert rc(MTSDF, square[:3], key=81) == INVALID and not ctx.has_image(81)  # an open contour: refused before anything is packed
    # the diagnostic's new value needs a device like the others
    buf = (C.c_uint8 * 16)()
    assert ctx.L.fdh_debug_read_surface(ctx.h, 4, buf) == ctx.L.fdh_debug_read_surface(ctx.h, 0, buf) != 0
    ctx.close()


def test_an_empty_outline_on_a_record_only_context():
    """an outline without edges is no error (step 4 of the specification): 0 segments, and segments that step 1 all drops, pack like any other"""
    ctx = HipContext(record_only=True)
    assert ctx.put_glyph_outline(90, np.zeros((0, 6), np.float32), 12, 11, mtsdf=True, sdf_range=4)[2:] == (12, 11) and ctx.has_image(90)
    out = (C.c_int * 4)()
    assert ctx.L.fdh_put_glyph_outline(ctx.h, 91, 12, 11, None, 0, MTSDF | RANGE(4), out) == 0 and tuple(out)[2:] == (12, 11)  # no pointer is needed for none
    back = np.array([[6, 5, 40, 5.5, 6, 5], [3, 3, MC.NAN, MC.NAN, 3, 3]], np.float32)
    assert ctx.put_glyph_outline(92, back, 12, 11, mtsdf=True)[2:] == (12, 11) and ctx.has_image(92)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the reference
def test_reference_known_answers():
    R = 4
    # an axis-aligned rectangle at fractional coordinates
    x0, y0, x1, y1 = 6.8, 5.7, 21.6, 17.2
    w, h = 28, 24
    segs = MC.poly([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])
    f = segs.astype(np.float64)
    x0, y0, x1, y1 = f[0, 0], f[0, 1], f[1, 4], f[2, 5]  # as float32 holds them
    sh = M.build_shape(segs)
    cols = sh.colours()
    assert len(cols) == 4 and len(set(cols)) == 3 and all(cols[i] != cols[(i + 1) % 4] for i in range(4))
    assert cols == [M.MAGENTA, M.YELLOW, M.CYAN, M.YELLOW]
    img = M.generate(segs, w, h, R)
    ys, xs = np.mgrid[0:h, 0:w]
    px, py = xs + 0.5, ys + 0.5
    cx, cy, hw, hh = (x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0) / 2, (y1 - y0) / 2
    qx, qy = np.abs(px - cx) - hw, np.abs(py - cy) - hh
    box = -(np.hypot(np.maximum(qx, 0), np.maximum(qy, 0)) + np.minimum(np.maximum(qx, qy), 0))  # positive inside
    cheb = -np.maximum(qx, qy)
    step = R / 255.0
    dec = M.decode(img, R)
    clip = lambda d: np.clip(d, -R / 2, R / 2)
    assert np.abs(dec[..., 3] - clip(box)).max() <= step, "alpha is the Euclidean box distance"
    med = M.decode(MC.median3(img), R)
    assert np.abs(med - clip(cheb)).max() <= step, "the median keeps the corners sharp"
    outside_corner = (qx > 1) & (qy > 1) & (cheb > -1.5)
    assert outside_corner.any() and (med[outside_corner] - dec[..., 3][outside_corner] > 0.2).all()  # where alpha rounds them
    # reversing every contour: alpha byte-identical (and here the colours too: the field is the same shape's)
    rev = segs[::-1][:, [4, 5, 2, 3, 0, 1]]
    assert M.build_shape(rev).orient == -sh.orient
    assert np.array_equal(M.generate(rev, w, h, R)[..., 3], img[..., 3])
    # a lens of two quadratics: two corners -> magenta, yellow
    lens = np.array([[4, 12, 14, 0, 24, 12], [24, 12, 14, 24, 4, 12]], np.float32)
    assert M.build_shape(lens).colours() == [M.MAGENTA, M.YELLOW]
    rev = lens[::-1][:, [4, 5, 2, 3, 0, 1]]
    assert np.array_equal(M.generate(rev, 28, 24, R)[..., 3], M.generate(lens, 28, 24, R)[..., 3])
    # a teardrop: one corner, two quadratics meeting smoothly at the far side -> each split in three, two edges per colour from the corner round;
    # given starting at the smooth vertex, the walk still starts at the corner
    tear = np.array([[14, 4, 26, 20, 14, 20], [14, 20, 2, 20, 14, 4]], np.float32)
    one = M.build_shape(tear[::-1].copy())
    assert one.colours() == [M.MAGENTA, M.MAGENTA, M.YELLOW, M.YELLOW, M.CYAN, M.CYAN]
    assert np.array_equal(one.edges[0].p[0], [14, 4]) and np.array_equal(one.edges[5].p[2], [14, 4])
    for a, b in zip(one.edges, one.edges[1:] + one.edges[:1]):
        assert np.array_equal(a.p[2], b.p[0])
    # no corner: white
    circle = []
    for k in range(16):
        a0, a1 = k * np.pi / 8, (k + 1) * np.pi / 8
        am = (a0 + a1) / 2
        circle.append([14 + 8 * np.cos(a0), 12 + 8 * np.sin(a0), 14 + 8 / np.cos(np.pi / 16) * np.cos(am), 12 + 8 / np.cos(np.pi / 16) * np.sin(am),
                       14 + 8 * np.cos(a1), 12 + 8 * np.sin(a1)])
    circle = np.array(circle, np.float32)
    for k in range(16):
        circle[k, 0:2] = circle[k - 1, 4:6]
    assert M.build_shape(circle).colours() == [M.WHITE] * 16
    dec = M.decode(M.generate(circle, 28, 24, R), R)
    want = clip(8 - np.hypot(px[:24, :28] - 14, py[:24, :28] - 12))
    assert np.abs(dec[..., 3] - want).max() <= step + 0.01 and np.abs(dec[..., 0] - want).max() <= step + 0.01  # (16 quadratics are a circle to 0.002)
    with pytest.raises(M.OpenContour):
        M.build_shape(segs[:3])
    assert not M.generate(np.zeros((0, 6), np.float32), 5, 4, R).any()


# ------------------------------------------------------------------------------------------------------------------ 3 - 5. the kernel's source on a CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_msdf.hip + fdh_msdf_host.h compiled as plain C++ under the sequential shim of tests/emu with waves of one lane, with and without
    tile culling -> the directory of ./emu and ./emu_nocull"""
    # emu_nocull: the build without tile culling (tools/msdf_bench.py's second library): culling must not change a texel
    tmp = emu_build.build(tmp_path_factory, "msdf_emu", ("k_msdf.hip", "fdh_msdf_host.h"), {"emu": (), "emu_nocull": ("-DFDH_MSDF_NO_CULL=1",)}, flags=("-DEMU_LANES_ALONE",))
    # fdh_msdf_host.h compiles standalone
    (tmp / "alone.cpp").write_text('#include "fdh_msdf_host.h"\nint main() { fdh::msdf::Shape s; return fdh::msdf::build_shape(nullptr, 0, &s) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "alone.cpp", "-o", "alone"], cwd=tmp)
    assert subprocess.run(["./alone"], cwd=tmp).returncode == 0
    return tmp


@pytest.fixture(scope="module")
def emulated(shim):
    """every font input through the shim -> {name: (texels, edge records, orientation, texels of the build without culling)}"""
    out = {}
    for name, segs, w, h, R in MC.inputs():
        out[name] = _through_the_shim(shim, name, segs, w, h, R)
    # an open contour is refused by the host code too
    MC.poly([(1, 1), (5, 1), (5, 5)])[:2].tofile(shim / "segs.raw")
    assert subprocess.run(["./emu", "8", "8", "4", "segs.raw"], cwd=shim).returncode == 3
    return out


@pytest.fixture(scope="module")
def hostile(shim):
    """every hostile input through the shim and, once, through the float64 reference ->
    {name: (texels, edge records, orientation, texels without culling, the reference's shape, its distances in float64)}"""
    out = {}
    for name, segs, w, h, R, _ in MC.hostile_inputs():
        sh = M.build_shape(segs)
        out[name] = _through_the_shim(shim, name, segs, w, h, R) + (sh, M.distances(sh, w, h))
    return out


def _through_the_shim(tmp, name, segs, w, h, R):
    """-> (texels, edge records, orientation, texels of the build without culling)"""
    segs.tofile(tmp / "segs.raw")
    r = subprocess.run(["./emu_nocull", str(w), str(h), str(R), "segs.raw"], cwd=tmp, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{name}: {r.returncode} {r.stdout}{r.stderr}"
    nocull = np.fromfile(tmp / "texels.raw", np.uint8).reshape(h, w, 4)
    r = subprocess.run(["./emu", str(w), str(h), str(R), "segs.raw"], cwd=tmp, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{name}: {r.returncode} {r.stdout}{r.stderr}"
    rec = np.fromfile(tmp / "edges.raw", np.float32)
    return np.fromfile(tmp / "texels.raw", np.uint8).reshape(h, w, 4), rec[:-1].reshape(-1, 24), float(rec[-1]), nocull


def test_the_reference_in_float32_stays_inside_the_cap():
    """The cap of 2 texels per image is a condition on the inputs: the reference's own formulas in float32 against float64 must meet it
    before anything else is held to it.  (All 106 inputs do; none had to be replaced.)"""
    worst = 0
    for name, segs, w, h, R in MC.inputs():
        sh = M.build_shape(segs)
        n = MC.over_tolerance(M.encode(M.distances(sh, w, h, np.float32), R), M.encode(M.distances(sh, w, h), R))
        worst = max(worst, n)
        assert n <= MC.CAP, f"{name}: {n} texels of the float32 reference are more than 1 LSB from the float64 reference"
    print(f"float32 reference against float64: at most {worst} texels per image beyond 1 LSB")


def test_the_kernel_source_under_a_host_shim(emulated):
    over = {}
    for name, segs, w, h, R in MC.inputs():
        got, rec, orient, _ = emulated[name]
        sh = M.build_shape(segs)
        assert [int(c) for c in rec[:, 6]] == sh.colours(), f"{name}: the edge colours"
        assert np.array_equal(rec[:, 0:6].astype(np.float64), np.array([e.p.ravel() for e in sh.edges])), f"{name}: the edges"
        assert orient == sh.orient, f"{name}: the orientation"
        n = MC.over_tolerance(got, M.encode(M.distances(sh, w, h), R))
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels are more than 1 LSB from the reference"
    print(f"texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")
    assert len(emulated) == 106


def test_tile_culling_changes_no_texel(emulated):
    for name, (texels, _, _, nocull) in emulated.items():
        assert np.array_equal(texels, nocull), f"{name}: {int((texels != nocull).any(axis=2).sum())} texels differ with culling off"


def test_sign_against_the_winding_number(emulated):
    checked = 0
    for name, segs, w, h, R in MC.inputs():
        checked += MC.check_sign(name + " (reference)", M.generate(segs, w, h, R), segs, w, h, R)
        MC.check_sign(name + " (kernel source)", emulated[name][0], segs, w, h, R)
    assert checked > 100000


# ------------------------------------------------------------------------------------------------------------------ 6. hostile outlines
def test_hostile_the_reference_in_float32_stays_inside_the_cap(hostile):
    """(a) the same condition on the hostile inputs: one that fails it is replaced, never excused"""
    over = {}
    for name, segs, w, h, R, _ in MC.hostile_inputs():
        sh, d64 = hostile[name][4:6]
        n = MC.over_tolerance(M.encode(M.distances(sh, w, h, np.float32), R), M.encode(d64, R))
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels of the float32 reference are more than 1 LSB from the float64 reference"
    print(f"float32 reference against float64, texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")


def test_hostile_the_kernel_source_under_a_host_shim(hostile):
    """(b)"""
    over = {}
    for name, segs, w, h, R, _ in MC.hostile_inputs():
        got, rec, orient, _, sh, d64 = hostile[name]
        assert [int(c) for c in rec[:, 6]] == sh.colours(), f"{name}: the edge colours"
        assert np.array_equal(rec[:, 0:6].astype(np.float64), np.array([e.p.ravel() for e in sh.edges]).reshape(-1, 6)), f"{name}: the edges"
        assert orient == sh.orient, f"{name}: the orientation"
        n = MC.over_tolerance(got, M.encode(d64, R))
        if n:
            over[name] = n
        assert n <= MC.CAP, f"{name}: {n} texels are more than 1 LSB from the reference"
    print(f"texels beyond 1 LSB per image (cap {MC.CAP}): {over or 'none in any image'}")
    assert len(hostile) == len(MC.hostile_inputs()) >= 70


def test_hostile_tile_culling_changes_no_texel(hostile):
    """(c)"""
    for name, (texels, _, _, nocull, _, _) in hostile.items():
        assert np.array_equal(texels, nocull), f"{name}: {int((texels != nocull).any(axis=2).sum())} texels differ with culling off"


def test_hostile_sign_against_the_winding_number(hostile):
    """(d) on every outline that does not cross itself.  Where the reference and the winding number disagree the winding number is right:
    that is what made step 1 of the specification turn folded quadratics into lines."""
    checked = 0
    for name, segs, w, h, R, simple in MC.hostile_inputs():
        if not simple:
            continue
        got, _, _, _, _, d64 = hostile[name]
        inside = MC.winding(segs, w, h) != 0
        n = MC.check_sign(name + " (reference)", M.encode(d64, R), segs, w, h, R, d64[..., 3], inside)
        assert n == MC.check_sign(name + " (kernel source)", got, segs, w, h, R, d64[..., 3], inside) > 0
        checked += n
    print(f"{checked} texels checked")


def test_hostile_folded_quadratics_are_lines(hostile):
    """step 1 on the cases that made it: the reference's shape (which the shim's records equal, see above)"""
    rect = M.build_shape(MC.poly([(4, 4), (28, 4), (28, 20), (4, 20)]))
    sh = hostile["quadratic folded onto its line"][4]
    assert all(e.line for e in sh.edges) and np.array_equal([e.p for e in sh.edges], [e.p for e in rect.edges]) and sh.colours() == rect.colours()
    assert [e.line for e in hostile["collinear control point inside the chord"][4].edges] == [False, True, True, True]  # an ordinary curve: kept
    for name in ("control point on P2", "control point on P0"):
        assert [e.line for e in hostile[name][4].edges] == [True] * 4, name
    for name, k in (("control point 1e-05 from P2", 1), ("control point 1e-05 from P0", 1), ("control point 0.001 off the chord", 0)):  # off the line: kept
        assert [e.line for e in hostile[name][4].edges] == [i != k for i in range(4)], name
    texels, rec, _, _, sh, _ = hostile["one edge doubling back on itself"]
    assert not sh.edges and rec.size == 0 and not texels.any()


def test_reconstruction_through_draw_msdf(emulated):
    """The field drawn by the oracle's draw_msdf (px_range 4, on black) at scales 1 and 3 against the box coverage of the outline scaled
    likewise, over the 94 inputs with R = 4.  A field without error correction does not match box coverage; by how much is measured
    here and written down in profiles/msdf.txt.  Asserted: the kernel's texels reconstruct as well as the reference's, within a quarter
    of an LSB in the mean and in the 99th percentile (their texels differ by 1 LSB at most, which a scale of 3 multiplies to about 12
    LSB on an edge pixel, on few pixels)."""
    from oracle import oracle as O

    orc = O.Oracle(atlas_size=2048, threads=4)
    cases = [c for c in MC.inputs() if c[4] == 4]
    assert len(cases) == 94
    for i, (name, segs, w, h, R) in enumerate(cases):
        orc.put_image(1000 + i, M.generate(segs, w, h, R))
        orc.put_image(3000 + i, emulated[name][0])
    for scale in (1, 3):
        ref = np.concatenate([MC.reconstruction_error(orc, O.rasterize_outline, 1000 + i, c[1], c[2], c[3], scale) for i, c in enumerate(cases)])
        emu = np.concatenate([MC.reconstruction_error(orc, O.rasterize_outline, 3000 + i, c[1], c[2], c[3], scale) for i, c in enumerate(cases)])
        rm, r99, em, e99 = ref.mean(), np.percentile(ref, 99), emu.mean(), np.percentile(emu, 99)
        print(f"scale {scale}: |alpha - coverage| in LSB over {ref.size} pixels: reference mean {rm:.3f}, 99th percentile {r99:.1f}, max {ref.max()}; "
              f"kernel source mean {em:.3f}, 99th percentile {e99:.1f}, max {emu.max()}")
        assert em <= rm + 0.25 and e99 <= r99 + 0.25
