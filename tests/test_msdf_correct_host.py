"""The distance-field correction pass (fdh_put_glyph_outline with FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT, step 5 of the specification in
include/figdraw_hip.h), what a CPU can check: the flag on a record-only context, known answers for the reference tests/msdf_correct_ref.py
itself, that reference in float32 against float64 on all 106 + 71 inputs (the cap is a condition on the inputs), the source of
k_msdf_correct under the host shim of tests/emu (tests/msdf_correct_emu) against the reference on the same inputs, and what the pass does to the
reconstruction of coverage through the oracle's draw_msdf (measured: profiles/msdf.txt, section 4)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emu_build
import msdf_cases as MC
import msdf_correct_ref as CR
import msdf_ref as M
from figdraw_amd.context import HipContext

ROOT = MC.ROOT
INVALID = -1
LCD_FILTER, LCD_CONTEXT, MTSDF, CORRECT = 1, 2, 4, 8
CAP = 1  # texels per image whose bytes may differ from correct(F, float64): a verdict may flip where |d(q)| is within rounding of R / 255


def RANGE(r):
    return r << 8


def all_inputs():
    """the 106 font inputs and the 71 hostile ones -> [(name, segs, w, h, R)].  None had to be replaced or dropped for the cap (see
    test_the_reference_in_float32_stays_inside_the_cap)."""
    return MC.inputs() + [c[:5] for c in MC.hostile_inputs()]


def differing(a, b):
    return int((a != b).any(axis=2).sum())


def check_invariants(name, F, G, marked):
    """what step 5 promises of every image, exactly: median and alpha unchanged, unmarked texels byte-equal, marked texels R = G = B"""
    assert np.array_equal(G[..., 3], F[..., 3]), f"{name}: alpha was touched"
    assert np.array_equal(MC.median3(G), MC.median3(F)), f"{name}: a median moved"
    assert np.array_equal(G[~marked], F[~marked]), f"{name}: an unmarked texel changed"
    gm = G[marked]
    assert (gm[:, 0] == gm[:, 1]).all() and (gm[:, 1] == gm[:, 2]).all(), f"{name}: a marked texel's channels disagree"


# ------------------------------------------------------------------------------------------------------------------ 1. the flag
def test_flag_on_a_record_only_context():
    src = open(os.path.join(ROOT, "include", "figdraw_hip.h")).read()
    assert re.search(r"\bFDH_GLYPH_MTSDF_CORRECT\s*=\s*8\b", src)
    ctx = HipContext(record_only=True)
    square = MC.poly([(2, 2), (10, 2), (10, 9), (2, 9)])
    rect = ctx.put_glyph_outline(71, square, 12, 11, mtsdf=True, sdf_range=4, correct=True)  # accepted, and the rectangle is packed
    assert rect[2:] == (12, 11) and rect[0] >= 0 and rect[1] >= 0 and ctx.has_image(71)
    assert ctx.put_glyph_outline(72, square, 12, 11, mtsdf=True, correct=True)[2:] == (12, 11)  # range 0 = 4

    def rc(flags, segs=square, key=80):
        segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 6)
        out = (C.c_int * 4)()
        return ctx.L.fdh_put_glyph_outline(ctx.h, key, 12, 11, segs.ctypes.data, len(segs), flags, out)

    assert rc(MTSDF | CORRECT) == 0 and rc(MTSDF | CORRECT | RANGE(1)) == 0 and rc(MTSDF | CORRECT | RANGE(64)) == 0
    assert rc(MTSDF) == 0 and rc(0) == 0                       # without the flag: as before
    assert rc(CORRECT) == INVALID                              # alone
    assert rc(CORRECT | RANGE(4)) == INVALID
    assert rc(CORRECT | LCD_FILTER) == INVALID and rc(CORRECT | LCD_CONTEXT) == INVALID
    assert rc(MTSDF | CORRECT | LCD_FILTER) == INVALID and rc(MTSDF | CORRECT | LCD_CONTEXT) == INVALID
    assert rc(MTSDF | CORRECT | RANGE(65)) == INVALID
    assert rc(MTSDF | CORRECT | 16) == INVALID and rc(MTSDF | CORRECT | 1 << 16) == INVALID  # bits that are still unknown
    assert rc(MTSDF | CORRECT, square[:3], key=81) == INVALID and not ctx.has_image(81)       # an open contour: refused before anything is packed
    assert rc(MTSDF | CORRECT, np.zeros((0, 6), np.float32), key=82) == 0 and ctx.has_image(82)  # an outline without edges is no error
    img = np.zeros((11, 12, 4), np.uint8)
    out = (C.c_int * 4)()
    for flags in (CORRECT, CORRECT | LCD_FILTER, CORRECT | MTSDF):  # fdh_put_glyph_image knows neither flag
        assert ctx.L.fdh_put_glyph_image(ctx.h, 83, 12, 11, img.ctypes.data, flags, out) == INVALID
    assert ctx.L.fdh_put_glyph_image(ctx.h, 83, 12, 11, img.ctypes.data, LCD_FILTER, out) == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 2. the reference
# One pair of texels, worked by hand.  a = (220, 220, 20), b = (60, 180, 180) (alpha 200 and 190): m(a) = 220, m(b) = 180, both inside.
#   (R, G): N = 220 - 220 = 0: no crossing.     (G, B): N = 200, D = 200 - (180 - 180) = 200: N < D fails, the channels meet at b's centre.
#   (R, B): N = 220 - 20 = 200, D = 200 - (60 - 180) = 320, t = 200 / 320 = 0.625.
#           V_R = 220 * 320 + 200 * (60 - 220) = 38400, V_G = 220 * 320 + 200 * (180 - 220) = 62400, V_B = 20 * 320 + 200 * (180 - 20) = 38400:
#           X = 38400, the interpolated median 38400 / 320 = 120; 2 X = 76800 < 255 * 320 = 81600: outside.  A candidate.
#   q = (0.5 + 0.625, 0.5) = (1.125, 0.5) for the horizontal pair a = texel (0, 0), b = texel (1, 0).
#   |2 m - 255| is 185 for a and 105 for b: an artefact marks a alone, which becomes (220, 220, 220).
# Whether it is an artefact is the shape's word: "the interpolated median is outside" is false where d(q) > R / 255 = 0.0157 (R = 4).
PAIR_A, PAIR_B = (220, 220, 20, 200), (60, 180, 180, 190)


def _box(x0, y0=-3.0, x1=9.0, y1=4.0):
    return MC.poly([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])


def test_reference_known_answers():
    F = np.array([[PAIR_A, PAIR_B]], np.uint8)  # 2 x 1
    assert CR.candidates(F) == [(True, 0, 0, (0, 2), 200, 320, False)]
    qx, qy = CR.crossing_points(CR.candidates(F))
    assert (float(qx[0]), float(qy[0])) == (1.125, 0.5)
    # q is 3.5 inside a box: the median's "outside" is false
    G, marked, arts = CR.correct(F, _box(-3.0), 4)
    assert marked.tolist() == [[True, False]] and G.tolist() == [[[220, 220, 220, 200], list(PAIR_B)]]
    assert len(arts) == 1 and arts[0][:6] == ((0, 0), (1, 0), (0, 2), 200, 320, False) and arts[0][6] == 3.5
    # the box elsewhere: q is outside, as the median says
    G, marked, arts = CR.correct(F, _box(3.0), 4)
    assert not marked.any() and np.array_equal(G, F) and not arts
    # the box's left side 0.01 to either side of q: within one quantisation step (0.0157) of the outline nobody is convicted
    for x0 in (1.125 + 0.01, 1.125 - 0.01):
        G, marked, arts = CR.correct(F, _box(x0), 4)
        assert not marked.any() and np.array_equal(G, F)
    # ... 0.02 inside it: convicted; with R = 8 (step 0.031) not
    assert CR.correct(F, _box(1.125 - 0.02), 4)[1].tolist() == [[True, False]]
    assert not CR.correct(F, _box(1.125 - 0.02), 8)[1].any()
    # the complement, 255 - v: both texels outside, the interpolated median inside (N = -200, D = -320, negated); the box elsewhere convicts it
    Fc = np.array([[[35, 35, 235, 55], [195, 75, 75, 65]]], np.uint8)
    assert CR.candidates(Fc) == [(True, 0, 0, (0, 2), 200, 320, True)]
    G, marked, _ = CR.correct(Fc, _box(3.0), 4)
    assert marked.tolist() == [[True, False]] and G.tolist() == [[[35, 35, 35, 55], [195, 75, 75, 65]]]
    assert not CR.correct(Fc, _box(-3.0), 4)[1].any()
    # equal depths mark both: b = (40, 200, 200) beside a = (200, 200, 40), crossing at t = 0.5
    Fe = np.array([[[200, 200, 40, 1], [40, 200, 200, 2]]], np.uint8)
    assert CR.candidates(Fe) == [(True, 0, 0, (0, 2), 160, 320, False)]
    G, marked, _ = CR.correct(Fe, _box(-3.0), 4)
    assert marked.all() and G.tolist() == [[[200, 200, 200, 1], [200, 200, 200, 2]]]
    # the same pair upright: 1 x 2, the outline mirrored in the diagonal
    Ft = F.transpose(1, 0, 2).copy()
    assert CR.candidates(Ft) == [(False, 0, 0, (0, 2), 200, 320, False)]
    G, marked, _ = CR.correct(Ft, _box(-3.0)[:, [1, 0, 3, 2, 5, 4]], 4)
    assert marked.tolist() == [[True], [False]] and G[0, 0].tolist() == [220, 220, 220, 200]
    # an outline of 0 segments has no artefacts
    G, marked, arts = CR.correct(F, np.zeros((0, 6), np.float32), 4)
    assert np.array_equal(G, F) and not marked.any() and not arts
    # a field whose channels all agree has no crossing at all
    name, segs, w, h, R = MC.inputs()[ord("*") - 33]
    A = M.generate(segs, w, h, R)
    A[..., 0] = A[..., 1] = A[..., 2] = A[..., 3]
    assert not CR.candidates(A)
    G, marked, _ = CR.correct(A, segs, R)
    assert np.array_equal(G, A) and not marked.any()
    # a 9 x 1 field has no vertical pairs, a 1 x 9 field no horizontal ones; random texels, so that there are candidates
    rng = np.random.RandomState(9)
    row = rng.randint(0, 256, (1, 9, 4)).astype(np.uint8)
    tri = MC.poly([(1, -3), (8, 0.5), (2, 4)])
    cr, cc = CR.candidates(row), CR.candidates(row.transpose(1, 0, 2))
    assert cr and all(c[0] for c in cr) and [(not c[0], c[2], c[1]) + c[3:] for c in cc] == cr
    G, marked, _ = CR.correct(row, tri, 2)
    check_invariants("9 x 1", row, G, marked)
    Gt, markedt, _ = CR.correct(row.transpose(1, 0, 2).copy(), tri[:, [1, 0, 3, 2, 5, 4]], 2)
    check_invariants("1 x 9", row.transpose(1, 0, 2), Gt, markedt)
    assert Gt.shape == (9, 1, 4) and np.array_equal(markedt.T, marked)


# ------------------------------------------------------------------------------------------------------------------ 3. the cap
@pytest.fixture(scope="module")
def reference():
    """every input through the float64 reference of steps 1 to 4, once, and through step 5 in float64 and in float32 ->
    {name: (F, G, marked, artefacts, G of float32)}"""
    out = {}
    for name, segs, w, h, R in all_inputs():
        F = M.generate(segs, w, h, R)
        G, marked, arts = CR.correct(F, segs, R)
        out[name] = (F, G, marked, arts, CR.correct(F, segs, R, np.float32)[0])
    return out


def test_the_reference_in_float32_stays_inside_the_cap(reference):
    """The cap of 1 texel per image is a condition on the inputs, checked first: step 5 with d(q) in float32 against float64, on the float64
    reference's field.  (All 106 + 71 inputs meet it; none had to be replaced or dropped.)"""
    over, marked_in = {}, 0
    for name, segs, w, h, R in all_inputs():
        F, G, marked, arts, G32 = reference[name]
        check_invariants(name + " (float64)", F, G, marked)
        n = differing(G32, G)
        if n:
            over[name] = n
        marked_in += bool(marked.any())
        assert n <= CAP, f"{name}: {n} texels of the float32 reference differ from the float64 reference"
    print(f"float32 reference against float64, texels that differ per image (cap {CAP}): {over or 'none in any image'}; {marked_in} of {len(reference)} images have marked texels")
    assert len(reference) == 106 + 71


# ------------------------------------------------------------------------------------------------------------------ 4. the kernel's source on a CPU
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_msdf.hip + fdh_msdf_host.h compiled as plain C++ under the sequential shim of tests/emu with the driver of tests/msdf_correct_emu
    -> the directory of ./emu, and of ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "msdf_correct_emu", ("k_msdf.hip", "fdh_msdf_host.h"), {"emu": (), "emu_san": emu_build.SAN})


def _through_the_shim(tmp, name, segs, w, h, R, exe="./emu", field=None):
    """-> (uncorrected texels, corrected texels, (workgroups, those with phase-2 rounds, rounds))"""
    np.ascontiguousarray(segs, np.float32).tofile(tmp / "segs.raw")
    args = [exe, str(w), str(h), str(R), "segs.raw"]
    if field is not None:
        np.ascontiguousarray(field, np.uint8).tofile(tmp / "field.raw")
        args.append("field.raw")
    r = subprocess.run(args, cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name}: {r.returncode} {r.stdout}{r.stderr}"
    stats = tuple(int(v) for v in re.match(r"workgroups (\d+) with_rounds (\d+) rounds (\d+)", r.stdout).groups())
    return np.fromfile(tmp / "texels.raw", np.uint8).reshape(h, w, 4), np.fromfile(tmp / "corrected.raw", np.uint8).reshape(h, w, 4), stats


@pytest.fixture(scope="module")
def emulated(shim):
    """every input through the shim -> {name: (F of the shim, G of the shim, statistics)}"""
    return {name: _through_the_shim(shim, name, segs, w, h, R) for name, segs, w, h, R in all_inputs()}


def test_the_kernel_source_under_a_host_shim(emulated):
    """correct(F_shim, float64) against the shim's own corrected texels: marked set and bytes equal but for the cap's 1 texel per image; the
    invariants exactly, with the marked set read off the shim's output"""
    over, tiles, busy, rounds, marked_total = {}, 0, 0, 0, 0
    for name, segs, w, h, R in all_inputs():
        F, G, stats = emulated[name]
        want, marked, _ = CR.correct(F, segs, R)
        n = differing(G, want)
        if n:
            over[name] = n
        assert n <= CAP, f"{name}: {n} texels differ from the reference's correction of the same field"
        got_marked = (G != F).any(axis=2)
        assert int((got_marked != marked).sum()) <= CAP, f"{name}: the marked set"
        check_invariants(name, F, G, got_marked)  # (a marked texel always changes: the two channels that cross differ in both texels of the pair)
        tiles, busy, rounds = tiles + stats[0], busy + stats[1], rounds + stats[2]
        marked_total += int(got_marked.sum())
    print(f"texels that differ from correct(F_shim) per image (cap {CAP}): {over or 'none in any image'}")
    print(f"{busy} of {tiles} tiles walked the edges, {rounds} rounds in all; {marked_total} texels changed")
    assert len(emulated) == 106 + 71


def test_an_input_with_work_to_do(emulated, reference):
    """'*' of the fixture, scaled by 2, R = 4: a suite in which nothing is ever corrected shows nothing"""
    F, G, stats = emulated["* x2"]
    n_shim, n_ref = differing(G, F), int(reference["* x2"][2].sum())
    print(f"'*' x2: {n_shim} texels corrected under the shim ({stats[1]} of {stats[0]} tiles walked the edges, {stats[2]} rounds), {n_ref} marked by the reference on its own field")
    assert n_shim > 0 and n_ref > 0 and stats[2] > 0


def test_the_shim_under_sanitizers(shim, emulated):
    """the same stand-alone program built with -fsanitize=address,undefined, run directly: '*' (artefacts), an image of 17 x 9 (a tile edge one
    texel inside the image), 8 x 8, 9 x 1 and 1 x 9, and a hand-made field of disagreeing channels through k_msdf_correct alone; same bytes as
    the plain build"""
    name, segs, w, h, R = MC.inputs()[ord("*") - 33]
    _, G, _ = _through_the_shim(shim, name, segs, w, h, R, exe="./emu_san")
    assert np.array_equal(G, emulated[name][1])
    rng = np.random.RandomState(17)
    tri = MC.poly([(1, -3), (8, 0.5), (2, 4)])
    for (w, h), outline in (((17, 9), MC.poly([(3.3, 2.2), (14.1, 1.7), (12.6, 7.4), (2.9, 6.8)])), ((8, 8), MC.poly([(1.5, 1.25), (6.5, 2), (4, 6.75)])),
                            ((9, 1), tri), ((1, 9), tri[:, [1, 0, 3, 2, 5, 4]])):
        noise = rng.randint(96, 160, (h, w, 4)).astype(np.uint8)  # medians on both sides of 127.5 and channels that cross: many candidates
        if min(w, h) == 1:  # (8 pairs of noise may hold none: the hand-made pair of the known answers, over and over)
            noise = np.array([PAIR_A if k % 2 == 0 else PAIR_B for k in range(9)], np.uint8).reshape(h, w, 4)
        for field in (None, noise):
            F, G, stats = _through_the_shim(shim, f"{w} x {h}", outline, w, h, 2, exe="./emu_san", field=field)
            F2, G2, _ = _through_the_shim(shim, f"{w} x {h}", outline, w, h, 2, field=field)
            assert np.array_equal(F, F2) and np.array_equal(G, G2)
            want, marked, _ = CR.correct(F, outline, 2)
            assert differing(G, want) <= CAP
            check_invariants(f"{w} x {h}", F, G, (G != F).any(axis=2))
            if field is not None:
                assert np.array_equal(F, noise) and stats[2] > 0 and len(CR.candidates(F)) > 0


# ------------------------------------------------------------------------------------------------------------------ 5. reconstruction
def test_reconstruction_through_draw_msdf(emulated, reference):
    """The statistic of test_msdf_host.py::test_reconstruction_through_draw_msdf -- the field drawn by the oracle's draw_msdf (px_range 4, on
    black) against the box coverage of the outline scaled likewise, over the 94 inputs with R = 4 -- at scales 1, 2 and 3 for four fields:
    the reference's uncorrected and corrected, the shim's uncorrected and corrected.  Measured values: profiles/msdf.txt, section 4.
    Asserted on the reference alone: at no scale is the maximum or the number of pixels beyond 64 LSB larger after the correction, and at
    scales 2 and 3 that number is strictly smaller.  Asserted on the shim: its corrected field reconstructs as well as the reference's,
    within a quarter of an LSB in the mean and in the 99th percentile."""
    from oracle import oracle as O

    orc = O.Oracle(atlas_size=4096, threads=4)
    cases = [c for c in MC.inputs() if c[4] == 4]
    assert len(cases) == 94
    fields = {"reference": lambda n: reference[n][0], "reference corrected": lambda n: reference[n][1],
              "kernel source": lambda n: emulated[n][0], "kernel source corrected": lambda n: emulated[n][1]}
    for k, get in enumerate(fields.values()):
        for i, c in enumerate(cases):
            orc.put_image(1000 * (k + 1) + i, get(c[0]))
    for scale in (1, 2, 3):
        s = {}
        for k, tag in enumerate(fields):
            e = np.concatenate([MC.reconstruction_error(orc, O.rasterize_outline, 1000 * (k + 1) + i, c[1], c[2], c[3], scale) for i, c in enumerate(cases)])
            s[tag] = (e.mean(), np.percentile(e, 99), int(e.max()), int((e > 64).sum()))
            print(f"scale {scale}: |alpha - coverage| in LSB over {e.size} pixels, {tag}: mean {s[tag][0]:.3f}, 99th percentile {s[tag][1]:.1f}, max {s[tag][2]}, beyond 64 LSB {s[tag][3]}")
        before, after, emu = s["reference"], s["reference corrected"], s["kernel source corrected"]
        assert after[2] <= before[2] and after[3] <= before[3], f"scale {scale}: the correction made the reference's field worse"
        if scale > 1:
            assert after[3] < before[3], f"scale {scale}: the correction removed no pixel beyond 64 LSB"
        assert emu[0] <= after[0] + 0.25 and emu[1] <= after[1] + 0.25
