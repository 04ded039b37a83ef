"""Glyph coverage against exact pixel areas, what a CPU can check.  Every other texel test of the coverage kernels compares them with the
oracle's fo_rasterize_lines, of which they are copies: an error of the algorithm is in both.  Here the yardstick is
tests/coverage_exact_ref.py -- polygon clipping in float64, nothing of the accumulation -- and the outlines are those of
tests/coverage_hostile_cases.py.  1. the reference's own known answers; 2. the oracle's rasterize_outline on every family, every texel
within 0.5 + e LSB of 255 c (the kernels' source under the host shim is held to the oracle's bytes on the same cases by
test_coverage_batch_host.py's third batch); 3. the flattening's 0.025 px claim against the true curves, as far towards the chord caps as
float32 chord ends let arithmetic decide.

Before the row piece was cut at x = 0 and x = w (its part left of the image was spread over the cells inside) test 2 failed with these
largest |texel - 255 c| - 0.5: sloped edges crossing a side 153.0 (the parallelogram's texel (0, 6) read 230, exact 76.5; 97 of 6260 texels
beyond the bar), the same with vertices to 3000 140.2, the whole width in one row 39.1, stars 17.3, slivers 1.1, nearly horizontal edges
14.6, overlapping contours 44.6, curves and cubic curves that leave the image 86.9, font outlines scaled 3.7 x 75.6 (142 of 19820 texels),
shapes 31.6 (the diamond that crosses mid-row, alone); vertices on the pixel grid passed."""
import numpy as np
import pytest

import coverage_cases as CC
import coverage_exact_ref as R
import coverage_hostile_cases as H
import msdf_cubic_cases as MCC
from oracle import oracle as O

REF_EPS = 1e-9  # LSB: the float64 reference's own rounding, 255 x a few ulps of coordinates up to 3000 (7e-13) with room to spare


# ------------------------------------------------------------------------------------------------------------------ 1. the reference itself
def test_reference_fractional_box():
    """the box of test_rasteriser_known_answers: every pixel's overlap with it, to 1e-12"""
    x0, y0, x1, y1 = 2.25, 1.5, 7.75, 5.25
    c = R.coverage(R.poly_lines([(x0, y0), (x1, y0), (x1, y1), (x0, y1)]), 10, 8)
    want = np.array([[max(0.0, min(x + 1, x1) - max(x, x0)) * max(0.0, min(y + 1, y1) - max(y, y0)) for x in range(10)] for y in range(8)])
    assert np.abs(c - want).max() <= 1e-12 and want.max() == 1.0


def test_reference_triangle_total():
    """the texels' total is the area of the triangle clipped to the image: one wholly inside (shoelace), one that leaves on three sides"""
    tri = [(1.3, 0.7), (8.6, 2.2), (3.1, 6.9)]
    area = 0.5 * abs(sum(tri[i][0] * tri[(i + 1) % 3][1] - tri[(i + 1) % 3][0] * tri[i][1] for i in range(3)))
    assert abs(R.coverage(R.poly_lines(tri), 10, 8).sum() - area) <= 1e-12
    assert abs(R.clipped_area(R.poly_lines(tri), 0, 0, 10, 8) - area) <= 1e-12
    out = R.poly_lines([(-4.5, 1.3), (13.75, 3.9), (-2.25, 9.6)])
    assert abs(R.coverage(out, 10, 8).sum() - R.clipped_area(out, 0, 0, 10, 8)) <= 1e-12
    # ... and a right triangle cut by the left side, by hand: (-2, 0) (2, 0) (2, 4) has the trapezium 0 <= x <= 2 under y = x + 2 inside
    assert abs(R.coverage(R.poly_lines([(-2, 0), (2, 0), (2, 4)]), 4, 4).sum() - 6.0) <= 1e-12


def test_reference_winding_and_hole():
    pts = [(2.25, 1.5), (7.75, 1.5), (6.5, 5.25), (1.1, 6.9)]
    one, other = R.coverage(R.poly_lines(pts), 10, 8), R.coverage(R.poly_lines(pts[::-1]), 10, 8)
    assert np.abs(one - other).max() <= 1e-12 and 0.0 < one[6, 2] < 1.0 and one[3, 4] == 1.0
    assert (R.signed_areas(R.poly_lines(pts), 10, 8) * R.signed_areas(R.poly_lines(pts[::-1]), 10, 8) <= 0.0).all()  # the signs do turn
    outer, hole = [(1, 1), (9, 1), (9, 7), (1, 7)], [(3.5, 3), (3.5, 5), (7, 5), (7, 3)]
    ring = R.coverage(np.concatenate([R.poly_lines(outer), R.poly_lines(hole)]), 10, 8)
    assert ring[4, 5] == 0.0 and ring[2, 5] == 1.0 and ring[4, 2] == 1.0 and ring[4, 3] == 0.5 and ring[0].max() == 0.0
    both = R.coverage(np.concatenate([R.poly_lines(outer), R.poly_lines(hole[::-1])]), 10, 8)  # the same winding: |2| clamps to 1
    assert np.array_equal(both, R.coverage(R.poly_lines(outer), 10, 8))
    assert len(R.contours(np.concatenate([R.poly_lines(outer), R.poly_lines(hole)]))) == 2


# ------------------------------------------------------------------------------------------------------------------ 2. the oracle
def test_the_bars():
    """E of coverage_hostile_cases.py: e is four times the measured excess (nothing where the oracle never exceeded 0.5), at most 1/16 LSB"""
    assert set(H.E) == set(H.families())
    for family, (measured, e) in H.E.items():
        assert e == 4.0 * max(measured, 0.0) and 0.0 <= e <= H.E_MAX, family


def test_the_case_families():
    """what the families must hold"""
    F = H.families()
    cross = F["sloped edges crossing a side"]
    assert sum(n.startswith("triangle") for n, _, _, _ in cross) == 60 and np.array_equal(cross[0][1], CC.poly([(-10, 1), (5, 2), (5, 6), (-10, 7)]), equal_nan=True)
    assert sum(n.startswith("triangle") for n, _, _, _ in F["sloped edges crossing a side, vertices to 3000"]) == 60
    assert [len(CC.flatten(O, s)) for _, s, _, _ in F["stars"]] == [400, 4000]
    assert len(F["curves that leave the image"]) == 4 == len(F["cubic curves that leave the image"]) and all(H.is_cubic(s) for _, s, _, _ in F["cubic curves that leave the image"])
    assert len(F["font outlines scaled 3.7 x"]) == 94 and len(F["shapes"]) == len(CC.shapes())
    for family, name, segs, w, h in H.cases():
        assert (w <= 17 and h <= 15) or family in ("font outlines scaled 3.7 x", "shapes"), name


@pytest.mark.parametrize("family", list(H.E))
def test_oracle_against_exact_areas(family):
    """every texel of every case: |texel - 255 c| <= 0.5 + e"""
    e = H.E[family][1] + REF_EPS
    worst, failed = (-1.0, None), []
    for name, segs, w, h in H.families()[family]:
        img = O.rasterize_outline(H.as6(segs), w, h)
        assert (img == img[..., :1]).all(), name  # premultiplied white
        c = H.exact(O, family, name)
        x, at, n = H.hold(img[..., 0], c, e)
        if x > worst[0]:
            worst = (x, f"{name}: texel (x {at[1]}, y {at[0]}) reads {int(img[at][0])}, exact {255.0 * c[at]:.6f}")
        if n:
            failed.append(f"{name}: {n} of {w * h} texels, the worst by {x:.6f}")
    print(f"{family}: largest |texel - 255 c| - 0.5 = {worst[0]:.6f} LSB, {worst[1]}; e = {e:.6f}")
    assert not failed, failed


def test_both_flattenings_give_the_same_lines():
    """a 6-float outline through the oracle's flattening (fdh_put_glyph_outline's) and, lifted, through the cubic call's: the same lines, so
    one exact image serves all routes of test_coverage_exact.py"""
    for family, name, segs, w, h in H.cases():
        if not H.is_cubic(segs):
            assert np.array_equal(CC.flatten(O, segs), MCC.flatten_lines(H.as8(segs))), name


# ------------------------------------------------------------------------------------------------------------------ 3. the flattening claim
def _distance_to_chords(curve, lines, k):
    """the largest distance of the curve (a function of t -> (n, 2), float64) over each chord's interval from that chord"""
    worst = 0.0
    for j in range(k):
        B = curve(np.linspace(j / k, (j + 1) / k, 33)[:, None])
        a, b = lines[j, :2].astype(np.float64), lines[j, 2:].astype(np.float64)
        d = b - a
        u = np.clip(((B - a) @ d) / (d @ d), 0.0, 1.0)[:, None]
        worst = max(worst, float(np.hypot(*(B - (a + u * d)).T).max()))
    return worst


ROUNDING = 1e-6  # px per px of coordinate: a chord end is a sum of 3 or 4 products of float32 Bernstein weights (a few roundings each) with
                 # the control points, at most about 10 x 2^-24 x max |coordinate| per axis; 1e-6 with room for both axes


def test_quadratic_flattening_up_to_the_cap():
    """fo_flatten_outline cuts a quadratic into n = ceil(sqrt(10 dev)) chords, dev = |P0 - 2 C + P1|, of error dev / (4 n^2) <= 0.025 px in
    exact arithmetic, and caps n at 64: the claim holds while dev <= 409.6.  The chord ends are float32: a curve is in the set where
    dev / (4 n^2) + ROUNDING max |coordinate| <= 0.025, so that arithmetic can decide -- which leaves curves up to dev = 407 of the cap's 409.6."""
    worst = {}
    for dev, p0, c, p1 in [(100.3, (-3, 40), (20, -10.15), (43, 40)), (247.0, (-60, 10), (10, 133.5), (80, 10)), (407.0, (-90, 102), (5, -101.5), (100, 102)),
                           (320.0, (0, 0), (160, 0), (0, 0.5)), (404.6, (-50, -30), (150, -30), (-50, 31))]:
        q = np.array([[*p0, *c, *p1]], np.float32)
        P = q.astype(np.float64).reshape(3, 2)
        got = np.hypot(*(P[0] - 2 * P[1] + P[2]))
        assert abs(got - dev) < 1.0 and got <= 409.6
        lines = CC.flatten(O, q)
        k = int(np.ceil(np.sqrt(10.0 * got)))
        assert got / (4 * k * k) + ROUNDING * np.abs(P).max() <= 0.025, dev  # the case can be decided
        assert len(lines) == k <= 64 and (lines[0, :2] == q[0, 0:2]).all() and (lines[-1, 2:] == q[0, 4:6]).all() and (lines[1:, :2] == lines[:-1, 2:]).all()
        worst[dev] = _distance_to_chords(lambda t: (1 - t) ** 2 * P[0] + 2 * (1 - t) * t * P[1] + t * t * P[2], lines, k)
    print("largest distance of a quadratic from its chords, by dev:", worst)
    assert len(CC.flatten(O, np.array([[-90, 102, 5, -101.5, 100, 102]], np.float32))) == 64  # the cap itself is reached
    assert all(0.0 < v <= 0.025 for v in worst.values()), worst
    assert worst[407.0] > 0.02  # and the bound is no loose one


def test_cubic_flattening_within_its_cap():
    """msdf::cubic::flatten_outline (msdf_cubic_cases.flatten_lines is it bit for bit: test_msdf_cubic_host.py) cuts a cubic into
    k = ceil(sqrt(30 dev)) chords, dev = max(|P0 - 2 P1 + P2|, |P1 - 2 P2 + P3|), of error at most 0.75 dev / k^2 <= 0.025 px in exact
    arithmetic, and caps k at 256: the claim holds while dev <= 0.025 * 256^2 / 0.75 = 2184.5.  Since k^2 is 30 dev rounded up, 0.75 dev / k^2
    is 0.025 but for the rounding up, and the float32 chord ends take that slack away long before the cap: a curve is in the set where
    0.75 dev / k^2 + ROUNDING max |coordinate| <= 0.025, which for a cubic that meets the bound (a parabola: both second differences equal)
    ends near dev = 360.  (Measured, not asserted: such a parabola of dev = 2100 lies 0.02512 px from its 251 chords.)
    A curve: P0, P1 and the two second differences a, b."""
    worst = {}
    for name, p0, p1, a, b in [("parabola, dev 361", (-270.75, 0), (-90.25, 361), (0, -361), (0, -361)), ("S, dev 133", (-40, 0), (-10, 70), (0, -133), (0, 133)),
                               ("askew, dev 328", (0, 0), (-60, 150), (200, -260), (-100, 50)), ("small parabola, dev 27.1", (0, 0), (10, -5), (0, 27.1), (0, 27.1))]:
        p0, p1, a, b = (np.array(v, np.float64) for v in (p0, p1, a, b))
        p2 = a - p0 + 2 * p1
        p3 = b - p1 + 2 * p2
        q = np.concatenate([p0, p1, p2, p3]).astype(np.float32)[None, :]
        P = q.astype(np.float64).reshape(4, 2)
        got = max(np.hypot(*(P[0] - 2 * P[1] + P[2])), np.hypot(*(P[1] - 2 * P[2] + P[3])))
        assert abs(got - max(np.hypot(*a), np.hypot(*b))) < 0.01 and got <= 2184.5
        lines = MCC.flatten_lines(q)
        k = int(np.ceil(np.sqrt(30.0 * got)))
        assert 0.75 * got / (k * k) + ROUNDING * np.abs(P).max() <= 0.025, name  # the case can be decided
        assert len(lines) == k <= 256 and (lines[0, :2] == q[0, 0:2]).all() and (lines[-1, 2:] == q[0, 6:8]).all() and (lines[1:, :2] == lines[:-1, 2:]).all()
        worst[name] = _distance_to_chords(lambda t: (1 - t) ** 3 * P[0] + 3 * (1 - t) ** 2 * t * P[1] + 3 * (1 - t) * t * t * P[2] + t ** 3 * P[3], lines, k)
    print("largest distance of a cubic from its chords:", worst)
    assert len(MCC.flatten_lines(np.array([[-546, 0, 0, 1092, 546, 0, 1092, 1092]], np.float32))) == 256  # dev = 2184: the cap itself is reached
    assert all(0.0 < v <= 0.025 for v in worst.values()), worst
    assert worst["parabola, dev 361"] > 0.02  # and the bound is no loose one
