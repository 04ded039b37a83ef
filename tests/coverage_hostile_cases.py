"""Outlines on which an exact-area rasteriser goes wrong if it can, for test_coverage_exact_host.py (the oracle and the kernels' source on a
CPU) and test_coverage_exact.py (the device): each family -> [(name, segs, w, h)], segs float32 (n, 6) in fdh_put_glyph_outline's format or
(n, 8) in fdh_put_glyph_outline_cubic's.  Every texel of every case is held to coverage_exact_ref.coverage(), c, of the flattened lines:

    |texel - 255 c| <= 0.5 + e

so a texel is floor(255 c + 0.5) wherever 255 c lies further than e from a rounding tie.  e is the float32 arithmetic's share and is set per
family in E below as (measured, e): `measured` is the largest excess over 0.5 of the oracle's rasterize_outline alone over the float64
reference on the family, on a CPU; e is four times that, because another compiler may round the same expressions' ties differently.  No e
may exceed 1/16 LSB (E_MAX).  (The tests add 1e-9 LSB for the float64 reference's own rounding, which decides exact ties such as 25.5.)
Where the oracle never exceeded 0.5 -- `measured` is negative: its nearest miss -- e is 0: a texel is then the correctly rounded 255 c."""
import functools

import numpy as np

import coverage_cases as CC
import coverage_exact_ref as R
import msdf_cubic_cases as MCC

NAN = float("nan")
E_MAX = 1.0 / 16.0
# family: (the largest excess of the oracle alone, e = 4 x that), in LSB
E = {
    "sloped edges crossing a side": (0.0, 0.0),                             # exact ties (25.5 read as 26) and nothing beyond
    "sloped edges crossing a side, vertices to 3000": (0.0044366, 0.0177464),  # float32 at coordinates of 3000: an ulp is 2.4e-4 px
    "the whole width in one row": (-0.0000064, 0.0),
    "stars": (0.0012871, 0.0051484),                                        # 4000 lines' contributions of alternating sign in one row sum
    "slivers": (-0.0098675, 0.0),
    "nearly horizontal edges": (-0.0005496, 0.0),
    "vertices on the pixel grid": (0.0, 0.0),
    "overlapping contours": (0.0, 0.0),
    "curves that leave the image": (-0.0000122, 0.0),
    "cubic curves that leave the image": (-0.0000122, 0.0),
    "font outlines scaled 3.7 x": (-0.0002423, 0.0),
    "shapes": (0.00003, 0.00012),
}


def mirrored(segs, w):
    """the outline reflected in the image's vertical centre line, x -> w - x (the winding turns: |sum| does not care)"""
    s = np.array(segs, np.float32)
    s[:, 0::2] = np.float32(w) - s[:, 0::2]
    return s


def random_triangles(seed, n, lo, hi, w, h):
    rng = np.random.RandomState(seed)
    return [(f"triangle {k} in [{lo}, {hi}]^2", CC.poly(rng.uniform(lo, hi, (3, 2))), w, h) for k in range(n)]


def aimed_triangles(seed, n, reach, w, h):
    """triangles of that size with a side that does pass through the image (of random ones that far out hardly any has one): the side runs
    through a random point of the image in a random direction to both sides, the third vertex is anywhere in [-reach, reach]^2"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        p, a = rng.uniform((0, 0), (w, h)), rng.uniform(0, 2 * np.pi)
        u = np.array([np.cos(a), np.sin(a)])
        out.append((f"aimed triangle {k}, reach {reach}", CC.poly([p - rng.uniform(0.3, 1.0) * reach * u, p + rng.uniform(0.3, 1.0) * reach * u, rng.uniform(-reach, reach, 2)]), w, h))
    return out


def star(spikes, cx=8.3, cy=7.6, r_in=2.0, r_out=11.0):
    a = np.arange(2 * spikes) * (np.pi / spikes)
    r = np.where(np.arange(2 * spikes) % 2 == 0, r_out, r_in)
    return CC.poly(np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1))


def quad(*pts):
    """a closed contour: a point (x, y) is a line to there, (cx, cy, x, y) a quadratic; the first point is the start"""
    rows, at = [], pts[0]
    for p in pts[1:] + (pts[0],):
        rows.append([at[0], at[1], NAN, NAN, p[0], p[1]] if len(p) == 2 else [at[0], at[1], p[0], p[1], p[2], p[3]])
        at = p[-2:]
    return np.array(rows, np.float32)


@functools.lru_cache(maxsize=None)
def families():
    """-> {family: [(name, segs, w, h)]}"""
    F = {}
    para = CC.poly([(-10, 1), (5, 2), (5, 6), (-10, 7)])
    diamond = CC.poly([(-2, 4), (5, -3), (12, 4), (5, 11)])
    F["sloped edges crossing a side"] = [
        ("parallelogram through the left side", para, 10, 8),
        ("parallelogram through the right side", mirrored(para, 10), 10, 8),
        ("diamond that crosses the sides mid-row", CC.shifted(diamond, 0.0, 0.5), 10, 8),
        ("wedge through both sides", CC.poly([(-4.5, 1.3), (13.75, 3.9), (-2.25, 6.6)]), 10, 8),
    ] + random_triangles(20261020, 60, -20, 30, 11, 9)
    F["sloped edges crossing a side, vertices to 3000"] = random_triangles(20261021, 60, -3000, 3000, 11, 9) + aimed_triangles(20261022, 20, 3000, 11, 9)
    band = [(-3, 2.2), (14, 2.7), (14, 6.5), (-3, 6.1)]  # its upper edge passes all 10 columns inside row 2
    F["the whole width in one row"] = [
        ("edge across the whole width", CC.poly(band), 10, 8),
        ("the same edge, left of the image", CC.poly([(x - 27, y) for x, y in band]), 10, 8),   # everything to cell 0: rows 2 .. 6 are full
        ("the same edge, right of the image", CC.poly([(x + 27, y) for x, y in band]), 10, 8),  # nothing
        ("steeper, across the width in two rows", CC.poly([(-1.5, 1.25), (11.5, 2.75), (11.5, 7.5), (-1.5, 7.0)]), 10, 8),
    ]
    F["stars"] = [("star of 200 spikes", star(200), 17, 15), ("star of 2000 spikes", star(2000), 17, 15)]
    sl = []
    for k, (wd, x_top, x_bot) in enumerate([(1e-3, 4.3, 4.3), (5e-3, 8.25, 9.75), (2e-2, 12.0, 3.5), (1e-3, -0.5, 1.5), (2e-2, 1.2, -0.7),
                                           (5e-3, 16.2, 17.6), (2e-2, 17.3, 15.1), (1e-2, -3.0, 20.0)]):
        sl.append((f"sliver {k}: {wd} wide, x {x_top} -> {x_bot}", CC.poly([(x_top, -2.5), (x_top + wd, -2.5), (x_bot + wd, 17.25), (x_bot, 17.25)]), 17, 15))
    F["slivers"] = sl
    F["nearly horizontal edges"] = [
        (f"rise {rise} over 25 px from y = {y0}", CC.poly([(-5, y0), (20, y0 + rise), (20, y0 + 3.4), (-5, y0 + 3.1)]), 17, 15)
        for rise in (1e-5, 1e-4, 1e-3, 1e-2) for y0 in (3.3, 4.0 - rise / 2)  # inside a row, and across a row boundary
    ]
    F["vertices on the pixel grid"] = [
        ("the image's own rectangle", CC.poly([(0, 0), (10, 0), (10, 8), (0, 8)]), 10, 8),
        ("half the image, corner to corner", CC.poly([(0, 0), (10, 8), (0, 8)]), 10, 8),
        ("diamond with a vertex at x = 0 and one at x = w", CC.poly([(0, 4), (5, 0), (10, 4), (5, 8)]), 10, 8),
        ("triangle on pixel corners", CC.poly([(3, 2), (7, 2), (5, 6)]), 10, 8),
        ("vertex at x = 0 mid-row, one at x = w mid-row", CC.poly([(0, 3.5), (4, 1), (10, 2.5), (6, 7)]), 10, 8),
        ("corners of the image and beyond", CC.poly([(0, 0), (10, 0), (15, 8), (-5, 8)]), 10, 8),
    ]
    sq = [(2.25, 1.5), (7.5, 1.5), (7.5, 5.25), (2.25, 5.25)]
    moved = [(x + 2.4, y + 1.3) for x, y in sq]
    F["overlapping contours"] = [
        ("two squares, the same winding", np.concatenate([CC.poly(sq), CC.poly(moved)]), 11, 9),         # |2| clamps to 1 where they overlap
        ("two squares, opposite winding", np.concatenate([CC.poly(sq), CC.poly(moved[::-1])]), 11, 9),   # and cancels there
        ("two triangles through the left side, the same winding",
         np.concatenate([CC.poly([(-6, 1.2), (7, 3.1), (-4, 7.7)]), CC.poly([(-3, 0.4), (9.5, 6.2), (-8, 5.5)])]), 11, 9),
    ]
    F["curves that leave the image"] = [
        ("arch", quad((-3, 7), (5.5, -6, 14, 7)), 11, 9),
        ("leaning arch", quad((-2.5, 8.2), (9, -9, 13.2, 5.1)), 11, 9),
        ("shallow arch over a band", quad((-6, 3.3), (5, 1.1, 16, 4.4), (16, 8.5), (-6, 7.7)), 11, 9),
        ("lens of two arches", quad((-2, 4.5), (5.5, -4, 13, 4.5), (5.5, 13, -2, 4.5)), 11, 9),
    ]
    F["cubic curves that leave the image"] = [
        ("cubic arch", MCC.cpath((-3, 7), (0, -6, 11, -6, 14, 7), (-3, 7)), 11, 9),
        ("leaning cubic arch", MCC.cpath((-2.5, 8.2), (2, -8, 16, -3, 13.2, 5.1), (-2.5, 8.2)), 11, 9),
        ("cubic S over a band", MCC.cpath((-6, 3.3), (2, -2, 8, 8, 16, 4.4), (16, 8.5), (-6, 7.7), (-6, 3.3)), 11, 9),
        ("lens of two cubics", MCC.cpath((-2, 4.5), (1, -3, 10, -3, 13, 4.5), (10, 12, 1, 12, -2, 4.5)), 11, 9),
    ]
    F["font outlines scaled 3.7 x"] = CC.scaled()
    F["shapes"] = CC.shapes()
    assert set(F) == set(E)
    return F


def cases():
    """every case of every family, in the families' order -> [(family, name, segs, w, h)]"""
    return [(fam, name, segs, w, h) for fam, cs in families().items() for name, segs, w, h in cs]


def is_cubic(segs):
    return np.asarray(segs).shape[-1] == 8


def lines6(O, segs):
    """what fdh_put_glyph_outline rasterises: the oracle's flattening of a 6-float outline; an 8-float one goes in as its flattened lines"""
    return MCC.flatten_lines(segs) if is_cubic(segs) else CC.flatten(O, segs)


def as6(segs):
    """the outline for the quadratic routes: an 8-float one as the straight lines the cubic routes make of it"""
    return MCC.lines_as_outline(MCC.flatten_lines(segs)) if is_cubic(segs) else segs


def as8(segs):
    """the outline for the cubic routes"""
    return segs if is_cubic(segs) else MCC.lift(segs)


_exact = {}


def exact(O, family, name):
    """the float64 coverage (h, w) of a case's flattened lines, made once"""
    if (family, name) not in _exact:
        segs, w, h = next((s, w, h) for nm, s, w, h in families()[family] if nm == name)
        c = R.coverage(lines6(O, segs), w, h)
        c.setflags(write=False)
        _exact[(family, name)] = c
    return _exact[(family, name)]


def hold(texels, c, e):
    """-> (the largest excess of |texel - 255 c| over 0.5, its (y, x), the number of texels beyond e); an image without texels: (-0.5, None, 0)"""
    if c.size == 0:
        return -0.5, None, 0
    x = R.excess(texels, c)
    at = np.unravel_index(int(np.argmax(x)), x.shape)
    return float(x[at]), (int(at[0]), int(at[1])), int((x > e).sum())
