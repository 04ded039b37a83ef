"""The exact coverage of a flattened glyph outline, for the coverage kernels and the oracle's rasteriser to be held to (test_coverage_exact_host.py
on a CPU, test_coverage_exact.py on the device).  Plain float64, and nothing of the scanline accumulation: every contour is clipped to every
pixel square (Sutherland-Hodgman, one half-plane after the other) and the clipped polygon's signed area is taken by the shoelace formula;

    c(x, y) = min(1, |sum over the contours of the signed area inside pixel (x, y)|)

which is include/figdraw_hip.h's own definition -- signed areas accumulated, |sum| clamped to 1 -- in exact arithmetic.  For an outline whose
contours do not overlap one another c is the geometric coverage (a hole, wound the other way, subtracts); where contours overlap it is the
accumulation rule, which is what the library specifies.  A contour that crosses itself is a sum of signed loops, to the clipper as to the
rule: Sutherland-Hodgman's degenerate bridges along a clip line enclose no area."""
import numpy as np


def contours(lines):
    """(m, 4) lines {x0, y0, x1, y1} -> [(k, 2) float64 vertices]: a new contour starts wherever a line does not start at the end of the line
    before it; a contour's vertices are its lines' starts, and its last line's end where that is not the first vertex again"""
    L = np.asarray(lines, np.float64).reshape(-1, 4)
    out, first = [], 0
    for i in range(1, len(L) + 1):
        if i == len(L) or L[i, 0] != L[i - 1, 2] or L[i, 1] != L[i - 1, 3]:
            if i > first:
                pts = L[first:i, 0:2]
                if L[i - 1, 2] != L[first, 0] or L[i - 1, 3] != L[first, 1]:
                    pts = np.concatenate([pts, L[i - 1:i, 2:4]])
                out.append(pts.copy())
            first = i
    return out


def clip(P, axis, bound, keep_below):
    """the polygon P (k, 2) cut by the half-plane coordinate[axis] <= bound (keep_below) or >= bound, all edges at once -> (k', 2)"""
    if len(P) == 0:
        return P
    Q = np.roll(P, -1, axis=0)
    a, b = P[:, axis], Q[:, axis]
    ina, inb = (a <= bound, b <= bound) if keep_below else (a >= bound, b >= bound)
    cross = ina != inb
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(cross, (bound - a) / np.where(cross, b - a, 1.0), 0.0)
    X = P + t[:, None] * (Q - P)
    X[:, axis] = bound  # on the line, exactly
    both = np.empty((2 * len(P), 2))  # per edge: its start where that is inside, then its crossing where it has one
    both[0::2], both[1::2] = P, X
    take = np.empty(2 * len(P), bool)
    take[0::2], take[1::2] = ina, cross
    return both[take]


def signed_area(P, ox=0.0, oy=0.0):
    """shoelace, about (ox, oy) so that a small polygon far from the origin loses nothing"""
    if len(P) < 3:
        return 0.0
    x, y = P[:, 0] - ox, P[:, 1] - oy
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def signed_areas(lines, w, h):
    """-> (h, w) float64: the sum over the contours of the signed area inside each pixel"""
    S = np.zeros((h, w))
    for P in contours(lines):
        if len(P) < 3:
            continue
        for y in range(h):
            row = clip(clip(P, 1, float(y), False), 1, float(y + 1), True)
            if len(row) < 3:
                continue
            lo, hi = row[:, 0].min(), row[:, 0].max()
            for x in range(w):
                if hi <= x or lo >= x + 1:  # nothing of the row's part of the contour in this column
                    continue
                cell = clip(clip(row, 0, float(x), False), 0, float(x + 1), True)
                S[y, x] += signed_area(cell, float(x), float(y))
    return S


def coverage(lines, w, h):
    """-> (h, w) float64 in [0, 1]"""
    return np.minimum(1.0, np.abs(signed_areas(lines, w, h)))


def clipped_area(lines, x0, y0, x1, y1):
    """|sum of the contours' signed areas| inside the rectangle, e.g. the whole image"""
    total = 0.0
    for P in contours(lines):
        for axis, bound, below in ((0, x0, False), (0, x1, True), (1, y0, False), (1, y1, True)):
            P = clip(P, axis, float(bound), below)
        total += signed_area(P, float(x0), float(y0))
    return abs(total)


def poly_lines(points):
    """a closed polygon -> (k, 4) lines"""
    pts = [tuple(map(float, p)) for p in points]
    return np.array([[a[0], a[1], b[0], b[1]] for a, b in zip(pts, pts[1:] + pts[:1])], np.float64)


def excess(texels, c):
    """(h, w) texels and exact coverage -> (h, w) |texel - 255 c| - 0.5: what the bar |texel - 255 c| <= 0.5 + e leaves for e"""
    return np.abs(np.asarray(texels, np.float64) - 255.0 * c) - 0.5
