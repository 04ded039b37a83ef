"""What the overlapping-contour tests share (test_msdf_overlap_host.py on a CPU, test_msdf_overlap.py on the device): 16 outlines whose
contours overlap, at 32 x 32 and smaller, in texel units; the helpers come from msdf_cases.  Coordinates keep texel centres (x + 0.5,
y + 0.5) off the outline and off the ties between two contours where that costs nothing: the tests measure the float32 reference against
the float64 one first, and an outline that fails there is on a tie."""
import numpy as np

import msdf_cases as MC

poly, path, winding, check_sign = MC.poly, MC.path, MC.winding, MC.check_sign


def rect(x0, y0, x1, y1):
    return poly([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])


def reverse(segs):
    """the same contour run the other way"""
    segs = np.asarray(segs, np.float32).reshape(-1, 6)
    return np.ascontiguousarray(segs[::-1][:, [4, 5, 2, 3, 0, 1]])


def round_contour(cx, cy, r, n=16, direction=1):
    """a round contour of n quadratics about (cx, cy), as msdf_cases.circle16 builds its 16; direction -1 runs the other way"""
    rows = []
    for k in range(n):
        a0, a1 = 2 * k * np.pi / n, 2 * (k + 1) * np.pi / n
        am, rc = (a0 + a1) / 2, r / np.cos(np.pi / n)
        rows.append([cx + r * np.cos(a0), cy + r * np.sin(a0), cx + rc * np.cos(am), cy + rc * np.sin(am), cx + r * np.cos(a1), cy + r * np.sin(a1)])
    rows = np.array(rows, np.float32)
    for k in range(n):
        rows[k, 0:2] = rows[k - 1, 4:6]
    return rows if direction > 0 else reverse(rows)


def join(*contours):
    return np.ascontiguousarray(np.concatenate(contours), np.float32)


def slab(x0, y0, x1, y1, half):
    """a bar of half-width `half` about the line (x0, y0) - (x1, y1), wound like rect()"""
    dx, dy = x1 - x0, y1 - y0
    l = float(np.hypot(dx, dy))
    nx, ny = -dy / l * half, dx / l * half
    return poly([(x0 - nx, y0 - ny), (x1 - nx, y1 - ny), (x1 + nx, y1 + ny), (x0 + nx, y0 + ny)])


RING = join(rect(4, 4, 28, 28), reverse(rect(10.25, 10.25, 21.75, 21.75)))
OSLASH = join(round_contour(16, 16, 11.2), round_contour(16, 16, 6.3, direction=-1), slab(4.2, 26.9, 27.8, 5.1, 1.6))
FIVE = [rect(2.75 + 2.5 * k, 2.75 + 2.5 * k, 29.25 - 2.5 * k, 29.25 - 2.5 * k) for k in range(5)]
FIVE_AND_A_HOLE = join(*FIVE, reverse(rect(14.25, 14.25, 17.75, 17.75)))


def inputs():
    """-> [(name, segs float32 (n, 6), w, h)]; every test takes them at R = 4, the sign test at R = 2, 4 and 8"""
    hostile = [c for c in MC.hostile_inputs() if c[0] == "two overlapping squares"][0]
    two = join(rect(3, 3, 13.25, 13.25), rect(8.75, 8.75, 21, 20))
    out = [
        ("two overlapping squares", two, 24, 23),
        ("two overlapping squares, reversed", join(*(reverse(c) for c in (two[:4], two[4:]))), 24, 23),
        ("plus sign of two bars", join(rect(4, 13.25, 28, 18.75), rect(13.25, 4, 18.75, 28)), 32, 32),
        ("square with an overlapping round contour", join(rect(4, 4, 19.75, 19.75), round_contour(19.25, 19.25, 8.4, 8)), 32, 32),
        ("square nested in a square of the same winding", join(rect(4, 4, 28, 28), rect(10.25, 10.25, 21.75, 21.75)), 32, 32),
        ("five squares nested, same winding", join(*FIVE), 32, 32),
        ("three mutually overlapping contours", join(rect(4, 4, 18.25, 18.25), rect(12.75, 8.25, 28, 21.75), rect(8.25, 13.75, 22.25, 28)), 32, 32),
        ("ring plus horizontal bar through the hole", join(RING, rect(1.75, 13.75, 30.25, 18.25)), 32, 32),
        ("ring plus tab reaching into the hole", join(RING, rect(13.75, 1.75, 18.25, 16.25)), 32, 32),
        ("round ring plus diagonal bar", OSLASH, 32, 32),
        ("round ring plus diagonal bar, reversed", join(*(reverse(c) for c in (OSLASH[:16], OSLASH[16:32], OSLASH[32:]))), 32, 32),
        ("two squares sharing part of an edge", join(rect(4, 4, 16, 16), rect(16, 8.25, 28, 22)), 32, 26),
        ("stem plus bowl", join(rect(6, 4, 11.25, 28), path((8.75, 6.25), (26.5, 6.25, 26.5, 14.5), (26.5, 22.75, 8.75, 22.75), (8.75, 6.25))), 32, 32),
        ("a square twice", np.tile(rect(4.5, 4.25, 16, 15.75), (2, 1)), 21, 20),
        ("five nested squares plus one hole", FIVE_AND_A_HOLE, 32, 32),
        ("the hostile set's two overlapping squares", hostile[1], hostile[2], hostile[3]),
    ]
    assert len(out) == 16 and all(w <= 32 and h <= 32 for _, _, w, h in out)
    return [(name, np.ascontiguousarray(segs, np.float32).reshape(-1, 6), w, h) for name, segs, w, h in out]


def tie_inputs():
    """Ties below the first rank together with a hole -> [(name, segs, w, h)].  Two filled contours have the very same A on the texels of the
    band they share, a third filled contour that contains both comes after them in contour order, and a hole covers the band: the term
    selected there has k >= 2, and which of the two tied contours it names is the header's tie rule (contour order), which an insertion
    that is not stable breaks.  Second form: the big square first (the order in which even an unstable insertion comes out right)."""
    a, b, big = rect(6, 10.25, 17.75, 21.75), rect(14.25, 10.25, 26, 21.75), rect(3, 3, 29, 29)
    hole = reverse(rect(11.25, 8.25, 20.75, 23.75))
    return [("two tied squares, a square around both, a hole", join(a, b, big, hole), 32, 32),
            ("a square around two tied squares, a hole", join(big, a, b, hole), 32, 32)]


def out_of_scope_inputs():
    """what step 6 says it does not cover -> [(name, segs, w, h)]"""
    return [("a hole reaching outside every filled contour", join(rect(4, 4, 20, 20), reverse(rect(14.25, 8.25, 27.75, 15.75))), 32, 24),
            ("one contour crossing itself", poly([(4, 4), (26, 4), (26, 14), (14, 14), (14, 26), (20, 26), (20, 9), (4, 9)]), 30, 30)]
