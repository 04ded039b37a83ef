"""Inputs of the coverage batch tests (test_coverage_batch_host.py, test_coverage_batch.py; tools/coverage_bench.py uses the font sets; coverage_hostile_cases.py holds scaled() and shapes() to exact areas): the
94 ASCII outlines of the font fixture and what is made of them, and the smallest shapes at which the batched kernels can go wrong."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
NONE = np.zeros((0, 6), np.float32)


def poly(pts):
    """a closed polygon as line segments"""
    pts = [tuple(map(float, p)) for p in pts]
    return np.array([[a[0], a[1], NAN, NAN, b[0], b[1]] for a, b in zip(pts, pts[1:] + pts[:1])], np.float32)


def shifted(segs, dx, dy=0.0):
    """the outline moved by (dx, dy): float32 additions (the control point of a straight line stays NaN)"""
    return (segs + np.array([dx, dy, dx, dy, dx, dy], np.float32)).astype(np.float32)


def font():
    """-> [(name, segs float32 (n, 6), w, h)]: data/Ubuntu.ttf at 20 px, codes 33 .. 126 (tests/golden/outlines_ubuntu20.npz)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "outlines_ubuntu20.npz"))
    out = []
    for code in range(33, 127):
        segs, (w, h) = z[f"segs_{code}"].astype(np.float32), z[f"size_{code}"]
        out.append((chr(code), segs, int(w), int(h)))
    return out


def variants(shifts=(0.0, 0.25, 0.5, 0.75)):
    """the font set once per sub-pixel variant: the same outline shifted in x (pixie_raster.nim:69-72), in the same image"""
    return [(f"{name} +{dx}", shifted(segs, dx), w, h) for dx in shifts for name, segs, w, h in font()]


def scaled():
    """every font outline 3.7 x about the image's centre: it leaves the image on all four sides"""
    out = []
    for name, segs, w, h in font():
        s = np.float32(3.7)
        out.append((f"{name} x3.7", shifted(segs * s, (1.0 - 3.7) * w / 2.0, (1.0 - 3.7) * h / 2.0), w, h))
    return out


def square(w, h):
    """a square with a margin of 1/4 of the image, at least 0.25: it fits a 1 x 1 image too, mostly outside it"""
    mx, my = max(w / 4.0, 0.25), max(h / 4.0, 0.25)
    return poly([(mx, my), (w - mx, my), (w - mx, h - my), (mx, h - my)])


def shapes():
    """-> [(name, segs, w, h)], a glyph without segments among them"""
    out = [(f"{w} x {h}", square(w, h), w, h) for w, h in ((1, 1), (9, 1), (1, 9), (8, 8), (7, 9), (17, 23))]  # no texels; partial tiles
    out.insert(3, ("0 segments", NONE, 5, 3))
    out += [
        ("65 x 3", poly([(0.5, 0.3), (64.5, 1.2), (3.0, 2.8)]), 65, 3),        # the row sum carried across 9 tiles
        ("130 x 9", poly([(1.25, 0.5), (129.5, 3.75), (128.0, 8.5), (0.75, 6.0)]), 130, 9),  # ... across 17
        ("3 x 70", poly([(0.4, 0.6), (2.7, 35.2), (1.1, 69.5)]), 3, 70),       # 9 bands of one tile
        ("integer rectangle", poly([(2, 2), (10, 2), (10, 8), (2, 8)]), 12, 10),  # lines on cell borders, horizontal lines
        ("leaves on all sides", poly([(-2, 4), (5, -3), (12, 4), (5, 11)]), 10, 8),  # cells clamped to 0 and to w
        ("leaves on all sides mid-row", poly([(-2, 4.5), (5, -2.5), (12, 4.5), (5, 11.5)]), 10, 8),  # the one above crosses x = 0 and x = w on row borders; this one inside rows
        ("covers everything", poly([(-3, -2), (14, -2.5), (13, 11), (-4, 10)]), 10, 8),
        ("sliver", poly([(4.2, 1.1), (4.5, 1.1), (4.6, 7.9), (4.3, 7.9)]), 9, 9),  # narrower than a cell: the narrow branch
        ("steep in one cell", poly([(3.1, 2.1), (3.9, 2.2), (3.4, 6.7)]), 9, 9),
        ("nearly horizontal", poly([(0.25, 1.0), (39.75, 1.6), (39.75, 4.5), (0.25, 4.2)]), 40, 6),  # one line across the width: the d * s run and a2
        ("curves", np.array([[1, 6, 5, -2, 9, 6], [9, 6, NAN, NAN, 1, 6]], np.float32), 10, 8),
    ]
    return out


def oracle_image(O, segs, w, h, lcd):
    """the texels of one glyph by the oracle alone: (h, w, 4) uint8"""
    img = O.rasterize_outline(segs, w, h)
    return O.lcd_filter(img) if lcd else img


def flatten(O, segs):
    """the oracle's fo_flatten_outline -> (m, 4) float32 lines"""
    import ctypes as C

    segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 6)
    L = O.lib()
    L.fo_flatten_outline.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.fo_flatten_outline.restype = C.c_int
    m = L.fo_flatten_outline(segs.ctypes.data, len(segs), None, 0)
    lines = np.zeros((max(m, 1), 4), np.float32)
    assert L.fo_flatten_outline(segs.ctypes.data, len(segs), lines.ctypes.data, m) == m
    return lines[:m]
