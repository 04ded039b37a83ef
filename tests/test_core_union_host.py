"""Host logic, no GPU: the saturated core of an upright SDF draw as a union of rectangles (fdh_record.cpp: local_core,
core_pixels, pack_bands; BinRec in fdh_types.h).

fdh_saturated_core_union returns the rectangles exactly as the bin launch decodes them from the draw's BinRec.  Over a sweep of
shapes -- half extents 3 .. 130 px at fractional origins; corner radii 0, 1, 7.5, 30 and beyond the half extent, equal and all
different; elliptical radii with ry = 2 rx and with zero components; fills, drop shadows (spread 0, 4, 24), inner shadows with an
offset, strokes of 1 and 5, and the clip push -- every pixel centre inside every rectangle must have a SATURATED coverage term,
evaluated here with the oracle's formulas (oracle/figdraw_oracle.c: sd_rounded_box, sd_elliptical_rounded_box, shade_main) in
float32: aa * dist + 0.5 <= 0, i.e. alpha exactly 1, for fills and pushes; sd <= 0, alpha exactly 1, for a shadow's body; alpha
exactly 0 inside a stroke; alpha below the no-op bound 0.49 / 255 deep inside an inner shadow.  The first rectangle must be the one
fdh_saturated_core reports (DrawRec::ix0..iy1), and that one must be what the commit before the union computed
(tests/golden/core_union_first_rect.json).  The Python restatement of the rule in tools/core_strip_count.py, which the GPU test's
prediction and profiles/core_union.txt rest on, must give the same rectangles."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import core_strip_count as CS  # noqa: E402

f32 = np.float32
AA = 1.2
F4, F2, I4, I12 = C.c_float * 4, C.c_float * 2, C.c_int * 4, C.c_int * 12

HALF_EXTENTS = [(3, 3), (3, 20.3), (7.5, 48.75), (20.3, 7.5), (20.3, 20.3), (48.75, 20.3), (48.75, 130), (130, 48.75), (130, 130), (130, 3)]
ORIGINS = [(10.3, 5.7), (4.0, 9.5), (7.62, 3.18)]
# node order TL, TR, BL, BR
RADII = [
    ((0, 0, 0, 0), None), ((1, 1, 1, 1), None), ((7.5, 7.5, 7.5, 7.5), None), ((30, 30, 30, 30), None), ((200, 200, 200, 200), None),
    ((0, 1, 7.5, 30), None), ((30, 7.5, 200, 1), None),
    ((4, 8, 12, 16), (8, 16, 24, 32)), ((0, 8, 12, 0), (10, 0, 24, 0)), ((8, 8, 5, 0), (8, 16, 10, 0)), ((30, 30, 30, 30), (60, 60, 60, 60)),
]
# (mode, factor, spread, inner-shadow offset, push)
MODES = [(3, 4.0, 0.0, None, 0), (3, 4.0, 0.0, None, 1), (7, 8.0, 0.0, None, 0), (7, 8.0, 4.0, None, 0), (7, 8.0, 24.0, None, 0),
         (9, 6.0, 2.0, (3.0, -2.0), 0), (9, 3.0, 0.0, (-4.5, 6.0), 0), (12, 1.0, 0.0, None, 0), (12, 5.0, 0.0, None, 0)]


def cases():
    k = 0
    for hx, hy in HALF_EXTENTS:
        for rx, ry in RADII:
            for mode, factor, spread, off, push in MODES:
                ox, oy = ORIGINS[k % len(ORIGINS)]
                k += 1
                w, h = 2.0 * hx, 2.0 * hy
                rect, shape = (ox, oy, w, h), (0.0, 0.0)
                if mode == 7:  # the padded quad around the shape (fdh_frontend.cpp: drop_shadows)
                    pad = float(CS.nim_round(spread) + CS.nim_round(1.5 * factor))
                    rect, shape = (ox, oy, w + 2 * pad, h + 2 * pad), (w, h)
                if mode == 9:
                    shape = off
                yield rect, rx, (ry if ry is not None else rx), mode, factor, spread, shape, push


def _lib():
    from figdraw_amd import context

    L = context.load()
    L.fdh_saturated_core.argtypes = [F4, F4, F4, C.c_int, C.c_float, C.c_float, F2, C.c_float, I4]
    L.fdh_saturated_core_union.argtypes = [F4, F4, F4, C.c_int, C.c_float, C.c_float, F2, C.c_float, C.c_int, I12, C.POINTER(C.c_int)]
    return L


def _union(L, case):
    rect, rx, ry, mode, factor, spread, shape, push = case
    out, n = I12(), C.c_int()
    assert L.fdh_saturated_core_union(F4(*rect), F4(*rx), F4(*ry), mode, factor, spread, F2(*shape), AA, push, out, C.byref(n)) == 0
    rects = [tuple(out[4 * k:4 * k + 4]) for k in range(3)]
    assert n.value == sum(1 for q in rects if q[2] > q[0] and q[3] > q[1])
    return rects


# ---------------------------------------------------------------- the oracle's coverage formulas, float32, over a pixel grid
def sd_rounded_box(px, py, bx, by, r):
    rr = np.where(px > 0, np.where(py > 0, r[0], r[1]), np.where(py > 0, r[2], r[3])).astype(f32)
    qx, qy = np.abs(px) - bx + rr, np.abs(py) - by + rr
    mx, my = np.maximum(qx, f32(0)), np.maximum(qy, f32(0))
    return np.minimum(np.maximum(qx, qy), f32(0)) + np.sqrt(mx * mx + my * my) - rr


def sd_ellipse(px, py, rx, ry):
    sx, sy = max(rx, f32(0.000001)), max(ry, f32(0.000001))
    ax, ay = px / sx, py / sy
    k0 = np.sqrt(ax * ax + ay * ay)
    bx, by = px / f32(sx * sx), py / f32(sy * sy)
    k1 = np.sqrt(bx * bx + by * by)
    return np.where(k0 <= f32(0.000001), -min(sx, sy), k0 * (k0 - f32(1)) / np.maximum(k1, f32(0.000001))).astype(f32)


def sd_elliptical_rounded_box(px, py, bx, by, packed):
    out = np.zeros(px.shape, f32)
    quadrant = [(px > 0) & (py > 0), (px > 0) & ~(py > 0), ~(px > 0) & (py > 0), ~(px > 0) & ~(py > 0)]
    for k in range(4):
        sel, m = f32(packed[k]), quadrant[k]
        if not m.any():
            continue
        if sel < 0:
            r = f32(-sel - f32(1))
            d = sd_rounded_box(px, py, bx, by, [r] * 4)
        else:
            pv = f32(np.floor(sel + f32(0.5)))
            hi = f32(np.floor(pv / f32(4096)))
            rx = f32(f32(pv - f32(4096) * hi) * bx / f32(4095))
            ry = f32(hi * by / f32(4095))
            if rx <= 0 or ry <= 0:
                qx, qy = np.abs(px) - bx, np.abs(py) - by
                mx, my = np.maximum(qx, f32(0)), np.maximum(qy, f32(0))
                d = np.minimum(np.maximum(qx, qy), f32(0)) + np.sqrt(mx * mx + my * my)
            elif rx == ry:
                d = sd_rounded_box(px, py, bx, by, [rx] * 4)
            else:
                qx, qy = np.abs(px) - bx + rx, np.abs(py) - by + ry
                corner = (qx > 0) & (qy > 0)
                with np.errstate(all="ignore"):
                    d = np.where(corner, sd_ellipse(qx, qy, rx, ry), np.maximum(qx - rx, qy - ry))
        out[m] = d.astype(f32)[m]
    return out


def saturated(rec, x0, y0, x1, y1):
    """is the coverage term saturated at every pixel centre of [x0, x1) x [y0, y1)?  Returns the number of pixels where it is not."""
    xs, ys = np.meshgrid(np.arange(x0, x1, dtype=f32), np.arange(y0, y1, dtype=f32))
    u = (xs + f32(0.5) - f32(rec.ox)) / f32(rec.w_px)
    v = (ys + f32(0.5) - f32(rec.oy)) / f32(rec.h_px)
    px, py = (u - f32(0.5)) * f32(2) * rec.p0, (v - f32(0.5)) * f32(2) * rec.p1
    aa = f32(rec.aa)  # (AA in this file's sweep; tests/test_hostile_shapes_host.py sweeps the factor too)
    sd = (lambda qx, qy, bx, by: sd_elliptical_rounded_box(qx, qy, bx, by, rec.r)) if rec.ellip else (lambda qx, qy, bx, by: sd_rounded_box(qx, qy, bx, by, rec.r))
    clamp01 = lambda t: np.minimum(np.maximum(t, f32(0)), f32(1))
    if rec.mode == 9:
        qx, qy = px, -py
        clip_a = f32(1) - clamp01(aa * sd(qx, qy, rec.p0, rec.p1) + f32(0.5))
        s = sd(qx - rec.p2, qy + rec.p3, rec.p0, rec.p1) + rec.f1
        sigma = max(f32(0.5) * rec.f0, f32(0.5))
        z = s / sigma
        a = np.exp(f32(-0.5) * z * z).astype(f32)
        alpha = clip_a * np.where(s < 0, np.minimum(a, f32(1)), f32(1)).astype(f32)
        return int((~(alpha < f32(0.49 / 255.0))).sum())
    dist = sd(px, -py, rec.p2, rec.p3)
    if rec.mode == 7:
        return int((~(dist - rec.f1 <= 0)).sum())
    if rec.mode == 12:
        h = rec.f0 * f32(0.5)
        s = np.abs(dist + h) - h
        return int((f32(1) - clamp01(aa * s + f32(0.5)) != 0).sum())
    if rec.mode == 11:  # (the hard-edged stroke: alpha exactly 0 inside)
        h = rec.f0 * f32(0.5)
        return int((np.abs(dist + h) - h < 0).sum())
    return int((f32(1) - clamp01(aa * dist + f32(0.5)) != f32(1)).sum())


def test_every_rectangle_of_the_union_is_saturated_and_the_first_is_the_draw_records():
    L = _lib()
    n_rects = n_extra = n_cases = 0
    for case in cases():
        rect, rx, ry, mode, factor, spread, shape, push = case
        rects = _union(L, case)
        one = I4()
        assert L.fdh_saturated_core(F4(*rect), F4(*rx), F4(*ry), mode, factor, spread, F2(*shape), AA, one) == 0
        if not push:  # (fdh_saturated_core describes the draw; a push's threshold is the fill's)
            assert tuple(one) == rects[0], (case, tuple(one), rects)
        rec = CS.Rec(rect, rx, ry, mode, factor, spread, shape, AA, bool(push))
        n_cases += 1
        for k, (x0, y0, x1, y1) in enumerate(rects):
            if not (x1 > x0 and y1 > y0):
                continue
            # inside the quad: the bin launch takes a core strip as covered
            assert x0 >= rec.ox and y0 >= rec.oy and x1 <= rec.ox + rec.w_px and y1 <= rec.oy + rec.h_px, (case, rects)
            bad = saturated(rec, x0, y0, x1, y1)
            assert bad == 0, (case, k, rects, bad)
            n_rects += 1
            n_extra += int(k > 0 and (x0, y0, x1, y1) != rects[0])
    assert n_cases == len(HALF_EXTENTS) * len(RADII) * len(MODES)
    assert n_rects > n_cases and n_extra > n_cases // 3  # the sweep does reach the bands


def test_python_restatement_gives_the_librarys_rectangles():
    L = _lib()
    for case in cases():
        rect, rx, ry, mode, factor, spread, shape, push = case
        rects = _union(L, case)
        want = {q for q in rects if q[2] > q[0] and q[3] > q[1]}
        rec = CS.Rec(rect, rx, ry, mode, factor, spread, shape, AA, bool(push))
        assert set(CS.core_rects(rec, True)) == want, (case, rects, CS.core_rects(rec, True))
        first = CS.core_rects(rec, False)
        assert (first[0] if first else (0, 0, 0, 0)) == rects[0], (case, rects, first)


def test_first_rectangle_is_what_the_commit_before_the_union_computed():
    """tests/golden/core_union_first_rect.json: fdh_saturated_core's answers for a few dozen cases of the sweep, recorded from the library
    of the commit before BinRec learned about the bands."""
    L = _lib()
    with open(os.path.join(ROOT, "tests", "golden", "core_union_first_rect.json")) as f:
        pinned = json.load(f)["records"]
    assert len(pinned) >= 36
    all_cases = list(cases())
    for p in pinned:
        rect, rx, ry, mode, factor, spread, shape, push = all_cases[p["case"]]
        assert push == 0 and [float(f32(v)) for v in rect] == p["rect"] and mode == p["mode"]
        one = I4()
        assert L.fdh_saturated_core(F4(*rect), F4(*rx), F4(*ry), mode, factor, spread, F2(*shape), AA, one) == 0
        assert list(one) == p["core"], (p, list(one))
        assert list(_union(L, all_cases[p["case"]])[0]) == p["core"]
