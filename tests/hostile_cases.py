"""Hostile geometry for the compositor, as data (no GPU, no library): the frames of tests/test_hostile_shapes.py,
tests/test_hostile_shapes_host.py and `tools/make_goldens.py hostile`.

Every fast path of the compositor is a geometric argument -- "a strip inside this rectangle is saturated", "inside a stroke the draw
is a no-op", "these four pixels share a corner".  The frames below put the arguments where they are tightest: sub-pixel boxes, radii
beyond the box, strokes wider than the node, shadows with blur 0 or wider than the frame, negative spread, AA factors from 0.05 to 50,
degenerate curves, empty clips, coordinates far outside the frame, hundreds of alpha-1 layers on one pixel.

Every frame is 250 x 190: 4 x 3 bins of 64 px, the last column and row partial, no multiple of the 32 x 8 strip either.  Coordinates
sit on fractional positions so that shapes straddle strip and bin boundaries.

CALL-LEVEL frames (FAMILIES) are lists in the format Oracle.replay, HipContext.replay_calls and ref_swiftshader.replay take; they reach
parameters no front-end produces.  NODE-LEVEL frames (hostile_nodes) are Renders: the front-end's decomposition, its skip rules and
culling are in the loop.

Each frame comes in two forms:
  direct  as it is: no phase holds more than 64 draws (`stack`, 300 draws, is the exception; the curves are two frames for that reason)
  lists   the frame plus copies shifted by (7.3, 4.6) each until a phase passes 64 draws: a bin launch, deep lists

Which of the direct forms the library composites WITHOUT a bin launch is its own rule (fdh_context.cpp direct_frame: at most 64 draws in
every phase, none of them a rotated quad or a curve): TAKES_DIRECT_LAUNCH says which of the frames here that is."""
import math
import random

W, H = 250, 190
WHITE = [1.0, 1.0, 1.0, 1.0]
GLASS = [0.2, 0.3, 0.4, 0.5]  # a translucent clear colour: the surface's alpha is in play
SHIFT = (7.3, 4.6)
Z4 = [0, 0, 0, 0]


def _sdf(rect, color, rx, mode=3, factor=4.0, spread=0.0, shape=(0.0, 0.0), ry=None, colors=None, fill_mode=0, mid=Z4, stop=Z4, mid_pos=0.5):
    """a draw_rounded_rect_sdf call; radii in node order TL, TR, BL, BR"""
    rx = [rx] * 4 if isinstance(rx, (int, float)) else list(rx)
    ry = rx if ry is None else ([ry] * 4 if isinstance(ry, (int, float)) else list(ry))
    cols = [list(c) for c in colors] if colors else [list(color)] * 4
    return ["draw_rounded_rect_sdf", [float(v) for v in rect], cols, [float(v) for v in rx], [float(v) for v in ry], int(mode), float(factor), float(spread),
            [float(shape[0]), float(shape[1])], int(fill_mode), list(mid), list(stop), float(mid_pos)]


def _solid(c):
    return {"kind": 0, "axis": 0, "start": list(c), "mid": Z4, "stop": Z4, "mid_pos": 128}


# ------------------------------------------------------------------------------------------------ call-level families
def slivers():
    """boxes 0.3, 0.5, 1.0, 1.5 and 2.49 px wide or tall in modes 3, 12 and 7; zero and negative sizes; sliver gradient quads"""
    out = [_sdf([20.4, 120.3, 150.7, 60.2], (40, 90, 200, 90), 6)]
    for k, mode in enumerate((3, 12, 7)):
        for i, t in enumerate((0.3, 0.5, 1.0, 1.5, 2.49)):
            col = [(220, 40, 40, 255), (20, 120, 60, 200), (0, 0, 0, 180)][k]
            x, y = 6.37 + 15.21 * i + 80.0 * k, 4.61 + 1.7 * i
            fac, spr = {3: (4.0, 0.0), 12: (1.0, 0.0), 7: (2.0, 0.0)}[mode]
            if mode == 7:  # the padded quad around a sliver shape (pad = round(1.5 blur))
                out.append(_sdf([x - 3, y - 3, t + 6, 46.5], col, 0, 7, fac, spr, (t, 40.5)))
                out.append(_sdf([x - 3 + 1.1, y + 55.3 - 3 + 9.77 * i, 46.5, t + 6], col, 0, 7, fac, spr, (40.5, t)))
            else:
                out.append(_sdf([x, y, t, 40.5], col, 0.5 * t if i % 2 else 0, mode, fac, spr))
                out.append(_sdf([x + 1.1, y + 55.3 + 9.77 * i, 40.5, t], col, 0.5 * t if i % 2 else 0, mode, fac, spr))
    out += [_sdf([100.5, 100.5, 0.0, 30.0], (255, 0, 0, 255), 0), _sdf([100.5, 100.5, 30.0, -4.0], (255, 0, 0, 255), 0),
            _sdf([100.5, 100.5, -20.0, -20.0], (255, 0, 0, 255), 4, 12, 3.0)]
    out.append(_sdf([200.6, 110.2, 1.0, 70.0], (255, 200, 0, 255), 0, fill_mode=2, mid=(0, 200, 255, 255), stop=(200, 0, 255, 120), mid_pos=0.3))
    out.append(_sdf([180.2, 185.4, 60.0, 0.7], (255, 200, 0, 255), 0, fill_mode=1, mid=(0, 200, 255, 255), stop=(200, 0, 255, 120), mid_pos=0.7))
    return out


def radii():
    """radius 0, below 1, equal to the half extent (a disc, a pill), far beyond it; four different; elliptical 100:1, 1:100, with a zero
    component, with rx = ry on some corners only -- each as a fill and, smaller, as a stroke"""
    big = [0, 0.4, 1000, (4, 26, 12, 18)]
    out = []
    for i, r in enumerate(big):
        x, y = 3.3 + 124.4 * (i % 2), 2.7 + 62.3 * (i // 2)
        out.append(_sdf([x, y, 118.5, 57.25], [(220, 40, 40, 255), (40, 180, 90, 150), (60, 90, 220, 255), (238, 140, 30, 200)][i], r))
    ell = [((100, 100, 100, 100), (1, 1, 1, 1)), ((1, 1, 1, 1), (100, 100, 100, 100)), ((20, 0, 20, 8), (0, 15, 10, 8)), ((12, 30, 12, 5), (12, 9, 40, 5))]
    for i, (rx, ry) in enumerate(ell):
        out.append(_sdf([5.6 + 61.2 * i, 128.4, 57.5, 38.6], (30, 30, 30, 255) if i % 2 else (120, 20, 160, 170), rx, ry=ry))
        out.append(_sdf([5.6 + 61.2 * i, 128.4, 57.5, 38.6], (255, 255, 255, 200), rx, 12, 2.5, ry=ry))
    out.append(_sdf([40.5, 168.2, 20.0, 20.0], (0, 160, 160, 255), 10))          # a disc
    out.append(_sdf([70.25, 169.75, 90.0, 18.0], (200, 30, 160, 180), 9))        # a pill
    out.append(_sdf([170.5, 168.5, 60.0, 19.0], (10, 10, 10, 255), 0.4, 12, 1.0))
    for i, r in enumerate(big):
        out.append(_sdf([30.6 + 124.4 * (i % 2), 14.3 + 62.3 * (i // 2), 64.0, 32.0], (250, 250, 250, 140), r, 12, 5.0))
    return out


def aa_factors():
    """set_aa_factor 0.05, 0.3, 4 and 50 over a fill, both annular modes, a clip push and a rect mask; restored between groups"""
    out = []
    for i, aa in enumerate((0.05, 0.3, 4.0, 50.0)):
        x = 3.4 + 61.7 * i
        out.append(["set_aa_factor", aa])
        out.append(_sdf([x, 4.3, 55.0, 40.0], (200, 40, 90, 255), (12, 3, 0, 20)))
        out.append(_sdf([x + 2.2, 50.6, 50.0, 30.0], (30, 30, 200, 180), 9, 11, 7.0))
        out.append(_sdf([x + 1.1, 86.2, 52.0, 30.0], (20, 140, 60, 230), 9, 12, 7.0))
        out += [["begin_mask", [x, 122.7, 54.0, 28.0], [10.0] * 4, [10.0] * 4], ["end_mask"],
                _sdf([x - 8.0, 118.0, 80.0, 20.5], (240, 160, 0, 255), 0), ["pop_mask"]]
        out += [["begin_rect_mask", [x + 0.5, 156.3, 53.0, 28.0], [14.0, 2.0, 6.0, 0.0], [14.0, 2.0, 6.0, 0.0]],
                _sdf([x - 8.0, 150.0, 80.0, 30.5], (90, 0, 140, 200), 4), ["pop_rect_mask"]]
        out.append(["set_aa_factor", 1.2])
    return out


def strokes():
    """modes 12 and 11 with weight 0, 0.2, the half extent, 30 on a 40 x 24 box (no interior is left) and negative; a fill followed by
    a stroke over the same quad (an LE_SHARE run); the same pair with different radii (no run)"""
    out = [_sdf([4.5, 100.25, 240.0, 85.5], (250, 250, 245, 200), 0)]
    for k, mode in enumerate((12, 11)):
        for i, wgt in enumerate((0.0, 0.2, 12.0, 30.0, -3.0)):
            out.append(_sdf([5.3 + 48.6 * i, 6.4 + 44.7 * k, 40.0, 24.0], (200, 30, 60, 255) if i % 2 else (20, 60, 200, 160), 5, mode, wgt))
    out.append(_sdf([10.6, 105.3, 100.0, 60.0], (40, 180, 90, 255), 14))
    out.append(_sdf([10.6, 105.3, 100.0, 60.0], (0, 0, 0, 200), 14, 12, 6.0))
    out.append(_sdf([130.4, 108.7, 100.0, 60.0], (238, 140, 30, 180), 14))
    out.append(_sdf([130.4, 108.7, 100.0, 60.0], (90, 45, 0, 220), (14, 2, 14, 30), 12, 6.0))
    out.append(_sdf([60.7, 150.2, 120.0, 36.0], (118, 168, 255, 230), 8, 12, 18.0))  # weight = the half extent
    return out


def shadows():
    """mode 7 with blur 0 and 100, spread -3, -500 and larger than the box; mode 8; mode 9 with blur 0 and 100, spread -8 and 40, offsets
    inside and beyond the box, radii 400 on a 200 x 10 quad; a gradient-filled shadow (the spread is ignored); black and coloured sources"""
    def drop(x, y, w, h, blur, spread, col, r=6, mode=7, **kw):
        pad = max(math.floor(spread + 0.5) + math.floor(1.5 * blur + 0.5), 0)  # (the front-end's padding, drop_shadows)
        return _sdf([x - pad, y - pad, w + 2 * pad, h + 2 * pad], col, r, mode, blur, spread, (w, h), **kw)

    black, red = (0, 0, 0, 150), (220, 30, 30, 170)
    out = [drop(10.5, 8.25, 50, 30, 0.0, 4.0, black), drop(80.3, 10.6, 50, 30, 100.0, 0.0, red), drop(150.7, 9.4, 50, 30, 6.0, -3.0, black),
           drop(20.2, 60.8, 50, 30, 6.0, -500.0, red), drop(100.6, 70.3, 20, 12, 4.0, 80.0, (0, 0, 0, 40)),
           drop(180.4, 62.5, 40, 24, 6.0, 40.0, (30, 30, 200, 120), mode=8)]
    out.append(_sdf([150.2, 60.3, 80.0, 50.0], red, 8, 7, 6.0, 3.0))  # no shape: the quad is the shape, the shadow is cut at its edge
    def inner(rect, blur, spread, off, col, r=8):
        return _sdf(rect, col, r, 9, blur, spread, off)

    out += [inner([8.6, 110.4, 60.0, 36.0], 0.0, 3.0, (0.0, 0.0), black), inner([75.2, 108.9, 60.0, 36.0], 100.0, 0.0, (2.0, -2.0), red),
            inner([142.8, 111.3, 60.0, 36.0], 5.0, -8.0, (0.0, 0.0), black), inner([8.6, 150.7, 60.0, 36.0], 5.0, 40.0, (3.0, 3.0), red),
            inner([75.2, 152.1, 60.0, 36.0], 6.0, 2.0, (50.0, -40.0), black), inner([142.8, 149.6, 60.0, 36.0], 6.0, 2.0, (200.0, 150.0), red),
            inner([24.7, 96.4, 200.0, 10.0], 3.0, 1.0, (1.0, 1.0), (0, 90, 0, 220), r=400)]
    out.append(drop(205.3, 120.6, 36, 50, 8.0, 12.0, (255, 70, 70, 170), fill_mode=2, mid=(70, 255, 70, 170), stop=(70, 110, 255, 170), mid_pos=0.4))
    out.append(_sdf([205.3 - 12, 10.6 - 12, 36 + 24, 40 + 24], None, 5, 7, 8.0, 0.0, (36, 40),
                    colors=[(255, 70, 70, 170), (255, 70, 70, 170), (70, 110, 255, 170), (70, 110, 255, 170)]))
    return out


def gradients():
    """fill modes 1 - 4 with mid position 0, 0.004, 0.5, 0.996 and 1 (clamped to 0.01 and 0.99 by the draw call); stops with alpha 0"""
    out = []
    for j, fm in enumerate((1, 2, 3, 4)):
        for i, mp in enumerate((0.0, 0.004, 0.5, 0.996, 1.0)):
            a = 0 if (i + j) % 3 == 0 else 255
            out.append(_sdf([3.3 + 49.1 * i, 2.7 + 46.6 * j, 44.5, 41.25], (240, 120, 20, 255 if i != 2 else 0), (0, 6, 12, 20)[j], 3 if (i + j) % 4 else 12, 4.0,
                            fill_mode=fm, mid=(30, 160, 220, a), stop=(90, 20, 180, 200), mid_pos=mp))
    return out


_CURVE_SHAPES = [
    ("regular", (-24.0, 12.0), (0.5, -30.0), (24.0, 10.0)),
    ("collinear", (-24.0, -12.0), (0.0, 0.0), (24.0, 12.0)),          # bb = 0
    ("p0_is_p1", (-20.0, 8.0), (-20.0, 8.0), (22.0, -9.0)),
    ("a_point", (3.5, -2.25), (3.5, -2.25), (3.5, -2.25)),
    ("cusp", (-18.0, 10.0), (20.0, -14.0), (-18.0, 10.0)),           # p0 = p2
    ("nearly_straight", (-25.0, -6.0), (0.0, 0.02), (25.0, 6.0)),  # (at 0.001 the closed-form root is noise: the oracle and the shaders part by 85 LSB)
]


def _curves(shapes):
    out = []
    k = 0
    for name, p0, p1, p2 in shapes:
        for cap in (1, 2, 3):  # scRound, scButt, scSquare: modes 18, 19, 20
            for wi, wgt in enumerate((0.0, 0.3, 3.0, 40.0)):
                x, y = 2.3 + 20.7 * (k % 9), 1.6 + 46.3 * wi
                col = [(10, 120, 60, 255), (150, 20, 160, 140), (0, 90, 160, 230)][cap - 1] if wgt < 40 else (160, 90, 0, 40)
                out.append(["draw_quadratic_bezier_sdf", [x, y, 60.0, 42.0], _solid(col), list(p0), list(p1), list(p2), wgt, cap])
            k += 1
    return out


def curves_a():
    """caps 18, 19, 20 x weights 0, 0.3, 3, 40: a regular span, collinear control points (bb = 0), p0 = p1"""
    return _curves(_CURVE_SHAPES[:3])


def curves_b():
    """... all three points equal, p0 = p2 (a cusp), a nearly straight span"""
    return _curves(_CURVE_SHAPES[3:])


def masks():
    """a clip 0.4 px wide (a second one, whose quad snaps to nothing, is in `transforms`); a clip with radius 500 on a 60 x 40 box; a nested clip whose box misses its parent's (its content is
    invisible); a rect mask 1 px tall; a rect mask with elliptical radii 30/80 by 10/60; a 12-px stroke drawn under each"""
    def content(x, y, w, h):
        return [_sdf([x, y, w, h], (43, 159, 234, 220), 6), _sdf([x, y, w, h], (120, 60, 0, 255), 6, 12, 12.0)]

    out = [_sdf([2.5, 2.5, 245.0, 185.0], (235, 235, 225, 255), 3)]
    # (30.8 .. 31.2: the quad snaps to one pixel column, whose centre lies 0.3 px outside the shape)
    out += [["begin_mask", [30.8, 10.2, 0.4, 60.0], [0.0] * 4, [0.0] * 4], ["end_mask"]] + content(10.5, 14.5, 60.0, 40.0) + [["pop_mask"]]
    out += [["begin_mask", [90.6, 8.4, 60.0, 40.0], [500.0] * 4, [500.0] * 4], ["end_mask"]] + content(80.2, 4.7, 90.0, 50.0) + [["pop_mask"]]
    out += [["begin_mask", [10.3, 100.6, 80.0, 50.0], [10.0] * 4, [10.0] * 4], ["end_mask"]] + content(20.1, 95.2, 50.0, 70.0)
    out += [["begin_mask", [150.2, 20.7, 40.0, 30.0], [4.0] * 4, [4.0] * 4], ["end_mask"]] + content(0.5, 0.5, 240.0, 180.0) + [["pop_mask"], ["pop_mask"]]
    out += [["begin_rect_mask", [5.5, 80.3, 200.0, 1.0], [0.0] * 4, [0.0] * 4]] + content(20.4, 62.3, 150.0, 36.0) + [["pop_rect_mask"]]
    out += [["begin_rect_mask", [110.4, 105.8, 120.0, 70.0], [30.0, 80.0, 30.0, 80.0], [10.0, 60.0, 10.0, 60.0]]] + content(100.3, 100.1, 140.0, 80.0) + [["pop_rect_mask"]]
    return out


def transforms():
    """rotate by 1e-4 rad, pi / 4, pi / 2 and pi; scale (-1, 0.02) over a 30 x 900 box; each with a fill and a stroke, four radii; a clip
    whose quad is empty"""
    out = [_sdf([3.5, 3.5, 243.0, 183.0], (240, 240, 250, 255), 0)]
    r4 = (2, 9, 0.5, 14)
    for i, ang in enumerate((1e-4, math.pi / 4, math.pi / 2, math.pi)):
        out += [["save_transform"], ["translate", 40.3 + 55.4 * i, 50.6 + 20.2 * (i % 2)], ["rotate", ang],
                _sdf([-30.5, -18.25, 61.0, 36.5], (220, 40, 40, 200), r4), _sdf([-30.5, -18.25, 61.0, 36.5], (0, 0, 0, 255), r4, 12, 4.0), ["restore_transform"]]
    out += [["save_transform"], ["translate", 200.6, 120.3], ["scale", -1.0, 0.02],
            _sdf([0.0, 0.0, 30.0, 900.0], (40, 180, 90, 220), r4), _sdf([0.0, 0.0, 30.0, 900.0], (0, 60, 0, 255), r4, 12, 3.0), ["restore_transform"]]
    out += [["save_transform"], ["translate", 60.2, 140.7], ["rotate", math.pi / 4], ["scale", -1.0, 0.02],
            _sdf([0.0, 0.0, 80.0, 1500.0], (60, 90, 220, 180), r4), _sdf([0.0, 0.0, 80.0, 1500.0], (0, 0, 90, 255), r4, 12, 3.0), ["restore_transform"]]
    # a clip 0.4 px wide around a pixel centre (30.3 .. 30.7): its quad snaps to NO pixel column, which the library records as a general
    # quad like the rotated ones above (the push stays: a clip that is not there would let its content through); its content is invisible
    out += [["begin_mask", [30.3, 100.2, 0.4, 60.0], [0.0] * 4, [0.0] * 4], ["end_mask"], _sdf([10.5, 104.5, 60.0, 40.0], (43, 159, 234, 220), 6),
            _sdf([10.5, 104.5, 60.0, 40.0], (120, 60, 0, 255), 6, 12, 12.0), ["pop_mask"]]
    return out


def far():
    """a box from -30000.5 to +30100 with radius 29000; a stroke spanning +-40000 horizontally; a shadow spanning +-40000 vertically
    (everything stays below the recorder's 1e6 guard)"""
    return [_sdf([-30000.5, -30000.5, 60100.5, 60100.5], (200, 220, 240, 200), 29000),
            _sdf([-40000.0, 60.3, 80000.0, 50.5], (200, 30, 60, 230), 10, 12, 6.0),
            _sdf([100.6, -40000.0, 60.0, 80000.0], (0, 0, 0, 150), 8, 7, 8.0, 2.0, (36.0, 79976.0)),
            _sdf([-29000.5, 130.4, 29100.0, 40.0], (20, 140, 60, 255), 20),   # ends inside the frame: a rounded cap at x = 99.5
            _sdf([180.3, 150.6, 39000.0, 39000.0], (90, 0, 140, 180), 30000)]  # a quarter disc of radius 19500 from the corner


def stack(n=300):
    """300 boxes with alpha 1 - 3 and radius 12, shifted by 0.1 px each, over one region"""
    return [_sdf([40.25 + 0.1 * i, 30.5 + 0.1 * i, 150.0, 110.0], ((37 * i) % 256, (91 * i) % 256, (53 * i) % 256, 1 + i % 3), 12) for i in range(n)]


# name -> (body builder, clear colour)
FAMILIES = {
    "slivers": (slivers, WHITE), "radii": (radii, WHITE), "aa_factors": (aa_factors, WHITE), "strokes": (strokes, GLASS), "shadows": (shadows, GLASS),
    "gradients": (gradients, GLASS), "curves_a": (curves_a, WHITE), "curves_b": (curves_b, WHITE), "masks": (masks, WHITE),
    "transforms": (transforms, WHITE), "far": (far, WHITE), "stack": (stack, GLASS),
}


def n_draws(body):
    """the draw calls of a body that can leave a record (a clip push is one; a draw of no size or no weight leaves none)"""
    n = 0
    for c in body:
        if c[0] == "draw_rounded_rect_sdf":
            n += c[1][2] > 0 and c[1][3] > 0
        elif c[0] == "draw_quadratic_bezier_sdf":
            n += c[6] > 0
        elif c[0] in ("begin_mask", "begin_rect_mask"):
            n += 1
    return n


def copies_for_lists(draws):
    """how many copies of a frame of `draws` draw calls pass 64 records in its phase: twice the calls it takes, since a sliver that covers
    no pixel centre or a draw off the frame leaves no record (tests/test_hostile_shapes_host.py counts the records)"""
    return 2 if draws > 64 else 128 // max(draws, 1) + 1


def calls(name, form="direct"):
    """the call stream of a call-level frame: begin_frame .. end_frame"""
    body_fn, clear = FAMILIES[name]
    body = body_fn()
    out = [["begin_frame", 1, list(clear)]]
    if form == "direct":
        out += body
    else:
        assert form == "lists"
        for c in range(copies_for_lists(n_draws(body))):
            out += [["save_transform"], ["translate", SHIFT[0] * c, SHIFT[1] * c]] + body + [["restore_transform"]]
    out.append(["end_frame"])
    return out


# ------------------------------------------------------------------------------------------------ node-level frames
NODE_SEEDS = (1, 2, 3, 4)
NODE_CLEAR = GLASS  # (under the opaque first root: the clear folds into it)
SIZES = (0.0, 0.3, 1.0, 1.5, 7.0, 40.0, 120.5, 3.0 * W)
CORNERS = (0, 1, 5, 1000)  # (Fig.corners are 16-bit integers: no radius below 1 but 0 at node level)
WEIGHTS = (0.0, 0.05, 0.5, 3.0, 60.0, 1000.0)
BLURS = (0.0, 0.3, 8.0, 200.0)
SPREADS = (-50.0, -3.0, 0.0, 4.0, 300.0)
MID_POS = (0, 1, 128, 254, 255)
ROTATIONS = (0.001, 45.0, 90.0, 180.0, -33.3)
ROTATED_SEEDS = (2, 4)  # seeds 1 and 3 stay upright: the front-end's streams reach the direct launch too
N_ROOTS = 7


def hostile_nodes(seed, copies=1):
    """a seeded mix of the same extremes on Fig nodes; `copies` > 1: the same nodes again, shifted by SHIFT each"""
    from figdraw_amd.scene import (Fig, FigFlags, FigKind, FillGradientAxis, RenderList, Renders, RenderShadow, RenderStroke, ShadowStyle, fill, linear, rect,
                                   rgba)

    lst = RenderList()
    lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(0, 0, W, H), fill=rgba(244, 244, 238, 255)))
    for c in range(copies):
        rnd = random.Random(seed)
        dx, dy = SHIFT[0] * c, SHIFT[1] * c

        def col(lo=60):
            return rgba(rnd.randrange(256), rnd.randrange(256), rnd.randrange(256), rnd.choice((255, rnd.randrange(lo, 255))))

        def some_fill():
            if rnd.random() < 0.5:
                return fill(col())
            return linear(col(), col(0), col(), axis=rnd.choice(list(FillGradientAxis)), midPos=rnd.choice(MID_POS))

        def node(parent, depth):
            bw, bh = rnd.choice(SIZES), rnd.choice(SIZES)
            if depth == 0 and rnd.random() < 0.75:  # (most roots have a visible size, or the frame is empty)
                bw, bh = rnd.choice(SIZES[4:] + SIZES[5:7]), rnd.choice(SIZES[4:] + SIZES[5:7])
            x, y = rnd.uniform(-0.3 * W, W), rnd.uniform(-0.3 * H, H)
            f = Fig(kind=FigKind.nkRectangle, screenBox=rect(x + dx, y + dy, bw, bh), fill=some_fill(), corners=[rnd.choice(CORNERS) for _ in range(4)])
            if rnd.random() < 0.3:
                f.cornerRadiiY = [rnd.choice(CORNERS) for _ in range(4)]
                f.flags |= FigFlags.NfEllipticalCorners
            if rnd.random() < 0.6:
                f.stroke = RenderStroke(weight=rnd.choice(WEIGHTS), fill=some_fill())
            if rnd.random() < 0.5:
                f.shadows = [RenderShadow(style=rnd.choice((ShadowStyle.DropShadow, ShadowStyle.InnerShadow)), blur=rnd.choice(BLURS), spread=rnd.choice(SPREADS),
                                          x=rnd.choice((0.0, 3.0, -400.0, 400.0, rnd.uniform(-20, 20))), y=rnd.choice((0.0, -2.0, 400.0, rnd.uniform(-20, 20))),
                                          fill=some_fill()) for _ in range(rnd.randrange(1, 4))]
            rot = rnd.random() < 0.3  # (drawn for every seed: the upright seeds hold the same nodes otherwise)
            angle = rnd.choice(ROTATIONS)
            if rot and seed in ROTATED_SEEDS:
                f.rotation = angle
            clip = rnd.random() < (0.45 if depth < 3 else 0.0)
            if clip:
                f.flags |= rnd.choice((FigFlags.NfClipContent, FigFlags.NfRectMaskContent))
            idx = lst.addRoot(f) if parent is None else lst.addChild(parent, f)
            if clip:
                for _ in range(rnd.randrange(1, 3)):
                    node(idx, depth + 1)

        for _ in range(N_ROOTS):
            node(None, 0)
    out = Renders()
    out.setLayer(0, lst)
    return out


# ------------------------------------------------------------------------------------------------ the frames, by name
NODE_FRAMES = tuple(f"nodes{s}" for s in NODE_SEEDS)
FRAMES = tuple(FAMILIES) + NODE_FRAMES
FORMS = ("direct", "lists")
# the direct forms the library composites without a bin launch: at most 64 draws per phase and no rotated quad, no curve
TAKES_DIRECT_LAUNCH = tuple(n for n in FAMILIES if n not in ("curves_a", "curves_b", "transforms", "stack")) + tuple(f"nodes{s}" for s in NODE_SEEDS if s not in ROTATED_SEEDS)
# frames of (c): the lists form as three row stripes (no multiples of 8 tall), and as a retained scene
STRIPES = ((0, 61), (61, 131), (131, H))
STRIPE_FRAMES = ("shadows", "masks", "nodes1")

# Pixels of a frame at which the HIP path may sit 2 LSB from the oracle: name, form -> [(x, y, reason)].  A pixel belongs here only if the
# reference's formula itself amplifies last-bit differences there (the oracle's formula, evaluated with the distance nudged by one float32
# ulp either way, gives another 8-bit result); at most MAX_AMPLIFIED per frame.
AMPLIFIED = {}
MAX_AMPLIFIED = 4
MAX_GOLDEN_OUTLIERS = 8  # pixels per frame the manifest may list (the oracle itself > 1 LSB from the golden there)


NODE_COPIES = 4  # copies of hostile_nodes(seed) in the lists form: more than 64 draws for every seed (the host test counts them)


def scene(name, form="direct"):
    """the Renders of a node-level frame"""
    seed = int(name[len("nodes"):])
    return hostile_nodes(seed, 1 if form == "direct" else NODE_COPIES)


def is_node_frame(name):
    return name in NODE_FRAMES


def clear_of(name):
    return NODE_CLEAR if is_node_frame(name) else FAMILIES[name][1]


def render(backend, name, form="direct"):
    """draw frame `name` on `backend` (an Oracle or a HipContext)"""
    if is_node_frame(name):
        backend.render_frame(scene(name, form), W, H, color=tuple(clear_of(name)))
    else:
        backend.W, backend.H = W, H
        (backend.replay_calls if hasattr(backend, "replay_calls") else backend.replay)(calls(name, form))
