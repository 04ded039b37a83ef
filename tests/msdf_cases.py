"""What the distance-field tests share (test_msdf_host.py on a CPU, test_msdf.py on the device): the inputs, the tolerance, the winding
test and the reconstruction statistics.  Inputs: the 94 outlines of tests/golden/outlines_ubuntu20.npz scaled by 2 about the origin
and moved by R = 4 texels into an image of (2 w + 2 R) x (2 h + 2 R), and a dozen of them at scale 1 with R = 2 (inputs()); and what a
font tool never emits but an application can pass (hostile_inputs())."""
import math
import os

import numpy as np

import msdf_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
CAP = 2  # texels per image that may differ from the reference by more than 1 LSB (a texel centre on a tie: float32 and float64 may pick different edges)


def inputs():
    """-> [(name, segs float32 (n, 6), w, h, R)]"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "outlines_ubuntu20.npz"))
    out = []
    for code in range(33, 127):
        segs, (w, h) = z[f"segs_{code}"].astype(np.float32), z[f"size_{code}"]
        out.append((f"{chr(code)} x2", segs * np.float32(2) + np.float32(4), 2 * int(w) + 8, 2 * int(h) + 8, 4))
    for code in list(range(33, 127))[::8][:12]:
        segs, (w, h) = z[f"segs_{code}"].astype(np.float32), z[f"size_{code}"]
        out.append((f"{chr(code)} x1", segs + np.float32(2), int(w) + 4, int(h) + 4, 2))
    return out


def poly(pts):
    """a closed polygon as line segments"""
    pts = [tuple(map(float, p)) for p in pts]
    return np.array([[a[0], a[1], NAN, NAN, b[0], b[1]] for a, b in zip(pts, pts[1:] + pts[:1])], np.float32)


def path(start, *steps):
    """a closed contour from `start`: a step (x, y) is a line to there, (cx, cy, x, y) a quadratic; the last step must return to `start`"""
    rows, at = [], tuple(map(float, start))
    for s in steps:
        s = tuple(map(float, s))
        rows.append([at[0], at[1], NAN, NAN, s[0], s[1]] if len(s) == 2 else [at[0], at[1], s[0], s[1], s[2], s[3]])
        at = s[-2:]
    assert at == tuple(map(float, start))
    return np.array(rows, np.float32)


def circle16(cx=14.0, cy=12.0, r=8.0):
    """a circle of 16 quadratics: no corner, every edge white"""
    rows = []
    for k in range(16):
        a0, a1 = k * np.pi / 8, (k + 1) * np.pi / 8
        am, rc = (a0 + a1) / 2, r / np.cos(np.pi / 16)
        rows.append([cx + r * np.cos(a0), cy + r * np.sin(a0), cx + rc * np.cos(am), cy + rc * np.sin(am), cx + r * np.cos(a1), cy + r * np.sin(a1)])
    rows = np.array(rows, np.float32)
    for k in range(16):
        rows[k, 0:2] = rows[k - 1, 4:6]
    return rows


def random_contour(rng):
    """3 to 8 vertices in a 40 x 32 image, coordinates rounded to 0.01; each side a line with probability 0.4, otherwise a quadratic with
    its control point uniform in the image grown by 5; R from 1, 2, 4, 8.  -> (segs, R)"""
    m = int(rng.randint(3, 9))
    v = np.round(np.stack([rng.uniform(0, 40, m), rng.uniform(0, 32, m)], 1), 2)
    rows = []
    for i in range(m):
        a, b = v[i], v[(i + 1) % m]
        if rng.uniform() < 0.4:
            rows.append([a[0], a[1], NAN, NAN, b[0], b[1]])
        else:
            rows.append([a[0], a[1], round(rng.uniform(-5, 45), 2), round(rng.uniform(-5, 37), 2), b[0], b[1]])
    return np.array(rows, np.float32), int(rng.choice([1, 2, 4, 8]))


def hostile_inputs():
    """What an application can pass and a font tool never does -> [(name, segs float32 (n, 6), w, h, R, simple)]; `simple`: the outline does
    not cross itself, so check_sign's winding test applies.  Every image stays at or below about 320 x 320: each goes through the float64
    reference."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "outlines_ubuntu20.npz"))
    out = []

    def add(name, segs, w, h, R, simple=True):
        out.append((name, np.ascontiguousarray(segs, np.float32).reshape(-1, 6), int(w), int(h), int(R), bool(simple)))

    def glyph(ch, scale, R, move=0):
        segs, (w, h) = z[f"segs_{ord(ch)}"].astype(np.float32), z[f"size_{ord(ch)}"]
        add(f"{ch} x{scale} R={R}" + (f" moved by {move}" if move else ""), segs * np.float32(scale) + np.float32(R + move),
            scale * int(w) + 2 * R + move, scale * int(h) + 2 * R + move, R)

    # a control point on an end point: the tangent there is the chord's (step 3 of the specification)
    add("control point on P2", path((4, 4), (28, 6), (28, 20, 28, 20), (4, 20), (4, 4)), 32, 24, 4)
    add("control point on P0", path((4, 4), (28, 6), (28, 6, 28, 20), (4, 20), (4, 4)), 32, 24, 4)
    for off in (1e-5, 1e-3):  # beside the end point, off the line: still quadratics, and the curve all but halts at that end
        add(f"control point {off} from P2", path((4, 4), (28, 6), (28 + off, 20 - off, 28, 20), (4, 20), (4, 4)), 32, 24, 4)
        add(f"control point {off} from P0", path((4, 4), (28, 6), (28 + off, 6 + off, 28, 20), (4, 20), (4, 4)), 32, 24, 4)
    # collinear control points: folded past P2 to x = 31 at t = 0.75 (step 1: the line P0 P2); inside the chord away from its middle (kept)
    add("quadratic folded onto its line", path((4, 4), (40, 4, 28, 4), (28, 20), (4, 20), (4, 4)), 44, 24, 4)
    add("collinear control point inside the chord", path((4, 4), (22, 4, 28, 4), (28, 20), (4, 20), (4, 4)), 32, 24, 4)
    # A single edge out to (23, 12.25) and back on its own line: P0 = P2, the control point beyond both: step 1 leaves no edge at all.
    # (Before step 1 said so, nothing could be held to 1 LSB here: the float32 reference left the float64 one on 65 texels.)
    add("one edge doubling back on itself", np.array([[6, 12, 40, 12.5, 6, 12]], np.float32), 44, 24, 4)
    for off in (0.001, 0.01, 0.1):  # |b|^2 = 4 off^2 and more: still quadratics, the cubic's coefficients up to 1e5
        add(f"control point {off} off the chord", path((4, 4), (19, 4 - off, 28, 4), (28, 20), (4, 20), (4, 4)), 32, 24, 4)
    add("spike 0.05 wide", poly([(4, 8), (15.975, 8), (16, 2), (16.025, 8), (28, 8), (28, 20), (4, 20)]), 32, 24, 4)
    add("sliver triangle 0.04 high", poly([(4, 10), (30, 10.02), (4, 10.04)]), 34, 20, 4)
    add("sharp U-turn", path((6, 8), (50, 8.5, 6, 9), (6, 8)), 36, 17, 4)
    add("two overlapping squares", np.concatenate([poly([(4, 4), (16, 4), (16, 16), (4, 16)]), poly([(10, 10), (24, 10), (24, 22), (10, 22)])]), 28, 26, 4, False)
    add("a square twice", np.tile(poly([(4.5, 4.25), (16, 4.25), (16, 15.75), (4.5, 15.75)]), (2, 1)), 21, 20, 4)
    add("two squares touching in a vertex", np.concatenate([poly([(4, 4), (14, 4), (14, 14), (4, 14)]), poly([(14, 14), (24, 14), (24, 22), (14, 22)])]), 28, 26, 4)
    add("sub-texel square", poly([(5.2, 5.3), (5.6, 5.3), (5.6, 5.7), (5.2, 5.7)]), 11, 11, 4)
    add("720-gon", poly([(32 + 27.5 * math.cos(k * math.pi / 360), 31 + 26.5 * math.sin(k * math.pi / 360)) for k in range(720)]), 64, 62, 4)
    add("outside the image on three sides", poly([(-5, -4), (30, -6), (28, 14), (-3, 12)]), 24, 20, 4)
    add("9 x 1 image", poly([(1, -3), (8, 0.5), (2, 4)]), 9, 1, 2)
    add("lens", np.array([[4, 12, 14, 0, 24, 12], [24, 12, 14, 24, 4, 12]], np.float32), 28, 24, 4)
    add("teardrop", np.array([[14, 20, 2, 20, 14, 4], [14, 4, 26, 20, 14, 20]], np.float32), 28, 24, 4)
    add("circle of 16 quadratics", circle16(), 28, 24, 4)
    glyph("g", 8, 8)     # 120 x 168
    glyph("&", 16, 16)   # 288 x 320
    glyph("R", 2, 1)
    glyph("8", 2, 64)
    glyph("@", 12, 4)    # 248 x 260
    glyph("a", 2, 4, move=224)  # coordinates up to 250 in 256 x 262
    rng = np.random.RandomState(20251017)
    for k in range(40):
        segs, R = random_contour(rng)
        add(f"random contour {k}", segs, 40, 32, R, False)
    return out


def over_tolerance(got, want):
    """the texels of an image that differ from the reference by more than 1 LSB in some channel"""
    return int((np.abs(got.astype(int) - want.astype(int)).max(axis=2) > 1).sum())


def flatten(segs, chords=64):
    """-> (m, 4) float64 lines"""
    lines = []
    for x0, y0, cx, cy, x1, y1 in np.asarray(segs, np.float32).astype(np.float64).reshape(-1, 6):
        if math.isnan(cx):
            lines.append((x0, y0, x1, y1))
            continue
        t = np.linspace(0.0, 1.0, chords + 1)
        xs = (1 - t) ** 2 * x0 + 2 * (1 - t) * t * cx + t * t * x1
        ys = (1 - t) ** 2 * y0 + 2 * (1 - t) * t * cy + t * t * y1
        xs[0], ys[0], xs[-1], ys[-1] = x0, y0, x1, y1
        lines += list(zip(xs[:-1], ys[:-1], xs[1:], ys[1:]))
    return np.array(lines, np.float64).reshape(-1, 4)


def winding(segs, w, h):
    """the winding number of the flattened outline about every texel centre, (h, w) int"""
    L = flatten(segs)
    ys, xs = np.mgrid[0:h, 0:w]
    px, py = xs + 0.5, ys + 0.5
    wn = np.zeros((h, w), int)
    for x0, y0, x1, y1 in L:
        if y0 == y1:
            continue
        up = (y0 <= py) & (py < y1)
        down = (y1 <= py) & (py < y0)
        side = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)
        wn += (up & (side > 0)).astype(int) - (down & (side < 0)).astype(int)
    return wn


def median3(img):
    r, g, b = (img[..., k].astype(int) for k in range(3))
    return np.maximum(np.minimum(r, g), np.minimum(np.maximum(r, g), b))


def check_sign(name, img, segs, w, h, R, true=None, inside=None):
    """For every texel whose true distance exceeds one quantisation step: median(R, G, B) > 127.5 iff alpha > 127.5 iff the texel
    centre is inside by non-zero winding.  `true`, `inside`: the reference's true distances and winding(...) != 0 where the caller has
    them already.  -> the number of texels checked"""
    if true is None:
        true = M.distances(M.build_shape(segs), w, h)[..., 3]
    far = np.abs(true) > R / 255.0
    if inside is None:
        inside = winding(segs, w, h) != 0
    a_in, m_in = img[..., 3] > 127.5, median3(img) > 127.5
    assert np.array_equal(a_in[far], inside[far]), f"{name}: alpha's sign against the winding test at {np.argwhere(far & (a_in != inside))[:4].tolist()}"
    assert np.array_equal(m_in[far], inside[far]), f"{name}: the median's sign against the winding test at {np.argwhere(far & (m_in != inside))[:4].tolist()}"
    return int(far.sum())


def reconstruction_error(orc, rasterize_outline, key, segs, w, h, scale):
    """|alpha drawn from the field at `scale` - box coverage of the outline scaled likewise| per pixel, in LSB.  The field is image `key` of
    the oracle `orc`; white on black, so the red channel of the frame is the alpha the draw produced."""
    W, H = int(round(w * scale)), int(round(h * scale))
    orc.begin_frame(W, H, True, (0.0, 0.0, 0.0, 1.0))
    orc.draw_msdf(key, (0.0, 0.0), (255, 255, 255, 255), (float(W), float(H)), 4.0, 0.5, 0.0, False, False)
    orc.end_frame()
    got = orc.read_pixels()[..., 0].astype(int)
    want = rasterize_outline((np.asarray(segs, np.float32) * np.float32(scale)).astype(np.float32), W, H)[..., 0].astype(int)
    return np.abs(got - want).ravel()
