"""What the distance-field tests share (test_msdf_host.py on a CPU, test_msdf.py on the device): the inputs, the tolerance, the winding
test and the reconstruction statistics.  Inputs: the 94 outlines of tests/golden/outlines_ubuntu20.npz scaled by 2 about the origin
and moved by R = 4 texels into an image of (2 w + 2 R) x (2 h + 2 R), and a dozen of them at scale 1 with R = 2."""
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


def check_sign(name, img, segs, w, h, R):
    """For every texel whose true distance exceeds one quantisation step: median(R, G, B) > 127.5 iff alpha > 127.5 iff the texel
    centre is inside by non-zero winding.  -> the number of texels checked"""
    true = M.distances(M.build_shape(segs), w, h)[..., 3]
    far = np.abs(true) > R / 255.0
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
