"""The independent reference of distance-field generation (fdh_put_glyph_outline with FDH_GLYPH_MTSDF), written from the specification
in include/figdraw_hip.h -- the comment at FDH_GLYPH_MTSDF -- in numpy float64.  It reads and calls no library code; the tests hold the
kernel's source under a host shim (test_msdf_host.py) and the compiled kernel (test_msdf.py) to it.  Same role as tilecode_ref.py.

    shape = build_shape(segs)            # steps 1 to 3: contours, orientation, coloured edges
    img = generate(segs, w, h, R)        # step 4: (h, w, 4) uint8

`dtype=np.float32` runs step 4 in single precision: what a float32 implementation of the same formulas can and cannot reproduce
(the tests measure the reference against itself before they hold anything else to it)."""
import math

import numpy as np

RED, GREEN, BLUE, YELLOW, MAGENTA, CYAN, WHITE = 1, 2, 4, 3, 5, 6, 7
CYCLE = (MAGENTA, YELLOW, CYAN)
SIN3 = math.sin(3.0)


class OpenContour(ValueError):
    pass


class Edge:
    """p: three points as float32 values held in float64 (a line: p[1] = p[0]); line; colour"""

    def __init__(self, p, line, colour=0):
        self.p = np.asarray(p, np.float64).reshape(3, 2)
        self.line = bool(line)
        self.colour = colour

    def tangents(self):
        """the directions at t = 0 and t = 1 (a control point on an end leaves the chord)"""
        chord = self.p[2] - self.p[0]
        t0, t1 = chord, chord
        if not self.line:
            a, b = self.p[1] - self.p[0], self.p[2] - self.p[1]
            if a[0] != 0.0 or a[1] != 0.0:
                t0 = a
            if b[0] != 0.0 or b[1] != 0.0:
                t1 = b
        return t0, t1


def _unit(v):
    l = math.sqrt(v[0] * v[0] + v[1] * v[1])
    return (v[0] / l, v[1] / l) if l > 0.0 else (0.0, 0.0)


def _lerp(a, b, t):
    return a + (b - a) * t


def _f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


def _point_at(e, t):
    if e.line:
        return _f32(_lerp(e.p[0], e.p[2], t))
    return _f32(_lerp(_lerp(e.p[0], e.p[1], t), _lerp(e.p[1], e.p[2], t), t))


def _third(e, k):
    t0, t1 = k / 3.0, (k + 1) / 3.0
    p0 = e.p[0] if k == 0 else _point_at(e, t0)
    p2 = e.p[2] if k == 2 else _point_at(e, t1)
    p1 = p0 if e.line else _f32(_lerp(_lerp(e.p[0], e.p[1], t0), _lerp(e.p[1], e.p[2], t0), t1))
    return Edge([p0, p1, p2], e.line)


def _colour_contour(c):
    m = len(c)
    corners = []
    for i in range(m):
        tin = _unit(c[(i - 1) % m].tangents()[1])
        tout = _unit(c[i].tangents()[0])
        dot = tin[0] * tout[0] + tin[1] * tout[1]
        cross = tin[0] * tout[1] - tin[1] * tout[0]
        if dot <= 0.0 or abs(cross) > SIN3:
            corners.append(i)
    n = len(corners)
    if n == 0:
        for e in c:
            e.colour = WHITE
        return c
    if n == 1:
        r = []
        for j in range(m):
            e = c[(corners[0] + j) % m]
            r += [e] if m >= 3 else [_third(e, k) for k in range(3)]
        for j, e in enumerate(r):
            e.colour = CYCLE[3 * j // len(r)]
        return r
    run = -1
    for j in range(m):
        i = (corners[0] + j) % m
        if i in corners:
            run += 1
        c[i].colour = YELLOW if (run == n - 1 and n % 3 == 1) else CYCLE[run % 3]
    return c


class Shape:
    def __init__(self):
        self.edges, self.contour, self.orient = [], [], 1.0

    def colours(self):
        return [e.colour for e in self.edges]


def build_shape(segs):
    """steps 1 to 3 of the specification; OpenContour when a contour does not close"""
    segs = np.asarray(segs, np.float32).reshape(-1, 6).astype(np.float64)
    s = Shape()
    cur, area, nc = [], 0.0, 0
    for q in segs:
        line = bool(np.isnan(q[2]))
        p0, p2 = q[0:2], q[4:6]
        p1 = p0 if line else q[2:4]
        if not line:
            b = p0 - 2.0 * p1 + p2
            a, c, e = p1 - p0, p2 - p0, p2 - p1
            folded = a[0] * c[1] == a[1] * c[0] and not (a[0] * e[0] > 0.0 or a[1] * e[1] > 0.0)
            if b[0] * b[0] + b[1] * b[1] <= 1e-6 or folded:
                line, p1 = True, p0
        if line and p0[0] == p2[0] and p0[1] == p2[1]:
            continue
        if cur and (cur[-1].p[2][0] != p0[0] or cur[-1].p[2][1] != p0[1]):
            raise OpenContour("a segment does not start where the one before it ended")
        cur.append(Edge([p0, p1, p2], line))
        area += 0.5 * (p0[0] * p2[1] - p2[0] * p0[1])
        if not line:
            area += ((p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0])) / 3.0
        if p2[0] == cur[0].p[0][0] and p2[1] == cur[0].p[0][1]:
            for e in _colour_contour(cur):
                s.edges.append(e)
                s.contour.append(nc)
            nc += 1
            cur = []
    if cur:
        raise OpenContour("the last contour does not close")
    s.orient = 1.0 if area >= 0.0 else -1.0
    return s


def _cbrt(x):
    return np.sign(x) * np.abs(x) ** (x.dtype.type(1) / x.dtype.type(3))


def _nearest_on_quadratic(P, px, py, dt):
    """-> t in [0, 1] per texel: the candidates are the ends and every stationary point of the squared distance inside (0, 1)"""
    P0, P1, P2 = (P[k].astype(dt) for k in range(3))
    a, b = P1 - P0, P0 - dt(2) * P1 + P2
    dx, dy = P0[0] - px, P0[1] - py

    def E(t):
        return dx + (dt(2) * a[0] + b[0] * t) * t, dy + (dt(2) * a[1] + b[1] * t) * t

    # |E|^2 ' / 4 = c3 t^3 + c2 t^2 + c1 t + c0
    c3 = b[0] * b[0] + b[1] * b[1]
    c2 = dt(3) * (a[0] * b[0] + a[1] * b[1])
    c1 = dt(2) * (a[0] * a[0] + a[1] * a[1]) + (dx * b[0] + dy * b[1])
    c0 = dx * a[0] + dy * a[1]
    sh = c2 / (dt(3) * c3)
    p = c1 / c3 - dt(3) * sh * sh               # y^3 + p y + q, t = y - sh
    q = dt(2) * sh * sh * sh - sh * c1 / c3 + c0 / c3
    disc = q * q / dt(4) + p * p * p / dt(27)
    roots = []
    with np.errstate(all="ignore"):
        sq = np.sqrt(np.maximum(disc, 0))
        one = _cbrt(-q / dt(2) + sq) + _cbrt(-q / dt(2) - sq) - sh
        m = dt(2) * np.sqrt(np.maximum(-p / dt(3), 0))
        arg = np.clip(dt(3) * q / (p * m), -1, 1)
        arg = np.where(np.isfinite(arg), arg, 0)
        th = np.arccos(arg) / dt(3)
        for k in range(3):
            tri = m * np.cos(th - dt(2.0 * math.pi * k / 3.0)) - sh
            roots.append(np.where(disc >= 0, one, tri))
    best_t = np.zeros_like(px)
    ex, ey = E(best_t)
    best_d2 = ex * ex + ey * ey
    e1x, e1y = P2[0] - px, P2[1] - py
    d1 = e1x * e1x + e1y * e1y
    upd = d1 < best_d2
    best_t = np.where(upd, dt(1), best_t)
    best_d2 = np.where(upd, d1, best_d2)
    for t in roots:
        with np.errstate(all="ignore"):
            for _ in range(3):  # Newton on g = E . T: the closed form cancels where one root is real
                ex, ey = E(t)
                tx, ty = a[0] + b[0] * t, a[1] + b[1] * t
                g = ex * tx + ey * ty
                gp = dt(2) * (tx * tx + ty * ty) + (ex * b[0] + ey * b[1])
                t = np.where(gp > 0, t - g / np.where(gp > 0, gp, 1), t)
            inside = (t > 0) & (t < 1)
            ex, ey = E(t)
            d2 = ex * ex + ey * ey
        upd = inside & (d2 < best_d2)
        best_t = np.where(upd, t, best_t)
        best_d2 = np.where(upd, d2, best_d2)
    return best_t


def _at(P, line, t, px, py, dt):
    """E = B(t) - p (the stored end at t = 0, 1) and the tangent direction at t"""
    P0, P1, P2 = (P[k].astype(dt) for k in range(3))
    if line:
        e = P2 - P0
        ex, ey = (P0[0] - px) + e[0] * t, (P0[1] - py) + e[1] * t
        tx, ty = np.full_like(px, e[0]), np.full_like(px, e[1])
    else:
        a, b = P1 - P0, P0 - dt(2) * P1 + P2
        ex, ey = (P0[0] - px) + (dt(2) * a[0] + b[0] * t) * t, (P0[1] - py) + (dt(2) * a[1] + b[1] * t) * t
        tx, ty = a[0] + b[0] * t, a[1] + b[1] * t
    ex = np.where(t <= 0, P0[0] - px, np.where(t >= 1, P2[0] - px, ex))
    ey = np.where(t <= 0, P0[1] - py, np.where(t >= 1, P2[1] - py, ey))
    return ex, ey, tx, ty


def distances(shape, w, h, dtype=np.float64):
    """step 4 before the encoding: (h, w, 4) signed distances in texels, positive inside; R, G, B pseudo-distances, A the true one"""
    dt = np.dtype(dtype).type
    ys, xs = np.mgrid[0:h, 0:w]
    px, py = (xs.ravel() + 0.5).astype(dt), (ys.ravel() + 0.5).astype(dt)
    n = px.size
    out = np.full((n, 4), -np.inf, dt)
    if not shape.edges:
        return out.reshape(h, w, 4)
    bd2 = np.full((4, n), np.inf, dt)
    bo = np.full((4, n), -1.0, dt)
    bt = np.zeros((4, n), dt)
    be = np.full((4, n), -1, np.int64)
    for i, e in enumerate(shape.edges):
        if e.line:
            P0, P2 = e.p[0].astype(dt), e.p[2].astype(dt)
            d = P2 - P0
            t = np.clip(((px - P0[0]) * d[0] + (py - P0[1]) * d[1]) / (d[0] * d[0] + d[1] * d[1]), 0, 1)
        else:
            t = _nearest_on_quadratic(e.p, px, py, dt)
        ex, ey, tx, ty = _at(e.p, e.line, t, px, py, dt)
        d2 = ex * ex + ey * ey
        den = (tx * tx + ty * ty) * d2
        with np.errstate(all="ignore"):
            ortho = np.where(den > 0, np.abs(tx * ey - ty * ex) / np.sqrt(np.where(den > 0, den, 1)), 0)
        for c in range(4):
            if c < 3 and not (e.colour >> c) & 1:
                continue
            better = (d2 < bd2[c]) | ((d2 == bd2[c]) & (ortho > bo[c]))
            bd2[c] = np.where(better, d2, bd2[c])
            bo[c] = np.where(better, ortho, bo[c])
            bt[c] = np.where(better, t, bt[c])
            be[c] = np.where(better, i, be[c])
    for c in range(4):
        d = np.full(n, -np.inf, dt)
        for i, e in enumerate(shape.edges):
            sel = be[c] == i
            if not sel.any():
                continue
            t = bt[c][sel]
            qx, qy = px[sel], py[sel]
            ex, ey, tx, ty = _at(e.p, e.line, t, qx, qy, dt)
            cr = ty * ex - tx * ey  # cross(T, p - N)
            di = np.sqrt(bd2[c][sel])
            di = np.where(cr >= 0, di, -di)
            if c < 3:
                t0, t1 = e.tangents()
                u0, u1 = _unit(t0), _unit(t1)
                for at_end, u in ((t <= 0, u0), (t >= 1, u1)):
                    pd = dt(u[1]) * ex - dt(u[0]) * ey
                    di = np.where(at_end & (np.abs(pd) <= np.abs(di)), pd, di)
            d[sel] = di * dt(shape.orient)
        out[:, c] = d
    return out.reshape(h, w, 4)


def encode(d, R):
    with np.errstate(all="ignore"):
        v = np.clip(0.5 + d.astype(np.float64) / float(R), 0.0, 1.0) if d.dtype == np.float64 else np.clip(np.float32(0.5) + d / np.float32(R), 0, 1)
    return np.floor(255 * v + 0.5).astype(np.uint8)


def decode(img, R):
    """texel values -> distances in texels (the centre of each quantisation step)"""
    return (img.astype(np.float64) / 255.0 - 0.5) * float(R)


def generate(segs, w, h, R=4, dtype=np.float64):
    return encode(distances(build_shape(segs), w, h, dtype), R or 4)
