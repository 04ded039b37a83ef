"""The independent reference of distance fields from outlines with cubic segments (fdh_put_glyph_outline_cubic with FDH_GLYPH_MTSDF),
written from the specification in include_glyphs/figdraw_hip_cubic.h in numpy float64.  What that specification leaves as it is comes from
msdf_ref (the encoding, the distance to a line and to a quadratic) and msdf_correct_ref (candidates, crossing_points); the cubic rules are
implemented here, and not the way the device does it: the nearest point of a cubic comes from ALL roots of the quintic
(B(t) - p) . B'(t) -- the eigenvalues of its companion matrix, each polished by Newton in float64 -- plus the two ends.

    shape = build_shape(segs8)             # steps 1 to 3
    img = generate(segs8, w, h, R)         # step 4: (h, w, 4) uint8
    G, marked, artefacts = correct(F, segs8, R)   # step 5

`dtype=np.float32` evaluates the distances in single precision at the float64 roots."""
import math

import numpy as np

import msdf_correct_ref as CR
import msdf_ref as M

LINE, QUADRATIC, CUBIC = 0, 1, 2
OpenContour = M.OpenContour


class Edge:
    """p: four points as float32 values held in float64 (a quadratic: P0, C, C, P3; a line: P0, P0, P0, P3); kind; colour"""

    def __init__(self, p, kind, colour=0):
        self.p = np.asarray(p, np.float64).reshape(4, 2)
        self.kind = kind
        self.colour = colour

    @property
    def line(self):
        return self.kind == LINE

    def p3(self):
        """the three points msdf_ref works on"""
        return self.p[[0, 1, 3]]

    def tangents(self):
        P = self.p
        t0 = t1 = P[3] - P[0]
        if self.kind != LINE:
            for j in (2, 1):
                a = P[j] - P[0]
                if a[0] != 0.0 or a[1] != 0.0:
                    t0 = a
            for j in (1, 2):
                b = P[3] - P[j]
                if b[0] != 0.0 or b[1] != 0.0:
                    t1 = b
        return t0, t1


def _blossom(e, r, s, u):
    P = e.p
    L = M._lerp
    if e.kind == LINE:
        return L(P[0], P[3], u)
    if e.kind == QUADRATIC:
        return L(L(P[0], P[1], s), L(P[1], P[3], s), u)
    q0, q1, q2 = L(P[0], P[1], r), L(P[1], P[2], r), L(P[2], P[3], r)
    return L(L(q0, q1, s), L(q1, q2, s), u)


def _third(e, k):
    t0, t1 = k / 3.0, (k + 1) / 3.0
    p0 = e.p[0] if k == 0 else M._f32(_blossom(e, t0, t0, t0))
    p3 = e.p[3] if k == 2 else M._f32(_blossom(e, t1, t1, t1))
    if e.kind == LINE:
        c1 = c2 = p0
    elif e.kind == QUADRATIC:
        c1 = c2 = M._f32(_blossom(e, t0, t0, t1))
    else:
        c1, c2 = M._f32(_blossom(e, t0, t0, t1)), M._f32(_blossom(e, t0, t1, t1))
    return Edge([p0, c1, c2, p3], e.kind)


def _colour_contour(c):
    m = len(c)
    corners = []
    for i in range(m):
        tin, tout = M._unit(c[(i - 1) % m].tangents()[1]), M._unit(c[i].tangents()[0])
        dot, cross = tin[0] * tout[0] + tin[1] * tout[1], tin[0] * tout[1] - tin[1] * tout[0]
        if dot <= 0.0 or abs(cross) > M.SIN3:
            corners.append(i)
    n = len(corners)
    if n == 0:
        for e in c:
            e.colour = M.WHITE
        return c
    if n == 1:
        r = []
        for j in range(m):
            e = c[(corners[0] + j) % m]
            r += [e] if m >= 3 else [_third(e, k) for k in range(3)]
        for j, e in enumerate(r):
            e.colour = M.CYCLE[3 * j // len(r)]
        return r
    run = -1
    for j in range(m):
        i = (corners[0] + j) % m
        if i in corners:
            run += 1
        c[i].colour = M.YELLOW if (run == n - 1 and n % 3 == 1) else M.CYCLE[run % 3]
    return c


def _quadratic_or_line(p0, c, p3):
    b = p0 - 2.0 * c + p3
    a, w, e = c - p0, p3 - p0, p3 - c
    folded = a[0] * w[1] == a[1] * w[0] and not (a[0] * e[0] > 0.0 or a[1] * e[1] > 0.0)
    if b[0] * b[0] + b[1] * b[1] <= 1e-6 or folded:
        return Edge([p0, p0, p0, p3], LINE)
    return Edge([p0, c, c, p3], QUADRATIC)


def holds_cubic(segs):
    segs = np.asarray(segs, np.float32).reshape(-1, 8)
    return bool((~np.isnan(segs[:, 2]) & ~np.isnan(segs[:, 4])).any())


def to_quadratic_format(segs):
    """a cubic-free outline in fdh_put_glyph_outline's 6-float format"""
    return np.ascontiguousarray(np.asarray(segs, np.float32).reshape(-1, 8)[:, [0, 1, 2, 3, 6, 7]])


def edge_area(e):
    """step 2: 1/2 of the integral of x dy - y dx along the edge"""
    P = e.p
    area = 0.5 * (P[0][0] * P[3][1] - P[3][0] * P[0][1])
    u, v, w = P[1] - P[0], P[2] - P[0], P[3] - P[0]
    cr = lambda a, b: a[0] * b[1] - a[1] * b[0]
    if e.kind == QUADRATIC:
        area += cr(u, w) / 3.0
    elif e.kind == CUBIC:
        area += (3.0 * cr(u, v) + 3.0 * cr(u, w) + 6.0 * cr(v, w)) / 20.0
    return area


def build_shape(segs):
    """steps 1 to 3 with the cubic rules; OpenContour when a contour does not close"""
    segs = np.asarray(segs, np.float32).reshape(-1, 8).astype(np.float64)
    s = M.Shape()
    cur, area, nc = [], 0.0, 0
    for q in segs:
        p0, p1, p2, p3 = q[0:2], q[2:4], q[4:6], q[6:8]
        if np.isnan(q[2]):
            e = Edge([p0, p0, p0, p3], LINE)
        elif np.isnan(q[4]):
            e = _quadratic_or_line(p0, p1, p3)
        else:
            if (p1 == p0).all() and (p2 == p0).all() and (p3 == p0).all():
                continue
            d = p3 - 3.0 * p2 + 3.0 * p1 - p0
            if d[0] * d[0] + d[1] * d[1] <= 1e-6:
                e = _quadratic_or_line(p0, M._f32((3.0 * (p1 + p2) - (p0 + p3)) / 4.0), p3)
            else:
                u, v, w = p1 - p0, p2 - p0, p3 - p0
                if w[0] == 0.0 and w[1] == 0.0:
                    on_line = u[0] * v[1] == u[1] * v[0]
                else:
                    on_line = u[0] * w[1] == u[1] * w[0] and v[0] * w[1] == v[1] * w[0]
                e = Edge([p0, p0, p0, p3], LINE) if on_line else Edge([p0, p1, p2, p3], CUBIC)
        if e.kind == LINE and e.p[0][0] == e.p[3][0] and e.p[0][1] == e.p[3][1]:
            continue
        if cur and (cur[-1].p[3][0] != e.p[0][0] or cur[-1].p[3][1] != e.p[0][1]):
            raise OpenContour("a segment does not start where the one before it ended")
        cur.append(e)
        area += edge_area(e)
        if e.p[3][0] == cur[0].p[0][0] and e.p[3][1] == cur[0].p[0][1]:
            for c in _colour_contour(cur):
                s.edges.append(c)
                s.contour.append(nc)
            nc += 1
            cur = []
    if cur:
        raise OpenContour("the last contour does not close")
    s.orient = 1.0 if area >= 0.0 else -1.0
    return s


def _power_basis(P):
    c1 = 3.0 * (P[1] - P[0])
    c2 = 3.0 * (P[0] - 2.0 * P[1] + P[2])
    c3 = P[3] - 3.0 * P[2] + 3.0 * P[1] - P[0]
    return c1, c2, c3


def cubic_roots(P, px, py):
    """every candidate parameter of the nearest point of the cubic P to the points (px, py), float64 -> (n, 5): the real parts of the five
    roots of the quintic g(t) = (B(t) - p) . B'(t), each polished by Newton on g (a polished non-real root is just one more parameter)"""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    c1, c2, c3 = _power_basis(P)
    dx, dy = P[0][0] - px, P[0][1] - py
    n = px.size
    g = np.zeros((n, 6))  # ascending powers
    for k in range(2):
        d = dx if k == 0 else dy
        e = [None, c1[k], c2[k], c3[k]]           # E = d + e1 t + e2 t^2 + e3 t^3
        b = [c1[k], 2.0 * c2[k], 3.0 * c3[k]]     # B'
        for j in range(3):
            g[:, j] += d * b[j]
            for i in range(1, 4):
                g[:, i + j] += e[i] * b[j]
    comp = np.zeros((n, 5, 5))
    comp[:, np.arange(1, 5), np.arange(0, 4)] = 1.0
    comp[:, :, 4] = -g[:, :5] / g[:, 5:6]
    t = np.linalg.eigvals(comp).real
    dxc, dyc = dx[:, None], dy[:, None]
    with np.errstate(all="ignore"):
        for _ in range(4):
            ex = dxc + ((c3[0] * t + c2[0]) * t + c1[0]) * t
            ey = dyc + ((c3[1] * t + c2[1]) * t + c1[1]) * t
            tx = (3.0 * c3[0] * t + 2.0 * c2[0]) * t + c1[0]
            ty = (3.0 * c3[1] * t + 2.0 * c2[1]) * t + c1[1]
            bx, by = 6.0 * c3[0] * t + 2.0 * c2[0], 6.0 * c3[1] * t + 2.0 * c2[1]
            gv, gp = ex * tx + ey * ty, tx * tx + ty * ty + ex * bx + ey * by
            tn = t - gv / np.where(gp != 0, gp, 1)
            t = np.where((gp != 0) & np.isfinite(tn), tn, t)
    return t


def _cubic_E(P, t, px, py, dt):
    c1, c2, c3 = (c.astype(dt) for c in _power_basis(P))
    P0 = P[0].astype(dt)
    ex = (P0[0] - px) + ((c3[0] * t + c2[0]) * t + c1[0]) * t
    ey = (P0[1] - py) + ((c3[1] * t + c2[1]) * t + c1[1]) * t
    return ex, ey


def nearest_on_cubic(P, px, py, dt):
    """-> t in [0, 1] per point: the ends, and every root inside (0, 1) that is strictly nearer"""
    roots = cubic_roots(P, px, py)
    tpx, tpy = px.astype(dt), py.astype(dt)
    P0, P3 = P[0].astype(dt), P[3].astype(dt)
    best_t = np.zeros(px.size, dt)
    best_d2 = (P0[0] - tpx) ** 2 + (P0[1] - tpy) ** 2
    d1 = (P3[0] - tpx) ** 2 + (P3[1] - tpy) ** 2
    upd = d1 < best_d2
    best_t, best_d2 = np.where(upd, dt(1), best_t), np.where(upd, d1, best_d2)
    for k in range(roots.shape[1]):
        with np.errstate(all="ignore"):  # (a root far outside [0, 1] may overflow float32; it is no candidate)
            t = roots[:, k].astype(dt)
            ex, ey = _cubic_E(P, t, tpx, tpy, dt)
            d2 = ex * ex + ey * ey
        upd = (t > 0) & (t < 1) & (d2 < best_d2)
        best_t, best_d2 = np.where(upd, t, best_t), np.where(upd, d2, best_d2)
    return best_t


def _at(e, t, px, py, dt):
    """E = B(t) - p (the stored end at t = 0, 1) and the tangent at t (step 3's at the ends of a cubic)"""
    if e.kind != CUBIC:
        return M._at(e.p3(), e.kind == LINE, t, px, py, dt)
    P = e.p
    c1, c2, c3 = (c.astype(dt) for c in _power_basis(P))
    ex, ey = _cubic_E(P, t, px, py, dt)
    tx = (dt(3) * c3[0] * t + dt(2) * c2[0]) * t + c1[0]
    ty = (dt(3) * c3[1] * t + dt(2) * c2[1]) * t + c1[1]
    u0, u1 = (M._unit(v) for v in e.tangents())
    P0, P3 = P[0].astype(dt), P[3].astype(dt)
    ex = np.where(t <= 0, P0[0] - px, np.where(t >= 1, P3[0] - px, ex))
    ey = np.where(t <= 0, P0[1] - py, np.where(t >= 1, P3[1] - py, ey))
    tx = np.where(t <= 0, dt(u0[0]), np.where(t >= 1, dt(u1[0]), tx))
    ty = np.where(t <= 0, dt(u0[1]), np.where(t >= 1, dt(u1[1]), ty))
    return ex, ey, tx, ty


def _nearest(e, px, py, dt):
    if e.kind == LINE:
        P0, P3 = e.p[0].astype(dt), e.p[3].astype(dt)
        d = P3 - P0
        return np.clip(((px - P0[0]) * d[0] + (py - P0[1]) * d[1]) / (d[0] * d[0] + d[1] * d[1]), 0, 1)
    if e.kind == QUADRATIC:
        return M._nearest_on_quadratic(e.p3(), px, py, dt)
    return nearest_on_cubic(e.p, px, py, dt)


def _offer(e, px, py, dt):
    t = _nearest(e, px, py, dt)
    ex, ey, tx, ty = _at(e, t, px, py, dt)
    d2 = ex * ex + ey * ey
    den = (tx * tx + ty * ty) * d2
    with np.errstate(all="ignore"):
        ortho = np.where(den > 0, np.abs(tx * ey - ty * ex) / np.sqrt(np.where(den > 0, den, 1)), 0)
    return t, d2, ortho, ty * ex - tx * ey


def distances(shape, w, h, dtype=np.float64):
    """step 4 before the encoding: (h, w, 4) signed distances in texels, positive inside"""
    dt = np.dtype(dtype).type
    ys, xs = np.mgrid[0:h, 0:w]
    px, py = (xs.ravel() + 0.5).astype(dt), (ys.ravel() + 0.5).astype(dt)
    n = px.size
    out = np.full((n, 4), -np.inf, dt)
    if not shape.edges:
        return out.reshape(h, w, 4)
    bd2, bo = np.full((4, n), np.inf, dt), np.full((4, n), -1.0, dt)
    bt, be = np.zeros((4, n), dt), np.full((4, n), -1, np.int64)
    for i, e in enumerate(shape.edges):
        t, d2, ortho, _ = _offer(e, px, py, dt)
        for c in range(4):
            if c < 3 and not (e.colour >> c) & 1:
                continue
            better = (d2 < bd2[c]) | ((d2 == bd2[c]) & (ortho > bo[c]))
            bd2[c], bo[c] = np.where(better, d2, bd2[c]), np.where(better, ortho, bo[c])
            bt[c], be[c] = np.where(better, t, bt[c]), np.where(better, i, be[c])
    for c in range(4):
        d = np.full(n, -np.inf, dt)
        for i, e in enumerate(shape.edges):
            sel = be[c] == i
            if not sel.any():
                continue
            t = bt[c][sel]
            ex, ey, tx, ty = _at(e, t, px[sel], py[sel], dt)
            cr = ty * ex - tx * ey
            di = np.sqrt(bd2[c][sel])
            di = np.where(cr >= 0, di, -di)
            if c < 3:
                u0, u1 = (M._unit(v) for v in e.tangents())
                for at_end, u in ((t <= 0, u0), (t >= 1, u1)):
                    pd = dt(u[1]) * ex - dt(u[0]) * ey
                    di = np.where(at_end & (np.abs(pd) <= np.abs(di)), pd, di)
            d[sel] = di * dt(shape.orient)
        out[:, c] = d
    return out.reshape(h, w, 4)


def generate(segs, w, h, R=4, dtype=np.float64):
    return M.encode(distances(build_shape(segs), w, h, dtype), R or 4)


def true_distance(shape, qx, qy, dtype=np.float64):
    """d(q) by A's rule at the float32 points (qx, qy)"""
    dt = np.dtype(dtype).type
    px, py = np.asarray(qx, np.float32).astype(dt).ravel(), np.asarray(qy, np.float32).astype(dt).ravel()
    n = px.size
    bd2, bo, bs = np.full(n, np.inf, dt), np.full(n, -1.0, dt), np.zeros(n, dt)
    for e in shape.edges:
        _, d2, ortho, side = _offer(e, px, py, dt)
        better = (d2 < bd2) | ((d2 == bd2) & (ortho > bo))
        bd2, bo, bs = np.where(better, d2, bd2), np.where(better, ortho, bo), np.where(better, side, bs)
    d = np.sqrt(bd2)
    return np.where(bs >= 0, d, -d) * dt(shape.orient)


def correct(img, segs, R=4, dtype=np.float64):
    """step 5 -> (the corrected image, the mask of marked texels, the artefacts); msdf_correct_ref.correct with d(q) over these edges"""
    F = np.ascontiguousarray(img, np.uint8)
    h, w = F.shape[:2]
    G, marked, artefacts = F.copy(), np.zeros((h, w), bool), []
    shape = build_shape(segs)
    cands = CR.candidates(F) if shape.edges else []
    if cands:
        dt = np.dtype(dtype).type
        d = true_distance(shape, *CR.crossing_points(cands), dtype)
        step = dt(R) / dt(255)
        Fi = F.astype(np.int64)
        depth = np.abs(2 * CR.median3(Fi[..., 0], Fi[..., 1], Fi[..., 2]) - 255)
        for (horizontal, xa, ya, ij, N, D, inside), dq in zip(cands, d):
            if not (dq < -step if inside else dq > step):
                continue
            xb, yb = (xa + 1, ya) if horizontal else (xa, ya + 1)
            artefacts.append(((xa, ya), (xb, yb), ij, N, D, inside, float(dq)))
            if depth[ya, xa] >= depth[yb, xb]:
                marked[ya, xa] = True
            if depth[yb, xb] >= depth[ya, xa]:
                marked[yb, xb] = True
    m = CR.median3(F[..., 0], F[..., 1], F[..., 2])
    for k in range(3):
        G[..., k] = np.where(marked, m, F[..., k])
    return G, marked, artefacts


def flatten(segs, chords=64):
    """-> the outline as 6-float line segments (for msdf_cases.winding): every curve in `chords` chords"""
    rows = []
    for x0, y0, ax, ay, bx, by, x1, y1 in np.asarray(segs, np.float32).astype(np.float64).reshape(-1, 8):
        if math.isnan(ax):
            rows.append((x0, y0, x1, y1))
            continue
        t = np.linspace(0.0, 1.0, chords + 1)
        u = 1 - t
        if math.isnan(bx):
            xs, ys = u * u * x0 + 2 * u * t * ax + t * t * x1, u * u * y0 + 2 * u * t * ay + t * t * y1
        else:
            xs = u ** 3 * x0 + 3 * u * u * t * ax + 3 * u * t * t * bx + t ** 3 * x1
            ys = u ** 3 * y0 + 3 * u * u * t * ay + 3 * u * t * t * by + t ** 3 * y1
        xs[0], ys[0], xs[-1], ys[-1] = x0, y0, x1, y1
        rows += list(zip(xs[:-1], ys[:-1], xs[1:], ys[1:]))
    return np.array([[a, b, np.nan, np.nan, c, d] for a, b, c, d in rows], np.float32).reshape(-1, 6)
