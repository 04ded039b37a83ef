"""The independent reference of overlapping-contour support in distance-field generation (fdh_put_glyph_outline with FDH_GLYPH_MTSDF |
FDH_GLYPH_MTSDF_OVERLAP), written from step 6 of the specification in include/figdraw_hip.h in numpy float64.  The per-contour fields are
msdf_ref's step 4 over one contour's edges; the areas, the ranking, the terms and the selection are this file's.  It reads and calls no
library code; the tests hold the kernels' source under a host shim (test_msdf_overlap_host.py) and the compiled kernels
(test_msdf_overlap.py) to it.

    cs = contours(segs)                      # step 1 again, contour by contour: [(rows of segs, area_c)], and the orientation o
    img = generate(segs, w, h, R)            # step 6: (h, w, 4) uint8
    d = distances(segs, w, h)                # before the encoding: (h, w, 4); [..., 3] is the new A
    G, marked, artefacts = correct(F, segs, R)   # step 5 with step 6's verdict distance

`dtype=np.float32` runs the per-contour fields and the ranking in single precision, as msdf_ref's switch does."""
import numpy as np

import msdf_correct_ref as CR
import msdf_ref as M

TERMS = 4


def contours(segs):
    """step 1's contours with step 2's sum over each one's own edges -> ([(segs of the contour (m, 6) float32, area_c)], o)"""
    segs = np.asarray(segs, np.float32).reshape(-1, 6)
    out, cur, own, total, start, last = [], [], 0.0, 0.0, None, None
    for row in segs:
        q = row.astype(np.float64)
        line = bool(np.isnan(q[2]))
        p0, p2 = q[0:2], q[4:6]
        p1 = p0 if line else q[2:4]
        if not line:
            b = p0 - 2.0 * p1 + p2
            a, c, e = p1 - p0, p2 - p0, p2 - p1
            folded = a[0] * c[1] == a[1] * c[0] and not (a[0] * e[0] > 0.0 or a[1] * e[1] > 0.0)
            if b[0] * b[0] + b[1] * b[1] <= 1e-6 or folded:
                line = True
        if line and p0[0] == p2[0] and p0[1] == p2[1]:
            continue
        if cur and (last[0] != p0[0] or last[1] != p0[1]):
            raise M.OpenContour("a segment does not start where the one before it ended")
        if not cur:
            start = p0
        cur.append(row)
        last = p2
        chord = 0.5 * (p0[0] * p2[1] - p2[0] * p0[1])
        total += chord
        own += chord
        if not line:
            bow = ((p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0])) / 3.0
            total += bow
            own += bow
        if p2[0] == start[0] and p2[1] == start[1]:
            out.append((np.array(cur, np.float32), own))
            cur, own = [], 0.0
    if cur:
        raise M.OpenContour("the last contour does not close")
    return out, (1.0 if total >= 0.0 else -1.0)


def _classes(segs):
    """-> ([msdf_ref shape of each contour, carrying the outline's orientation], [filled?])"""
    cs, o = contours(segs)
    shapes, filled = [], []
    for rows, area in cs:
        s = M.build_shape(rows)  # steps 1 and 3 are per contour: the same edges and colours as in the whole outline
        s.orient = o
        shapes.append(s)
        filled.append(o * area >= 0.0)
    return shapes, filled


def _rank(a, filled):
    """a: (n, N) the contours' A at N points -> (value of the largest term (N,), index of the selected contour (N,))"""
    n, N = a.shape
    fi = [c for c in range(n) if filled[c]]
    gi = [c for c in range(n) if not filled[c]]
    F = a[fi]
    of = np.argsort(-F, axis=0, kind="stable")  # descending, ties in contour order
    best = np.full(N, -np.inf, a.dtype)
    pick = np.full(N, -1, np.int64)
    if gi:
        G = a[gi]
        og = np.argsort(G, axis=0, kind="stable")  # ascending
    cols = np.arange(N)
    for k in range(min(TERMS, len(fi))):
        cf = of[k]
        af = F[cf, cols]
        who = np.asarray(fi)[cf]
        f = af
        if k < len(gi):
            cg = og[k]
            ag = G[cg, cols]
            hole = ag < af
            f = np.where(hole, ag, af)
            who = np.where(hole, np.asarray(gi)[cg], who)
        up = f > best
        best = np.where(up, f, best)
        pick = np.where(up, who, pick)
    return best, pick


def distances(segs, w, h, dtype=np.float64):
    """step 6 before the encoding: (h, w, 4) signed distances, all four of the selected contour; -inf everywhere for an outline without edges"""
    shapes, filled = _classes(segs)
    if not shapes:
        return M.distances(M.Shape(), w, h, dtype)
    d = np.stack([M.distances(s, w, h, dtype).reshape(-1, 4) for s in shapes])  # (n, N, 4)
    _, pick = _rank(np.ascontiguousarray(d[..., 3]), filled)
    return d[pick, np.arange(d.shape[1])].reshape(h, w, 4)


def generate(segs, w, h, R=4, dtype=np.float64):
    return M.encode(distances(segs, w, h, dtype), R or 4)


def true_distance(segs, qx, qy, dtype=np.float64):
    """step 6's A at the points (qx, qy): the largest term over the contours' true distances (msdf_correct_ref.true_distance per contour)"""
    shapes, filled = _classes(segs)
    a = np.stack([CR.true_distance(s, qx, qy, dtype) for s in shapes])
    return _rank(a, filled)[0]


def correct(img, segs, R=4, dtype=np.float64):
    """step 5 with d(q) of step 6 -> (the corrected image, the mask of marked texels, the artefacts), as msdf_correct_ref.correct"""
    F = np.ascontiguousarray(img, np.uint8)
    h, w = F.shape[:2]
    marked, artefacts = np.zeros((h, w), bool), []
    cands = CR.candidates(F) if contours(segs)[0] else []
    if cands:
        dt = np.dtype(dtype).type
        d = true_distance(segs, *CR.crossing_points(cands), dtype)
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
    G = F.copy()
    m = CR.median3(F[..., 0], F[..., 1], F[..., 2])
    for k in range(3):
        G[..., k] = np.where(marked, m, F[..., k])
    return G, marked, artefacts
