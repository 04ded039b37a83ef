"""The independent reference of the distance-field correction pass (fdh_put_glyph_outline with FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT),
written from step 5 of the specification in include/figdraw_hip.h in numpy: integers for everything but the verdict, and for that the true
signed distance of msdf_ref (step 4, A's rule) at the crossing point, in float64.  It reads and calls no library code; the tests hold the
kernel's source under a host shim (test_msdf_correct_host.py) and the compiled kernel (test_msdf_correct.py) to it.

    G, marked, artefacts = correct(F, segs, R)      # F: (h, w, 4) uint8 of step 4; G likewise; marked: (h, w) bool;
                                                    # artefacts: [((xa, ya), (xb, yb), (i, j), N, D, inside, d)]

`dtype=np.float32` takes d(q) in single precision: what a float32 implementation of the same formulas can and cannot reproduce."""
import numpy as np

import msdf_ref as M

CHANNEL_PAIRS = ((0, 1), (1, 2), (0, 2))


def median3(r, g, b):
    return np.maximum(np.minimum(r, g), np.minimum(np.maximum(r, g), b))


def true_distance(shape, qx, qy, dtype=np.float64):
    """d(q) of step 4 by A's rule at the points (qx, qy) (float32 values): all edges, ties to the larger orthogonality, no pseudo-distance,
    times the orientation; the formulas are msdf_ref's"""
    dt = np.dtype(dtype).type
    px, py = np.asarray(qx, np.float32).astype(dt).ravel(), np.asarray(qy, np.float32).astype(dt).ravel()
    n = px.size
    bd2, bo, bs = np.full(n, np.inf, dt), np.full(n, -1.0, dt), np.zeros(n, dt)
    for e in shape.edges:
        if e.line:
            P0, P2 = e.p[0].astype(dt), e.p[2].astype(dt)
            d = P2 - P0
            t = np.clip(((px - P0[0]) * d[0] + (py - P0[1]) * d[1]) / (d[0] * d[0] + d[1] * d[1]), 0, 1)
        else:
            t = M._nearest_on_quadratic(e.p, px, py, dt)
        ex, ey, tx, ty = M._at(e.p, e.line, t, px, py, dt)
        d2 = ex * ex + ey * ey
        den = (tx * tx + ty * ty) * d2
        with np.errstate(all="ignore"):
            ortho = np.where(den > 0, np.abs(tx * ey - ty * ex) / np.sqrt(np.where(den > 0, den, 1)), 0)
        better = (d2 < bd2) | ((d2 == bd2) & (ortho > bo))
        bd2 = np.where(better, d2, bd2)
        bo = np.where(better, ortho, bo)
        bs = np.where(better, ty * ex - tx * ey, bs)  # cross(T, p - N)
    d = np.sqrt(bd2)
    return np.where(bs >= 0, d, -d) * dt(shape.orient)


def candidates(img):
    """the integer half of step 5 -> [(horizontal, xa, ya, (i, j), N, D, inside)], in the order: horizontal pairs then vertical ones, row by row,
    and the channel pairs in the specification's order"""
    F = np.asarray(img).astype(np.int64)
    h, w = F.shape[:2]
    m = median3(F[..., 0], F[..., 1], F[..., 2])
    out = []
    for horizontal in (True, False):
        a, b = (F[:, :-1], F[:, 1:]) if horizontal else (F[:-1], F[1:])
        ma, mb = (m[:, :-1], m[:, 1:]) if horizontal else (m[:-1], m[1:])
        if a.size == 0:
            continue
        for i, j in CHANNEL_PAIRS:
            N = a[..., i] - a[..., j]
            D = N - (b[..., i] - b[..., j])
            neg = D < 0
            N, D = np.where(neg, -N, N), np.where(neg, -D, D)
            crosses = (D > 0) & (N > 0) & (N < D)
            V = [a[..., k] * D + N * (b[..., k] - a[..., k]) for k in range(3)]
            X = median3(*V)
            inside, outside = 2 * X > 255 * D, 2 * X < 255 * D
            cand = crosses & (((2 * ma > 255) & (2 * mb > 255) & outside) | ((2 * ma < 255) & (2 * mb < 255) & inside))
            for ya, xa in np.argwhere(cand):
                out.append((horizontal, int(xa), int(ya), (i, j), int(N[ya, xa]), int(D[ya, xa]), bool(inside[ya, xa])))
    return out


def crossing_points(cands):
    """-> (qx, qy) float32: the centre of a moved by the float32 quotient N / D along the pair, the sum rounded to float32"""
    qx, qy = np.zeros(len(cands), np.float32), np.zeros(len(cands), np.float32)
    for k, (horizontal, xa, ya, _, N, D, _) in enumerate(cands):
        t = np.float32(N) / np.float32(D)
        ax, ay = np.float32(xa) + np.float32(0.5), np.float32(ya) + np.float32(0.5)
        qx[k], qy[k] = (ax + t, ay) if horizontal else (ax, ay + t)
    return qx, qy


def correct(img, segs, R=4, dtype=np.float64):
    """step 5 -> (the corrected image, the mask of marked texels, the artefacts)"""
    F = np.ascontiguousarray(img, np.uint8)
    h, w = F.shape[:2]
    G, marked, artefacts = F.copy(), np.zeros((h, w), bool), []
    shape = M.build_shape(segs)
    cands = candidates(F) if shape.edges else []
    if cands:
        dt = np.dtype(dtype).type
        d = true_distance(shape, *crossing_points(cands), dtype)
        step = dt(R) / dt(255)
        Fi = F.astype(np.int64)
        depth = np.abs(2 * median3(Fi[..., 0], Fi[..., 1], Fi[..., 2]) - 255)
        for (horizontal, xa, ya, ij, N, D, inside), dq in zip(cands, d):
            if not (dq < -step if inside else dq > step):
                continue
            xb, yb = (xa + 1, ya) if horizontal else (xa, ya + 1)
            artefacts.append(((xa, ya), (xb, yb), ij, N, D, inside, float(dq)))
            if depth[ya, xa] >= depth[yb, xb]:
                marked[ya, xa] = True
            if depth[yb, xb] >= depth[ya, xa]:
                marked[yb, xb] = True
    m = median3(F[..., 0], F[..., 1], F[..., 2])
    for k in range(3):
        G[..., k] = np.where(marked, m, F[..., k])
    return G, marked, artefacts
