#!/usr/bin/env python3
"""Edge strip-draws of the rectangle frames with the saturated core as ONE rectangle and as the union of three, counted on the CPU.

No GPU and no library: the rectangles of a frame come from figdraw_amd/scenes.py, the draws a rectangle node turns into
(fdh_frontend.cpp: drop shadows, fill, stroke, inner shadows) and the core rule (fdh_record.cpp: local_core, core_pixels,
pack_bands; fdh_device.h: bin_entry_tail) are restated here.  tests/test_core_union_host.py pins the restatement against the
library.  A strip is 32 x 8 px on the frame's grid; a strip-draw is a (draw, strip) pair whose strip touches the draw's
clipped pixel bounds; it is a core strip when the strip lies inside one of the core's rectangles, an edge strip otherwise
(a stroke's or an inner shadow's core strips leave the entry: its edge strips are the ones that stay).  No occlusion and
no clipping beyond the bounds.

usage: core_strip_count.py            the tables of profiles/core_union.txt (eight bench frames, bench1080, the 8K frame)
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

f32 = np.float32
CORE_SLACK = 1.0 / 16.0
TILE_W, TILE_H = 32, 8
MODE_FILL, MODE_DROP, MODE_INSET, MODE_STROKE, MODE_BLUR = 3, 7, 9, 12, 17


def nim_round(x):
    x = f32(x)
    return f32(math.floor(float(x + f32(0.5)))) if x >= 0 else f32(-math.floor(float(-x + f32(0.5))))


def clamp_radius(r, m):
    return f32(0) if r <= 0 else nim_round(max(f32(1), min(f32(r), f32(m))))


def pack_radii(rx, ry, hx, hy):
    """rounded_radii_vec: rx, ry in node order TL, TR, BL, BR -> (DrawRec::r in shader order TR, BR, TL, BL, elliptical?)"""
    order = (1, 3, 0, 2)
    if all(f32(rx[i]) == f32(ry[i]) for i in range(4)):
        m = min(f32(hx), f32(hy))
        return [clamp_radius(rx[i], m) for i in order], False
    cm = min(f32(hx), f32(hy))
    out = []
    for i in order:
        cx, cy = clamp_radius(rx[i], hx), clamp_radius(ry[i], hy)
        if f32(rx[i]) == f32(ry[i]):
            out.append(f32(-(clamp_radius(rx[i], cm) + f32(1))))
        elif cx == cy:
            out.append(f32(-(cx + f32(1))))
        else:
            qx = nim_round(min(max(f32(cx / max(f32(hx), f32(0.000001))), f32(0)), f32(1)) * f32(4095))
            qy = nim_round(min(max(f32(cy / max(f32(hy), f32(0.000001))), f32(0)), f32(1)) * f32(4095))
            out.append(f32(qx + qy * f32(4096)))
    return out, True


class Rec:
    """the fields of a DrawRec the core rule reads, for a rounded rectangle drawn under the identity transform"""

    def __init__(self, rect, rx, ry, mode, factor, spread, shape=(0.0, 0.0), aa=1.2, push=False):
        x, y, w, h = (f32(v) for v in rect)
        self.mode, self.push, self.aa = mode, push, f32(aa)
        inset = mode == MODE_INSET
        qhx, qhy = f32(w * f32(0.5)), f32(h * f32(0.5))
        has_shape = shape[0] > 0 and shape[1] > 0
        shx = qhx if inset else f32((f32(shape[0]) if has_shape else w) * f32(0.5))
        shy = qhy if inset else f32((f32(shape[1]) if has_shape else h) * f32(0.5))
        self.p0, self.p1 = qhx, qhy
        self.p2, self.p3 = (f32(shape[0]), f32(shape[1])) if inset else (shx, shy)
        self.r, self.ellip = pack_radii(rx, ry, shx, shy)
        self.f0, self.f1 = f32(factor), f32(spread)
        x0, y0 = math.ceil(float(x)), math.ceil(float(y))
        x1, y1 = math.ceil(float(f32(x + w))), math.ceil(float(f32(y + h)))
        self.ox, self.oy, self.w_px, self.h_px = x0, y0, x1 - x0, y1 - y0
        self.valid = w > 0 and h > 0 and x1 > x0 and y1 > y0

    def bounds(self, W, H):
        """the quad's pixel bounds clipped to the frame"""
        return (min(max(self.ox, 0), W), min(max(self.oy, 0), H), min(max(self.ox + self.w_px, 0), W), min(max(self.oy + self.h_px, 0), H))


def local_core(r):
    """local_core (fdh_record.cpp): [first, H, V] as (xl, xr, yb, yt) in the shader's local frame, y up; None = no core"""
    if not r.aa > 0:
        return None
    aa = float(r.aa)
    if r.push or r.mode in (MODE_FILL, MODE_BLUR):
        e = 0.5 / aa
    elif r.mode == MODE_DROP:
        e = max(0.0, -float(r.f1))
    elif r.mode in (11, MODE_STROKE):
        e = max(0.0, float(r.f0)) + 0.5 / aa
    elif r.mode == MODE_INSET:
        e = max(0.0, 3.7 * max(0.5 * float(r.f0), 0.5) + float(r.f1))
    else:
        return None
    inset = r.mode == MODE_INSET
    qhx, qhy = float(r.p0), float(r.p1)
    bx, by = (qhx, qhy) if inset else (float(r.p2), float(r.p3))
    if not (qhx > 0 and qhy > 0 and bx > 0 and by > 0):
        return None
    crx, cry = [0.0] * 4, [0.0] * 4
    for k in range(4):
        sel = float(r.r[k])
        if not r.ellip:
            crx[k] = cry[k] = max(sel, 0.0)
        elif sel < 0:
            crx[k] = cry[k] = -sel - 1.0
        else:
            pv = math.floor(sel + 0.5)
            hi = math.floor(pv / 4096.0)
            crx[k] = (pv - 4096.0 * hi) * bx / 4095.0
            cry[k] = hi * by / 4095.0
    TR, BR, TL, BL = 0, 1, 2, 3
    if not r.ellip:
        k = 0.2929
        rr = [max(c - e, 0.0) for c in crx]
        mr, ml, mt, mb = max(rr[TR], rr[BR]), max(rr[TL], rr[BL]), max(rr[TR], rr[TL]), max(rr[BR], rr[BL])
        first = (-(bx - e) + k * ml, (bx - e) - k * mr, -(by - e) + k * mb, (by - e) - k * mt)
        Hb = (-(bx - e), bx - e, -(by - e) + mb, (by - e) - mt)
        Vb = (-(bx - e) + ml, (bx - e) - mr, -(by - e), by - e)
    else:
        Hb = (-(bx - e), bx - e, -min(by - e, by - max(cry[BR], cry[BL])), min(by - e, by - max(cry[TR], cry[TL])))
        Vb = (-min(bx - e, bx - max(crx[TL], crx[BL])), min(bx - e, bx - max(crx[TR], crx[BR])), -(by - e), by - e)
        ah = max(Hb[1] - Hb[0], 0.0) * max(Hb[3] - Hb[2], 0.0)
        av = max(Vb[1] - Vb[0], 0.0) * max(Vb[3] - Vb[2], 0.0)
        first = Hb if ah >= av else Vb
    out = [first, Hb, Vb]
    if inset:
        px, py = float(r.p2), float(r.p3)
        out = [(c[0] + px, c[1] + px, c[2] - py, c[3] - py) for c in out]
    return out


def core_pixels(r, c):
    """core_pixels (fdh_record.cpp): a local rectangle's pixel centres [x0, x1) x [y0, y1), or None"""
    xl, xr, yb, yt = c
    if not (xr > xl and yt > yb):
        return None
    qhx, qhy = float(r.p0), float(r.p1)
    cxl = r.ox + r.w_px * (xl / (2.0 * qhx) + 0.5) + CORE_SLACK
    cxr = r.ox + r.w_px * (xr / (2.0 * qhx) + 0.5) - CORE_SLACK
    cyt = r.oy + r.h_px * (0.5 - yt / (2.0 * qhy)) + CORE_SLACK
    cyb = r.oy + r.h_px * (0.5 - yb / (2.0 * qhy)) - CORE_SLACK
    ix0, ix1 = math.ceil(cxl - 0.5), math.floor(cxr - 0.5) + 1
    iy0, iy1 = math.ceil(cyt - 0.5), math.floor(cyb - 0.5) + 1
    ix0, ix1 = max(ix0, r.ox), min(ix1, r.ox + r.w_px)
    iy0, iy1 = max(iy0, r.oy), min(iy1, r.oy + r.h_px)
    if not (ix1 > ix0 and iy1 > iy0):
        return None
    c16 = lambda v: int(min(max(v, -32768), 32767))
    return (c16(ix0), c16(iy0), c16(ix1), c16(iy1))


def core_rects(r, union=True):
    """the rectangles the bin launch tests, after BinRec's packing (pack_bands / bin_entry_tail): a list of up to three"""
    lc = local_core(r) if r.valid else None
    if lc is None:
        return []
    c = core_pixels(r, lc[0])
    if c is None:
        return []
    out = [c]
    if not union:
        return out
    h, v = core_pixels(r, lc[1]), core_pixels(r, lc[2])
    if h and h[0] <= c[0] and h[2] >= c[2] and h[1] >= c[1] and h[3] <= c[3]:
        q = (c[0] - min(c[0] - h[0], 255), c[1] + min(h[1] - c[1], 65535), c[2] + min(h[2] - c[2], 255), c[3] - min(c[3] - h[3], 65535))
        if q[2] > q[0] and q[3] > q[1] and q != c:
            out.append(q)
    if v and v[1] <= c[1] and v[3] >= c[3] and v[0] >= c[0] and v[2] <= c[2]:
        q = (c[0] + min(v[0] - c[0], 65535), c[1] - min(c[1] - v[1], 255), c[2] - min(c[2] - v[2], 65535), c[3] + min(v[3] - c[3], 255))
        if q[2] > q[0] and q[3] > q[1] and q != c:
            out.append(q)
    return out


def strip_counts(r, rects, W, H):
    """(strips the draw's clipped bounds touch, of them inside one of `rects`) on the frame's 32 x 8 grid"""
    x0, y0, x1, y1 = r.bounds(W, H)
    if not (x1 > x0 and y1 > y0):
        return 0, 0
    sx0, sx1, sy0, sy1 = x0 // TILE_W, (x1 - 1) // TILE_W + 1, y0 // TILE_H, (y1 - 1) // TILE_H + 1
    inside = np.zeros((sy1 - sy0, sx1 - sx0), bool)
    for cx0, cy0, cx1, cy1 in rects:
        a0, a1 = max(-(-cx0 // TILE_W), sx0), min(cx1 // TILE_W, sx1)  # strip columns / rows wholly inside the rectangle
        b0, b1 = max(-(-cy0 // TILE_H), sy0), min(cy1 // TILE_H, sy1)
        if a1 > a0 and b1 > b0:
            inside[b0 - sy0:b1 - sy0, a0 - sx0:a1 - sx0] = True
    return inside.size, int(inside.sum())


def node_draws(n, ui=1.0, aa=1.2):
    """the rounded-rectangle draws of an nkRectangle node (fdh_frontend.cpp: drop_shadows, rounded_shape, inner_shadows) as (class, Rec)"""
    from figdraw_amd.scene import FigFlags, FigKind, FillKind, ShadowStyle

    if n.kind != FigKind.nkRectangle or n.rotation:
        return []
    alpha_max = lambda f: f.start[3] if f.kind == FillKind.flColor else max(f.start[3], f.stop[3]) if f.kind == FillKind.flLinear2 else max(f.start[3], f.mid[3], f.stop[3])
    s = lambda v: f32(f32(v) * f32(ui))
    box = [s(v) for v in n.screenBox]
    rx = [s(f32(int(c))) for c in n.corners]
    ry = [s(f32(int(c))) for c in n.cornerRadiiY] if n.flags & FigFlags.NfEllipticalCorners else list(rx)
    out = []
    for sh in n.shadows:
        if sh.style != ShadowStyle.DropShadow or (sh.blur <= 0 and sh.spread <= 0) or alpha_max(sh.fill) == 0:
            continue
        sb, ss = s(sh.blur), s(sh.spread)
        pad = max(f32(nim_round(ss) + nim_round(f32(1.5) * sb)), f32(0))
        quad = (f32(f32(box[0] + s(sh.x)) - pad), f32(f32(box[1] + s(sh.y)) - pad), f32(box[2] + f32(2) * pad), f32(box[3] + f32(2) * pad))
        out.append(("drop shadow", Rec(quad, rx, ry, MODE_DROP, sb, ss, (box[2], box[3]), aa)))
    kind = "elliptical" if Rec(box, rx, ry, MODE_FILL, 4.0, 0.0, aa=aa).ellip else "circular"
    if alpha_max(n.fill) > 0:
        out.append(("fill, " + kind, Rec(box, rx, ry, MODE_FILL, 4.0, 0.0, aa=aa)))
    if alpha_max(n.stroke.fill) > 0 and n.stroke.weight > 0:
        out.append(("stroke, " + kind, Rec(box, rx, ry, MODE_STROKE, s(n.stroke.weight), 0.0, aa=aa)))
    for sh in n.shadows:
        if sh.style != ShadowStyle.InnerShadow or (sh.blur <= 0 and sh.spread <= 0) or alpha_max(sh.fill) == 0:
            continue
        out.append(("inner shadow", Rec(box, rx, ry, MODE_INSET, s(sh.blur), s(sh.spread), (s(sh.x), s(sh.y)), aa)))
    return out


CLASSES = ("fill, elliptical", "stroke, elliptical", "drop shadow", "fill, circular", "stroke, circular", "inner shadow")


def count_frame(renders, W, H, ui=1.0):
    """{class: [strip-draws touched, edge strip-draws with one rectangle, with the union]} for one frame"""
    tot = {c: [0, 0, 0] for c in CLASSES}
    for lst in renders.layers.values():
        for n in lst.nodes:
            for cls, r in node_draws(n, ui):
                touched, one = strip_counts(r, core_rects(r, False), W, H)
                _, three = strip_counts(r, core_rects(r, True), W, H)
                t = tot[cls]
                t[0] += touched; t[1] += touched - one; t[2] += touched - three
    return tot


def table(title, frames):
    print(title)
    print(f"{'draw class':22s} {'strip-draws':>12s} {'edge, one rect':>15s} {'edge, union':>12s} {'change':>8s}")
    tot = {c: [0, 0, 0] for c in CLASSES}
    for f in frames:
        for c, v in f.items():
            for k in range(3):
                tot[c][k] += v[k]
    rows = [(c, tot[c]) for c in CLASSES] + [("all", [sum(tot[c][k] for c in CLASSES) for k in range(3)])]
    for c, v in rows:
        ch = 100.0 * (v[2] - v[1]) / v[1] if v[1] else 0.0
        print(f"{c:22s} {v[0]:12d} {v[1]:15d} {v[2]:12d} {ch:+7.1f}%")
    print()


def main():
    from figdraw_amd import scenes

    W, H = 3840, 2160
    frames = [count_frame(scenes.make_render_tree_100(W, H, frame=f, full_frame_blur=True), W, H) for f in range(8)]
    table(f"bench frames 0..7 ({W}x{H}, 300 rects, full-frame blur): sum over the eight frames", frames)
    table("bench frame 0 alone", frames[:1])
    W, H = 1920, 1080
    table(f"bench1080 ({W}x{H}, frame 0, no full-frame blur)", [count_frame(scenes.make_render_tree_100(W, H, frame=0), W, H)])
    W, H = 7680, 4320
    table(f"8K frame ({W}x{H}, frame 0)", [count_frame(scenes.make_render_tree_100(W, H, frame=0, full_frame_blur=True), W, H)])


if __name__ == "__main__":
    main()
