"""The cases of tests/test_blur_exact.py and the child process that renders them.

`python blur_exact_child.py ROUTE OUT.npz` renders every case of one blur route on the GPU through the per-call path (begin_frame, draw_image
1:1, draw_backdrop_blur with zero radii on an integer rectangle, end_frame) and writes the frames and blur surfaces it read back.  The
switches that pick a route (FDH_FORCE_BLUR_PATH, FDH_BLUR_FUSED) are read once per process: the parent sets them in the child's environment
(ROUTES below), so a route is a fresh interpreter.  The float64 reference runs in the parent."""
import sys
from collections import namedtuple

import numpy as np

# route -> (environment of the child, set_blur_route argument, what it runs)
ROUTES = {
    "valu2": ({"FDH_FORCE_BLUR_PATH": "1"}, 0, "k_blur_h<2>, k_blur_v<2,4>"),
    "valu8": ({"FDH_FORCE_BLUR_PATH": "2"}, 0, "k_blur_h<8|10|12>, k_blur_v<8|10|12,4>"),
    "mx": ({"FDH_FORCE_BLUR_PATH": "3"}, 0, "k_blur_mx horizontal and vertical"),
    "fx": ({"FDH_FORCE_BLUR_PATH": "3"}, 1, "k_blur_fx"),
    "small": ({}, 1, "k_blur_small"),
    "native": ({}, None, "1024 x 384: the matrix pipe taken natively (both routes)"),
}
REMOVED_ENV = ("FDH_FORCE_BLUR_PATH", "FDH_BLUR_FUSED")  # whatever the caller's environment holds, the child gets the route's own

# every k-step count a radius in (0.5, 64] can select: horizontal 4 - 11, vertical 3 - 10 (35 and 44 are the radii of NK = 7 horizontal and
# NK = 8 vertical, 16 that of the fused pair (5,4)), and the fused pairs (4,3) (4,4) (5,4) (5,5) (6,5) (6,6): tests/test_blur_exact.py asserts it
RADII_ALL = [0.8, 3, 9, 12, 16, 18, 24, 30, 35, 40, 44, 50, 58, 64]
RADII_FEW = [3, 18, 64]
WHITE, GLASS = (1.0, 1.0, 1.0, 1.0), (0.2, 0.3, 0.4, 0.5)
STRIPE = (43, 117)

# name: shape-kind[-clip]-rRADIUS.  kind: blur_ref.noise.  clip: the node sits under an open clip (begin_mask over the whole frame), so the
# vertical pass writes the blurred snapshot to its own surface and does not composite it.  blur_route: set_blur_route for this case (None: the route's).
Case = namedtuple("Case", "name shape w h kind clip rect radius stripe blur_route")


def _case(shape, w, h, kind, clip, rect, radius, stripe=None, blur_route=None, tag=""):
    name = f"{shape}{tag}-{kind}{'-clip' if clip else ''}-r{radius:g}"
    return Case(name, shape, w, h, kind, clip, tuple(rect), float(radius), stripe, blur_route)


def pick_nout(extent, quantum, reach):
    """blur_pick_nout (figdraw_amd/csrc/k_blur_valu.hip) restated: padded extent x instructions per output, the cheapest of 8 / 10 / 12"""
    best, best_cost = 8, 1e300
    for n in (8, 10, 12):
        unit = quantum * n
        padded = float((extent + unit - 1) // unit * unit)
        cost = padded * (2.0 * (2 * reach + 1) + 4.0 * (n + 2 * reach) / n + 6.0)
        if cost < best_cost:
            best, best_cost = n, cost
    return best


NOUT_FRAME = (704, 64)
NOUT_WIDTHS, NOUT_HEIGHTS = (300, 600, 700), (32, 40, 48)


def fused_supported(reach):
    """blur_fused_supported (k_blur_mx.hip): the filter widths k_blur_fx is built for"""
    nkh, nkv = (32 + 2 * reach + 3 + 15) // 16, (32 + 2 * reach + 15) // 16
    return 3 <= nkh <= 6 and nkh in (nkv, nkv + 1)


def cases(route, reach_of):
    """the cases of a route; reach_of(radius) -> tap reach (the library's)"""
    out = []
    valu = route in ("valu2", "valu8", "small")

    def takes(radius):
        if route == "fx":
            return fused_supported(reach_of(radius))
        if route == "small":
            return reach_of(radius) <= 24
        return True

    def both(shape, w, h, rect, radii, **kw):  # the three-channel forms (opaque on white) and the four-channel ones (premultiplied on glass, under a clip)
        for r in radii:
            if not takes(r):
                continue
            out.append(_case(shape, w, h, "opaque", False, rect, r, **kw))
            if route != "fx":  # (a node under a clip never takes k_blur_fx)
                out.append(_case(shape, w, h, "premul", True, rect, r, **kw))
            if route in ("fx", "mx") and rect == (0, 0, w, h):  # translucent, composited by the pass: k_blur_fx's four-channel form and its partner
                out.append(_case(shape, w, h, "premul", False, rect, r, **kw))

    if route == "native":
        w, h = 1024, 384
        for br in (0, 1):
            for r in RADII_FEW:
                out.append(_case("native", w, h, "opaque", False, (0, 0, w, h), r, blur_route=br, tag=f"-route{br}"))
                out.append(_case("native", w, h, "premul", False, (0, 0, w, h), r, blur_route=br, tag=f"-route{br}"))
        return out
    # 1. full-frame node; the odd pitch makes the rows of k_blur_h alternate between its 16-byte, 8-byte and scalar store branches
    both("full", 264, 200, (0, 0, 264, 200), RADII_ALL)
    for r in RADII_FEW:
        if takes(r):
            out.append(_case("full", 264, 200, "checker", False, (0, 0, 264, 200), r))
    if valu:
        both("fullodd", 263, 199, (0, 0, 263, 199), RADII_ALL)
    # 4. a frame smaller than the filter: every window clamps at both ends
    both("tiny", 40, 36, (0, 0, 40, 36), RADII_FEW)
    # 6. a stripe whose bounds are no multiple of 8
    both("stripe", 264, 200, (0, 0, 264, 200), RADII_FEW, stripe=STRIPE)
    if route == "fx":
        return out
    # 2. interior node at an odd origin, no edge on a multiple of 4, 32 or 64
    both("inner", 264, 200, (37, 29, 150, 101), RADII_ALL)
    # 3. nodes hanging over two opposite frame corners
    both("cornerA", 264, 200, (-20, -10, 100, 80), RADII_FEW)
    both("cornerB", 264, 200, (200, 150, 100, 80), RADII_FEW)
    both("tinynode", 40, 36, (13, 11, 9, 7), RADII_FEW)
    # 5. nodes one pixel wide and one pixel tall
    both("col", 264, 200, (50, 60, 1, 90), RADII_FEW)
    both("row", 264, 200, (50, 60, 90, 1), RADII_FEW)
    # 7. every NOUT build of the 8 - 12 outputs-per-thread passes, named after the build blur_pick_nout selects along x and along y
    if route == "valu8":
        fw, fh = NOUT_FRAME
        for nw in NOUT_WIDTHS:
            for nh in NOUT_HEIGHTS:
                for r in RADII_FEW:
                    reach = reach_of(r)
                    tag = f"-h{pick_nout(nw, 64, reach)}v{pick_nout(nh, 4, reach)}-{nw}x{nh}"
                    out.append(_case("nout", fw, fh, "opaque", False, (2, 5, nw, nh), r, tag=tag))
                    out.append(_case("nout", fw, fh, "premul", True, (2, 5, nw, nh), r, tag=tag))
    return out


def image_key(c):
    return 0x62780000 + {"opaque": 0, "premul": 1, "checker": 2}[c.kind] * 0x100 + [(264, 200), (263, 199), (40, 36), NOUT_FRAME, (1024, 384)].index((c.w, c.h))


def image_seed(c):
    return 20260 + image_key(c) % 0x10000


def calls(c, blur):
    """the calls of a case's frame (with the blur node) or of its source frame (without)"""
    z, white = [0.0] * 4, [[255, 255, 255, 255]] * 4
    out = [["begin_frame", 1, list(WHITE if c.kind != "premul" else GLASS)]]
    if c.clip:
        out += [["begin_mask", [0.0, 0.0, float(c.w), float(c.h)], z, z], ["end_mask"]]
    out.append(["draw_image", image_key(c), [0.0, 0.0], white])
    if blur:
        out.append(["draw_backdrop_blur", [float(v) for v in c.rect], z, z, c.radius])
    if c.clip:
        out.append(["pop_mask"])
    out.append(["end_frame"])
    return out


def main(route, out_path):
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.dirname(os.path.abspath(__file__))):
        if p not in sys.path:
            sys.path.insert(0, p)
    import blur_ref as BR
    from figdraw_amd.context import HipContext

    env, blur_route, _ = ROUTES[route]
    for k in REMOVED_ENV:
        assert os.environ.get(k) == env.get(k), (k, os.environ.get(k), "the child's environment is not the route's")
    reach_of = lambda r: BR.lib_taps(r)[0]
    ctx = HipContext(device=0, atlas_size=2048)
    if blur_route is not None:
        ctx.set_blur_route(blur_route)
    out, have = {}, set()
    for c in cases(route, reach_of):
        key = image_key(c)
        if key not in have:
            ctx.put_image(key, BR.noise(c.w, c.h, image_seed(c), c.kind))
            have.add(key)
        if c.blur_route is not None:
            ctx.set_blur_route(c.blur_route)
        ctx.W, ctx.H = c.w, c.h
        sname = f"src|{c.w}x{c.h}-{c.kind}{'-clip' if c.clip else ''}"
        if sname not in out:  # what the same calls without the blur node render, on this context
            ctx.replay_calls(calls(c, False))
            out[sname] = ctx.read_pixels()
        if c.stripe:
            ctx.set_stripe(*c.stripe)
        ctx.replay_calls(calls(c, True))
        out[c.name + "|frame"] = ctx.read_pixels()
        out[c.name + "|h"] = ctx.debug_read_surface(1)
        out[c.name + "|snap"] = ctx.debug_read_surface(2)
        ctx.profile(1)
        st = ctx.frame_stats()
        out[c.name + "|ms"] = np.array([st.ms_blur_fused, st.ms_blur_h, st.ms_blur_v, st.ms_blur_big_h, st.ms_blur_big_v, st.n_blurs], dtype=np.float64)
        if c.stripe:
            ctx.set_stripe(0, 0)
    ctx.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
