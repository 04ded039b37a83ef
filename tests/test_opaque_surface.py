"""The opaque-surface kernels change no byte.  A frame that is cleared with a colour of alpha 255 (after clear folding) takes
k_composite_tiles<4 | 32> and the three-channel forms of k_blur_mx / k_blur_fx (Context::decide_opaque); FDH_OPAQUE=0 turns that off.
Every frame below is rendered twice -- in this process and in a fresh child process with FDH_OPAQUE=0 (the switch is read once per
process) -- and must come out byte for byte the same in all four channels; frames that start opaque must hold alpha 255 everywhere;
frames that do not (clear alpha 254, no clear, a translucent folded panel) must keep the generic kernels, which the equality with the
child shows: a forced alpha byte would differ.  Against the oracle: at most 1 LSB on at most 0.5 % of the pixels, the suite's bar."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import diff_stats

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

OPAQUE_BLUE = (0.2, 0.4, 0.9, 1.0)


def _small_nodes(dx=0.0, dy=0.0):
    """One draw of each path the no-clip build has, on a 131 x 70 frame (three bins by two; the width is no multiple of 4, so the
    right-hand strips store pixel by pixel): each node about 70 x 36, so that it has a core strip (32 x 8), edge strips and strips it
    misses; the last one is opaque and stacked over the first (the occlusion cut)."""
    from figdraw_amd.scene import (Fig, FigFlags, FigKind, FillGradientAxis, RenderShadow, RenderStroke, ShadowStyle, fill, linear, rect,
                                   rgba)

    R = FigKind.nkRectangle
    return [
        # a one-colour fill
        Fig(kind=R, screenBox=rect(3 + dx, 2 + dy, 72, 38), fill=rgba(220, 40, 40, 155), corners=[6] * 4),
        # a 3-stop gradient
        Fig(kind=R, screenBox=rect(40 + dx, 20 + dy, 80, 40), corners=[5, 9, 3, 7],
            fill=linear(rgba(18, 112, 64, 255), rgba(40, 180, 90, 200), rgba(78, 224, 188, 120), axis=FillGradientAxis.fgaX, midPos=128)),
        # a stroke alone (no fill)
        Fig(kind=R, screenBox=rect(10 + dx, 24 + dy, 76, 40), fill=rgba(0, 0, 0, 0), corners=[8] * 4,
            stroke=RenderStroke(weight=3.0, fill=fill(rgba(255, 255, 255, 210)))),
        # elliptical corners
        Fig(kind=R, screenBox=rect(50 + dx, 4 + dy, 78, 36), fill=rgba(238, 140, 30, 220), corners=[30, 12, 20, 8], cornerRadiiY=[12, 16, 9, 14],
            flags=FigFlags.NfEllipticalCorners),
        # a black drop shadow (blend_black) under a translucent fill
        Fig(kind=R, screenBox=rect(20 + dx, 8 + dy, 70, 36), fill=rgba(40, 180, 90, 155), corners=[7] * 4,
            shadows=[RenderShadow(style=ShadowStyle.DropShadow, blur=6.0, spread=3.0, x=4.0, y=5.0, fill=fill(rgba(0, 0, 0, 155)))]),
        # an inner shadow with a gradient
        Fig(kind=R, screenBox=rect(28 + dx, 26 + dy, 74, 38), fill=rgba(60, 90, 220, 155), corners=[6] * 4,
            shadows=[RenderShadow(style=ShadowStyle.InnerShadow, blur=8.0, spread=3.0, x=2.0, y=-3.0,
                                  fill=linear(rgba(25, 25, 40, 100), rgba(65, 65, 95, 180), axis=FillGradientAxis.fgaDiagBLTR))]),
        # fill + stroke + inner shadow of one node: one distance field for the run
        Fig(kind=R, screenBox=rect(6 + dx, 12 + dy, 90, 44), fill=rgba(118, 168, 255, 140), corners=[10] * 4,
            stroke=RenderStroke(weight=4.0, fill=fill(rgba(90, 45, 0, 220))),
            shadows=[RenderShadow(style=ShadowStyle.InnerShadow, blur=5.0, spread=2.0, x=-2.0, y=2.0, fill=fill(rgba(40, 40, 60, 150)))]),
        # an opaque core over the first node: what lies under it in a strip it covers is cut
        Fig(kind=R, screenBox=rect(0 + dx, 0 + dy, 66, 34), fill=rgba(250, 200, 40, 255)),
    ]


def small_tree(copies=1, background=None):
    """`copies` of the nodes, each shifted a little: one copy is a frame of a handful of draws (a direct launch), eight make a phase of
    more than 64 draws, which is binned into lists.  `background`: a full-frame panel in front (clear folding takes it)."""
    from figdraw_amd.scene import Fig, FigKind, RenderList, Renders, rect, rgba

    lst = RenderList()
    if background is not None:
        lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(0, 0, 131, 70), fill=rgba(*background)))
    for c in range(copies):
        for n in _small_nodes(dx=float(5 * c % 23), dy=float(3 * c % 11)):
            lst.addRoot(n)
    out = Renders()
    out.setLayer(0, lst)
    return out


def blur_tree(w, h, radius, box=None, second_node=False):
    """content, then a backdrop-blur node with a translucent tint (mode 17 with alpha < 1) over `box` (default: the whole frame), more
    content, and optionally a second, 360 x 240 node (another phase, over what the first one's kernels wrote)"""
    from figdraw_amd.scene import Fig, FigKind, rect, rgba

    import ref_scenes as RS

    sc = RS.random_scene(77, float(w), float(h), n=40, clips=False, blur=False)
    lst = next(iter(sc.layers.values()))
    x, y, bw, bh = box if box else (0, 0, w, h)
    lst.addRoot(Fig(kind=FigKind.nkBackdropBlur, screenBox=rect(x, y, bw, bh), fill=rgba(255, 255, 255, 60), blur=radius))
    lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(w * 0.2, h * 0.3, w * 0.4, h * 0.25), fill=rgba(250, 200, 40, 160), corners=[18] * 4))
    if second_node:
        lst.addRoot(Fig(kind=FigKind.nkBackdropBlur, screenBox=rect(w * 0.5, h * 0.2, 360, 240), corners=[20] * 4, fill=rgba(0, 0, 0, 0), blur=18.0))
        lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(w * 0.5, h * 0.2, 360, 240), corners=[20] * 4, fill=rgba(255, 225, 55, 120)))
    return sc


# name -> (scene builder, its arguments, w, h, clear colour, blur route or None, the frame starts opaque)
def _cases():
    out = {}
    for copies in (1, 8):
        tag = "direct" if copies == 1 else "lists"
        out[f"small_{tag}_opaque"] = (small_tree, (copies,), 131, 70, OPAQUE_BLUE, None, True)
        out[f"small_{tag}_alpha254"] = (small_tree, (copies,), 131, 70, (0.2, 0.4, 0.9, 254.0 / 255.0), None, False)
        out[f"small_{tag}_folded_opaque"] = (small_tree, (copies, (30, 60, 90, 255)), 131, 70, (0.0, 0.0, 0.0, 0.0), None, True)
        out[f"small_{tag}_folded_155"] = (small_tree, (copies, (255, 255, 255, 155)), 131, 70, (0.0, 0.0, 0.0, 0.0), None, False)
    for radius in (5.0, 18.0):
        for route in (0, 1):
            out[f"blur_r{int(radius)}_route{route}"] = (blur_tree, (1024, 384, radius), 1024, 384, OPAQUE_BLUE, route, True)
    out["region_two_pass"] = (blur_tree, (1056, 448, 18.0, (16, 16, 1024, 416)), 1056, 448, OPAQUE_BLUE, 0, True)
    out["two_phases"] = (blur_tree, (1024, 384, 18.0, None, True), 1024, 384, OPAQUE_BLUE, 1, True)
    return out


CASES = _cases()
# frames render_all adds to the cases' own: the small trees again without a clear, the radius-18 frame as two row stripes
DERIVED = {"small_direct_no_clear": "small_direct_alpha254", "small_lists_no_clear": "small_lists_alpha254",
           "blur_r18_route0_stripes": "blur_r18_route0", "blur_r18_route1_stripes": "blur_r18_route1"}
NAMES = sorted(list(CASES) + list(DERIVED))
STARTS_OPAQUE = [n for n in NAMES if CASES[DERIVED.get(n, n)][6] and not n.endswith("no_clear")]


STRIPES = ((0, 192), (192, 384))
_ORACLE = {}


def render_all():
    """every frame of this file on one device, name -> pixels.  (Run in this process and, by the fixture, in a child.)"""
    from figdraw_amd.context import HipContext

    frames = {}
    for name, (build, args, w, h, clear, route, _) in CASES.items():
        sc = build(*args)
        ctx = HipContext(device=0)
        if route is not None:
            ctx.set_blur_route(route)
        ctx.render_frame(sc, w, h, color=clear)
        frames[name] = ctx.read_pixels().copy()
        if name.endswith("alpha254"):
            # the same tree again WITHOUT a clear, over the surface (alpha < 255 in places) the frame above left
            ctx.render_frame(sc, w, h, clear=False)
            frames[name.replace("alpha254", "no_clear")] = ctx.read_pixels().copy()
        if name + "_stripes" in DERIVED:
            whole = np.zeros_like(frames[name])
            for y0, y1 in STRIPES:
                ctx.set_stripe(y0, y1)
                ctx.render_frame(sc, w, h, color=clear)
                whole[y0:y1] = ctx.read_pixels()[y0:y1]
            ctx.set_stripe(0, 0)
            frames[name + "_stripes"] = whole
        ctx.close()
    return frames


@pytest.fixture(scope="module")
def both():
    """(frames of this process, frames of a child process with FDH_OPAQUE=0)"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_opaque_surface as T\n"
            "np.savez(sys.argv[1], **T.render_all())\n") % (ROOT, HERE)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "off.npz")
        subprocess.check_call([sys.executable, "-c", code, path], env=dict(os.environ, FDH_OPAQUE="0"))
        off = dict(np.load(path))
    return render_all(), off


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_switch_changes_no_byte(both, name):
    on, off = both
    assert on[name].shape == off[name].shape
    assert np.array_equal(on[name], off[name]), (name, int((on[name] != off[name]).any(axis=2).sum()), "pixels differ; alpha:",
                                                 int((on[name][..., 3] != off[name][..., 3]).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", STARTS_OPAQUE)
def test_a_frame_that_starts_opaque_stays_opaque(both, name):
    on, off = both
    assert (on[name][..., 3] == 255).all() and (off[name][..., 3] == 255).all(), name


@pytest.mark.gpu
def test_frames_that_do_not_start_opaque_hold_other_alphas(both):
    """(the cases that must keep the generic kernels do have alphas a forced byte would change)"""
    on, _ = both
    for name in ("small_direct_alpha254", "small_lists_alpha254", "small_direct_no_clear", "small_lists_no_clear", "small_direct_folded_155",
                 "small_lists_folded_155"):
        assert (on[name][..., 3] != 255).any(), name


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [5, 18])
def test_both_blur_routes_give_the_same_bytes_with_the_switch_on_and_off(both, radius):
    on, off = both
    ref = on[f"blur_r{radius}_route1"]
    for frames in (on, off):
        for route in (0, 1):
            assert np.array_equal(frames[f"blur_r{radius}_route{route}"], ref), (radius, route, frames is on)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
def test_stripes_of_the_blurred_frame_equal_the_whole_frame(both, route):
    on, off = both
    for frames in (on, off):
        assert np.array_equal(frames[f"blur_r18_route{route}_stripes"], on[f"blur_r18_route{route}"]), (route, frames is on)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_match_the_oracle(both, name):
    from oracle import oracle as O

    build, args, w, h, clear, _, _ = CASES[name]
    key = (build.__name__, args, clear)  # (the two routes of a blurred frame share their reference)
    if key not in _ORACLE:
        orc = O.Oracle(threads=8)
        orc.render_frame(build(*args), w, h, color=clear)
        _ORACLE[key] = orc.read_pixels().copy()
    mx, n0, n1 = diff_stats(both[0][name], _ORACLE[key])
    assert mx <= 1 and n0 <= 0.005 * w * h, (name, "vs oracle", mx, n0, n1)
