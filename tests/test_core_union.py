"""The saturated core as a union of rectangles changes no byte.  With FDH_CORE_UNION=1 (the default) a draw's BinRec carries, beside
DrawRec's own core rectangle, the full-width and the full-height band between the corner cells, and the bin launch (or a direct
launch's own entry making) marks the strips inside any of the three as core strips; FDH_CORE_UNION=0 leaves the one rectangle.  A
core strip is one where coverage is saturated, which is exactly what the per-pixel paths would have computed there, so every frame
below must come out byte for byte the same from two fresh child processes, one per setting (the switch is read once per process), and
within the suite's bar of the oracle (at most 1 LSB on at most 0.5 % of the pixels).

Frames of 256 x 192 and 200 x 136 (no multiples of the 64-px bin): a dozen rounded rectangles whose bands and corner cells straddle
strip and bin boundaries -- radius 0, radius 30 on a 100 x 70 box, four different radii, elliptical corners with ry = 2 rx, strokes
of 5, translucent and opaque fills, a drop shadow with blur 12 / spread 10, an inner shadow with an offset, a rectangle partly off
the left and top edge --, once as a frame of at most 64 draws (a direct launch), once as several shifted copies (binned into lists),
each with and without a clipped child (the build with masks); the lists frame again as two row stripes, and the clipped direct frame
again as a retained scene (spliced records carry the BinRec).  That the switch does something is shown on the device by the bin
lists' digest, which must differ between the two settings for the binned frames, and by the CPU restatement of the rule
(tools/core_strip_count.py), which must predict fewer edge strips with the union for every frame."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import diff_stats

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLEAR = (0.2, 0.4, 0.9, 1.0)


def nodes(dx=0.0, dy=0.0, clip=False):
    from figdraw_amd.scene import Fig, FigFlags, FigKind, RenderList, RenderShadow, RenderStroke, ShadowStyle, fill, rect, rgba

    R = FigKind.nkRectangle
    lst = RenderList()
    add = lst.addRoot
    add(Fig(kind=R, screenBox=rect(5.5 + dx, 4.25 + dy, 90, 50), fill=rgba(220, 40, 40, 155)))  # radius 0
    add(Fig(kind=R, screenBox=rect(70.3 + dx, 10.6 + dy, 100, 70), fill=rgba(40, 180, 90, 255), corners=[30] * 4))  # opaque, r = 30
    add(Fig(kind=R, screenBox=rect(20.75 + dx, 90.5 + dy, 120, 80), fill=rgba(60, 90, 220, 155), corners=[4, 26, 12, 18],
            stroke=RenderStroke(weight=5.0, fill=fill(rgba(0, 0, 0, 155)))))
    add(Fig(kind=R, screenBox=rect(130.2 + dx, 60.4 + dy, 110, 90), fill=rgba(238, 140, 30, 220), corners=[6, 10, 14, 8],
            cornerRadiiY=[12, 20, 28, 16], flags=FigFlags.NfEllipticalCorners, stroke=RenderStroke(weight=5.0, fill=fill(rgba(90, 45, 0, 220)))))
    add(Fig(kind=R, screenBox=rect(150 + dx, 100.5 + dy, 90, 60), fill=rgba(250, 250, 250, 200), corners=[14] * 4,
            shadows=[RenderShadow(style=ShadowStyle.DropShadow, blur=12.0, spread=10.0, x=-5.0, y=4.0, fill=fill(rgba(0, 0, 0, 155)))]))
    add(Fig(kind=R, screenBox=rect(10.5 + dx, 50.5 + dy, 100, 80), fill=rgba(118, 168, 255, 140), corners=[9] * 4,
            shadows=[RenderShadow(style=ShadowStyle.InnerShadow, blur=4.0, spread=1.0, x=3.0, y=-2.0, fill=fill(rgba(40, 40, 60, 150)))]))
    add(Fig(kind=R, screenBox=rect(-30.5 + dx, -20.25 + dy, 120, 90), fill=rgba(255, 225, 55, 120), corners=[30] * 4,
            stroke=RenderStroke(weight=5.0, fill=fill(rgba(95, 72, 0, 185)))))  # partly off the left and top edge
    add(Fig(kind=R, screenBox=rect(40.5 + dx, 150.25 + dy, 180, 40), fill=rgba(200, 30, 160, 180), corners=[20] * 4))  # a pill
    add(Fig(kind=R, screenBox=rect(64 + dx, 64 + dy, 100, 70), fill=rgba(20, 160, 70, 130), corners=[30] * 4,
            stroke=RenderStroke(weight=5.0, fill=fill(rgba(255, 255, 255, 210)))))  # on a bin corner
    add(Fig(kind=R, screenBox=rect(200.4 + dx, 6.6 + dy, 44, 120), fill=rgba(30, 30, 30, 255), corners=[22, 22, 5, 0],
            cornerRadiiY=[44, 44, 10, 0], flags=FigFlags.NfEllipticalCorners))  # opaque, elliptical, taller than wide
    add(Fig(kind=R, screenBox=rect(100.5 + dx, 30.5 + dy, 20, 20), fill=rgba(255, 255, 255, 200), corners=[10] * 4))  # a disc: no band
    if clip:
        outer = add(Fig(kind=R, screenBox=rect(120.5 + dx, 20.5 + dy, 100, 70), fill=rgba(220, 220, 230, 200), corners=[20, 8, 30, 12],
                        flags=FigFlags.NfClipContent))
        lst.addChild(outer, Fig(kind=R, screenBox=rect(100 + dx, 40 + dy, 150, 40), fill=rgba(43, 159, 234, 200), corners=[10] * 4))
    return lst


def tree(copies, clip, dx=0.0, dy=0.0):
    from figdraw_amd.scene import Renders

    lst = nodes(dx, dy, clip)
    for c in range(1, copies):
        more = nodes(dx + 7.3 * c, dy + 4.6 * c, False)
        for n in more.nodes:
            lst.addRoot(n)
    out = Renders()
    out.setLayer(0, lst)
    return out


# name -> (copies, clipped child, dx, dy, w, h)
CASES = {
    "direct": (1, False, -28.0, -20.0, 200, 136),
    "direct_clip": (1, True, 0.0, 0.0, 256, 192),
    "lists": (4, False, 0.0, 0.0, 256, 192),
    "lists_clip": (4, True, -28.0, -20.0, 200, 136),
}
STRIPES = ((0, 104), (104, 192))
NAMES = sorted(list(CASES) + ["lists_stripes", "direct_clip_retained"])
_ORACLE = {}


def render_all():
    """every frame of this file on one device: name -> pixels, and name -> the bin lists' digest (hash, entries)"""
    from figdraw_amd.context import HipContext

    frames, digests = {}, {}
    for name, (copies, clip, dx, dy, w, h) in CASES.items():
        sc = tree(copies, clip, dx, dy)
        ctx = HipContext(device=0)
        ctx.render_frame(sc, w, h, color=CLEAR)
        frames[name] = ctx.read_pixels().copy()
        digests[name] = [int(v) for v in ctx.bin_digest()[:2]]
        if name == "lists":
            whole = np.zeros_like(frames[name])
            for y0, y1 in STRIPES:
                ctx.set_stripe(y0, y1)
                ctx.render_frame(sc, w, h, color=CLEAR)
                whole[y0:y1] = ctx.read_pixels()[y0:y1]
            ctx.set_stripe(0, 0)
            frames["lists_stripes"] = whole
        if name == "direct_clip":
            ctx.scene_retain(sc, w, h, color=CLEAR)
            ctx.scene_render()
            frames["direct_clip_retained"] = ctx.read_pixels().copy()
        ctx.close()
    return frames, digests


@pytest.fixture(scope="module")
def both():
    """(frames, digests) of a child process with FDH_CORE_UNION=1 and of one with FDH_CORE_UNION=0"""
    code = ("import sys, json, numpy as np\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_core_union as T\n"
            "frames, digests = T.render_all()\n"
            "np.savez(sys.argv[1], **frames)\n"
            "json.dump(digests, open(sys.argv[2], 'w'))\n") % (ROOT, HERE)
    out = []
    with tempfile.TemporaryDirectory() as td:
        for v in ("1", "0"):
            path, dpath = os.path.join(td, f"u{v}.npz"), os.path.join(td, f"u{v}.json")
            subprocess.check_call([sys.executable, "-c", code, path, dpath], env=dict(os.environ, FDH_CORE_UNION=v))
            with open(dpath) as f:
                out.append((dict(np.load(path)), json.load(f)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_switch_changes_no_byte(both, name):
    (on, _), (off, _) = both
    assert on[name].shape == off[name].shape
    assert np.array_equal(on[name], off[name]), (name, int((on[name] != off[name]).any(axis=2).sum()), "pixels differ")


@pytest.mark.gpu
def test_stripes_and_the_retained_scene_equal_the_whole_frame(both):
    for frames, _ in both:
        assert np.array_equal(frames["lists_stripes"], frames["lists"])
        assert np.array_equal(frames["direct_clip_retained"], frames["direct_clip"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_match_the_oracle(both, name):
    from oracle import oracle as O

    copies, clip, dx, dy, w, h = CASES[name]
    if name not in _ORACLE:
        orc = O.Oracle(threads=8)
        orc.render_frame(tree(copies, clip, dx, dy), w, h, color=CLEAR)
        _ORACLE[name] = orc.read_pixels().copy()
    for frames, _ in both:
        mx, n0, n1 = diff_stats(frames[name], _ORACLE[name])
        assert mx <= 1 and n0 <= 0.005 * w * h, (name, "vs oracle", mx, n0, n1)


@pytest.mark.gpu
def test_strips_change_class(both):
    """the binned frames' lists differ between the two settings (the digest hashes every entry's strip words), and no entry appears:
    removed cores can only shrink the lists"""
    (_, on), (_, off) = both
    for name in ("lists", "lists_clip"):
        assert on[name][0] != off[name][0], (name, on[name], off[name])
        assert 0 < on[name][1] <= off[name][1], (name, on[name], off[name])


def test_the_cpu_count_predicts_fewer_edge_strips_for_every_frame():
    """(no GPU) tools/core_strip_count.py on the frames above: the union turns edge strips into core strips in each of them, and
    in every draw class the sweep of shapes is meant to reach"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import core_strip_count as CS

    for name, (copies, clip, dx, dy, w, h) in CASES.items():
        tot = CS.count_frame(tree(copies, clip, dx, dy), w, h)
        one, union = sum(v[1] for v in tot.values()), sum(v[2] for v in tot.values())
        assert union < one, (name, tot)
        if copies > 1:
            for cls in ("fill, elliptical", "stroke, elliptical", "fill, circular", "stroke, circular", "drop shadow"):
                assert tot[cls][2] < tot[cls][1], (name, cls, tot[cls])
