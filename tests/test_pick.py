"""Picking on the GPU (include/figdraw_hip_pick.h, k_pick.hip): which draw, and which node, owns a pixel of the last submitted frame.

  - exact against the oracle's arithmetic: every draw of a scene's call stream replayed alone on the oracle (transparent-black clear, every
    transform and mask call kept) gives A_k = rint(255 a_k) per pixel; the expected hits at threshold t are the non-shadow draws with
    A_k >= t, front to back.  Pixels where a draw that can decide the answer has A_k = t - 1 or t are left out: the 1-LSB band within
    which the kernels and the oracle may round differently.  Caps on that share are asserted.
  - known answers where the reference's debugtools are approximate (rounded corners, rotation, rounded clips, partial cover, glyph
    margins), untagged draws, points off the frame, stripes;
  - the same answers whatever route the frame took (direct / binned, clear folded or not, damage-tracked partial frames, fdh_replay,
    contexts in flight)."""
import math
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import ref_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRAW_CALLS = ("draw_rounded_rect_sdf", "draw_image", "draw_msdf", "draw_quadratic_bezier_sdf", "draw_filled_quad", "draw_rect", "draw_image_adj",
              "draw_backdrop_blur")
STATE_CALLS = ("save_transform", "restore_transform", "translate", "rotate", "scale", "apply_transform", "set_aa_factor", "set_text_subpixel_shift",
               "begin_mask", "end_mask", "pop_mask", "begin_rect_mask", "pop_rect_mask")
WHITE = [255, 255, 255, 255]


def draw_records(calls):
    """(call index, record index, is_shadow) of every draw call of a recorded stream, in painter's order, and the frame's record count.
    Records: one per draw call and per clip / rect-mask begin and end; a backdrop blur (radius > 0.5) first re-opens the clips open
    around it, as records of the phase it starts."""
    out, r, open_ops = [], 0, 0
    for ci, c in enumerate(calls):
        name = c[0]
        if name in ("begin_mask", "begin_rect_mask"):
            r += 1; open_ops += 1
        elif name in ("pop_mask", "pop_rect_mask"):
            r += 1; open_ops -= 1
        elif name in DRAW_CALLS:
            if name == "draw_backdrop_blur" and c[4] > 0.5 and c[1][2] > 0 and c[1][3] > 0:
                r += open_ops
            shadow = name == "draw_rounded_rect_sdf" and 7 <= c[5] <= 10
            out.append((ci, r, shadow))
            r += 1
    return out, r


def oracle_alphas(calls, w, h, images=None, atlas_size=1024):
    """A[k] = the oracle's alpha channel (h, w) with draw call k alone over a transparent-black clear, every transform and mask call of the
    stream kept; a backdrop blur's composite replayed as a white mode-3 rounded rect over its rect and radii (its coverage)"""
    from oracle import oracle as O

    o = O.Oracle(atlas_size=atlas_size, threads=8)
    for k, v in (images or {}).items():
        o.put_image(k, v)
    o.W, o.H = w, h
    draws, _ = draw_records(calls)
    state = [c[0] in STATE_CALLS for c in calls]
    out = np.zeros((len(draws), h, w), np.uint8)
    for k, (ci, _, _) in enumerate(draws):
        d = calls[ci]
        if d[0] == "draw_backdrop_blur":
            d = ["draw_rounded_rect_sdf", d[1], [WHITE] * 4, d[2], d[3], 3, 4.0, 0.0, [0, 0], 0, [0, 0, 0, 0], [0, 0, 0, 0], 0.5]
        seq = [["begin_frame", 1, [0, 0, 0, 0]]] + [c for j, c in enumerate(calls[:ci]) if state[j]] + [d]
        seq += [c for j, c in enumerate(calls[ci + 1:], start=ci + 1) if state[j]] + [["end_frame"]]
        o.replay(seq)
        out[k] = o.read_pixels()[..., 3]
    o.close()
    return out


def expectation(A, draws, t, shadows=False):
    """per pixel: the expected top hit (record index, -1 for none) and the two exclusion masks (top hit, full list)"""
    K = A.shape[0]
    ridx = np.array([r for _, r, _ in draws], np.int64)
    considered = np.array([shadows or not s for _, _, s in draws], bool)
    ok = (A >= t) & considered[:, None, None]
    band = ((A == t - 1) | (A == t)) & considered[:, None, None]
    rev = ok[::-1]
    has = rev.any(0)
    pos = K - 1 - rev.argmax(0)
    top = np.where(has, ridx[pos], -1)
    front = np.arange(K)[:, None, None] >= np.where(has, pos, 0)[None]
    return top, (band & front).any(0), band.any(0), ok, ridx


def band_shares(A, draws, t, shadows=False):
    _, ex_top, ex_list, _, _ = expectation(A, draws, t, shadows)
    return float(ex_top.mean()), float(ex_list.mean())


def _images():
    from conftest import GOLDEN
    from figdraw_amd.scenes import load_glyph_fixture

    return load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz"))


# name: (builder(images), w, h, needs the glyph fixture)
SCENES = {
    "nested_clips": (lambda im: RS.nested_clips(), 320, 240, False),
    "deep_clips_24": (lambda im: RS.deep_clips(depth=24), 400, 300, False),
    "rect_mask_nested": (lambda im: RS.rect_mask_nested(), 320, 240, False),
    "backdrop_blur": (lambda im: RS.backdrop_blur(), 320, 240, False),
    "rotation_and_transform": (lambda im: RS.rotation_and_transform(), 320, 240, False),
    "drawables": (lambda im: RS.drawables(), 420, 300, False),
    "elliptical_and_fractional": (lambda im: RS.elliptical_and_fractional(), 320, 240, False),
    "layers_clip": (lambda im: RS.layers_clip(800.0, 375.0), 800, 375, False),
    "rgb_boxes_sdf": (lambda im: RS.rgb_boxes_sdf(), 800, 600, False),
    "random_scene_3": (lambda im: RS.random_scene(3, 400.0, 300.0), 400, 300, False),
    # beyond the scenes the issue measured (their band shares checked against the caps on the CPU first: tools/pick_bench.py --bands)
    "deep_clips_40": (lambda im: RS.deep_clips(depth=40), 400, 300, False),
    "curves": (lambda im: RS.curves(), 640, 420, False),
    "images_and_msdf_variants": (lambda im: RS.images_and_msdf_variants(images=im), 360, 260, True),
    "text_frontend": (lambda im: RS.text_frontend(images=im), 300, 120, True),
}
TOP_THRESHOLDS = (128, 64)
LIST_THRESHOLD = 64  # (at 128, random_scene(3)'s translucent fills put whole areas in the band behind the top hit: 2.8 % of its pixels)
TOP_CAP, LIST_CAP = 0.005, 0.01


def scene_stream(name):
    """the scene, its frame size, its images, and its call stream as a record-only context records it with culling off"""
    from figdraw_amd.context import HipContext

    fn, w, h, needs = SCENES[name]
    images = _images() if needs else None
    sc = fn(images)
    used = RS.used_images(sc, images) if images else {}
    rec = HipContext(record_only=True)
    for k, v in used.items():
        rec.put_image(k, v)
    rec.set_cull(0)
    rec.record_begin()
    rec.render_frame(sc, w, h)
    calls = rec.record_calls()
    rec.close()
    return sc, w, h, used, calls


def _picking_ctx(sc, w, h, used, **kw):
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=1024, device=0, **kw)
    for k, v in used.items():
        ctx.put_image(k, v)
    ctx.set_cull(0)
    ctx.set_pick(True)
    ctx.render_frame(sc, w, h)
    return ctx


def check_against_oracle(name, shadows=False):
    sc, w, h, used, calls = scene_stream(name)
    draws, n_recs = draw_records(calls)
    A = oracle_alphas(calls, w, h, used)
    ctx = _picking_ctx(sc, w, h, used)
    tags = ctx.pick_draw_tags()
    assert len(tags) == n_recs, (name, len(tags), n_recs)
    flags = ctx.PICK_SHADOWS if shadows else 0
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pts = rng.uniform((0.0, 0.0), (float(w), float(h)), size=(2000, 2)).astype(np.float32)
    px, py = np.floor(pts[:, 0]).astype(int), np.floor(pts[:, 1]).astype(int)
    report = []
    for t in TOP_THRESHOLDS:
        top, ex_top, _, _, _ = expectation(A, draws, t, shadows)
        got = ctx.pick_region(threshold=t, flags=flags)
        share = float(ex_top.mean())
        bad = (got != top) & ~ex_top
        report.append(f"{name} t={t}: top hit left out {100 * share:.3f} %, wrong {int(bad.sum())}")
        print(report[-1])
        assert share <= TOP_CAP, report[-1]
        assert not bad.any(), (report[-1], np.argwhere(bad)[:5].tolist(), got[bad][:5].tolist(), top[bad][:5].tolist())
    t = LIST_THRESHOLD
    _, _, ex_list, ok, ridx = expectation(A, draws, t, shadows)
    share = float(ex_list.mean())
    hits, counts = ctx.pick_points(pts, threshold=t, flags=flags, max_hits=16)
    wrong = 0
    for i in range(len(pts)):
        x, y = px[i], py[i]
        want = ridx[np.nonzero(ok[:, y, x])[0][::-1]][:16].tolist()
        got = hits[i, :counts[i]]
        assert all(tuple(tags[d]) == (z, n) for d, z, n in zip(got["draw"], got["zlevel"], got["id"])), (name, i)
        ks = {r: k for k, (_, r, _) in enumerate(draws)}
        assert all(abs(int(a) - int(A[ks[d], y, x])) <= 1 for d, a in zip(got["draw"], got["alpha"])), (name, i)
        if ex_list[y, x]:
            continue
        if got["draw"].tolist() != want:
            wrong += 1
    report.append(f"{name} t={t}: full list left out {100 * share:.3f} %, wrong points {wrong} of {len(pts)}")
    print(report[-1])
    assert share <= LIST_CAP, report[-1]
    assert wrong == 0, report[-1]
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_pick_matches_the_oracle(name):
    check_against_oracle(name)


@pytest.mark.gpu
def test_pick_with_shadows_matches_the_oracle():
    """FDH_PICK_SHADOWS: drop and inset shadows count as hits (random_scene(3) has both)"""
    check_against_oracle("random_scene_3", shadows=True)


@pytest.mark.gpu
def test_blur_composite_substitute_has_the_blur_quads_coverage():
    """The oracle check replays a backdrop blur's composite as a white mode-3 rounded rect over the same rect and radii: a frame of the blur
    quad alone and a frame of that rect alone pick the same pixels at every threshold (same bounds, same AA factor, same coverage)."""
    from figdraw_amd.context import HipContext

    rect, rx = (37.3, 21.6, 150.2, 97.9), (18.0, 6.0, 30.0, 12.0)
    maps = []
    for blur in (True, False):
        ctx = HipContext(device=0)
        ctx.set_pick(True)
        ctx.begin_frame(256, 160, True, (0.0, 0.0, 0.0, 0.0))
        if blur:
            ctx.draw_backdrop_blur(rect, rx, rx, 9.0)
        else:
            ctx.draw_rounded_rect_sdf(rect, [WHITE] * 4, rx, rx, 3)
        ctx.end_frame()
        maps.append([ctx.pick_region(threshold=t) for t in (1, 64, 128, 200, 255)])
        ctx.close()
    for a, b in zip(*maps):
        assert np.array_equal(a, b)
    assert (maps[0][2] == 0).sum() > 10000


# ---- known answers where the reference's debugtools are approximate
def _panel_ctx(w=200, h=150):
    from figdraw_amd.context import HipContext

    ctx = HipContext(device=0)
    ctx.set_pick(True)
    ctx.begin_frame(w, h)
    ctx.set_pick_tag(0, 1)
    ctx.draw_rect((0.0, 0.0, float(w), float(h)), (200, 200, 200, 255))  # the panel: record 0
    return ctx


def _top(ctx, x, y, t=128):
    hits, counts = ctx.pick_points([(x, y)], threshold=t, max_hits=1)
    return (int(hits[0, 0]["zlevel"]), int(hits[0, 0]["id"]), int(hits[0, 0]["draw"])) if counts[0] else None


@pytest.mark.gpu
def test_known_answers():
    # a rounded button: inside its bounds, outside its corner arc (distance to the arc centre > radius + 1) -> the panel beneath
    ctx = _panel_ctx()
    ctx.set_pick_tag(0, 2)
    ctx.draw_rounded_rect_sdf((40.0, 40.0, 100.0, 60.0), [[30, 60, 200, 255]] * 4, (20.0,) * 4, (20.0,) * 4, 3)
    # a card rotated by 30 degrees about its centre (90, 110)
    ctx.set_pick_tag(0, 3)
    ctx.save_transform()
    ctx.translate(150.0, 110.0)
    ctx.rotate(math.radians(30.0))
    ctx.translate(-150.0, -110.0)
    ctx.draw_rect((130.0, 95.0, 40.0, 30.0), (200, 40, 40, 255))
    ctx.restore_transform()
    # a 30 %-alpha overlay (rint(255 * 0.3) = 77): hit at t = 64, not at t = 128
    ctx.set_pick_tag(0, 4)
    ctx.draw_rect((5.0, 120.0, 30.0, 25.0), (0, 0, 0, 77))
    # an untagged draw occludes
    ctx.set_pick_tag(-1, -1)
    ctx.draw_rect((170.0, 5.0, 25.0, 25.0), (0, 255, 0, 255))
    ctx.end_frame()
    assert _top(ctx, 90.0, 70.0) == (0, 2, 1)        # the button's middle
    x, y = 41.5, 41.5                                # its top-left corner cut-out: the arc centre is (60, 60), radius 20
    assert math.hypot(60.0 - (x + 0.0), 60.0 - (y + 0.0)) > 21.0
    assert _top(ctx, x, y) == (0, 1, 0)
    assert _top(ctx, 150.0, 110.0) == (0, 3, 2)      # the card's centre
    # near a corner of the card's bounding box (half extents 20 cos 30 + 15 sin 30 = 24.8 by 23.0), more than a pixel outside the card: the
    # pixel centre in the card's own frame (either sense of rotation puts it there)
    bx, by = 150.0 + 22.0, 110.0 + 21.0
    assert abs(bx + 0.5 - 150.0) < 24.8 and abs(by + 0.5 - 110.0) < 23.0
    a = math.radians(30.0)
    lx = math.cos(a) * (bx + 0.5 - 150.0) + math.sin(a) * (by + 0.5 - 110.0)
    ly = -math.sin(a) * (bx + 0.5 - 150.0) + math.cos(a) * (by + 0.5 - 110.0)
    assert max(abs(lx) - 20.0, abs(ly) - 15.0) > 1.0
    assert _top(ctx, bx, by) == (0, 1, 0)
    assert _top(ctx, 20.0, 130.0, t=64) == (0, 4, 3)
    assert _top(ctx, 20.0, 130.0, t=128) == (0, 1, 0)
    assert _top(ctx, 180.0, 15.0) == (-1, -1, 4)
    hits, counts = ctx.pick_points([(180.0, 15.0)], threshold=128, max_hits=16)
    assert counts[0] == 2 and hits[0, 1]["id"] == 1  # the panel behind the untagged draw, second
    # points outside the frame: no hits, no error
    hits, counts = ctx.pick_points([(-0.5, 10.0), (200.0, 10.0), (10.0, 150.0), (10.0, -3.0), (float("nan"), 1.0)], max_hits=4)
    assert counts.tolist() == [0] * 5
    region = ctx.pick_region(-2, -2, 4, 4)
    assert (region[:2, :] == -1).all() and (region[:, :2] == -1).all() and (region[2:, 2:] == 0).all()
    ctx.close()

    # a child clipped by its parent's rounded clip is not hit in the clip's corner
    ctx = _panel_ctx()
    ctx.set_pick_tag(0, 5)
    ctx.begin_mask((50.0, 30.0, 100.0, 80.0), (30.0,) * 4, (30.0,) * 4)
    ctx.end_mask()
    ctx.set_pick_tag(0, 6)
    ctx.draw_rect((40.0, 20.0, 120.0, 100.0), (10, 10, 10, 255))
    ctx.set_pick_tag(0, 5)
    ctx.pop_mask()
    ctx.end_frame()
    assert _top(ctx, 100.0, 70.0) == (0, 6, 2)
    assert math.hypot(80.0 - 52.5, 60.0 - 32.5) > 31.0
    assert _top(ctx, 52.0, 32.0) == (0, 1, 0)
    assert _top(ctx, 45.0, 70.0) == (0, 1, 0)  # outside the clip, inside the child's rect
    ctx.close()


@pytest.mark.gpu
def test_glyph_quad_is_hit_on_ink_not_in_its_margin():
    from figdraw_amd.context import HipContext

    img = np.zeros((32, 32, 4), np.uint8)
    img[8:24, 8:24] = 255  # ink in the middle, a transparent margin of 8 texels
    ctx = HipContext(device=0)
    ctx.put_image(7, img)
    ctx.set_pick(True)
    ctx.begin_frame(100, 80, True, (0.0, 0.0, 0.0, 0.0))
    ctx.set_pick_tag(2, 9)
    ctx.draw_image(7, (20.0, 10.0), [[0, 0, 0, 255]] * 4, (32.0, 32.0))
    ctx.end_frame()
    assert _top(ctx, 36.0, 26.0) == (2, 9, 0)
    assert _top(ctx, 22.0, 12.0) is None and _top(ctx, 49.0, 40.0) is None
    ctx.close()


@pytest.mark.gpu
def test_stripe_rows_outside_the_stripe_are_refused():
    from figdraw_amd.context import FigdrawHipError, HipContext

    sc = RS.random_scene(3, 400.0, 300.0)
    ctx = HipContext(device=0)
    ctx.set_stripe(100, 200)
    ctx.set_pick(True)
    ctx.render_frame(sc, 400, 300)
    hits, counts = ctx.pick_points([(50.0, 150.0)], max_hits=4)
    assert counts[0] >= 1
    assert ctx.pick_region(0, 100, 400, 100).shape == (100, 400)
    for call in (lambda: ctx.pick_points([(50.0, 150.0), (50.0, 99.0)]), lambda: ctx.pick_region(0, 150, 10, 51)):
        with pytest.raises(FigdrawHipError) as e:
            call()
        assert e.value.code == -1  # FDH_ERR_INVALID
    ctx.close()


@pytest.mark.gpu
def test_queries_need_a_picking_frame():
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(device=0)
    ctx.render_frame(RS.nested_clips(), 320, 240)
    with pytest.raises(FigdrawHipError):
        ctx.pick_region()
    with pytest.raises(FigdrawHipError):
        ctx.pick_points([(1.0, 1.0)])
    ctx.set_pick(True)
    ctx.render_frame(RS.nested_clips(), 320, 240)
    assert (ctx.pick_region() >= 0).all()
    assert ctx.top_node_at(5.0, 5.0) == (0, 0)
    vis = ctx.visible_pixels()
    assert sum(vis.values()) == 320 * 240 and vis[(0, 0)] > 0
    ctx.close()


# ---- every route gives the same answers
_ROUTE_PTS = np.random.default_rng(5).uniform((0.0, 0.0), (400.0, 300.0), size=(3000, 2)).astype(np.float32)


def _answers(ctx):
    out = [ctx.pick_region(threshold=t) for t in (64, 128)]
    hits, counts = ctx.pick_points(_ROUTE_PTS, threshold=64, max_hits=16)
    return out + [hits["draw"] * (np.arange(16)[None] < counts[:, None]) - (np.arange(16)[None] >= counts[:, None]), counts]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


ROUTE_SCENES = {"few_draws": lambda: RS.nested_clips(400.0, 300.0), "random": lambda: RS.random_scene(3, 400.0, 300.0)}

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_pick as T
from figdraw_amd.context import HipContext
ctx = HipContext(device=0)
ctx.set_pick(True)
ctx.render_frame(T.ROUTE_SCENES[sys.argv[3]](), 400, 300)
np.savez(sys.argv[2], *T._answers(ctx))
print("child: OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["FDH_DIRECT", "FDH_FOLD_CLEAR"])
def test_direct_and_binned_folded_and_unfolded_frames_pick_alike(env, tmp_path):
    """the same frame (a few draws: direct; and a larger one) in this process and in a child with FDH_DIRECT=0 (binned) / FDH_FOLD_CLEAR=0"""
    from figdraw_amd.context import HipContext

    for key, fn in ROUTE_SCENES.items():
        ctx = HipContext(device=0)
        ctx.set_pick(True)
        ctx.render_frame(fn(), 400, 300)
        here = _answers(ctx)
        st = ctx.frame_stats()
        if env == "FDH_FOLD_CLEAR" and key == "random":
            assert st.clear_folded == 1.0  # (its first draw is an opaque full-frame panel)
        ctx.close()
        out = tmp_path / f"{key}.npz"
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out), key], env=dict(os.environ, **{env: "0"}), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0 and "child: OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        z = np.load(out)
        _same(here, [z[f"arr_{i}"] for i in range(len(here))])


@pytest.mark.gpu
def test_damage_tracked_replayed_and_in_flight_frames_pick_alike():
    from figdraw_amd.context import HipContext
    from figdraw_amd.scene import fill, rgba

    scenes = [RS.random_scene(s, 400.0, 300.0, n=30) for s in (11, 12, 13, 14)]
    want = []
    for sc in scenes:
        f = HipContext(device=0)
        f.set_pick(True)
        f.render_frame(sc, 400, 300)
        want.append(_answers(f))
        f.close()
    # damage tracking: frame 11, the same again (nothing composited), 12, 11, then 11 with one node's fill changed (a partial frame)
    t = HipContext(device=0)
    t.set_damage_tracking(True)
    t.set_pick(True)
    sc2 = RS.random_scene(11, 400.0, 300.0, n=30)
    next(iter(sc2.layers.values())).nodes[-1].fill = fill(rgba(1, 2, 3, 255))
    for sc, w in ((scenes[0], want[0]), (scenes[0], want[0]), (scenes[1], want[1]), (scenes[0], want[0])):
        t.render_frame(sc, 400, 300)
        _same(_answers(t), w)
    t.render_frame(sc2, 400, 300)
    assert not t.damage_bins().all()  # a partial frame
    f = HipContext(device=0)
    f.set_pick(True)
    f.render_frame(sc2, 400, 300)
    _same(_answers(t), _answers(f))
    f.close()
    # fdh_replay of the last frame
    before = _answers(t)
    t.replay(3)
    _same(_answers(t), before)
    t.close()
    # four contexts in flight
    ctxs = [HipContext(device=0) for _ in scenes]
    for c in ctxs:
        c.set_pick(True)
    for _ in range(3):
        for c, sc in zip(ctxs, scenes):
            c.render_frame(sc, 400, 300)
    for c, w in zip(ctxs, want):
        _same(_answers(c), w)
        c.close()
