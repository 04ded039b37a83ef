"""CPU suite: what a frame records is what the commit before RecordedFrame / FrameEnv / CallLog recorded.

tests/golden/recorded_frame_pins.json was written by tools/make_recorded_frame_pins.py from the library of that commit (the file names
it); every case here replays on the tree's library and must give the same answers through the C ABI: the record digest after each
frame, the sha256 of record_json where the call recorder runs, culled_draws, walk_stats' group count, the pick tag table where
picking is on, and for refusals the code and the message.  Record-only contexts: no GPU.  Each case sits on a path the move touched
(lane sets in rotation, the join of a sibling group, consolidate_pieces, the SerialOnly fallback, binbox_shift, the reopen path of a
blur under open clips, the call log's pause and take-back, cull rows under a stripe, a retained scene's splices, refusals)."""
import hashlib
import json
import os

import numpy as np
import pytest

import ref_scenes as RS
from figdraw_amd import scene as S
from figdraw_amd.context import FigdrawHipError, HipContext
from figdraw_amd.scenes import make_clip_mask_benchmark, make_non_clip_benchmark, make_render_tree_100
from test_parallel_walk import _wide_scene

PIN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recorded_frame_pins.json")
Z4 = [0.0] * 4


def snap(ctx, tags=False):
    out = {"digest": f"{ctx.record_digest():016x}", "culled": ctx.culled_draws(), "groups": ctx.walk_stats()[1]}
    if tags:
        t = ctx.pick_draw_tags()
        out["tags"] = [len(t), hashlib.sha256(np.ascontiguousarray(t, dtype=np.int32).tobytes()).hexdigest()]
    return out


def frames(scene, w, h, threads, cull=1, n=2, ui_scale=1.0):
    ctx = HipContext(record_only=True)
    ctx.set_cull(cull)
    ctx.set_walk_threads(threads)
    out = []
    for _ in range(n):  # (more than one frame: the lane sets rotate, pool threads and their recorders are used again)
        ctx.render_frame(scene, w, h, ui_scale=ui_scale)
        out.append(snap(ctx))
    ctx.close()
    return out


def refusal(fn):
    try:
        fn()
    except FigdrawHipError as e:
        return [e.code, str(e)]
    return None


def one_rect_scene():
    sc = S.Renders()
    sc.setLayer(0, S.RenderList())
    sc.layers[0].addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(1, 1, 20, 20), fill=S.rgba(1, 2, 3, 255)))
    return sc


def rects_scene(n, w, h, seed=11, blurs=()):
    """n random rounded rects; blurs: (x, y, w, h, radius) backdrop-blur roots, placed after the rects at thirds of the list"""
    rng = np.random.default_rng(seed)
    lst = S.RenderList()
    at = {(k + 1) * n // (len(blurs) + 1): b for k, b in enumerate(blurs)}
    for k in range(n + 1):
        if k in at:
            x, y, bw, bh, r = at[k]
            lst.addRoot(S.Fig(kind=S.FigKind.nkBackdropBlur, screenBox=S.rect(x, y, bw, bh), blur=r, corners=[4] * 4, fill=S.rgba(255, 255, 255, 40)))
        if k == n:
            break
        x, y = float(rng.uniform(-10, w - 10)), float(rng.uniform(-10, h - 10))
        lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(x, y, float(rng.uniform(6, 70)), float(rng.uniform(6, 50))), corners=[k % 7] * 4,
                          fill=S.rgba(int(rng.integers(0, 255)), int(rng.integers(0, 255)), 160, 255 if k % 3 else 180),
                          stroke=S.RenderStroke(weight=1.5 if k % 4 == 0 else 0.0, fill=S.fill(S.rgba(0, 0, 0, 220)))))
    sc = S.Renders()
    sc.setLayer(0, lst)
    return sc


def consolidate_scene(w=800, h=600):
    lst = S.RenderList()
    for g in range(14):  # 14 parents x 60 children: 14 forked groups in one frame (test_many_groups_in_one_frame_consolidate)
        parent = lst.addRoot(S.Fig(kind=S.FigKind.nkFrame, screenBox=S.rect(0, 40.0 * g, w, 40)))
        for k in range(60):
            lst.addChild(parent, S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(12.0 * k, 40.0 * g + 4, 10, 30), corners=[2] * 4,
                                       fill=S.rgba((k * 37) & 255, (g * 53) & 255, 90, 255)))
    sc = S.Renders()
    sc.setLayer(0, lst)
    return sc


def drawable_scene():
    lst = S.RenderList()
    for k in range(120):
        lst.addRoot(S.Fig(kind=S.FigKind.nkDrawable, screenBox=S.rect(5.0 * k, 10.0, 40, 40), drawStroke=S.RenderStroke(weight=3.0, fill=S.fill(S.rgba(10, 20, 30, 255)), join=S.StrokeJoin.sjMiter, cap=S.StrokeCap.scButt),
                          drawOps=[S.drawableBezier([(0, 0), (40, 40), (0, 40), (40, 0), (5, 30)], steps=2)]))
    sc = S.Renders()
    sc.setLayer(0, lst)
    return sc


def deep_scene():
    lst = S.RenderList()
    for k in range(100):
        lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(3.0 * k, 3.0, 20, 20), fill=S.rgba(1, 2, 3, 255)))
    deep = lst.addRoot(S.Fig(kind=S.FigKind.nkFrame, screenBox=S.rect(0, 0, 10, 10)))
    for _ in range(2100):
        deep = lst.addChild(deep, S.Fig(kind=S.FigKind.nkFrame, screenBox=S.rect(0, 0, 10, 10)))
    for k in range(100):
        lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(3.0 * k, 40.0, 20, 20), fill=S.rgba(1, 2, 3, 255)))
    sc = S.Renders()
    sc.setLayer(0, lst)
    return sc


def per_call_frame(ctx, w=320, h=200):
    """a blur inside two open clips and a fast rect mask (the reopen path); a blur of radius 0.4 (the live frame is its snapshot), one
    wholly outside the frame, a rect mask inside a rect mask (the fallback: a real mask, under the call log's pause), culled draws"""
    red, blue = S.rgba(220, 30, 30, 255), S.rgba(20, 40, 230, 200)
    r4 = [6.0] * 4
    ctx.begin_frame(w, h, True, (1.0, 1.0, 1.0, 1.0))
    ctx.save_transform()
    ctx.translate(3.0, 2.0)
    ctx.draw_rect((0, 0, 300, 180), red)
    ctx.begin_mask((10, 10, 280, 160), r4, r4)
    ctx.end_mask()
    ctx.draw_rounded_rect_sdf((20, 20, 100, 60), [blue] * 4, r4, r4, 3)
    ctx.begin_mask((30, 30, 200, 120), Z4, Z4)
    ctx.end_mask()
    ctx.begin_rect_mask((40, 40, 160, 90), r4, r4)
    ctx.draw_rect((35, 35, 90, 40), blue)
    ctx.draw_backdrop_blur((50, 50, 120, 60), r4, r4, 9.0)
    ctx.draw_rounded_rect_sdf((60, 60, 40, 30), [red] * 4, r4, r4, 3)
    ctx.draw_backdrop_blur((70, 60, 50, 30), Z4, Z4, 0.4)
    ctx.draw_backdrop_blur((900, 900, 50, 30), Z4, Z4, 12.0)
    ctx.draw_rect((-500, -500, 20, 20), red)  # (outside: culled where culling is on)
    ctx.begin_rect_mask((70, 55, 60, 40), r4, r4)
    ctx.draw_rect((72, 57, 30, 20), red)
    ctx.pop_rect_mask()
    ctx.pop_rect_mask()
    ctx.pop_mask()
    ctx.draw_rounded_rect_sdf((400, 20, 100, 60), [blue] * 4, r4, r4, 3)
    ctx.pop_mask()
    ctx.restore_transform()
    ctx.end_frame()


def retained_sequence(ctx, w=320, h=200, on_render=None):
    """retain, update_nodes, replace_root, insert_root, then a change of ui_scale: on_render(ctx, step) after each render"""
    sc = RS.random_scene(21, float(w), float(h), n=30, clips=True, blur=True)
    lst = sc.layers[0]
    ctx.scene_retain(sc, w, h)
    on_render(ctx, "retain")
    n = lst.nodes[lst.rootIds[3]]
    n.fill = S.fill(S.rgba(9, 200, 90, 255))
    ctx.scene_update_nodes(0, lst.rootIds[3], [n])
    ctx.scene_render()
    on_render(ctx, "update_nodes")
    box = S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(40, 30, 120, 70), fill=S.rgba(200, 100, 0, 255), corners=[5] * 4, flags=S.FigFlags.NfClipContent)
    kid = S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(30, 50, 200, 20), fill=S.rgba(0, 100, 200, 200), parent=0, rotation=11.0)
    box.childCount = 1
    ctx.scene_replace_root(0, 1, [box, kid])
    ctx.scene_render()
    on_render(ctx, "replace_root")
    ctx.scene_insert_root(0, 2, [S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(5, 5, 60, 190), fill=S.rgba(90, 0, 90, 120), corners=[9] * 4)])
    ctx.scene_render()
    on_render(ctx, "insert_root")
    ctx.L.fdh_set_ui_scale(ctx.h, 1.25)
    ctx.scene_render()
    on_render(ctx, "ui_scale")


# ---------------------------------------------------------------------------------------------- the cases
def case_reference_scenes():
    scenes = {k: v[:3] for k, v in RS.REFERENCE_PNG_SCENES.items()}
    scenes.update(RS.SWIFTSHADER_SCENES)
    return {name: {f"t{t}": frames(fn(float(w), float(h)), w, h, t, n=1) for t in (0, 3)} for name, (fn, w, h) in sorted(scenes.items())}


def _trees():
    return {"bench": (make_render_tree_100(3840, 2160, 3, full_frame_blur=True), 3840, 2160), "non_clip": (make_non_clip_benchmark(), 1200, 800),
            "sub_clip": (make_clip_mask_benchmark("sub_clip"), 1200, 800), "rect_mask": (make_clip_mask_benchmark("rect_mask"), 1200, 800),
            "wide5": (_wide_scene(5, 1280, 720), 1280, 720)}


def case_trees():
    return {name: {f"t{t}c{c}": frames(sc, w, h, t, cull=c) for t in (0, 1, 2, 5) for c in (0, 1)} for name, (sc, w, h) in _trees().items()}


def case_consolidate():
    return {f"t{t}": frames(consolidate_scene(), 800, 600, t) for t in (0, 3)}


def case_serial_only_fallback():
    return frames(drawable_scene(), 640, 480, 3)  # frame 1 falls back (the "rect" image is made), frame 2 forks


def case_wide_frame():
    return {f"t{t}": frames(rects_scene(80, 8200, 64, seed=3), 8200, 64, t) for t in (0, 3)}  # 129 bins along x: binbox_shift 1


def case_per_call():
    out = {}
    for log in (True, False):
        ctx = HipContext(record_only=True)
        if log:
            ctx.set_cull(2)  # culling while the call recorder runs: culled calls are taken back out of the log
            ctx.record_begin()
        per_call_frame(ctx)
        r = snap(ctx)
        if log:
            r["json_sha256"] = hashlib.sha256(ctx.L.fdh_record_json(ctx.h)).hexdigest()
        per_call_frame(ctx)  # (the log is off again: culling by the default rule)
        r["second"] = snap(ctx)
        out["log" if log else "plain"] = r
        ctx.close()
    return out


def case_stripe():
    ctx = HipContext(record_only=True)
    ctx.set_stripe(40, 80)
    sc = rects_scene(120, 320, 200, seed=5, blurs=((20, 10, 200, 60, 14.0), (60, 90, 180, 80, 6.0)))
    out = []
    for _ in range(2):
        ctx.render_frame(sc, 320, 200)
        out.append(snap(ctx))
    ctx.close()
    return out


def case_retained():
    out = {}
    for pick in (False, True):
        ctx = HipContext(record_only=True)
        ctx.set_pick(pick)
        steps = {}
        retained_sequence(ctx, on_render=lambda c, step: steps.__setitem__(step, snap(c, tags=pick)))
        out["pick" if pick else "plain"] = steps
        ctx.close()
    return out


def case_refusals():
    out = {}
    r4 = [2.0] * 4
    red = S.rgba(255, 0, 0, 255)
    fill = S.fill(red)
    draws = {
        "draw_rounded_rect_sdf": lambda c: c.draw_rounded_rect_sdf((1, 1, 9, 9), [red] * 4, r4, r4, 3),
        "draw_rounded_rect_fill": lambda c: c.draw_rounded_rect_fill((1, 1, 9, 9), fill, r4, r4, 3),
        "draw_image": lambda c: c.draw_image(5, (1, 1), [red] * 4),
        "draw_image_adj": lambda c: c.draw_image_adj(5, (1, 1), red, (8, 8)),
        "draw_msdf": lambda c: c.draw_msdf(5, (1, 1), red, (8, 8), 4.0),
        "draw_quadratic_bezier_sdf": lambda c: c.draw_quadratic_bezier_sdf((1, 1, 20, 20), fill, (0, 0), (5, 9), (9, 0), 2.0, 0),
        "draw_filled_quad": lambda c: c.draw_filled_quad([0, 0, 9, 0, 9, 9, 0, 9], [red] * 4),
        "draw_rect": lambda c: c.draw_rect((1, 1, 9, 9), red),
        "draw_backdrop_blur": lambda c: c.draw_backdrop_blur((1, 1, 30, 30), r4, r4, 8.0),
        "begin_mask": lambda c: c.begin_mask((1, 1, 30, 30), r4, r4),
        "begin_rect_mask": lambda c: c.begin_rect_mask((1, 1, 30, 30), r4, r4),
    }

    def good(ctx):  # after each refusal, one good frame
        ctx.render_frame(one_rect_scene(), 64, 48)
        return snap(ctx)

    def begun(ctx):
        ctx.begin_frame(64, 48, True, (1.0, 1.0, 1.0, 1.0))

    def left_open(open_call):
        def run(ctx):
            begun(ctx)
            open_call(ctx)
            ctx.end_frame()
        return run

    def abandon(ctx):  # a frame refused at end_frame stays begun: close what is open, end it
        for undo in (ctx.end_mask, ctx.pop_rect_mask, ctx.pop_mask):
            refusal(undo)
        refusal(ctx.end_frame)

    for name, call in draws.items():
        ctx = HipContext(record_only=True)
        out[name + "_before_begin"] = {"refused": refusal(lambda: call(ctx)), "then": good(ctx)}
        ctx.close()
    steps = {
        "begin_frame_twice": (lambda c: (begun(c), begun(c)), True),
        "end_frame_without_begin": (lambda c: c.end_frame(), False),
        "end_frame_mask_open": (left_open(lambda c: (c.begin_mask((1, 1, 30, 30), r4, r4), c.end_mask())), True),
        "end_frame_rect_mask_open": (left_open(lambda c: c.begin_rect_mask((1, 1, 30, 30), r4, r4)), True),
        "restore_transform_empty": (lambda c: (begun(c), c.restore_transform()), True),
        "pop_rect_mask_none": (lambda c: (begun(c), c.pop_rect_mask()), True),
    }
    for name, (run, in_frame) in steps.items():
        ctx = HipContext(record_only=True)
        r = {"refused": refusal(lambda: run(ctx))}
        if in_frame:
            abandon(ctx)
        r["then"] = good(ctx)
        out[name] = r
        ctx.close()
    for t in (0, 3):
        ctx = HipContext(record_only=True)
        ctx.set_walk_threads(t)
        out[f"deep_tree_t{t}"] = {"refused": refusal(lambda: ctx.render_frame(deep_scene(), 640, 480)), "then": good(ctx)}
        ctx.close()
    return out


CASES = {"reference_scenes": case_reference_scenes, "trees": case_trees, "consolidate": case_consolidate, "serial_only_fallback": case_serial_only_fallback,
         "wide_frame": case_wide_frame, "per_call": case_per_call, "stripe": case_stripe, "retained": case_retained, "refusals": case_refusals}


@pytest.fixture(scope="module")
def pins():
    with open(PIN_FILE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_record_what_the_parent_recorded(name, pins):
    got = json.loads(json.dumps(CASES[name]()))  # (tuples -> lists, int keys -> strings: as the file holds them)
    want = pins[name]
    if isinstance(got, dict):
        assert sorted(got) == sorted(want)
        for key in got:
            assert got[key] == want[key], f"{name}/{key}"
    assert got == want


def test_the_cases_reach_the_paths_they_are_for(pins):
    """the pins themselves: groups forked where they should, the fallback fell back, something was culled, the refusals refused"""
    assert pins["consolidate"]["t3"][0]["groups"] == 14 and pins["consolidate"]["t0"][0]["groups"] == 0
    assert [f["groups"] for f in pins["serial_only_fallback"]] == [0, 1]
    assert all(pins["trees"][n]["t5c1"][1]["groups"] > 0 for n in pins["trees"])
    assert pins["per_call"]["log"]["culled"] > 0 and pins["stripe"][0]["culled"] > 0
    assert all(v["refused"] is not None for v in pins["refusals"].values())
    assert pins["retained"]["pick"]["insert_root"]["tags"][0] > 0
