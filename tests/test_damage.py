"""Damage tracking (include/figdraw_hip_damage.h): a tracking context composites only the bins whose inputs changed, and its surface
must stay bit for bit what a full render of the last frame gives.  CPU tests pin the C ABI and the blur rule (fdh_damage_closure);
GPU tests hold a tracking context against a fresh context that renders every frame in full."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_scenes as RS
from figdraw_amd import context
from figdraw_amd.context import FigdrawHipError, HipContext
from figdraw_amd.scene import rect, rgba, fill
from figdraw_amd.scenes import make_non_clip_benchmark, make_render_tree_100

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "figdraw_hip_damage.h")
NEW_API = ("fdh_set_damage_tracking", "fdh_damage_bins", "fdh_damage_changed_bins", "fdh_damage_closure")
INVALID, NO_DEVICE = -1, -2


def _reach(radius):
    L = context.load()
    dense = (C.c_float * 256)()
    frag = (C.c_uint16 * (11 * 2 * 64 * 8))()
    r, k = C.c_int(), C.c_int()
    assert L.fdh_blur_weight_fragments(C.c_float(radius), 0, dense, frag, C.byref(r), C.byref(k)) == 0
    return r.value


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_header_declares_and_library_exports_the_damage_api():
    src = open(HEADER).read()
    assert '#include "figdraw_hip.h"' in src
    declared = re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", src)
    assert sorted(declared) == sorted(NEW_API)
    L = context.load()
    for name in NEW_API:
        assert hasattr(L, name), name
    # the base header is left as it was: the new entry points live in their own header
    assert not any(n in open(os.path.join(ROOT, "include", "figdraw_hip.h")).read() for n in NEW_API)


def test_damage_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "damage_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "damage_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "damage_abi_smoke: OK" in r.stdout
    src = open(os.path.join(ROOT, "tests", "damage_abi_smoke.c")).read()
    assert all(re.search(r"\b%s\b" % n, src) for n in NEW_API)


def test_record_only_context_refuses_the_mode():
    ctx = HipContext(record_only=True)
    with pytest.raises(FigdrawHipError) as e:
        ctx.set_damage_tracking(True)
    assert e.value.code == INVALID
    ctx.set_damage_tracking(False)
    with pytest.raises(FigdrawHipError) as e:
        ctx.damage_bins()
    assert e.value.code == NO_DEVICE
    ctx.close()


def _grid(bx, by, *changed):
    m = np.zeros((by, bx), dtype=bool)
    for x, y in changed:
        m[y, x] = True
    return m


def test_closure_change_outside_every_reach():
    node = ((256, 256, 320, 320), 4.0)  # reach 8: bins 3..5
    ch = _grid(10, 8, (0, 0), (9, 7), (2, 2))
    assert np.array_equal(HipContext.damage_closure(ch, [node]), ch)
    assert np.array_equal(HipContext.damage_closure(ch), ch)


def test_closure_change_touching_one_node():
    r = _reach(12.0)
    x0, y0, x1, y1 = 300, 200, 420, 260
    node = ((x0, y0, x1, y1), 12.0)
    bx0, by0, bx1, by1 = (x0 - r) // 64, (y0 - r) // 64, (x1 + r - 1) // 64, (y1 + r - 1) // 64
    ch = _grid(12, 9, (bx1, by1), (0, 8))
    out = HipContext.damage_closure(ch, [node])
    want = ch.copy()
    want[by0:by1 + 1, bx0:bx1 + 1] = True
    assert np.array_equal(out, want)
    # the same change one bin past the reach: nothing grows
    ch2 = _grid(12, 9, (bx1 + 1, by1))
    assert np.array_equal(HipContext.damage_closure(ch2, [node]), ch2)


def test_closure_chain_of_two_nodes():
    # node A's expansion reaches node B's region, which it would not from the change alone; listed B first: the fixed point does not
    # depend on the order the nodes are visited in
    a = ((64, 64, 128, 128), 4.0)    # reach 8: bins 0..2
    b = ((190, 64, 250, 128), 4.0)   # bins 2..4
    ch = _grid(8, 4, (0, 0))
    want = np.zeros_like(ch)
    want[0:3, 0:5] = True
    for nodes in ([a, b], [b, a]):
        assert np.array_equal(HipContext.damage_closure(ch, nodes), want)
    # a change that touches neither
    ch2 = _grid(8, 4, (7, 3))
    assert np.array_equal(HipContext.damage_closure(ch2, [b, a]), ch2)


def test_closure_full_frame_node():
    node = ((0, 0, 1920, 1080), 18.0)
    ch = _grid(30, 17, (29, 16))
    assert HipContext.damage_closure(ch, [node]).all()
    assert not HipContext.damage_closure(np.zeros_like(ch), [node]).any()


def test_closure_refuses_bad_arguments():
    with pytest.raises(FigdrawHipError):
        HipContext.damage_closure(np.zeros((2, 2), bool), [((0, 0, 1, 1), 2.0)] * 65)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _pair(route=None):
    t, f = HipContext(device=0), HipContext(device=0)
    t.set_damage_tracking(True)
    if route is not None:
        t.set_blur_route(route)
        f.set_blur_route(route)
    return t, f


def _same(t, f, what=""):
    a, b = t.read_pixels(), f.read_pixels()
    assert a.shape == b.shape, what
    if not np.array_equal(a, b):
        ys, xs = np.nonzero((a != b).any(axis=2))
        pytest.fail(f"{what}: {len(ys)} pixels differ, first at ({xs[0]}, {ys[0]}); bins {sorted(set(zip((xs // 64).tolist(), (ys // 64).tolist())))[:8]}")


def _run(frames, route=None, check_sound=True):
    """frames: callables ctx -> None that render one frame each.  The tracking context's surface is compared with a full render after
    every frame; every bin where the full renders of consecutive frames differ must be in fdh_damage_bins."""
    t, f = _pair(route)
    prev = None
    try:
        for i, fr in enumerate(frames):
            fr(t)
            fr(f)
            _same(t, f, f"frame {i}")
            cur = f.read_pixels()
            if check_sound and prev is not None and prev.shape == cur.shape:
                diff = (prev != cur).any(axis=2)
                ys, xs = np.nonzero(diff)
                dmg = t.damage_bins()
                assert dmg[ys // 64, xs // 64].all(), f"frame {i}: a changed pixel lies outside the damage"
            prev = cur
    finally:
        t.close()
        f.close()


def _scene(fn, w, h, **kw):
    return lambda ctx: ctx.render_frame(fn(**kw) if kw else fn(float(w), float(h)), w, h)


REF = ["rgb_boxes_sdf", "rgb_boxes", "linear_gradient", "layers_clip", "rect_mask_mixed_batch", "drawables", "elliptical_and_fractional",
       "nested_clips", "deep_clips", "rect_mask_nested", "backdrop_blur", "rotation_and_transform", "rotated_tree", "curves", "circle_rect"]


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
def test_reference_scenes_in_sequence(route):
    w, h = 640, 480
    frames = []
    for name in REF:
        fn = getattr(RS, name)
        frames += [_scene(fn, w, h), _scene(fn, w, h)]  # each scene twice: the second is an unchanged frame
    _run(frames, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
def test_random_scenes_in_sequence(route):
    w, h = 513, 389
    frames = [(lambda s: (lambda ctx: ctx.render_frame(RS.random_scene(s, float(w), float(h), n=40), w, h)))(s) for s in (3, 3, 4, 5, 5, 6)]
    _run(frames, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("ffb", [False, True])
def test_bench_tree_frames(route, ffb):
    w, h = 1920, 1080
    frames = [(lambda k: (lambda ctx: ctx.render_frame(make_render_tree_100(float(w), float(h), frame=k, full_frame_blur=ffb), w, h)))(k)
              for k in (0, 1, 2, 2, 3)]
    _run(frames, route)


@pytest.mark.gpu
def test_non_clip_benchmark_one_cell_toggled():
    sc = make_non_clip_benchmark()
    lst = next(iter(sc.layers.values()))
    frames = []
    for k in range(4):
        def fr(ctx, k=k):
            n = lst.nodes[5 + 3 * k]
            n.fill = fill(rgba(255, 0, 0, 255) if k % 2 else rgba(0, 0, 255, 255))
            ctx.render_frame(sc, 1200, 800)
        frames.append(fr)
    # (the edit is made once per frame: both contexts render the same scene object after it)
    t, f = _pair()
    try:
        for i, fr in enumerate(frames):
            fr(t)
            f.render_frame(sc, 1200, 800)
            _same(t, f, f"frame {i}")
            if i:
                assert t.damage_bins().sum() < t.damage_bins().size // 4
    finally:
        t.close(); f.close()


def _imm(w, h, draw, clear=True, color=(1.0, 1.0, 1.0, 1.0)):
    def fr(ctx):
        ctx.begin_frame(w, h, clear, color)
        draw(ctx)
        ctx.end_frame()
    return fr


Z4 = (0.0, 0.0, 0.0, 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
def test_immediate_mode_edits(route):
    w, h = 700, 500

    def base(ctx, dx=0, blur=(300, 200, 120, 90), order=0, rot=0.0, quad=True):
        ctx.draw_rect((20, 20, 200, 150), (200, 40, 40, 255))
        pair = [((100 + dx, 100, 180, 140), (40, 200, 40, 200)), ((160, 140, 180, 140), (40, 40, 200, 180))]
        for r, c in (pair if order == 0 else pair[::-1]):
            ctx.draw_rect(r, c)
        if quad:
            ctx.draw_filled_quad((400 + rot, 300, 560, 320 + rot, 540, 460, 380, 440), [(255, 128, 0, 255)] * 4)
        if blur is not None:
            ctx.draw_backdrop_blur(blur, Z4, Z4, 6.0)
        ctx.draw_rect((500, 40, 60, 60), (10, 10, 10, 128))

    frames = [
        _imm(w, h, lambda c: base(c)),
        _imm(w, h, lambda c: base(c)),                                # unchanged
        _imm(w, h, lambda c: base(c, blur=(320, 210, 120, 90))),      # the blur node moves
        _imm(w, h, lambda c: base(c, blur=None)),                     # ... and is removed
        _imm(w, h, lambda c: base(c, blur=(300, 200, 120, 90))),
        _imm(w, h, lambda c: base(c, dx=150)),                        # a draw slides under the node's reach
        _imm(w, h, lambda c: base(c, dx=400)),                        # ... and out of it
        _imm(w, h, lambda c: base(c, dx=400, order=1)),               # two overlapping draws swap, records unchanged
        _imm(w, h, lambda c: base(c, dx=400, order=1, rot=25.0)),     # a general quad changes
        _imm(w, h, lambda c: base(c, dx=400, order=1, rot=25.0), color=(0.2, 0.3, 0.4, 1.0)),  # clear colour
        _imm(w, h, lambda c: base(c, dx=400, order=1, rot=25.0), color=(0.2, 0.3, 0.4, 1.0)),
        _imm(w + 37, h - 11, lambda c: base(c)),                      # resize
        _imm(w + 37, h - 11, lambda c: base(c, dx=30)),
    ]
    _run(frames, route)


@pytest.mark.gpu
def test_stripes_refuse_the_mode():
    ctx = HipContext(device=0)
    try:
        ctx.set_stripe(0, 64)
        with pytest.raises(FigdrawHipError) as e:
            ctx.set_damage_tracking(True)
        assert e.value.code == INVALID
        ctx.set_stripe(0, 0)
        ctx.set_damage_tracking(True)
        with pytest.raises(FigdrawHipError) as e:
            ctx.set_stripe(0, 64)
        assert e.value.code == INVALID
        ctx.set_damage_tracking(False)
        ctx.set_stripe(0, 64)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_tracking_off_and_on_again():
    """tracking on: frame A; off: frame B; on: frame A again -- the surface holds B, so the third frame must not be taken for A's
    successor (the frame after an untracked one is rendered in full)"""
    w, h = 400, 300
    a = _imm(w, h, lambda c: c.draw_rect((20, 20, 100, 80), (255, 0, 0, 255)))
    b = _imm(w, h, lambda c: c.draw_rect((200, 150, 100, 80), (0, 0, 255, 255)))
    t, f = _pair()
    try:
        a(t)
        t.set_damage_tracking(False)
        b(t)
        t.set_damage_tracking(True)
        a(t)
        a(f)
        _same(t, f, "A after B rendered untracked")
        assert t.damage_bins().all()
        # the same through fdh_replay: an untracked replay of B between two tracked frames of A
        t.set_damage_tracking(False)
        b(t)
        t.set_damage_tracking(True)
        a(t)
        t.set_damage_tracking(False)
        b(t)
        t.replay(1)
        t.set_damage_tracking(True)
        a(t)
        _same(t, f, "A after a replayed untracked B")
    finally:
        t.close(); f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", [0, 1])
def test_more_blur_nodes_than_the_resolve_takes(route):
    """70 backdrop-blur nodes (the resolve takes 64): the frame is rendered in full and reports every bin, and so is the next one,
    whose signatures could otherwise be compared against a frame only partly signed"""
    w, h = 640, 480

    def many(n, dx=0):
        def d(c):
            c.draw_rect((10 + dx, 10, 300, 200), (200, 60, 20, 255))
            for k in range(n):
                c.draw_backdrop_blur((20 + (k % 10) * 60, 20 + (k // 10) * 60, 30, 30), Z4, Z4, 3.0)
                c.draw_rect((30 + (k % 10) * 60, 30 + (k // 10) * 60, 10, 10), (k * 3 % 256, 90, 200, 200))
        return _imm(w, h, d)

    t, f = _pair(route)
    try:
        for i, fr in enumerate([many(70), many(70), many(60), many(60), many(60, dx=40), many(70, dx=40), many(70)]):
            fr(t); fr(f)
            _same(t, f, f"frame {i}")
            if i in (0, 1, 2, 5, 6):
                assert t.damage_bins().all(), f"frame {i}: a frame with more than 64 nodes, or the one after it, is full"
    finally:
        t.close(); f.close()


@pytest.mark.gpu
def test_no_clear_frame_is_full():
    w, h = 320, 240
    t, f = _pair()
    try:
        for ctx in (t, f):
            _imm(w, h, lambda c: c.draw_rect((10, 10, 50, 50), (255, 0, 0, 255)))(ctx)
            _imm(w, h, lambda c: c.draw_rect((100, 10, 50, 50), (0, 0, 255, 128)), clear=False)(ctx)
        _same(t, f, "no-clear frame")
        assert t.damage_bins().all()
    finally:
        t.close(); f.close()


@pytest.mark.gpu
def test_tightness_and_identical_frame():
    w, h = 3840, 2160

    def fr(x, y):
        return _imm(w, h, lambda c: (c.draw_rect((100, 100, 900, 500), (30, 90, 160, 255)), c.draw_rect((x, y, 40, 40), (250, 20, 20, 255))))

    t, f = _pair()
    try:
        fr(2000, 1000)(t)
        assert t.damage_bins().all()  # the first tracked frame
        fr(2000, 1000)(t)
        assert t.damage_bins().sum() == 0
        before = t.read_pixels()
        fr(2000, 1000)(t)
        assert t.damage_bins().sum() == 0 and np.array_equal(t.read_pixels(), before)
        fr(2130, 1070)(t)
        d = t.damage_bins()
        allowed = np.zeros_like(d)
        for x, y in ((2000, 1000), (2130, 1070)):
            allowed[max(0, y // 64 - 1):(y + 40 - 1) // 64 + 2, max(0, x // 64 - 1):(x + 40 - 1) // 64 + 2] = True
        assert d.any() and not (d & ~allowed).any()
        fr(2130, 1070)(f)
        _same(t, f, "moved rect")
    finally:
        t.close(); f.close()


@pytest.mark.gpu
def test_device_mask_is_the_closure_of_the_changed_bins():
    w, h = 640, 480
    nodes = [((200, 150, 330, 260), 9.0), ((300, 240, 420, 330), 5.0)]

    def fr(dx):
        def d(c):
            c.draw_rect((40 + dx, 40, 60, 60), (255, 0, 0, 255))
            c.draw_rect((150, 150, 200, 80), (0, 128, 0, 255))
            for (x0, y0, x1, y1), r in nodes:
                c.draw_backdrop_blur((x0, y0, x1 - x0, y1 - y0), Z4, Z4, r)
            c.draw_rect((500, 400, 30, 30), (0, 0, 255, 255))
        return _imm(w, h, d)

    t = HipContext(device=0)
    t.set_damage_tracking(True)
    try:
        for dx in (0, 0, 90, 180, 500):
            fr(dx)(t)
            changed, mask = t.damage_changed_bins(), t.damage_bins()
            assert np.array_equal(mask, HipContext.damage_closure(changed, nodes))
    finally:
        t.close()


@pytest.mark.gpu
def test_frame_device_ptr_across_full_frame_blur_then_partial_frames():
    w, h = 1280, 720
    t, f = _pair(route=1)
    try:
        frames = [_scene(lambda ww, hh: make_render_tree_100(ww, hh, frame=0, full_frame_blur=True), w, h),
                  _imm(w, h, lambda c: c.draw_rect((10, 10, 80, 80), (255, 0, 0, 255))),
                  _imm(w, h, lambda c: c.draw_rect((10, 10, 80, 80), (255, 0, 0, 255))),
                  _imm(w, h, lambda c: c.draw_rect((30, 10, 80, 80), (255, 0, 0, 255)))]
        for i, fr in enumerate(frames):
            fr(t)
            fr(f)
            ptr, pw, ph, pitch = t.frame_device_ptr()
            t.sync()
            got = np.empty((ph, pw, 4), np.uint8)
            hip = C.CDLL("libamdhip64.so")  # (the runtime the library runs on: the surface is a device pointer of this process)
            assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(ptr), C.c_size_t(pitch * ph), 2) == 0  # device -> host
            assert np.array_equal(got, f.read_pixels()), f"frame {i}: fdh_frame_device_ptr does not hold the frame"
    finally:
        t.close(); f.close()


@pytest.mark.gpu
def test_update_image_in_view():
    w, h = 320, 240
    img_a = np.zeros((32, 32, 4), np.uint8); img_a[..., 0] = 255; img_a[..., 3] = 255
    img_b = img_a.copy(); img_b[8:24, 8:24, 1] = 255
    t, f = _pair()
    try:
        for ctx in (t, f):
            ctx.put_image(7, img_a)
        draw = _imm(w, h, lambda c: (c.draw_rect((0, 0, 40, 40), (0, 0, 0, 255)),
                                     c.draw_image(7, (100.0, 80.0), [(255, 255, 255, 255)] * 4, (32.0, 32.0))))
        for step in range(3):
            if step == 2:
                for ctx in (t, f):
                    ctx.update_image(7, img_b)
            draw(t); draw(f)
            _same(t, f, f"step {step}")
    finally:
        t.close(); f.close()


@pytest.mark.gpu
def test_retained_scene_under_tracking():
    w, h = 640, 480
    rnd = random.Random(9)
    sc = RS.random_scene(9, float(w), float(h), n=60, clips=True, blur=True)
    lst = next(iter(sc.layers.values()))
    t, f = _pair()
    try:
        t.scene_retain(sc, w, h)
        t.scene_render()
        f.render_frame(sc, w, h)
        _same(t, f, "retained frame 0")
        for step in range(6):
            i = rnd.randrange(len(lst.nodes))
            n = lst.nodes[i]
            x, y, bw, bh = n.screenBox
            n.screenBox = rect(x + rnd.uniform(-9, 9), y + rnd.uniform(-9, 9), bw, bh)
            t.scene_update_nodes(0, i, [n])
            t.scene_render()
            f.render_frame(sc, w, h)
            _same(t, f, f"retained step {step}")
        t.replay(2)
        _same(t, f, "replay")
    finally:
        t.close(); f.close()


@pytest.mark.gpu
def test_four_tracking_contexts_in_flight():
    w, h = 800, 600
    ts = [HipContext(device=0) for _ in range(4)]
    for t in ts:
        t.set_damage_tracking(True)
    f = HipContext(device=0)
    try:
        for k in range(4):
            for j, t in enumerate(ts):
                t.render_frame(make_render_tree_100(float(w), float(h), frame=k + j, copies=20), w, h)
        for j, t in enumerate(ts):
            f.render_frame(make_render_tree_100(float(w), float(h), frame=3 + j, copies=20), w, h)
            _same(t, f, f"context {j}")
    finally:
        for t in ts:
            t.close()
        f.close()


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import ref_scenes as RS
from figdraw_amd.context import HipContext
t, f = HipContext(device=0), HipContext(device=0)
t.set_damage_tracking(True)
for s in (11, 11, 12, 13):
    sc = RS.random_scene(s, 400.0, 300.0, n=30)
    t.render_frame(sc, 400, 300); f.render_frame(sc, 400, 300)
    assert np.array_equal(t.read_pixels(), f.read_pixels()), s
print("child: OK")
"""


@pytest.mark.gpu
def test_forced_slot_path_in_a_child_process():
    env = dict(os.environ, FDH_FORCE_KERNEL_PATHS="3")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child: OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
