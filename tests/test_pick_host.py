"""Picking (include/figdraw_hip_pick.h), host side -- CPU suite, no GPU: the public header as strict C99 with every entry point
exported and called (tests/pick_abi_smoke.c), the tags the scene front-end gives every draw record (serial and on the walk pool, for
frames and for retained scenes after every kind of edit), and that picking changes no record the kernels read."""
import copy
import dataclasses
import os
import random
import re
import subprocess

import numpy as np
import pytest

import ref_scenes as RS
from figdraw_amd.context import HipContext
from figdraw_amd.scene import Fill, Renders, RenderList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICK_H = os.path.join(ROOT, "include", "figdraw_hip_pick.h")


def _pick_symbols():
    return sorted(set(re.findall(r"FDH_API\s+[\w\s\*]+?\b(fdh_\w+)\s*\(", open(PICK_H).read())))


def test_pick_header_is_strict_c99_and_every_symbol_is_exported_and_called(tmp_path):
    import ctypes as C

    from figdraw_amd import context

    context.build()
    names = _pick_symbols()
    assert len(names) == 5, names
    lib = C.CDLL(context.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]
    src = os.path.join(ROOT, "tests", "pick_abi_smoke.c")
    assert not [n for n in names if not re.search(r"\b%s\b" % n, open(src).read())]
    exe = tmp_path / "pick_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src, "-o", str(exe),
                           "-L", lib_dir, "-l:libfigdraw_hip.so", "-Wl,-rpath," + lib_dir, "-lm"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pick_abi_smoke: OK" in r.stdout


# ---- front-end tags, identified by colour.  Every node gets colours of its own: RGB = (k & 255, k >> 8, role), k = 1 + the node's position
# over all layers, the alpha kept (alpha decides which draws the front-end makes).  A recorded draw call's colours then name its node.
ROLES = {"fill": 101, "stroke": 102, "shadow": 103, "image": 104, "glyph": 105, "textrect": 106, "drawstroke": 107}
COLOUR_ARGS = {"draw_rounded_rect_sdf": (2, 10, 11), "draw_quadratic_bezier_sdf": (2,), "draw_filled_quad": (2,), "draw_image": (3,),
               "draw_msdf": (3,), "draw_rect": (2,), "draw_image_adj": (3,)}


def _code(k, role, c):
    return (k & 255, (k >> 8) & 255, ROLES[role], int(c[3]))


def _recode_fill(f, k, role):
    return dataclasses.replace(f, start=_code(k, role, f.start), mid=_code(k, role, f.mid), stop=_code(k, role, f.stop))


def recolour(sc):
    """a deep copy of the scene with one set of colours per node; -> (scene, {k: (zlevel, node index)})"""
    sc = copy.deepcopy(sc)
    owner, k = {}, 0
    for z, lst in sc.layers.items():
        for i, n in enumerate(lst.nodes):
            k += 1
            owner[k] = (z, i)
            n.fill = _recode_fill(n.fill, k, "fill")
            n.stroke.fill = _recode_fill(n.stroke.fill, k, "stroke")
            n.drawStroke.fill = _recode_fill(n.drawStroke.fill, k, "drawstroke")
            n.image_fill = _recode_fill(n.image_fill, k, "image")
            for s in n.shadows:
                s.fill = _recode_fill(s.fill, k, "shadow")
            for g in n.glyphs:
                g.colors = [_code(k, "glyph", c) for c in g.colors]
            for t in n.textRects:
                t.fill = _recode_fill(t.fill, k, "textrect")
    return sc, owner


def _codes_in(x, out):
    if isinstance(x, dict):
        for v in x.values():
            _codes_in(v, out)
    elif isinstance(x, list):
        if len(x) == 4 and all(isinstance(v, int) for v in x):
            if x[2] in ROLES.values():
                out.add(x[0] + 256 * x[1])
        else:
            for v in x:
                _codes_in(v, out)


def expected_tags(calls, owner):
    """what each record of a recorded call stream must carry: (zlevel, id) of the node its call's colours name, or None for a record no
    colour identifies (clip and rect-mask records, blur composites, clips re-opened after a blur)"""
    out, open_ops = [], 0
    for c in calls:
        name = c[0]
        if name in ("begin_mask", "begin_rect_mask"):
            out.append(None)
            open_ops += 1
        elif name in ("pop_mask", "pop_rect_mask"):
            out.append(None)
            open_ops -= 1
        elif name == "draw_backdrop_blur":
            rect, radius = c[1], c[4]
            if radius > 0.5 and rect[2] > 0 and rect[3] > 0:
                out += [None] * open_ops  # (the phase that starts here re-opens the clips open around it)
            out.append(None)
        elif name in COLOUR_ARGS:
            codes = set()
            for a in COLOUR_ARGS[name]:
                if a < len(c):
                    _codes_in(c[a], codes)
            assert len(codes) == 1, (c, codes)
            out.append(owner[codes.pop()])
    return out


def _tag_scenes():
    from conftest import GOLDEN
    from figdraw_amd.scenes import load_glyph_fixture

    imgs = load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz"))
    return {
        "random_scene_3": (RS.random_scene(3, 400.0, 300.0), 400, 300, {}),
        "random_scene_11_many": (RS.random_scene(11, 640.0, 480.0, n=300), 640, 480, {}),
        "drawables": (RS.drawables(), 420, 300, {}),
        "text_frontend": (RS.text_frontend(images=imgs), 300, 120, imgs),
        "rotation_and_transform": (RS.rotation_and_transform(), 320, 240, {}),
    }


def _ctx(images, sc):
    ctx = HipContext(record_only=True)
    for k, v in RS.used_images(sc, images).items() if images else ():
        ctx.put_image(k, v)
    ctx.set_cull(0)
    return ctx


@pytest.mark.parametrize("name", ["random_scene_3", "random_scene_11_many", "drawables", "text_frontend", "rotation_and_transform"])
def test_frontend_tags_name_the_node_of_every_draw(name):
    """Every draw call of the recorded stream, identified by its colour, carries the tag of the node the colour belongs to; the same tags
    come out of the walk with one thread and with eight (the pool decomposes sibling groups of 48 and more: random_scene_11_many)."""
    sc0, w, h, images = _tag_scenes()[name]
    sc, owner = recolour(sc0)
    ctx = _ctx(images, sc)
    ctx.set_pick(True)
    ctx.record_begin()
    ctx.render_frame(sc, w, h)
    calls = ctx.record_calls()
    tags = ctx.pick_draw_tags()
    want = expected_tags(calls, owner)
    assert len(want) == len(tags), (len(want), len(tags))
    n_checked = 0
    for i, t in enumerate(want):
        if t is not None:
            assert tuple(tags[i]) == t, (name, i, tuple(tags[i]), t)
            n_checked += 1
    assert n_checked >= 0.6 * len(want) and n_checked > 0
    # the walk pool: tags with 1 and with 8 threads (no call recorder: it keeps the walk serial)
    per_threads = {}
    for threads in (1, 8):
        ctx.set_walk_threads(threads)
        ctx.render_frame(sc, w, h)
        per_threads[threads] = ctx.pick_draw_tags()
        if threads == 8 and name == "random_scene_11_many":
            assert ctx.walk_stats()[1] > 0  # (a sibling group went to the pool)
    assert np.array_equal(per_threads[1], tags) and np.array_equal(per_threads[8], tags)
    ctx.close()


def test_call_level_tags():
    ctx = HipContext(record_only=True)
    ctx.set_pick(True)
    ctx.set_pick_tag(3, 4)
    ctx.begin_frame(64, 64)
    ctx.draw_rect((0, 0, 10, 10), (255, 0, 0, 255))
    ctx.set_pick_tag(1, 2)
    ctx.draw_rect((0, 0, 10, 10), (255, 0, 0, 255))
    ctx.begin_mask((0, 0, 20, 20), (0, 0, 0, 0), (0, 0, 0, 0))
    ctx.end_mask()
    ctx.set_pick_tag(7, 8)
    ctx.draw_rect((0, 0, 10, 10), (255, 0, 0, 255))
    ctx.pop_mask()
    ctx.end_frame()
    assert ctx.pick_draw_tags().tolist() == [[-1, -1], [1, 2], [1, 2], [7, 8], [7, 8]]
    ctx.close()


# ---- retained scenes: node ids as the retained layer holds them after every edit
def _subtrees(lst):
    root_of, out = [], []
    for i, n in enumerate(lst.nodes):
        root_of.append(i if n.parent < 0 else root_of[n.parent])
    for r in lst.rootIds:
        idx = [i for i in range(len(lst.nodes)) if root_of[i] == r]
        pos = {g: k for k, g in enumerate(idx)}
        sub = []
        for g in idx:
            f = copy.deepcopy(lst.nodes[g])
            f.parent = -1 if g == r else pos[f.parent]
            sub.append(f)
        out.append(sub)
    return out


class RetainedMirror:
    """the retained layer's node array and root list as the library keeps them: a replaced root's subtree is compacted out (the other
    nodes keep their order) and the new subtree appended; an inserted one is appended"""

    def __init__(self, lst):
        self.nodes = [copy.deepcopy(n) for n in lst.nodes]
        self.roots = list(lst.rootIds)

    def _append(self, sub):
        base = len(self.nodes)
        for k, f in enumerate(sub):
            g = copy.deepcopy(f)
            g.parent = -1 if k == 0 else f.parent + base
            self.nodes.append(g)
        return base

    def replace(self, slot, sub):
        root_of = []
        for i, n in enumerate(self.nodes):
            root_of.append(i if n.parent < 0 or n.parent >= i else root_of[n.parent])
        old = self.roots[slot]
        remap, kept = {}, []
        for i, n in enumerate(self.nodes):
            if root_of[i] != old:
                remap[i] = len(kept)
                kept.append(n)
        for n in kept:
            if n.parent >= 0:
                n.parent = remap[n.parent]
        self.nodes = kept
        self.roots = [remap[r] if s != slot else -1 for s, r in enumerate(self.roots)]
        self.roots[slot] = self._append(sub)

    def insert(self, slot, sub):
        self.roots.insert(slot, self._append(sub))

    def scene(self):
        lst = RenderList()
        lst.nodes = [copy.deepcopy(n) for n in self.nodes]
        lst.rootIds = list(self.roots)
        sc = Renders()
        sc.setLayer(0, lst)
        return sc


@pytest.mark.parametrize("seed", [4, 9])
def test_retained_scene_tags_follow_every_edit(seed):
    """After fdh_scene_update_nodes, fdh_scene_replace_root with a smaller and with a larger subtree and fdh_scene_insert_root, the tags of
    fdh_scene_render -- cached roots reused -- equal those of fdh_render_frame of the same node array (ids as the retained layer holds
    them: a replacement compacts the layer, and the reused roots' cached ids must move with it)."""
    rnd = random.Random(seed)
    w, h = 512, 384
    base = RS.random_scene(seed, float(w), float(h), n=40, clips=True, blur=False)
    lst = next(iter(base.layers.values()))
    subs = _subtrees(lst)
    flat = RetainedMirror(RenderList())
    for s in subs:
        flat.insert(len(flat.roots), s)
    ret = HipContext(record_only=True)
    ret.set_cull(0)
    ret.set_pick(True)
    ret.scene_retain(flat.scene(), w, h)

    def check(what):
        ret.scene_render()
        walked, reused = ret.scene_stats()
        assert reused > 0, what
        fresh = HipContext(record_only=True)
        fresh.set_cull(0)
        fresh.set_pick(True)
        fresh.render_frame(flat.scene(), w, h)
        assert ret.record_digest() == fresh.record_digest(), what
        got, want = ret.pick_draw_tags(), fresh.pick_draw_tags()
        assert np.array_equal(got, want), (what, np.argwhere((got != want).any(axis=1))[:5].ravel().tolist())
        assert (got[:, 1] >= 0).all()
        fresh.close()

    ret.scene_render()
    # property update (ids do not move)
    i = rnd.randrange(len(flat.nodes))
    n = copy.deepcopy(flat.nodes[i])
    n.fill = Fill(start=(10, 200, 30, 255))
    flat.nodes[i] = n
    ret.scene_update_nodes(0, i, [n])
    check("update")
    # replace an early root with a smaller subtree (every later node's index moves down), then one with a larger subtree
    big = max(range(3), key=lambda s: len(subs[s]))
    small = [copy.deepcopy(subs[big][0])]
    flat.replace(big, small)
    ret.scene_replace_root(0, big, small)
    check("replace smaller")
    larger = [copy.deepcopy(subs[big][0])] + [copy.deepcopy(n) for n in sum(subs[-3:], [])[:6]]
    for k, f in enumerate(larger[1:], start=1):
        f.parent = 0
    flat.replace(0, larger)
    ret.scene_replace_root(0, 0, larger)
    check("replace larger")
    ins = [copy.deepcopy(subs[1][0])]
    flat.insert(2, ins)
    ret.scene_insert_root(0, 2, ins)
    check("insert")
    ret.close()


# ---- picking changes no record
@pytest.mark.parametrize("name", ["nested_clips", "deep_clips", "rect_mask_nested", "backdrop_blur", "rotation_and_transform", "drawables",
                                  "elliptical_and_fractional", "layers_clip", "rgb_boxes_sdf", "curves"])
def test_picking_changes_no_record(name):
    """fdh_debug_record_digest and the recorded call stream are the same with picking never touched, on, and turned on then off"""
    fn = getattr(RS, name)
    sc = fn()
    w, h = 400, 300
    out = []
    for mode in ("never", "on", "on_off"):
        ctx = HipContext(record_only=True)
        if mode != "never":
            ctx.set_pick(True)
            ctx.render_frame(sc, w, h)
        if mode == "on_off":
            ctx.set_pick(False)
        ctx.record_begin()
        ctx.render_frame(sc, w, h)
        out.append((ctx.record_digest(), ctx.record_calls()))
        if mode == "on":
            assert len(ctx.pick_draw_tags()) > 0
        ctx.close()
    assert out[0] == out[1] == out[2]
