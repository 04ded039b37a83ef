"""GPU suite: the compositor's atlas path on hostile draws (tests/hostile_atlas_cases.py) -- modes 0 and 13 - 16 against the oracle, against
what the reference's own shaders made of the same frames (tests/golden/ss_hostile_atlas_<name>.png), and against themselves under every
switch that picks another path.  The companion of tests/test_hostile_shapes.py, with its bars and its scheme.

The atlas path of k_composite_strip.inc is a chain of geometric arguments: a strip's texel window from three of its pixels, staged in LDS
while it is small and inside the level; a pixel that IS its texel, read as a 16-byte run; bounds shrunk to the ink above a cut; a level
of detail clamped to the last level.  The frames put them where they are tightest, each as a frame of at most 64 records per phase and
as shifted copies that pass 64 (bin launch, deep lists).

Bars.  Against the oracle: at most 1 LSB (the pixels of hostile_atlas_cases.AMPLIFIED, each with its reason: 2), and the share of pixels
that differ at all at most the larger of 0.5 % and the share on which the ORACLE differs from the shaders' golden of that frame
(manifest.json).  Against the golden: at most 2 LSB outside the pixels the manifest lists -- where the oracle itself is more than 1 LSB
from the golden, at most 8 per frame (tests/test_hostile_atlas_host.py holds the list to that).  The families without a golden
(ORACLE_ONLY) are held to the oracle alone here; the oracle is held to a float64 restatement of the shader there.

All frames come from child processes, one per setting (the switches are read once per process): the default's are held to the bars, the
others' must equal the default's bit for bit."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import hostile_atlas_cases as HA
from conftest import diff_stats, load_png

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# setting -> (environment, set_cull mode or None)
SETTINGS = {"default": ({}, None)}
SETTINGS.update({f"FDH_FORCE_KERNEL_PATHS={v}": ({"FDH_FORCE_KERNEL_PATHS": str(v)}, None) for v in (1, 2, 3, 8, 19)})
SETTINGS.update({f"{k}={v}": ({k: str(v)}, None) for k, v in (("FDH_INK_BOUNDS", 0), ("FDH_DIRECT", 0), ("FDH_DEEP_MIN", 0), ("FDH_DEEP_MIN", 1),
                                                             ("FDH_FOLD_CLEAR", 0), ("FDH_OPAQUE", 0))})
SETTINGS["set_cull=0"] = ({}, 0)
# frames drawn again after fdh_compact_atlas has moved every entry: 1:1 texels, the window and the edge entries, the mip chains
COMPACTED = ("one_to_one", "window", "minified")


def compaction_order(imgs):
    """the order fdh_compact_atlas repacks in: tallest first, then widest, then by key (include_glyphs/figdraw_hip_atlas.h)"""
    def size(k):
        v = imgs[k][0] if isinstance(imgs[k], list) else imgs[k]
        return v.shape[0], v.shape[1]

    return sorted(imgs, key=lambda k: (-size(k)[0], -size(k)[1], k))


def render_all(cull=None):
    """(a child process) every frame in both forms on one context -> name/form: pixels; name/form: [ms_bin]; the rectangles after a
    compaction.  The lists forms are rendered twice (the second frame on has the bin order); those of STRIPE_FRAMES again as three row
    stripes, stitched; those of the node-level frames again as retained scenes; the frames of COMPACTED again on a keep-mode context
    after fdh_compact_atlas, and on a fresh context that put the images in compaction order."""
    from figdraw_amd.context import HipContext

    t0 = time.time()
    ctx = HipContext(atlas_size=HA.ATLAS, device=0)
    HA.put_images(ctx)
    if cull is not None:
        ctx.set_cull(cull)
    frames, info = {}, {}
    for name in HA.FRAMES:
        for form in HA.FORMS:
            key = f"{name}/{form}"
            for _ in range(2 if form == "lists" else 1):
                HA.render(ctx, name, form)
                ctx.sync()
            frames[key] = ctx.read_pixels().copy()
            ctx.profile(1)
            info[key] = [float(ctx.frame_stats().ms_bin)]
            if form == "lists" and name in HA.STRIPE_FRAMES:
                whole = np.zeros_like(frames[key])
                for y0, y1 in HA.STRIPES:
                    ctx.set_stripe(y0, y1)
                    HA.render(ctx, name, form)
                    whole[y0:y1] = ctx.read_pixels()[y0:y1]
                ctx.set_stripe(0, 0)
                frames[f"{name}/stripes"] = whole
            if form == "lists" and HA.is_node_frame(name):
                ctx.scene_retain(HA.scene(name, form), HA.W, HA.H, color=tuple(HA.clear_of(name)))
                ctx.scene_render()
                frames[f"{name}/retained"] = ctx.read_pixels().copy()
    ctx.close()
    # ---- the same frames after a compaction has moved the entries
    keep = HipContext(atlas_size=HA.ATLAS, device=0)
    keep.set_atlas_keep(True)
    if cull is not None:
        keep.set_cull(cull)
    before = HA.put_images(keep)
    for name in COMPACTED:
        HA.render(keep, name)
        assert np.array_equal(keep.read_pixels(), frames[f"{name}/direct"]), name
    stats = keep.compact_atlas()
    after = {k: keep.image_rect(k) for k in before}
    for name in COMPACTED:
        HA.render(keep, name)
        frames[f"{name}/compacted"] = keep.read_pixels().copy()
    keep.close()
    fresh = HipContext(atlas_size=HA.ATLAS, device=0)
    if cull is not None:
        fresh.set_cull(cull)
    placed = HA.put_images(fresh, order=compaction_order(HA.images()))
    for name in COMPACTED:
        HA.render(fresh, name)
        frames[f"{name}/fresh"] = fresh.read_pixels().copy()
    fresh.close()
    info["compaction"] = {"moved": sum(before[k] != after[k] for k in before), "entries": len(before), "stats": stats,
                          "after": {str(k): list(v) for k, v in after.items()}, "fresh": {str(k): list(v) for k, v in placed.items()}}
    info["seconds"] = time.time() - t0
    return frames, info


_RUNS = {}


def run(setting):
    """(frames, info) of a fresh child process under `setting`; one child per setting and session"""
    if setting not in _RUNS:
        env, cull = SETTINGS[setting]
        code = ("import sys, json, numpy as np\n"
                "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                "import test_hostile_atlas as T\n"
                "frames, info = T.render_all(%r)\n"
                "np.savez(sys.argv[1], **frames)\n"
                "json.dump(info, open(sys.argv[2], 'w'))\n") % (ROOT, HERE, cull)
        with tempfile.TemporaryDirectory() as td:
            path, ipath = os.path.join(td, "frames.npz"), os.path.join(td, "info.json")
            try:
                r = subprocess.run([sys.executable, "-c", code, path, ipath], env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired:
                pytest.exit(f"hostile atlas: the child under {setting} hung; nothing more is started on this device", returncode=3)
            if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stderr:  # a fault: no further child, no further test on the device
                pytest.exit(f"hostile atlas: the child under {setting} died with {r.returncode}: {r.stderr[-2000:]}", returncode=3)
            assert r.returncode == 0, (setting, r.returncode, r.stderr[-2000:])
            with open(ipath) as f:
                _RUNS[setting] = (dict(np.load(path)), json.load(f))
    return _RUNS[setting]


def _forced():
    return os.environ.get("FDH_FORCE_KERNEL_PATHS")  # (tools/suite_off_defaults.sh runs the suite under a forced build)


def _far_pixels(a, b, bar, allowed):
    """pixels where a and b differ by more than `bar`, but for those of `allowed`, each of which may differ by bar + 1"""
    d = np.abs(a.astype(int) - b.astype(int)).max(axis=2)
    bad = d > bar
    for x, y in allowed:
        bad[y, x] = d[y, x] > bar + 1
    ys, xs = np.nonzero(bad)
    return [(int(x), int(y), int(d[y, x])) for x, y in zip(xs, ys)]


def _share_cap(entry):
    ref = entry["oracle_vs_swiftshader"]["n_gt0"] if entry.get("golden", "") is not None else 0  # (no golden: the project's 0.5 % alone)
    return max(0.005, ref / (HA.W * HA.H)) * HA.W * HA.H


def _hold_to_the_oracle(got, want, name, form, entry):
    amplified = [(x, y) for x, y, _ in HA.AMPLIFIED.get((name, form), [])]
    assert len(amplified) <= HA.MAX_AMPLIFIED
    far = _far_pixels(got, want, 1, amplified)
    assert not far, (name, form, "vs oracle: beyond 1 LSB at (x, y, difference)", far[:20], len(far))
    n0 = diff_stats(got, want)[1]
    assert n0 <= _share_cap(entry), (name, form, "vs oracle: too many pixels differ", n0, _share_cap(entry))


@pytest.mark.parametrize("form", HA.FORMS)
@pytest.mark.parametrize("name", HA.FRAMES)
def test_frames_match_the_oracle_and_the_shaders(name, form, golden_manifest, capsys):
    """(a) measured on an MI355X: profiles/hostile_atlas.txt"""
    from test_hostile_atlas_host import oracle_frame

    got = run("default")[0][f"{name}/{form}"]
    want = oracle_frame(name, form)
    entry = golden_manifest[f"hostile_atlas_{name}"]
    o_mx, o_n0, o_n1 = diff_stats(got, want)
    line = f"\n  hostile atlas {name:13s} {form:6s}: vs oracle max {o_mx} LSB, {o_n0} px differ, {o_n1} by > 1"
    gold = None
    if form == "direct" and name in HA.GOLDEN_FRAMES:
        gold = load_png(f"ss_hostile_atlas_{name}.png")
        g_mx, g_n0, g_n1 = diff_stats(got, gold)
        ref = entry["oracle_vs_swiftshader"]
        line += f"; vs the shaders' golden max {g_mx}, {g_n0} px differ, {g_n1} by > 1 (the oracle against it: max {ref['max']}, {ref['n_gt0']}, {ref['n_gt1']})"
    with capsys.disabled():
        print(line, end="")
    _hold_to_the_oracle(got, want, name, form, entry)
    if gold is not None:
        listed = [tuple(p) for p in entry["oracle_gt1"]]
        assert len(listed) <= HA.MAX_GOLDEN_OUTLIERS
        d = np.abs(got.astype(int) - gold.astype(int)).max(axis=2)
        for x, y in listed:
            d[y, x] = 0
        ys, xs = np.nonzero(d > 2)
        assert len(xs) == 0, (name, "vs the reference's shaders: beyond 2 LSB at", list(zip(xs.tolist(), ys.tolist()))[:20], len(xs))


@pytest.mark.parametrize("setting", [s for s in SETTINGS if s != "default"])
def test_no_switch_changes_a_pixel(setting):
    """(b) every build of the kernel forced onto every frame, no shrinking to the ink (what holds draw_msdf's cut to "changes no pixel"),
    no direct launches, no / only deep strips, no folded clear, no opaque-surface stores, no culling: the frames of the default, bit for
    bit.  `rotated`, `rotated_mix` and `minified` do not take build <2> alone: that they equal themselves under every forced build is what
    shows their own builds agree with it."""
    base, other = run("default")[0], run(setting)[0]
    assert base.keys() == other.keys()
    for key in base:
        assert np.array_equal(base[key], other[key]), (setting, key, int((base[key] != other[key]).any(axis=2).sum()), "pixels differ")


def test_stripes_and_retained_scenes_equal_the_whole_frame():
    """(c) three row stripes that are no multiples of 8 tall, stitched; fdh_scene_retain + fdh_scene_render for the node-level frames"""
    frames = run("default")[0]
    for name in HA.STRIPE_FRAMES:
        assert np.array_equal(frames[f"{name}/stripes"], frames[f"{name}/lists"]), name
    for name in HA.NODE_FRAMES:
        assert np.array_equal(frames[f"{name}/retained"], frames[f"{name}/lists"]), name


def test_a_compaction_moves_the_entries_and_no_pixel_it_should_not(golden_manifest, capsys):
    """(c) fdh_compact_atlas between two renders of a frame on a keep-mode context: the entries move, the uv rects change.  The second
    frame equals a fresh context's after the same puts in compaction order -- bit for bit where texels land 1:1 on pixels (`one_to_one`);
    the others are held to the oracle, its images put in that order, with the bars of (a)"""
    from oracle import oracle as O

    frames, info = run("default")
    c = info["compaction"]
    assert c["after"] == c["fresh"], "the repacked rectangles are those of the same puts in compaction order"
    assert c["moved"] > c["entries"] // 2, c
    o = O.Oracle(atlas_size=HA.ATLAS, threads=8)
    rects = HA.put_images(o, order=compaction_order(HA.images()))
    assert {str(k): list(v) for k, v in rects.items()} == c["after"]
    with capsys.disabled():
        print(f"\n  hostile atlas compaction: {c['moved']} of {c['entries']} entries moved", end="")
    for name in COMPACTED:
        same = np.array_equal(frames[f"{name}/compacted"], frames[f"{name}/fresh"])
        with capsys.disabled():
            print(f"; {name}: equals the fresh context's frame: {same}", end="")
        if name == "one_to_one":
            assert same, (name, int((frames[f"{name}/compacted"] != frames[f"{name}/fresh"]).any(axis=2).sum()), "pixels differ")
        HA.render(o, name)
        want = o.read_pixels().copy()
        for form in ("compacted", "fresh"):
            _hold_to_the_oracle(frames[f"{name}/{form}"], want, name, form, golden_manifest[f"hostile_atlas_{name}"])


def test_the_frames_go_where_they_are_aimed(capsys):
    """(d) the direct forms of the families whose quads are all upright, unmirrored and sampled at level 0 take no bin launch, every other
    direct form and every lists form takes one (rotated, mirrored and minified quads never go the direct way); every frame is drawn on;
    what the module took"""
    frames, info = run("default")
    with capsys.disabled():
        print("\n  ms_bin of the direct forms:", {n: round(info[f"{n}/direct"][0], 4) for n in HA.FRAMES}, end="")
        print(f"\n  a child of this module (every frame, form, stripe, retained scene and compaction): {info['seconds']:.1f} s", end="")
    for name in HA.FRAMES:
        clear = np.floor(np.array(HA.clear_of(name)) * 255 + 0.5).astype(np.uint8)
        for form in HA.FORMS:
            assert int((frames[f"{name}/{form}"] != clear).any(axis=2).sum()) > 2000, (name, form)
        assert info[f"{name}/lists"][0] > 0, (name, "the lists form took no bin launch", info[f"{name}/lists"])
        direct = name in HA.TAKES_DIRECT_LAUNCH and _forced() not in ("3", "8", "19")
        assert (info[f"{name}/direct"][0] == 0) == direct, (name, "ms_bin of the direct form", info[f"{name}/direct"])
