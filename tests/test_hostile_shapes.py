"""GPU suite: the compositor's kernels on hostile geometry (tests/hostile_cases.py) -- against the oracle, against what the reference's own
shaders made of the same frames (tests/golden/ss_hostile_<name>.png), and against themselves under every switch that picks another path.

Every fast path of k_composite*.hip and k_bin_upload.hip is a geometric argument; the frames put the arguments where they are tightest
(sub-pixel boxes, radii beyond the box, strokes wider than the node, shadows with blur 0 or wider than the frame, negative spread, AA
factors 0.05 .. 50, degenerate curves, empty clips, coordinates +-40000, 300 alpha-1 layers), each as a frame of at most 64 draws per
phase and as shifted copies that pass 64 (bin launch, deep lists).

Bars.  Against the oracle: at most 1 LSB (the pixels of hostile_cases.AMPLIFIED, each with its reason: 2), and the share of pixels that
differ at all at most the larger of 0.5 % (the project's bar) and the share on which the ORACLE differs from the shaders' golden of that
frame (manifest.json; `stack` and some node frames exceed 0.5 % between the reference pair itself).  Against the golden: at most 2 LSB
(north star) outside the pixels the manifest lists -- where the oracle itself is more than 1 LSB from the golden, at most 8 per frame
(tests/test_hostile_shapes_host.py holds the list to that).

All frames come from child processes, one per setting (the switches are read once per process): the default's are held to the bars, the
others' must equal the default's bit for bit."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import hostile_cases as HC
from conftest import diff_stats, load_png

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# setting -> (environment, set_cull mode or None)
SETTINGS = {"default": ({}, None)}
SETTINGS.update({f"FDH_FORCE_KERNEL_PATHS={v}": ({"FDH_FORCE_KERNEL_PATHS": str(v)}, None) for v in (1, 2, 3, 8, 19)})
SETTINGS.update({f"{k}={v}": ({k: str(v)}, None) for k, v in (("FDH_DIRECT", 0), ("FDH_CORE_UNION", 0), ("FDH_DEEP_MIN", 0), ("FDH_DEEP_MIN", 1),
                                                             ("FDH_FOLD_CLEAR", 0), ("FDH_OPAQUE", 0))})
SETTINGS["set_cull=0"] = ({}, 0)
# the frames without clip operations, rotated quads or curves: the build of the compositor that has the deep strips
PLAIN_BUILD = ("slivers", "radii", "strokes", "shadows", "gradients", "far", "stack")


def render_all(cull=None):
    """(a child process) every frame in both forms on one context -> name/form: pixels; name/form: [ms_bin, deep_bins, digest hash, digest entries].
    The lists forms are rendered four times (the second frame on has the bin order, the third the count of deep bins); those of
    STRIPE_FRAMES again as three row stripes, stitched; those of the node-level frames again as retained scenes."""
    from figdraw_amd.context import HipContext

    ctx = HipContext(device=0)
    if cull is not None:
        ctx.set_cull(cull)
    frames, info = {}, {}
    for name in HC.FRAMES:
        for form in HC.FORMS:
            key = f"{name}/{form}"
            for _ in range(4 if form == "lists" else 1):
                HC.render(ctx, name, form)
                ctx.sync()
            frames[key] = ctx.read_pixels().copy()
            deep = float(ctx.frame_stats().deep_bins)
            digest = [int(v) for v in ctx.bin_digest()[:2]]
            ctx.profile(1)
            info[key] = [float(ctx.frame_stats().ms_bin), deep] + digest
            if form == "lists" and name in HC.STRIPE_FRAMES:
                whole = np.zeros_like(frames[key])
                for y0, y1 in HC.STRIPES:
                    ctx.set_stripe(y0, y1)
                    HC.render(ctx, name, form)
                    whole[y0:y1] = ctx.read_pixels()[y0:y1]
                ctx.set_stripe(0, 0)
                frames[f"{name}/stripes"] = whole
            if form == "lists" and HC.is_node_frame(name):
                ctx.scene_retain(HC.scene(name, form), HC.W, HC.H, color=tuple(HC.clear_of(name)))
                ctx.scene_render()
                frames[f"{name}/retained"] = ctx.read_pixels().copy()
    ctx.close()
    return frames, info


_RUNS = {}


def run(setting):
    """(frames, info) of a fresh child process under `setting`; one child per setting and session"""
    if setting not in _RUNS:
        env, cull = SETTINGS[setting]
        code = ("import sys, json, numpy as np\n"
                "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                "import test_hostile_shapes as T\n"
                "frames, info = T.render_all(%r)\n"
                "np.savez(sys.argv[1], **frames)\n"
                "json.dump(info, open(sys.argv[2], 'w'))\n") % (ROOT, HERE, cull)
        with tempfile.TemporaryDirectory() as td:
            path, ipath = os.path.join(td, "frames.npz"), os.path.join(td, "info.json")
            try:
                r = subprocess.run([sys.executable, "-c", code, path, ipath], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
            except subprocess.TimeoutExpired:
                pytest.exit(f"hostile shapes: the child under {setting} hung; nothing more is started on this device", returncode=3)
            if r.returncode < 0 or r.returncode in (134, 139):  # a fault: no further child, no further test on the device
                pytest.exit(f"hostile shapes: the child under {setting} died with {r.returncode}: {r.stderr[-2000:]}", returncode=3)
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


@pytest.mark.parametrize("form", HC.FORMS)
@pytest.mark.parametrize("name", HC.FRAMES)
def test_frames_match_the_oracle_and_the_shaders(name, form, golden_manifest, capsys):
    """(a) measured on an MI355X: profiles/hostile_shapes.txt"""
    from test_hostile_shapes_host import oracle_frame

    got = run("default")[0][f"{name}/{form}"]
    want = oracle_frame(name, form)
    entry = golden_manifest[f"hostile_{name}"]
    o_mx, o_n0, o_n1 = diff_stats(got, want)
    line = f"\n  hostile {name:10s} {form:6s}: vs oracle max {o_mx} LSB, {o_n0} px differ, {o_n1} by > 1"
    gold = None
    if form == "direct":
        gold = load_png(f"ss_hostile_{name}.png")
        g_mx, g_n0, g_n1 = diff_stats(got, gold)
        ref = entry["oracle_vs_swiftshader"]
        line += f"; vs the shaders' golden max {g_mx}, {g_n0} px differ, {g_n1} by > 1 (the oracle against it: max {ref['max']}, {ref['n_gt0']}, {ref['n_gt1']})"
    with capsys.disabled():
        print(line, end="")
    amplified = [(x, y) for x, y, _ in HC.AMPLIFIED.get((name, form), [])]
    assert len(amplified) <= HC.MAX_AMPLIFIED
    far = _far_pixels(got, want, 1, amplified)
    assert not far, (name, form, "vs oracle: beyond 1 LSB at (x, y, difference)", far[:20], len(far))
    cap = max(0.005, entry["oracle_vs_swiftshader"]["n_gt0"] / (HC.W * HC.H)) * HC.W * HC.H
    assert o_n0 <= cap, (name, form, "vs oracle: too many pixels differ", o_n0, cap)
    if gold is not None:
        listed = [tuple(p) for p in entry["oracle_gt1"]]
        assert len(listed) <= HC.MAX_GOLDEN_OUTLIERS
        d = np.abs(got.astype(int) - gold.astype(int)).max(axis=2)
        for x, y in listed:
            d[y, x] = 0
        ys, xs = np.nonzero(d > 2)
        assert len(xs) == 0, (name, "vs the reference's shaders: beyond 2 LSB at", list(zip(xs.tolist(), ys.tolist()))[:20], len(xs))


@pytest.mark.parametrize("setting", [s for s in SETTINGS if s != "default"])
def test_no_switch_changes_a_pixel(setting):
    """(b) every build of the kernel forced onto every frame, no direct launches, one core rectangle, no / only deep strips, no folded
    clear, no opaque-surface stores, no culling: the frames of the default, bit for bit"""
    base, other = run("default")[0], run(setting)[0]
    assert base.keys() == other.keys()
    for key in base:
        assert np.array_equal(base[key], other[key]), (setting, key, int((base[key] != other[key]).any(axis=2).sum()), "pixels differ")


def test_stripes_and_retained_scenes_equal_the_whole_frame():
    """(c) three row stripes that are no multiples of 8 tall, stitched; fdh_scene_retain + fdh_scene_render (node-level frames: a call-level
    frame has no retained form)"""
    frames = run("default")[0]
    for name in HC.STRIPE_FRAMES:
        assert np.array_equal(frames[f"{name}/stripes"], frames[f"{name}/lists"]), name
    for name in HC.NODE_FRAMES:
        assert np.array_equal(frames[f"{name}/retained"], frames[f"{name}/lists"]), name


def test_the_frames_go_where_they_are_aimed(capsys):
    """(d) direct forms without a bin launch (where the library's rule allows one: no rotated quad, no curve), lists forms with one; deep
    strips under FDH_DEEP_MIN=1 (the build without clip operations has them); the union of core rectangles changes the bin lists of
    `radii`; every frame is drawn on"""
    frames, info = run("default")
    deep = run("FDH_DEEP_MIN=1")[1]
    with capsys.disabled():
        print("\n  ms_bin of the direct forms:", {n: round(info[f"{n}/direct"][0], 4) for n in HC.FRAMES}, end="")
        print("\n  deep bins under FDH_DEEP_MIN=1:", {n: deep[f"{n}/lists"][1] for n in HC.FRAMES}, end="")
    for name in HC.FRAMES:
        clear = np.round(np.array(HC.clear_of(name)) * 255).astype(np.uint8)
        for form in HC.FORMS:
            assert int((frames[f"{name}/{form}"] != clear).any(axis=2).sum()) > 2000, (name, form)
        assert info[f"{name}/lists"][0] > 0, (name, "the lists form took no bin launch", info[f"{name}/lists"])
        direct = name in HC.TAKES_DIRECT_LAUNCH and _forced() not in ("3", "8", "19")
        assert (info[f"{name}/direct"][0] == 0) == direct, (name, "ms_bin of the direct form", info[f"{name}/direct"])
    for name in PLAIN_BUILD:
        if _forced() in ("1", "2", "3", "8", "19"):  # (a forced build is not the one with the deep strips)
            assert deep[f"{name}/lists"][1] == 0, (name, deep[f"{name}/lists"])
        else:
            assert deep[f"{name}/lists"][1] > 0, (name, deep[f"{name}/lists"])
    assert all(v[1] == 0 for v in run("FDH_DEEP_MIN=0")[1].values())
    one = run("FDH_CORE_UNION=0")[1]
    assert info["radii/lists"][2] != one["radii/lists"][2], (info["radii/lists"], one["radii/lists"])
    assert 0 < info["radii/lists"][3] <= one["radii/lists"][3]
