"""GPU suite: the HIP path (through the C ABI) against the oracle and the committed goldens.

Bar (north_star): within 2 LSB per channel of the reference's output.  What is asserted here is tighter:
  * HIP vs oracle on the same scene: max 1 LSB, and at most 0.5 % of pixels differ at all
    (float32 both sides; the HIP kernels use v_rcp/v_sqrt/v_exp approximations, the oracle libm)
  * HIP vs the reference's golden PNGs / the reference's GLSL on SwiftShader: max 2 LSB
"""
import numpy as np
import pytest

import ref_scenes as RS
from conftest import diff_stats, load_png

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from figdraw_amd.context import HipContext

    ctx = HipContext(device=0)
    yield ctx
    ctx.close()


def _oracle(fn, w, h):
    from oracle import oracle as O

    o = O.Oracle(threads=8)
    o.render_frame(fn(float(w), float(h)), w, h)
    return o.read_pixels()


ALL = {k: v[:3] for k, v in RS.REFERENCE_PNG_SCENES.items()}
ALL.update(RS.SWIFTSHADER_SCENES)


@pytest.mark.parametrize("name", sorted(ALL))
def test_scene_matches_oracle_and_goldens(hip, name):
    fn, w, h = ALL[name]
    hip.render_frame(fn(float(w), float(h)), w, h)
    got = hip.read_pixels()
    want = _oracle(fn, w, h)
    mx, n0, n1 = diff_stats(got, want)
    assert mx <= 1, (name, "vs oracle", mx, n0, n1)
    assert n0 <= 0.005 * w * h, (name, "vs oracle: too many 1-LSB pixels", n0)
    mx, n0, n1 = diff_stats(got, load_png(f"ss_{name}.png"))
    assert mx <= 2, (name, "vs reference GLSL on SwiftShader", mx, n0, n1)
    if name in RS.REFERENCE_PNG_SCENES and name != "layers_rect_mask":
        mx, n0, n1 = diff_stats(got, load_png("ref_" + RS.REFERENCE_PNG_SCENES[name][3]))
        assert mx <= 2, (name, "vs reference golden PNG", mx, n0, n1)


@pytest.mark.parametrize("name", sorted(RS.OUTLIER_SCENES))
def test_counted_goldens(hip, name):
    """rotated quads and curves against the reference's shaders on SwiftShader (ref_scenes.OUTLIER_SCENES): within 2 LSB but for the
    counted pixels the golden itself differs on from any float evaluation; against the oracle the usual bar"""
    fn, w, h, allowed = RS.OUTLIER_SCENES[name]
    hip.render_frame(fn(float(w), float(h)), w, h)
    got = hip.read_pixels()
    mx, n0, n1 = diff_stats(got, _oracle(fn, w, h))
    assert mx <= 1 and n0 <= 0.005 * w * h, (name, "vs oracle", mx, n0, n1)
    gold = load_png(f"ss_{name}.png")
    far = np.abs(got.astype(int) - gold.astype(int)).max(axis=2) > 2
    n_gt2 = int(far.sum())
    assert n_gt2 <= allowed, (name, "vs reference GLSL on SwiftShader", n_gt2)
    if name == "rotated_tree":  # (whatever the count: every such pixel's centre lies on an edge of a rotated quad -- test_oracle.py says why)
        from figdraw_amd.context import HipContext

        rec = HipContext(record_only=True)
        rec.record_begin()
        rec.render_frame(fn(float(w), float(h)), w, h)
        quads = RS.quads_of_call_stream(rec.record_calls())
        rec.close()
        ys, xs = np.nonzero(far)
        assert RS.worst_distance_to_a_quad_edge(zip(xs, ys), quads) < 0.05


FUZZ = [(1, 333, 217, True, True), (2, 640, 480, True, False), (3, 257, 129, False, True), (4, 1000, 70, True, True),
        (5, 65, 600, False, False), (6, 512, 512, False, False), (7, 799, 601, True, True), (8, 1283, 721, False, True),
        (9, 9000, 90, True, True), (10, 70, 8400, False, True)]  # > 128 bins along an axis: bin boxes in 128-px units


@pytest.mark.parametrize("seed,w,h,clips,blur", FUZZ)
def test_random_scenes_match_oracle(hip, seed, w, h, clips, blur):
    """Seeded random scenes at odd frame sizes: the bin kernel's strip masks, saturated cores, bin-time stroke removal
    and occlusion culling (only legal in phases without mask ops: `clips` toggles that) must not change a pixel."""
    sc = RS.random_scene(seed, float(w), float(h), n=60, clips=clips, blur=blur)
    hip.render_frame(sc, w, h)
    got = hip.read_pixels()
    want = _oracle(lambda *_: sc, w, h)
    mx, n0, n1 = diff_stats(got, want)
    assert mx <= 1, (seed, "vs oracle", mx, n0, n1)
    assert n0 <= 0.005 * w * h, (seed, "vs oracle: too many 1-LSB pixels", n0)


def test_render_is_deterministic_and_replay_is_idempotent(hip):
    fn, w, h = RS.SWIFTSHADER_SCENES["backdrop_blur"]
    hip.render_frame(fn(float(w), float(h)), w, h)
    a = hip.read_pixels()
    hip.replay(3)
    b = hip.read_pixels()
    hip.render_frame(fn(float(w), float(h)), w, h)
    c = hip.read_pixels()
    assert (a == b).all() and (a == c).all()


@pytest.mark.parametrize("paths", [1, 2, 3, 8, 19])
def test_every_kernel_build_gives_the_same_pixels(hip, paths):
    """k_composite_tiles comes in five builds picked per phase: <4> SDF draws without clip operations, <0> + clip masks,
    <2> + the 4-wide atlas path, <8> + the 4-wide path for rotated SDF quads, <3> + everything incl. the one-pixel-slot path (the
    first three live in the uniform-regions translation unit, the last two in the default one).  Forcing the more general builds
    (1: <0>, 2: <2>, 8: <8>, 3: <3>, 19: <3> at the register budget of phases with atlas quads off the 4-wide path) onto scenes that do not need them (a child process with FDH_FORCE_KERNEL_PATHS) must not
    change a pixel -- the rotated scenes included, whose quads <8> and <3> shade with the same code."""
    import os
    import subprocess
    import sys
    import tempfile

    names = ["oneframe", "nested_clips", "elliptical_and_fractional", "backdrop_blur", "rotation_and_transform"]
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import ref_scenes as RS\n"
        "from figdraw_amd.context import HipContext\n"
        "ctx = HipContext(device=0)\n"
        "out = {}\n"
        "for n in %r:\n"
        "    fn, w, h = RS.SWIFTSHADER_SCENES[n]\n"
        "    ctx.render_frame(fn(float(w), float(h)), w, h); out[n] = ctx.read_pixels()\n"
        "sc = RS.random_scene(21, 700.0, 500.0, n=70)\n"
        "ctx.render_frame(sc, 700, 500); out['fuzz'] = ctx.read_pixels()\n"
        "from figdraw_amd.scenes import make_rotated_tree\n"
        "ctx.render_frame(make_rotated_tree(1280, 720, 3, copies=30), 1280, 720); out['rotated'] = ctx.read_pixels()\n"
        "# glyph rows turned by 2 degrees: atlas quads off the 4-wide path -- by default the slot build's 168-register form <19>, forced 3: <3> itself\n"
        "from figdraw_amd.scenes import make_glyph_scene, load_glyph_fixture\n"
        "imgs = load_glyph_fixture(%r)\n"
        "ctx2 = HipContext(atlas_size=1024, device=0)\n"
        "sc = make_glyph_scene(900.0, 500.0, imgs, cols=22, rows=22, rotation=2.0)\n"
        "for k, v in RS.used_images(sc, imgs).items(): ctx2.put_image(k, v)\n"
        "ctx2.render_frame(sc, 900, 500); out['rotated_glyphs'] = ctx2.read_pixels()\n"
        "np.savez(sys.argv[1], **out)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)), names,
         os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glyphs_ubuntu20.npz"))
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("default", {}), ("forced", {"FDH_FORCE_KERNEL_PATHS": str(paths)})):
            path = os.path.join(td, tag + ".npz")
            subprocess.check_call([sys.executable, "-c", code, path], env={**os.environ, **env})
            res[tag] = dict(np.load(path))
        for k in res["default"]:
            assert np.array_equal(res["default"][k], res["forced"][k]), (paths, k)


def test_invert_known_answers_of_the_references_tests():
    """The reference's own assertions on NfInvertY (tests/trender_image_msdf_invert.nim:224-262, tests/trender_text_invert.nim:918-943:
    row profiles and ink bounds, ref_scenes.check_*) on the HIP path's frames, which must also be the oracle's within the suite's bar."""
    import os

    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import load_glyph_fixture
    from oracle import oracle as O

    glyphs = load_glyph_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glyphs_ubuntu20.npz"))
    text = RS.text_invert(640.0, 360.0, glyphs)
    for sc, imgs, w, h, check in ((RS.image_msdf_invert(), RS.invert_test_images(), 720, 520, RS.check_image_msdf_invert),
                                  (text, RS.used_images(text, glyphs), 640, 360, RS.check_text_invert)):
        ctx, orc = HipContext(device=0, atlas_size=1024), O.Oracle(atlas_size=1024, threads=8)
        for k in sorted(imgs):
            ctx.put_image(k, imgs[k]); orc.put_image(k, imgs[k])
        ctx.render_frame(sc, w, h); orc.render_frame(sc, w, h)
        got = ctx.read_pixels()
        check(got)
        mx, n0, n1 = diff_stats(got, orc.read_pixels())
        # (the 24 x 24 images are drawn 7.5 times their size: whole bands of the bilinear ramp between two texel rows sit on x.5, and
        # v_rcp's last bit decides them -- 0.9 % of the frame at 1 LSB; the suite's usual count bar is for frames of UI content)
        assert mx <= 1 and n0 <= 0.015 * w * h, (mx, n0, n1)
        ctx.close()


def test_direct_launches_give_the_same_pixels():
    """Round 6: a frame every phase of which holds at most 64 draws has no bin launch -- the compositor's waves make their bin's list
    entries themselves, with the functions k_bin_draws makes them with (bin_entry_head / bin_entry_tail; fdh_context.cpp direct_frame).
    FDH_DIRECT=0 keeps the bin launch: the frames must be equal bit for bit -- scenes of every build of the kernel that has the path (no
    clips, clips and rect masks, atlas quads), stroke interiors that drop out of their entries, a blur node (two phases), a frame size that
    is no multiple of 64, and one scene ABOVE the limit that must not take the path."""
    import os
    import subprocess
    import sys
    import tempfile

    names = ["rgb_boxes_sdf", "rgb_boxes", "linear_gradient", "layers_clip", "layers_rect_mask", "oneframe", "elliptical_and_fractional", "nested_clips", "rect_mask_nested",
             "backdrop_blur", "rect_mask_mixed_batch"]
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import ref_scenes as RS\n"
        "from figdraw_amd.context import HipContext\n"
        "from figdraw_amd.scenes import make_render_tree_100\n"
        "ALL = {k: v[:3] for k, v in RS.REFERENCE_PNG_SCENES.items()}; ALL.update(RS.SWIFTSHADER_SCENES)\n"
        "ctx = HipContext(device=0)\n"
        "out = {}; bins = {}\n"
        "for n in %r:\n"
        "    fn, w, h = ALL[n]\n"
        "    ctx.render_frame(fn(float(w), float(h)), w, h); out[n] = ctx.read_pixels(); ctx.profile(1); bins[n] = ctx.frame_stats().ms_bin\n"
        "ctx.render_frame(make_render_tree_100(700, 500, 2, copies=8), 700, 500); out['tree8'] = ctx.read_pixels(); ctx.profile(1); bins['tree8'] = ctx.frame_stats().ms_bin\n"
        "ctx.render_frame(make_render_tree_100(700, 500, 2, copies=40), 700, 500); out['tree40'] = ctx.read_pixels(); ctx.profile(1); bins['tree40'] = ctx.frame_stats().ms_bin\n"
        "np.savez(sys.argv[1], **out)\n"
        "print('BINMS', bins)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)), names)
    with tempfile.TemporaryDirectory() as td:
        res, binms = {}, {}
        for tag, env in (("bin", {"FDH_DIRECT": "0"}), ("direct", {"FDH_DIRECT": "1"})):
            path = os.path.join(td, tag + ".npz")
            r = subprocess.run([sys.executable, "-c", code, path], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res[tag] = dict(np.load(path))
            binms[tag] = eval([ln for ln in r.stdout.splitlines() if ln.startswith("BINMS ")][-1][6:])
    assert all(v > 0 for v in binms["bin"].values()), binms
    if os.environ.get("FDH_FORCE_KERNEL_PATHS") not in ("3", "8", "19"):  # (tools/suite_off_defaults.sh: the slot / rotated builds have no direct form)
        assert binms["direct"]["rgb_boxes_sdf"] == 0 and binms["direct"]["nested_clips"] == 0 and binms["direct"]["tree8"] == 0, binms   # no bin launch
    assert binms["direct"]["tree40"] > 0, binms  # (283 draws in its first phase: over the limit)
    for k in res["bin"]:
        assert np.array_equal(res["bin"][k], res["direct"][k]), (k, int((res["bin"][k] != res["direct"][k]).any(axis=2).sum()))


@pytest.mark.parametrize("deep_min", [1, 12])
def test_deep_strips_give_the_same_pixels(deep_min):
    """Round 6: the strips of the bins with the frame's longest lists are shaded by a workgroup of four waves -- three evaluate the draws'
    source terms, one blends them out of a ring in LDS, in list order (k_composite_deep, composite_strip's kRole).  Same operations on the
    same values as the one-wave strips: frames must not change by a bit whether no bin (FDH_DEEP_MIN=0), every bin that holds a draw (1) or
    the deep ones (12) go that way -- the bench tree at 1080p, at a size that is no multiple of 32 and at 4K with its blur nodes (solid /
    gradient / 3-stop fills, strokes, drop and inner shadows, elliptical corners, shared distance fields, opaque cores that cut the lists),
    fuzz scenes.  Child processes (the threshold is read once); every scene is rendered four times: the second frame on has the order, the
    third the sorting waves' count of deep bins."""
    import os
    import subprocess
    import sys
    import tempfile

    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import ref_scenes as RS\n"
        "from figdraw_amd.context import HipContext\n"
        "from figdraw_amd.scenes import make_render_tree_100\n"
        "out = {}; q = {}\n"
        "cases = [('tree1080', lambda: make_render_tree_100(1920, 1080, 3), 1920, 1080), ('tree_odd', lambda: make_render_tree_100(1003, 617, 1, copies=60), 1003, 617),\n"
        "         ('tree720', lambda: make_render_tree_100(1280, 720, 7), 1280, 720),\n"
        "         ('tree4k_blur', lambda: make_render_tree_100(3840, 2160, 0, full_frame_blur=True), 3840, 2160),\n"
        "         ('fuzz31', lambda: RS.random_scene(31, 900.0, 500.0, n=120, clips=False, blur=False), 900, 500),\n"
        "         ('fuzz32', lambda: RS.random_scene(32, 640.0, 360.0, n=200, clips=False, blur=True), 640, 360)]\n"
        "for name, fn, w, h in cases:\n"
        "    ctx = HipContext(device=0)\n"
        "    for i in range(4):\n"
        "        ctx.render_frame(fn(), w, h); ctx.sync()\n"
        "    out[name] = ctx.read_pixels(); q[name] = ctx.frame_stats().deep_bins; ctx.close()\n"
        "np.savez(sys.argv[1], **out)\n"
        "print('DEEP', q)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        res, deep = {}, {}
        for tag, env in (("off", {"FDH_DEEP_MIN": "0"}), ("on", {"FDH_DEEP_MIN": str(deep_min)})):
            path = os.path.join(td, tag + ".npz")
            r = subprocess.run([sys.executable, "-c", code, path], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res[tag] = dict(np.load(path))
            deep[tag] = eval([ln for ln in r.stdout.splitlines() if ln.startswith("DEEP ")][-1][5:])
    assert all(v == 0 for v in deep["off"].values()), deep
    # (the fuzz scenes' first phase holds rotated quads: another build of the kernel, no deep strips -- they ride along as a check that
    # the switch changes nothing there either)
    if os.environ.get("FDH_FORCE_KERNEL_PATHS") not in ("1", "2", "3", "8", "19"):
        assert deep["on"]["tree1080"] > 0 and deep["on"]["tree_odd"] > 0 and deep["on"]["tree720"] > 0 and (deep_min > 1 or deep["on"]["tree4k_blur"] > 0), deep
    else:  # (tools/suite_off_defaults.sh: a forced build is not the <4> build -- no deep strips, and deep_bins reports what the launch ran)
        assert all(v == 0 for v in deep["on"].values()), deep
    for k in res["off"]:
        assert np.array_equal(res["off"][k], res["on"][k]), (deep_min, k, int((res["off"][k] != res["on"][k]).any(axis=2).sum()), deep["on"][k])


@pytest.mark.parametrize("w,h,copies,frame", [(1280, 720, 40, 0), (1920, 1080, 100, 5), (803, 601, 25, 2)])
def test_rotated_tree_matches_oracle(w, h, copies, frame):
    """Every rectangle of the renderlist_100 tree rotated by -30 .. 30 degrees (config 9 of tools/perf_configs.py): rotated quads
    four pixels per lane (32-bit edge functions, two-triangle barycentrics), strips outside a quad dropped at bin time, saturated
    cores of rotated boxes (uniform blends, removed stroke interiors, occlusion) -- against the oracle's per-pixel rasteriser."""
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import make_rotated_tree
    from oracle import oracle as O

    sc = make_rotated_tree(w, h, frame, copies=copies)
    ctx = HipContext(device=0)
    ctx.render_frame(sc, w, h)
    got = ctx.read_pixels()
    o = O.Oracle(threads=8)
    o.render_frame(sc, w, h)
    mx, n0, n1 = diff_stats(got, o.read_pixels())
    assert mx <= 1 and n0 <= 0.005 * w * h, (mx, n0, n1)
    ctx.set_stripe(h // 3 // 8 * 8, h // 3 // 8 * 8 + 104)  # a row stripe of it: the same pixels
    ctx.render_frame(sc, w, h)
    y0 = h // 3 // 8 * 8
    assert np.array_equal(ctx.read_pixels()[y0:y0 + 104], got[y0:y0 + 104])
    ctx.close()


@pytest.mark.parametrize("rotation", [2.0, -11.0, 90.0])
def test_rotated_glyph_rows_match_oracle(rotation):
    """Config 11 of tools/perf_configs.py in small: text rows (mode-0 glyph quads with a vertical tint) and MSDF images under a
    rotated transform -- rotated atlas quads four pixels per lane (two-triangle coverage, barycentric uv between the atlas corners,
    per-triangle LOD and fwidth) -- against the oracle."""
    import os

    from conftest import GOLDEN
    from figdraw_amd.scenes import load_glyph_fixture, make_glyph_scene

    w, h = 900, 500
    imgs = load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz"))
    sc = make_glyph_scene(w, h, imgs, cols=22, rows=20, rotation=rotation)
    ctx, o = _atlas_ctx_pair(sc, RS.used_images(sc, imgs), 1024)
    ctx.render_frame(sc, w, h)
    o.render_frame(sc, w, h)
    mx, n0, n1 = diff_stats(ctx.read_pixels(), o.read_pixels())
    assert mx <= 1 and n0 <= 0.005 * w * h, (rotation, mx, n0, n1)
    ctx.close()


@pytest.mark.parametrize("w,h,n,seed,rotation", [(1280, 720, 300, 7, 0.0), (900, 700, 160, 11, 0.0), (1000, 640, 200, 5, 13.0)])
def test_curves_scene_matches_oracle(w, h, n, seed, rotation):
    """Stroked nkDrawable curves, lines and arcs (config 10 of tools/perf_configs.py): quadratic-bezier spans four pixels per lane
    (hardware transcendentals, both cases of the cubic selected), strips far from a curve dropped at bin time, lines as rotated
    boxes, join quads -- against the oracle's libm evaluation, pixel by pixel.

    The usual bar -- within 1 LSB of the oracle on every pixel -- holds here only because the kernels follow the oracle's
    arithmetic where the reference's formula is ill-conditioned: sdBezier (atlas.frag:121-160) solves the cubic in closed form
    and, in the one-root case, forms (sqrt(h) - q) / 2 where sqrt(h) ~ |q|; what survives the cancellation is rounding noise, so a
    last-bit difference in the input or in sqrt(h) moves a pixel's distance by up to a tenth of a pixel.  Measured on the first
    scene: the one-pixel-slot path with libm's powf / acosf (same formula) 76 pixels beyond 1 LSB; four pixels per lane with IEEE
    division / square root and no fused multiply-adds up to the roots 23; with the uv formed as the oracle's rasteriser forms it
    (the quad's two triangles, barycentrics in double precision) 0 (tools/debug/curves_diff.py)."""
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import make_curves_scene
    from oracle import oracle as O

    sc = make_curves_scene(w, h, n=n, seed=seed, rotation=rotation)  # (rotation: the drawables under rotated transforms -- bezier quads as rotated quads)
    ctx = HipContext(device=0)
    ctx.render_frame(sc, w, h)
    got = ctx.read_pixels()
    o = O.Oracle(threads=8)
    o.render_frame(sc, w, h)
    mx, n0, n1 = diff_stats(got, o.read_pixels())
    assert mx <= 1 and n0 <= 0.005 * w * h, (mx, n0, n1)
    ctx.close()


@pytest.mark.parametrize("path", [1, 2, 3])
def test_every_blur_path_matches_oracle(path):
    """The blur passes exist as three builds picked by region size and filter width: 2 outputs per thread (small regions),
    8-12 outputs per thread, and the matrix-pipe passes (large regions).  FDH_FORCE_BLUR_PATH puts every
    blur of a frame on one of them (a child process); each must stay within 1 LSB of the oracle for every filter width,
    with taps clamped at all four frame edges."""
    import os
    import subprocess
    import sys
    import tempfile

    # (the matrix-pipe passes need rows on 16-byte boundaries: widths that are not multiples of 4 fall back to path 2)
    white, glass = (1.0, 1.0, 1.0, 1.0), (0.2, 0.3, 0.4, 0.5)  # a translucent clear colour: the fused composite has to blend
    cases = [("sweep", 700, 420, None, white), ("sweep_odd", 333, 517, None, white), ("sweep_glass", 644, 388, None, glass),
             ("backdrop", 320, 240, None, white), ("backdrop_glass", 320, 240, None, glass), ("fuzz7", 799, 601, 7, white),
             ("fuzz7_clips", 800, 600, 7, white),  # a blur inside an open clip: the vertical pass writes the snapshot, unfused
             ("fuzz8", 1284, 720, 8, glass)]
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import ref_scenes as RS\n"
        "from figdraw_amd.context import HipContext\n"
        "ctx = HipContext(device=0)\n"
        "out = {}\n"
        "for name, w, h, seed, color in %r:\n"
        "    sc = RS.random_scene(seed, float(w), float(h), n=60, clips=(seed == 7), blur=True) if seed else (RS.backdrop_blur if name.startswith('backdrop') else RS.blur_sweep)(float(w), float(h))\n"
        "    ctx.render_frame(sc, w, h, color=color); out[name] = ctx.read_pixels()\n"
        "np.savez(sys.argv[1], **out)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)), cases)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "o.npz")
        subprocess.check_call([sys.executable, "-c", code, out], env={**os.environ, "FDH_FORCE_BLUR_PATH": str(path)})
        got = dict(np.load(out))
    from oracle import oracle as O

    for name, w, h, seed, color in cases:
        if seed:
            sc = RS.random_scene(seed, float(w), float(h), n=60, clips=(seed == 7), blur=True)
        else:
            sc = (RS.backdrop_blur if name.startswith("backdrop") else RS.blur_sweep)(float(w), float(h))
        o = O.Oracle(threads=8)
        o.render_frame(sc, w, h, color=color)
        want = o.read_pixels()
        mx, n0, n1 = diff_stats(got[name], want)
        assert mx <= 1, (path, name, "vs oracle", mx, n0, n1)
        assert n0 <= 0.005 * w * h, (path, name, "vs oracle: too many 1-LSB pixels", n0)


def test_matrix_pipe_blur_weights_keep_flat_colours():
    """The matrix-pipe passes multiply the taps as ONE f16 each (round 5): the rounding error is carried from the
    centre tap outwards so that the weights still sum to 1 (to ~1e-7).  A flat backdrop must therefore come out of a full-frame blur
    node exactly as it went in, for every filter width, both on the fused route and on the two passes, through a transparent and
    through a tinting node -- FDH_FORCE_BLUR_PATH=3 puts every blur on the matrix pipe (a child process)."""
    import os
    import subprocess
    import sys
    import tempfile

    w, h = 512, 192
    radii = [0.8, 1.0, 2.5, 5.0, 9.0, 13.0, 18.0, 27.5, 40.0, 64.0]
    colours = [(37, 129, 255, 255), (255, 255, 255, 255), (1, 2, 3, 255), (200, 100, 50, 255)]
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from ref_scenes import Fig, FigKind, RenderList, Renders, rect, rgba, RECT\n"
        "from figdraw_amd.context import HipContext\n"
        "ctx = HipContext(device=0)\n"
        "bad = []\n"
        "for route in (1, 0):\n"
        "    ctx.set_blur_route(route)\n"
        "    for radius in %r:\n"
        "        for c in %r:\n"
        "            lst = RenderList()\n"
        "            lst.addRoot(Fig(kind=RECT, screenBox=rect(0, 0, %d, %d), fill=rgba(*c)))\n"
        "            lst.addRoot(Fig(kind=FigKind.nkBackdropBlur, screenBox=rect(0, 0, %d, %d), fill=rgba(0, 0, 0, 0), blur=radius))\n"
        "            sc = Renders(); sc.layers[0] = lst\n"
        "            ctx.render_frame(sc, %d, %d); got = ctx.read_pixels()\n"
        "            if not (got == np.array(c, dtype=np.uint8)).all(): bad.append((route, radius, c, int((got != np.array(c, dtype=np.uint8)).any(axis=2).sum())))\n"
        "print('BAD', bad)\n"
        "sys.exit(1 if bad else 0)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)), radii, colours, w, h, w, h, w, h)
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "FDH_FORCE_BLUR_PATH": "3"}, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("kind", RS.HOSTILE_BLUR_KINDS)
@pytest.mark.parametrize("radius", RS.HOSTILE_BLUR_RADII)
def test_matrix_pipe_blur_on_hostile_content_matches_blur_frag(kind, radius, capsys):
    """The matrix-pipe passes (k_blur_fx, k_blur_mx) multiply every tap as ONE f16 with the rounding error carried outwards -- the one place
    where the product's arithmetic is deliberately narrower than blur.frag's float (glsl/blur.frag:11-32, glcontext.nim:1743-1786).  UI
    content forgives that; this is the content that does not: opaque white noise and a 0 / 255 checkerboard of 1-pixel cells at a size the
    kernels take natively (no FDH_FORCE_BLUR_PATH), both routes, against what the reference's own shader makes of it on SwiftShader
    (tests/golden/ss_blur_big_*.png, north-star bar: 2 LSB) and against the oracle (1 LSB).  The counts are printed: tools/blur_weights_pin.py
    commits them next to those of the 22-bit hi + lo build (profiles/r06_blur_weights_pin.txt)."""
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    w, h = RS.HOSTILE_BLUR_SIZE
    src = RS.hostile_blur_source(kind)
    gold = load_png(f"ss_blur_big_{kind}_r{radius:g}.png")
    want = O.blur_image(src, radius)
    ctx = HipContext(device=0, atlas_size=2048)
    ctx.put_image(RS.HOSTILE_BLUR_KEY, src)
    sc = RS.hostile_blur_scene(radius)
    for route, field in ((1, "ms_blur_fused"), (0, "ms_blur_big_h")):
        ctx.set_blur_route(route)
        ctx.render_frame(sc, w, h)
        got = ctx.read_pixels()
        ctx.profile(1)
        st = ctx.frame_stats()  # (radius 64 is wider than the fused kernel's widest build: both routes are then the two passes)
        assert getattr(st, field) > 0 or (radius > 30 and st.ms_blur_big_h > 0), (route, "the frame did not take the matrix-pipe kernel this test is about")
        g_mx, g_n0, g_n1 = diff_stats(got, gold)
        o_mx, o_n0, o_n1 = diff_stats(got, want)
        with capsys.disabled():
            print(f"\n  blur r={radius:g} {kind} route={route}: vs blur.frag golden max {g_mx} LSB ({g_n0} px differ, {g_n1} by > 1); vs oracle max {o_mx} ({o_n0} px)", end="")
        assert g_mx <= 2, (kind, radius, route, "vs the reference shader's frame", g_mx, g_n0, g_n1)
        assert o_mx <= 1, (kind, radius, route, "vs oracle", o_mx, o_n0, o_n1)
        # one f16 per tap moves 1.6 - 2.6 % of white noise's pixels by one step against the oracle (the 22-bit build: 0.01 %;
        # profiles/r06_blur_weights_pin.txt) -- the bar of the numpy restatement (tests/test_abi_and_sharding.py): 4 %; the checkerboard's
        # exact result is the same everywhere (0 - 8 pixels differ)
        assert o_n0 <= 0.04 * w * h, (kind, radius, route, o_n0)
    ctx.close()


def test_contexts_in_flight_do_not_disturb_each_other(hip):
    """bench.py keeps several frames in flight on one GPU (one context = one stream + surface set each): every context
    must end up with exactly the frame it renders alone."""
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import make_render_tree_100

    w, h = 1280, 720
    scenes = [make_render_tree_100(w, h, frame=f, copies=40, full_frame_blur=True) for f in range(4)]
    alone = []
    for sc in scenes:
        hip.render_frame(sc, w, h)
        alone.append(hip.read_pixels())
    # Repeated: a library WITH packed-FP32 instructions fails here in roughly half the context-runs (the compositor's
    # v_pk_* misread an operand while another context's v_mfma shares the SIMD: DESIGN.md section 4, tools/race_probe.py).
    for _ in range(8):
        ctxs = [HipContext(device=0) for _ in scenes]
        for c, sc in zip(ctxs, scenes):
            c.render_frame(sc, w, h)
        for _ in range(6):  # interleaved enqueues, no waiting in between
            for c in ctxs:
                c.replay_async(3)
        for c, want in zip(ctxs, alone):
            c.sync()
            assert np.array_equal(c.read_pixels(), want)
            c.close()


def test_workload_scene_1080p_matches_oracle(hip):
    """BASELINE config 2: renderlist_100 at 1920x1080 (304 nodes / 706 draws)."""
    from figdraw_amd.scenes import make_render_tree_100

    w, h = 1920, 1080
    sc = make_render_tree_100(w, h, frame=0)
    hip.render_frame(sc, w, h)
    got = hip.read_pixels()
    want = _oracle(lambda *_: sc, w, h)
    mx, n0, n1 = diff_stats(got, want)
    assert mx <= 1, (mx, n0, n1)
    assert n0 <= 0.005 * w * h


def test_4k_config_matches_oracle_and_stripes(hip):
    """BASELINE config 3 at full size (S300@4K + full-frame blur, the bench frame):
    (a) the whole 3840x2160 frame against the oracle (<= 1 LSB, <= 0.5 % of the pixels differing),
    (b) a horizontal band rendered as its own stripe equals the same rows of the full render,
    (c) every row was written (alpha 255 everywhere: no stale rows from an earlier frame)."""
    from figdraw_amd.scenes import make_render_tree_100

    w, h = 3840, 2160
    sc = make_render_tree_100(w, h, frame=3, full_frame_blur=True)
    hip.render_frame(sc, w, h)
    full = hip.read_pixels()
    assert full.shape == (h, w, 4)
    st = hip.frame_stats()
    assert st.n_draws >= 700 and st.n_blurs == 2
    want = _oracle(lambda *_: sc, w, h)
    mx, n0, n1 = diff_stats(full, want)
    assert mx <= 1, ("4K frame vs oracle", mx, n0, n1)
    assert n0 <= 0.005 * w * h, ("4K frame vs oracle: too many 1-LSB pixels", n0)
    hip.set_stripe(1000, 1300)
    hip.render_frame(sc, w, h)
    band = hip.read_pixels(0, 1000, w, 300)
    hip.set_stripe(0, 0)
    assert (band == full[1000:1300]).all()
    assert full[..., 3].min() == 255


def test_8k_config5_row_stripes_match_full_frame_and_oracle(hip):
    """BASELINE config 5 on one GPU: a frame of S300 at 7680x4320 rendered as the eight row stripes the 8-GPU run gives its
    ranks (`stripe_rows(4320, 8, r)`, each with its redundant blur halo), stitched: equal to the full render bit for bit, and
    the full render within 1 LSB of the oracle."""
    from figdraw_amd.scenes import make_render_tree_100
    from figdraw_amd.sharding import stripe_rows

    w, h = 7680, 4320
    sc = make_render_tree_100(w, h, frame=5, full_frame_blur=True)
    hip.render_frame(sc, w, h)
    full = hip.read_pixels()
    stitched = np.zeros_like(full)
    for r in range(8):
        y0, y1 = stripe_rows(h, 8, r)
        hip.set_stripe(y0, y1)
        hip.render_frame(sc, w, h)
        stitched[y0:y1] = hip.read_pixels(0, y0, w, y1 - y0)
    hip.set_stripe(0, 0)
    assert np.array_equal(stitched, full)
    want = _oracle(lambda *_: sc, w, h)
    mx, n0, n1 = diff_stats(full, want)
    assert mx <= 1, ("8K frame vs oracle", mx, n0, n1)
    assert n0 <= 0.005 * w * h


def test_contexts_in_flight_at_4k_match_the_oracle(hip):
    """The bench's mode at the bench's size: four contexts replay different 4K frames on their own streams (matrix-pipe blur
    passes of one beside the compositor waves of the others).  Each context must end with the frame it renders alone, and one
    of them is also held against the oracle.  (With packed-FP32 instructions in the library this fails within a few rounds:
    DESIGN.md section 4.)"""
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import make_render_tree_100

    w, h = 3840, 2160
    scenes = [make_render_tree_100(w, h, frame=f, full_frame_blur=True) for f in range(4)]
    alone = []
    for sc in scenes:
        hip.render_frame(sc, w, h)
        alone.append(hip.read_pixels())
    ctxs = [HipContext(device=0) for _ in scenes]
    try:
        for c, sc in zip(ctxs, scenes):
            c.render_frame(sc, w, h)
        for _ in range(6):
            for _ in range(6):
                for c in ctxs:
                    c.replay_async(3)
            for c, want in zip(ctxs, alone):
                c.sync()
                assert np.array_equal(c.read_pixels(), want)
        mx, n0, n1 = diff_stats(ctxs[2].read_pixels(), _oracle(lambda *_: scenes[2], w, h))
        assert mx <= 1 and n0 <= 0.005 * w * h, (mx, n0, n1)
    finally:
        for c in ctxs:
            c.close()


def test_8k_full_frame_blur_matches_oracle(hip):
    """BASELINE config 5's frame size with a wide full-frame blur: the matrix-pipe passes walk 16+ blocks per wave here (the 4K
    frame: 4) with 6 k-steps per block; the whole frame against the oracle."""
    from figdraw_amd.scene import Fig, FigKind, RenderList, Renders, rect, rgba

    w, h = 7680, 4320
    lst = RenderList()
    lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(0, 0, w, h), fill=rgba(245, 245, 250, 255)))
    for i in range(48):
        lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect((i * 1531) % w - 100, (i * 977) % h - 80, 500 + 37 * (i % 7), 300 + 29 * (i % 5)),
                        fill=rgba(40 * (i % 6), 200 - 30 * (i % 5), 90 + 20 * (i % 8), 255), corners=[(i * 5) % 40] * 4))
    lst.addRoot(Fig(kind=FigKind.nkBackdropBlur, screenBox=rect(0, 0, w, h), fill=rgba(255, 255, 255, 30), blur=28.0))
    sc = Renders()
    sc.setLayer(0, lst)
    hip.render_frame(sc, w, h)
    got = hip.read_pixels()
    want = _oracle(lambda *_: sc, w, h)
    mx, n0, n1 = diff_stats(got, want)
    assert mx <= 1, (mx, n0, n1)
    assert n0 <= 0.005 * w * h


def test_backend_level_calls_match_oracle(hip):
    """Drive the BackendContext surface directly (no scene front-end), incl. set_aa_factor and mode 8/11."""
    from oracle import oracle as O

    w, h = 200, 160
    z = [0, 0, 0, 0]
    calls = [
        ["begin_frame", 1, [0.9, 0.95, 1.0, 1.0]],
        ["draw_rounded_rect_sdf", [10.5, 10.25, 120, 80], [[200, 30, 30, 255]] * 4, [12, 0, 30, 6], [12, 0, 30, 6], 3, 4, 0, [0, 0], 0, z, z, 0.5],
        ["set_aa_factor", 0.6],
        ["draw_rounded_rect_sdf", [60, 50, 120, 90], [[30, 30, 200, 180]] * 4, [20] * 4, [20] * 4, 11, 9, 0, [0, 0], 0, z, z, 0.5],
        ["draw_rounded_rect_sdf", [20, 60, 150, 90], [[0, 0, 0, 120]] * 4, [10] * 4, [10] * 4, 8, 12, 4, [100, 50], 0, z, z, 0.5],
        ["set_aa_factor", 1.2],
        ["save_transform"], ["translate", 30, 20], ["scale", 0.5, 1.5],
        ["draw_rounded_rect_sdf", [100, 20, 160, 40], [[10, 200, 90, 255], [200, 200, 20, 255], [20, 20, 200, 128], [255, 255, 255, 255]], [8] * 4, [8] * 4, 3, 4, 0, [0, 0], 0, z, z, 0.5],
        ["restore_transform"],
        ["end_frame"],
    ]
    hip.W, hip.H = w, h
    hip.replay_calls(calls)
    got = hip.read_pixels()
    o = O.Oracle()
    o.W, o.H = w, h
    o.replay(calls)
    mx, n0, n1 = diff_stats(got, o.read_pixels())
    assert mx <= 1, (mx, n0, n1)


def test_error_behaviour(hip):
    from figdraw_amd.context import FigdrawHipError

    with pytest.raises(FigdrawHipError):  # endFrame without beginFrame (glcontext.nim:1984)
        hip.end_frame()
    hip.begin_frame(64, 64)
    with pytest.raises(FigdrawHipError):  # beginFrame twice (glcontext.nim:1953)
        hip.begin_frame(64, 64)
    hip.begin_mask([0, 0, 10, 10], [0] * 4, [0] * 4)
    hip.end_mask()
    with pytest.raises(FigdrawHipError):  # "Not all masks have been popped." (glcontext.nim:1985)
        hip.end_frame()
    hip.pop_mask()
    hip.end_frame()
    # unknown image id: warn + no-op (glcontext.nim:1310-1315)
    hip.begin_frame(64, 64)
    hip.draw_image(12345, (0, 0), [(255, 255, 255, 255)] * 4)
    hip.end_frame()
    assert (hip.read_pixels() == 255).all()


def _atlas_ctx_pair(sc, images, atlas_size):
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    ctx = HipContext(atlas_size=atlas_size, device=0)
    o = O.Oracle(atlas_size=atlas_size, threads=8)
    for k, img in images.items():
        assert ctx.put_image(k, img) == o.put_image(k, img)  # same skyline packer, same rects
    return ctx, o


@pytest.mark.parametrize("name", sorted(RS.ATLAS_SCENES))
def test_atlas_scenes_match_oracle_and_goldens(name):
    import os

    from conftest import GOLDEN
    from figdraw_amd.scenes import load_glyph_fixture

    fn, w, h = RS.ATLAS_SCENES[name]
    all_images = load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz"))
    sc = fn(float(w), float(h), all_images)
    ctx, o = _atlas_ctx_pair(sc, RS.used_images(sc, all_images), RS.ATLAS_GOLDEN_SIZE)
    ctx.render_frame(sc, w, h)
    o.render_frame(sc, w, h)
    got = ctx.read_pixels()
    mx, n0, n1 = diff_stats(got, o.read_pixels())
    assert mx <= 1 and n0 <= 0.005 * w * h, (name, "vs oracle", mx, n0, n1)
    gold = load_png(f"ss_{name}.png")
    mx, n0, n1 = diff_stats(got, gold)
    # north star: +-2 LSB against the reference's shaders, every scene, no exception.  (The MSDF scene's golden itself sits 2 LSB
    # from the float32 oracle on 13 pixels: SwiftShader's 16-bit texture-coordinate grid, tests/test_oracle.py
    # test_the_goldens_two_lsb_pixels_are_the_samplers_coordinate_grid.)
    n_gt2 = int((np.abs(got.astype(int) - gold.astype(int)).max(axis=2) > 2).sum())
    assert n_gt2 <= RS.ATLAS_TOLERANCE.get(name, (2, 0.001, 0))[2], (name, "vs reference GLSL on SwiftShader", mx, n0, n1, n_gt2)
    ctx.close()


def test_flippy_image_matches_oracle_and_reference_png():
    """tests/trender_image.nim with data/img1.flippy through fdh_put_flippy; bad containers raise (formatflippy.nim:120-147)."""
    import os

    from conftest import GOLDEN

    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    data = open(os.path.join(GOLDEN, "img1.flippy"), "rb").read()
    ctx = HipContext(atlas_size=2048, device=0)
    o = O.Oracle(atlas_size=2048, threads=8)
    assert ctx.put_flippy(RS.FLIPPY_IMAGE_KEY, data) == o.put_flippy(RS.FLIPPY_IMAGE_KEY, data) == (4, 4, 100, 100)
    sc = RS.image_flippy()
    ctx.render_frame(sc, 800, 600)
    o.render_frame(sc, 800, 600)
    got = ctx.read_pixels()
    mx, n0, n1 = diff_stats(got, o.read_pixels())
    assert mx <= 1 and n0 <= 0.005 * 800 * 600, ("vs oracle", mx, n0, n1)
    mx, n0, n1 = diff_stats(got, load_png("ref_render_image.png"))
    assert mx <= 2, ("vs reference PNG", mx, n0, n1)
    for bad in (b"", b"flop" + data[4:], data[:4] + b"\x02\0\0\0" + data[8:], data[:40]):
        with pytest.raises(Exception, match="[Ff]lippy"):
            ctx.put_flippy(99, bad)
    ctx.close()


def test_submit_thread_hands_over_frames_in_order():
    """fdh_end_frame returns after preparing the frame; the context's submit thread issues the launches while the caller records
    the next frame.  A burst of different frames with no synchronisation in between, reads at arbitrary points, a frame-size
    change mid-burst (surfaces are reallocated: the frame in submission must be waited for) and the per-call entry points must
    leave exactly what a FDH_CREATE_SYNC_SUBMIT context renders."""
    import random

    from figdraw_amd.context import HipContext

    rnd = random.Random(5)
    a, b = HipContext(device=0), HipContext(device=0, sync_submit=True)
    sizes = [(640, 360), (640, 360), (800, 450), (800, 450), (333, 217), (640, 360)]
    for step in range(40):
        w, h = sizes[(step // 7) % len(sizes)]
        sc = RS.random_scene(100 + step % 9, float(w), float(h), n=30 + step % 20, clips=step % 3 == 0, blur=step % 4 == 1)
        a.render_frame(sc, w, h)
        b.render_frame(sc, w, h)
        if rnd.random() < 0.3:
            assert np.array_equal(a.read_pixels(), b.read_pixels()), step
    assert np.array_equal(a.read_pixels(), b.read_pixels())
    # per-call frames back to back (no sync), then a read
    for k in range(6):
        for c in (a, b):
            c.begin_frame(320, 200, True, (1.0, 1.0, 1.0, 1.0))
            c.draw_rounded_rect_sdf((10.0 + 7 * k, 12.0, 200.0, 120.0), [(200, 40 * k, 30, 255)] * 4, (12.0,) * 4, (12.0,) * 4, 3)
            c.end_frame()
    assert np.array_equal(a.read_pixels(), b.read_pixels())
    a.close()
    b.close()


def test_c_player_drives_the_library_like_the_bindings_do():
    """tools/call_player.c (C99) is the driver bench.py times: the recorded BackendContext calls of a frame through the per-call entry
    points, whole scenes through fdh_render_frame, and the same with one host thread per group of contexts.  Whatever the driver,
    a context must end up holding exactly the frame the Python binding renders on a context of its own."""
    from figdraw_amd import call_stream as CS
    from figdraw_amd.context import HipContext

    w, h = 960, 540
    scenes = [RS.random_scene(300 + i, float(w), float(h), n=40 + 3 * i, clips=i % 2 == 0, blur=i % 3 == 0) for i in range(6)]
    ref = HipContext(device=0, sync_submit=True)
    want = []
    for sc in scenes:
        ref.render_frame(sc, w, h)
        want.append(ref.read_pixels())
    player = CS.Player()
    # (a) the per-call stream of every scene
    rec = HipContext(record_only=True)
    ctx = HipContext(device=0)
    for sc, px in zip(scenes, want):
        rec.record_begin()
        rec.render_frame(sc, w, h)
        player.play(ctx, CS.pack(rec.record_calls()), w, h)
        assert np.array_equal(ctx.read_pixels(), px)
    ctx.close()
    # (b) whole scenes, four contexts, one / two / four host threads; frame k = scene k % 6 on context k % 4
    cs = [sc.to_c() for sc in scenes]
    frames = 22
    for threads in (1, 2, 4):
        ctxs = [HipContext(device=0) for _ in range(4)]
        player.play_scenes(ctxs, cs, frames, w, h, threads=threads)
        for i, c in enumerate(ctxs):
            k_last = max(k for k in range(frames) if k % 4 == i)
            assert np.array_equal(c.read_pixels(), want[k_last % 6]), (threads, i)
            c.close()
    ref.close()


def _ink_bounds_frames(out_path):
    """(child process of test_ink_bounds_change_no_pixel) atlas draws at many scales / thresholds / ranges -> npz of frames"""
    import os

    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import load_glyph_fixture

    imgs = load_glyph_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glyphs_ubuntu20.npz"))
    w, h = 1100, 700
    ctx = HipContext(atlas_size=1024, device=0)
    codes = [65, 105, 87, 46, 103, 64, 124, 81]
    for c in codes:
        ctx.put_image(1000 + c, imgs[1000 + c])
        ctx.put_image(2000 + c, imgs[2000 + c])
    ctx.put_image(3000, imgs[3000])
    out = {}
    for case, (subpixel, ox, oy) in enumerate(((False, 0.0, 0.0), (True, 0.37, 0.61), (False, 0.5, 0.25))):
        ctx.set_text_subpixel(subpixel, 0.0)
        ctx.begin_frame(w, h, True, (0.93, 0.95, 0.98, 1.0))
        ctx.draw_rect((0.0, 0.0, float(w), float(h)), (235, 240, 250, 255))
        y = 6.0 + oy
        for row, (scale, px_range, thr, mtsdf, flip) in enumerate(((0.6, 4.0, 0.5, False, False), (1.0, 4.0, 0.5, False, False), (1.5, 4.0, 0.5, False, True),
                                                                   (3.0, 4.0, 0.5, False, False), (2.0, 2.0, 0.4, False, False), (2.0, 8.0, 0.6, False, False),
                                                                   (1.5, 4.0, 0.5, True, False), (2.5, 4.0, 0.3, True, True), (1.2, 1.0, 0.5, False, False))):
            x = 5.0 + ox
            for i, c in enumerate(codes):
                size = 32.0 * scale
                ctx.draw_msdf(2000 + c, (x, y), (10 + 20 * i, 60, 200 - 20 * i, 200 + 5 * i), (size, size), px_range, thr, 0.0, mtsdf, flip)
                if subpixel:
                    ctx.set_text_subpixel_shift(0.11 * i)
                ctx.draw_image(1000 + c, (x + size + 2.0, y + 3.0), [(20, 30, 120, 255)] * 2 + [(160, 20, 40, 230)] * 2)   # 1:1 (unless shifted)
                ctx.draw_image(1000 + c, (x + size + 22.0, y + 1.0), [(0, 0, 0, 255)] * 4, (2.3 * imgs[1000 + c].shape[1], 2.3 * imgs[1000 + c].shape[0]), i % 2 == 1)
                x += size + 70.0
            y += 32.0 * scale + 6.0
        ctx.save_transform()
        ctx.translate(700.0, 420.0)
        ctx.scale(1.7, 0.8)
        for i, c in enumerate(codes):
            ctx.draw_msdf(2000 + c, (40.0 * i, 0.0), (200, 40, 30, 255), (36.0, 36.0), 4.0, 0.5, 0.0, False, False)
            ctx.draw_msdf(2000 + c, (40.0 * i, 50.0), (30, 40, 200, 255), (36.0, 36.0), 4.0, 0.5, 1.5, False, False)  # a stroke variant (never shrunk)
        ctx.restore_transform()
        ctx.draw_image(3000, (820.0, 500.0), [(255, 255, 255, 255)] * 4, (150.0, 150.0))
        ctx.end_frame()
        out[f"frame{case}"] = ctx.read_pixels()
    ctx.close()
    np.savez(out_path, **out)


def test_ink_bounds_change_no_pixel():
    """An atlas draw's pixel bounds shrink to the part of its image that can give non-zero coverage (glyph images: alpha > 0; MSDF
    fills: a distance level safely below threshold - 0.5 / screen range, from boxes measured at fdh_put_image).  Skipped strips would
    have blended with alpha 0 -- so frames with the shrink (default) and without (FDH_INK_BOUNDS=0) must be the same bit for bit:
    MSDF / MTSDF at 0.6x .. 3x, three ranges and thresholds, flips, sub-pixel shifts, scaled and 1:1 glyph images, an anisotropic
    transform, stroke variants beside them."""
    import os
    import subprocess
    import sys
    import tempfile

    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_hip_parity as T; T._ink_bounds_frames(sys.argv[1])" % (os.path.dirname(here), here)
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("shrunk", {}), ("full", {"FDH_INK_BOUNDS": "0"})):
            path = os.path.join(td, tag + ".npz")
            subprocess.check_call([sys.executable, "-c", code, path], env={**os.environ, **env})
            res[tag] = dict(np.load(path))
    # an image updated in place brings its own bounds: a glyph with little ink replaced by a full one is drawn whole
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import load_glyph_fixture

    imgs = load_glyph_fixture(os.path.join(here, "golden", "glyphs_ubuntu20.npz"))
    thin = imgs[2000 + 105].copy()                      # MSDF 'i'
    full = np.full_like(thin, 255)
    frames = []
    for first in (thin, full):
        c = HipContext(atlas_size=256, device=0)
        c.put_image(9, first)
        if first is thin:
            c.update_image(9, full)
        c.begin_frame(200, 120, True, (1.0, 1.0, 1.0, 1.0))
        c.draw_msdf(9, (20.0, 10.0), (200, 30, 30, 255), (96.0, 96.0), 4.0, 0.5, 0.0, False, False)
        c.draw_image(9, (130.0, 10.0), [(0, 0, 0, 255)] * 4, (64.0, 64.0))
        c.end_frame()
        frames.append(c.read_pixels())
        c.close()
    assert np.array_equal(frames[0], frames[1]), int((frames[0] != frames[1]).any(axis=2).sum())
    for k in sorted(res["full"]):
        a, b = res["shrunk"][k], res["full"][k]
        assert np.array_equal(a, b), (k, int((a != b).any(axis=2).sum()))
        assert int((a != a[0, 0]).any(axis=2).sum()) > 20000  # (the frames are not blank)


def test_hostile_arguments_never_crash_or_hang():
    """tools/abuse.py: NaN, infinities, 1e30, negative and zero sizes, huge blur radii, 1-pixel and 8192-wide frames, missing images,
    unbalanced masks through the per-call entry points.  Every call returns (an error code or a frame), nothing crashes or hangs,
    and the context renders a normal frame bit for bit afterwards.  (A NaN blur radius once walked the tap table off its end.)"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for seed in ("11", "23"):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "abuse.py"), "150"], env={**os.environ, "SEED": seed}, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "still renders correctly" in r.stdout, (seed, r.returncode, r.stdout[-600:], r.stderr[-1200:])


def test_contexts_on_several_host_threads():
    """tools/thread_churn.py: four host threads each create, use and destroy contexts of their own at the same time (frames of
    several sizes, submit thread on and off, reads at arbitrary points).  A handle is single-threaded, different handles are
    independent: every frame must equal the one a lone context renders."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (six runs: until the end of round 4 one run in twenty came out wrong -- first frames of fresh contexts whose staging blocks the
    # driver had recycled; a single run passed most of the time.  Staging blocks are kept in a process-wide store since.)
    for _ in range(6):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "thread_churn.py"), "4", "8"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and ": 0 wrong" in r.stdout, (r.returncode, r.stdout[-600:], r.stderr[-1200:])


def test_fused_full_frame_blur_equals_the_two_pass_route():
    """A blur node covering the whole frame runs both passes as ONE out-of-place kernel (k_blur_fx), the surfaces alternating
    between phases.  Same sums in the same grouping, the intermediate rounded to RGBA8 as the H pass stores it: the frames must
    equal the two-pass route's (FDH_BLUR_FUSED=0, a child process) bit for bit -- radii across the instantiated filter widths,
    frame sizes that are not multiples of 32, a translucent clear colour (the fused composite has to blend), two full-frame
    nodes in one frame (the surfaces flip twice), row stripes -- and stay within the suite's bar of the oracle."""
    import os
    import subprocess
    import sys
    import tempfile

    from oracle import oracle as O

    root, here = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))
    cases = [("r18", 1280, 720, 18.0, (1.0, 1.0, 1.0, 1.0), None, 1), ("r4_odd", 1000, 527, 4.0, (1.0, 1.0, 1.0, 1.0), None, 1),
             ("r12_glass", 644, 388, 12.0, (0.2, 0.3, 0.4, 0.5), None, 1), ("r21", 960, 540, 21.0, (1.0, 1.0, 1.0, 1.0), None, 1),
             ("r9_twice", 800, 450, 9.0, (1.0, 1.0, 1.0, 1.0), None, 2), ("r18_stripe", 1280, 720, 18.0, (1.0, 1.0, 1.0, 1.0), (184, 368), 1),
             # (round 5: every instantiation of the rebuilt kernel -- (NKH, NKV) = (5, 4), (6, 5), (6, 6) beside (4, 3), (4, 4), (5, 5) above;
             # two and three H-blocks in the register stash; a width that leaves the last workgroup with idle strips; a translucent clear)
             ("r16", 900, 500, 16.0, (1.0, 1.0, 1.0, 1.0), None, 1), ("r24", 1000, 600, 24.0, (0.9, 0.8, 0.7, 0.6), None, 1),
             ("r27_stripe", 1100, 640, 27.0, (1.0, 1.0, 1.0, 1.0), (100, 420), 1)]
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_hip_parity import _full_frame_blur_scene\n"
        "from figdraw_amd.context import HipContext\n"
        "out = {}\n"
        "for name, w, h, radius, clear, stripe, nblur in %r:\n"
        "    ctx = HipContext(device=0)\n"
        "    if stripe: ctx.set_stripe(*stripe)\n"
        "    ctx.render_frame(_full_frame_blur_scene(w, h, radius, nblur), w, h, color=clear)\n"
        "    out[name] = ctx.read_pixels(); ctx.close()\n"
        "np.savez(sys.argv[1], **out)\n"
    ) % (root, here, cases)
    with tempfile.TemporaryDirectory() as td:
        res = {}
        # (FDH_FORCE_BLUR_PATH=3: the reference route is the matrix-pipe pair at every size -- the small-region passes sum in
        # another order and differ from either at rounding ties)
        for tag, env in (("fused", {"FDH_FORCE_BLUR_PATH": "3"}), ("two_pass", {"FDH_FORCE_BLUR_PATH": "3", "FDH_BLUR_FUSED": "0"})):
            path = os.path.join(td, tag + ".npz")
            subprocess.check_call([sys.executable, "-c", code, path], env={**os.environ, **env})
            res[tag] = dict(np.load(path))
    for name, w, h, radius, clear, stripe, nblur in cases:
        a, b = res["fused"][name], res["two_pass"][name]
        rows = slice(*stripe) if stripe else slice(0, h)
        assert np.array_equal(a[rows], b[rows]), (name, int((a[rows] != b[rows]).any(axis=2).sum()))
        orc = O.Oracle(threads=8)
        orc.render_frame(_full_frame_blur_scene(w, h, radius, nblur), w, h, color=clear)
        mx, n0, n1 = diff_stats(a[rows], orc.read_pixels()[rows])
        assert mx <= 1 and n0 <= 0.005 * w * h, (name, "vs oracle", mx, n0, n1)


def _full_frame_blur_scene(w, h, radius, nblur=1):
    """the bench scene's recipe at any size: shadowed rects, `nblur` backdrop-blur nodes covering the whole frame with more rects
    between and after them"""
    from figdraw_amd.scene import Fig, FigKind, rect, rgba

    sc = RS.random_scene(77, float(w), float(h), n=50, clips=False, blur=False)
    lst = next(iter(sc.layers.values()))
    for k in range(nblur):
        lst.addRoot(Fig(kind=FigKind.nkBackdropBlur, screenBox=rect(0, 0, w, h), fill=rgba(255, 255, 255, 30 * k), blur=radius))
        lst.addRoot(Fig(kind=FigKind.nkRectangle, screenBox=rect(w * 0.2 + 40 * k, h * 0.3, w * 0.4, h * 0.25), fill=rgba(250, 200, 40, 160), corners=[18] * 4))
    return sc


@pytest.mark.parametrize("which", ["non_clip", "sub_clip", "rect_mask"])
def test_reference_benchmark_workloads_match_oracle(hip, which):
    """The two workloads the reference benchmarks itself with, node for node: examples/windy_non_clip_benchmark.nim:82-108
    (180 x 10 rounded cells, all roots) and examples/windy_clip_mask_benchmark.nim:147-186 (a clipping viewport of 180 x 6 cells,
    each clipping its overflowing children with a second clip level or with the analytic rect mask) at their 1200 x 800."""
    from figdraw_amd.scenes import make_clip_mask_benchmark, make_non_clip_benchmark

    sc = make_non_clip_benchmark() if which == "non_clip" else make_clip_mask_benchmark(which)
    w, h = 1200, 800
    hip.render_frame(sc, w, h)
    got = hip.read_pixels()
    want = _oracle(lambda *_: sc, w, h)
    mx, n0, n1 = diff_stats(got, want)
    assert mx <= 1 and n0 <= 0.005 * w * h, (which, "vs oracle", mx, n0, n1)
    assert len(np.unique(got.reshape(-1, 4), axis=0)) > 20  # (a real picture)


@pytest.mark.parametrize("depth", [16, 17, 24, 40])
def test_clip_nesting_beyond_the_lds_stack_matches_oracle(hip, depth):
    """clips nested deeper than the 16 levels the compositor keeps in LDS (the reference has no limit: one mask plane per
    level, glcontext.nim:1886-1914): levels 17.. live in a global plane sized for the frame's deepest nest"""
    w, h = 400, 300
    sc = RS.deep_clips(float(w), float(h), depth)
    hip.render_frame(sc, w, h)
    got = hip.read_pixels()
    want = _oracle(lambda *_: sc, w, h)
    mx, n0, n1 = diff_stats(got, want)
    assert mx <= 1 and n0 <= 0.005 * w * h, (depth, "vs oracle", mx, n0, n1)


def _sweep_scene(seed, mx=False):
    """the scene tools/fuzz_sweep.py builds for `seed` (sizes, node count, clips / blur / atlas all drawn from the seed)"""
    import os
    import random

    from conftest import GOLDEN
    from figdraw_amd.scenes import load_glyph_fixture

    rnd = random.Random(seed * 7919)
    w, h = rnd.randrange(40, 1400), rnd.randrange(40, 900)
    if mx:
        w = (w + 3) & ~3
    atlas = seed % 2 == 0
    imgs = load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz")) if atlas else None
    sc = RS.random_scene(seed, float(w), float(h), n=rnd.randrange(5, 90), clips=rnd.random() < 0.6, blur=mx or rnd.random() < 0.5, images=imgs)
    return sc, w, h, (RS.used_images(sc, imgs) if atlas else {})


# The seeds of the 500-seed sweep (tools/fuzz_sweep.py) that miss the suite's usual bar -- at most 1 LSB, at
# most 0.5 % of the pixels differing -- and why.  They are held to the north star's own tolerance (+-2 LSB per channel) here so
# that GPUTEST tracks them: 59: ONE pixel 2 LSB off in an elliptical clip corner with 100+ px radii (the reference's approximate
# ellipse distance divides by a small number there and amplifies the 1-ulp difference between v_rcp / v_sqrt and libm);
# 134 (every blur on the matrix pipe): one pixel of an atlas scene 2 LSB off; 2135: a 60-level gradient across a quad 60 px tall
# puts every row's colour on x.5 -- 17 % of one rectangle's pixels differ by 1 LSB, none by more.
@pytest.mark.parametrize("seed,mx", [(59, False), (134, True), (2135, False)])
def test_fuzz_sweep_outliers_stay_within_the_north_star_tolerance(seed, mx):
    import os
    import subprocess
    import sys
    import tempfile

    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_hip_parity import _sweep_scene\n"
        "from figdraw_amd.context import HipContext\n"
        "sc, w, h, imgs = _sweep_scene(%d, %r)\n"
        "ctx = HipContext(atlas_size=1024, device=0)\n"
        "for k, v in imgs.items(): ctx.put_image(k, v)\n"
        "ctx.render_frame(sc, w, h); np.save(sys.argv[1], ctx.read_pixels())\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)), seed, mx)
    sc, w, h, imgs = _sweep_scene(seed, mx)
    with tempfile.TemporaryDirectory() as td:  # (a child process: FDH_FORCE_BLUR_PATH is read once per process)
        path = os.path.join(td, "got.npy")
        env = dict(os.environ, **({"FDH_FORCE_BLUR_PATH": "3"} if mx else {}))
        subprocess.check_call([sys.executable, "-c", code, path], env=env)
        got = np.load(path)
    from oracle import oracle as O

    orc = O.Oracle(atlas_size=1024, threads=8)
    for k, v in imgs.items():
        orc.put_image(k, v)
    orc.render_frame(sc, w, h)
    mx_lsb, n0, n1 = diff_stats(got, orc.read_pixels())
    assert mx_lsb <= 2, (seed, "beyond the north star's +-2 LSB", mx_lsb, n0, n1)
    assert n1 <= 4, (seed, "more than a handful of pixels beyond 1 LSB", n1)
    assert n0 <= 0.05 * w * h, (seed, n0)


@pytest.mark.parametrize("seed,w,h,clips", [(11, 400, 300, True), (12, 777, 333, False), (13, 1024, 512, True), (14, 250, 640, False)])
def test_random_atlas_scenes_match_oracle(seed, w, h, clips):
    """Random scenes mixing SDF rects with glyph runs, scaled / flipped images and (M)(T)SDF quads, some rotated, some
    under clips: the 4-wide atlas path, the one-pixel-slot path (rotated, minified) and the kernel-variant selection."""
    import os

    from conftest import GOLDEN
    from figdraw_amd.scenes import load_glyph_fixture

    all_images = load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz"))
    sc = RS.random_scene(seed, float(w), float(h), n=50, clips=clips, blur=(seed % 2 == 1), images=all_images)
    ctx, o = _atlas_ctx_pair(sc, RS.used_images(sc, all_images), 1024)
    ctx.render_frame(sc, w, h)
    o.render_frame(sc, w, h)
    mx, n0, n1 = diff_stats(ctx.read_pixels(), o.read_pixels())
    assert mx <= 1 and n0 <= 0.005 * w * h, (seed, mx, n0, n1)
    ctx.close()


@pytest.mark.parametrize("subpixel,variants", [(False, False), (True, False), (True, True)])
def test_text_frontend_matches_oracle(subpixel, variants):
    """Selection rectangles, underline / strikethrough and renderer-side glyph snapping (shift or glyph variants)."""
    import os

    from conftest import GOLDEN
    from figdraw_amd.scenes import load_glyph_fixture

    w, h = 300, 120
    all_images = load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz"))
    sc = RS.text_frontend(float(w), float(h), all_images)
    used = {k: all_images[k] for k in sorted({1000 + ord(c) for c in "figdrawabcdefghij"})}
    ctx, o = _atlas_ctx_pair(sc, used, 256)
    ctx.set_text_subpixel(subpixel, 0.0, glyph_variants=variants)
    o.set_text_subpixel(subpixel, 0.0, glyph_variants=variants)
    ctx.render_frame(sc, w, h)
    o.render_frame(sc, w, h)
    got, want = ctx.read_pixels(), o.read_pixels()
    mx, n0, n1 = diff_stats(got, want)
    assert mx <= 1 and n0 <= 0.005 * w * h, (subpixel, variants, mx, n0, n1)
    assert (got[..., :3] != got[0, 0, :3]).any()
    ctx.close()


def test_t10k_glyph_config_4k_matches_oracle():
    """BASELINE config 4: 10 000 glyph quads (5 000 coverage glyphs 1:1 + 5 000 magnified MSDF) at 3840x2160."""
    import os

    from conftest import GOLDEN
    from figdraw_amd.scenes import load_glyph_fixture, make_glyph_scene

    w, h = 3840, 2160
    all_images = load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz"))
    sc = make_glyph_scene(w, h, all_images)
    ctx, o = _atlas_ctx_pair(sc, RS.used_images(sc, all_images), 1024)
    ctx.render_frame(sc, w, h)
    st = ctx.frame_stats()
    assert st.n_draws == 10001
    o.render_frame(sc, w, h)
    mx, n0, n1 = diff_stats(ctx.read_pixels(), o.read_pixels())
    assert mx <= 1 and n0 <= 0.005 * w * h, (mx, n0, n1)
    ctx.close()


def test_atlas_grow_and_update(hip):
    """The atlas doubles when full (glcontext.nim:536-539) and drops its entries, like resetImageAtlas."""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=64, device=0)
    assert ctx.atlas_size() == 64
    ctx.put_image(1, np.full((20, 20, 4), 255, np.uint8))
    assert ctx.has_image(1)
    ctx.put_image(2, np.full((60, 60, 4), 128, np.uint8))  # needs 68 px: grows to 128
    assert ctx.atlas_size() == 128 and ctx.has_image(2) and not ctx.has_image(1)
    ctx.update_image(2, np.full((60, 60, 4), 255, np.uint8))
    ctx.begin_frame(64, 64, True, (0, 0, 0, 1))
    ctx.draw_image(2, (2, 2), [(255, 255, 255, 255)] * 4)
    ctx.end_frame()
    img = ctx.read_pixels()
    assert (img[2:62, 2:62] == 255).all() and (img[0, 0] == [0, 0, 0, 255]).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# Culling (fdh_set_cull): the frame with and without it must be the same bit for bit.
def _render_both(ctx, sc, w, h, stripe=None):
    out = []
    for mode in (0, 1):
        ctx.set_cull(mode)
        if stripe:
            ctx.set_stripe(*stripe)
        ctx.render_frame(sc, w, h)
        out.append((ctx.read_pixels(0, stripe[0], w, stripe[1] - stripe[0]) if stripe else ctx.read_pixels(), ctx.frame_stats().n_draws, ctx.culled_draws()))
    ctx.set_cull(1)
    ctx.set_stripe(0, 0)
    return out


@pytest.mark.parametrize("kind", ["non_clip", "sub_clip", "rect_mask"])
def test_culling_changes_no_pixel_of_the_reference_benchmark_tables(hip, kind):
    """examples/windy_non_clip_benchmark.nim / windy_clip_mask_benchmark.nim at full size: 180 rows in an 800 px window -- most
    cells never reach a pixel.  Culled and unculled frames must be identical (and culling must actually remove records)."""
    from figdraw_amd.scenes import make_clip_mask_benchmark, make_non_clip_benchmark

    w, h = 1200, 800
    sc = make_non_clip_benchmark() if kind == "non_clip" else make_clip_mask_benchmark(kind)
    (full, n_full, c0), (culled, n_culled, c1) = _render_both(hip, sc, w, h)
    assert c0 == 0 and n_culled < n_full // 2, (n_full, n_culled, c1)
    assert np.array_equal(full, culled)


@pytest.mark.parametrize("seed,w,h", [(3, 640, 400), (11, 811, 463), (29, 256, 256), (31, 1283, 97)])
def test_culling_changes_no_pixel_of_scenes_hanging_over_the_frame_edges(hip, seed, w, h):
    from test_culling import _off_frame_scene

    sc = _off_frame_scene(w, h, seed)
    (full, n_full, _), (culled, n_culled, c1) = _render_both(hip, sc, w, h)
    assert c1 > 0 and n_culled < n_full
    assert np.array_equal(full, culled)
    want = _oracle(lambda *_: sc, w, h)
    mx, n0, n1 = diff_stats(culled, want)
    assert mx <= 1 and n0 <= 0.005 * w * h, (seed, mx, n0, n1)


@pytest.mark.parametrize("stripe", [(0, 136), (272, 408), (944, 1080)])
def test_stripe_culling_changes_no_pixel_of_the_stripe(hip, stripe):
    """fdh_set_stripe + culling: draws beyond the stripe's rows (+ the reach of the scene's two blur nodes) are not recorded; the
    stripe's rows must equal the unculled stripe's and the full frame's."""
    from figdraw_amd.scenes import make_render_tree_100

    w, h = 1920, 1080
    sc = make_render_tree_100(w, h, frame=2, full_frame_blur=True)
    hip.set_cull(0)
    hip.render_frame(sc, w, h)
    whole = hip.read_pixels()
    (full, n_full, _), (culled, n_culled, c1) = _render_both(hip, sc, w, h, stripe)
    assert c1 > 0 and n_culled < n_full, (n_full, n_culled)
    assert np.array_equal(full, culled)
    assert np.array_equal(culled, whole[stripe[0]:stripe[1]])


@pytest.mark.parametrize("route", [0, 1])
def test_a_stripe_of_a_large_blur_node_runs_the_whole_frames_kernels(route):
    """Which blur passes take a launch -- matrix pipe or VALU, whose sums differ in the last bits -- goes by the NODE's footprint,
    not by the rows a stripe leaves of it: a 136-row stripe of a 1920x1080 full-frame blur (0.33 Mpx with its halo: under the
    0.4-Mpx crossover) must equal the whole frame's rows bit for bit on the two-pass route too (round 4: it differed in 1 - 5
    pixels by 1 LSB there; the one-kernel route, the default, never did)."""
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import make_render_tree_100

    w, h = 1920, 1080
    sc = make_render_tree_100(w, h, frame=2, full_frame_blur=True)
    ctx = HipContext(device=0)
    ctx.set_blur_route(route)
    ctx.render_frame(sc, w, h)
    whole = ctx.read_pixels().copy()
    for y0, y1 in ((0, 136), (272, 408), (944, 1080)):
        ctx.set_stripe(y0, y1)
        ctx.render_frame(sc, w, h)
        assert np.array_equal(ctx.read_pixels()[y0:y1], whole[y0:y1]), (route, y0, y1)


def test_replay_refuses_a_stripe_the_records_were_not_culled_for(hip):
    from figdraw_amd.context import FigdrawHipError
    from figdraw_amd.scenes import make_render_tree_100

    w, h = 1280, 720
    sc = make_render_tree_100(w, h, frame=1, full_frame_blur=True)
    hip.set_stripe(0, 96)
    hip.render_frame(sc, w, h)
    hip.replay(1)
    hip.set_stripe(400, 496)
    with pytest.raises(FigdrawHipError):
        hip.replay(1)
    hip.set_stripe(0, 0)
    hip.render_frame(sc, w, h)
    hip.replay(1)


# ---------------------------------------------------------------------------------------------------------------------
# A 50-seed slice of tools/fuzz_sweep.py: the sweep's own random sizes / node counts / clip, blur and atlas
# choices, held to the north star's tolerance: at most 2 LSB per channel, at most 4 pixels beyond 1 LSB.
@pytest.mark.parametrize("lo", [200, 210, 220, 230, 240])
def test_fuzz_sweep_slice_within_the_north_star_tolerance(lo):
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    for seed in range(lo, lo + 10):
        sc, w, h, imgs = _sweep_scene(seed)
        ctx = HipContext(atlas_size=1024, device=0)
        orc = O.Oracle(atlas_size=1024, threads=8)
        for k, v in imgs.items():
            ctx.put_image(k, v)
            orc.put_image(k, v)
        ctx.render_frame(sc, w, h)
        orc.render_frame(sc, w, h)
        mx, n0, n1 = diff_stats(ctx.read_pixels(), orc.read_pixels())
        ctx.close()
        assert mx <= 2 and n1 <= 4, (seed, "beyond the north star's +-2 LSB", mx, n0, n1)
        assert n0 <= 0.05 * w * h, (seed, n0)


# ---------------------------------------------------------------------------------------------------------------------
# The walk pool (fdh_set_walk_threads): frames recorded by several threads -- pieces gathered by k_upload_frame, extension indices
# re-based on the way, bin boxes built on the device -- must equal the frames the calling thread records alone, bit for bit.
def _render_with_threads(ctx, sc, w, h, threads):
    ctx.set_walk_threads(threads)
    ctx.render_frame(sc, w, h)
    px = ctx.read_pixels()
    groups = ctx.walk_stats()[1]
    ctx.set_walk_threads(-1)
    return px, groups


@pytest.mark.parametrize("which", ["bench", "non_clip", "sub_clip", "rect_mask", "wide5", "wide9", "many_groups"])
def test_frames_recorded_on_the_walk_pool_equal_the_serial_ones(hip, which):
    from figdraw_amd import scene as S
    from figdraw_amd.scenes import make_clip_mask_benchmark, make_non_clip_benchmark, make_render_tree_100
    from test_parallel_walk import _wide_scene

    if which == "bench":
        w, h, sc = 3840, 2160, make_render_tree_100(3840, 2160, 4, full_frame_blur=True)
    elif which == "non_clip":
        w, h, sc = 1200, 800, make_non_clip_benchmark()
    elif which in ("sub_clip", "rect_mask"):
        w, h, sc = 1200, 800, make_clip_mask_benchmark(which)
    elif which.startswith("wide"):
        w, h = (1280, 720) if which == "wide5" else (1920, 1080)
        sc = _wide_scene(int(which[4:]), w, h)  # rotated quads (extension indices), clips around the group, blur roots between groups
    else:
        w, h = 800, 600
        lst = S.RenderList()
        for g in range(14):  # 14 forked groups: more pieces than the upload's run table holds -> consolidated
            parent = lst.addRoot(S.Fig(kind=S.FigKind.nkFrame, screenBox=S.rect(0, 40.0 * g, w, 40)))
            for k in range(60):
                lst.addChild(parent, S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(12.0 * k, 40.0 * g + 4, 10, 30), corners=[2] * 4,
                                           fill=S.rgba((k * 37) & 255, (g * 53) & 255, 90, 255), rotation=5.0 if k % 9 == 0 else 0.0))
        sc = S.Renders()
        sc.setLayer(0, lst)
    serial, g0 = _render_with_threads(hip, sc, w, h, 0)
    for threads in (1, 3):
        forked, g = _render_with_threads(hip, sc, w, h, threads)
        assert g0 == 0 and g > 0
        assert np.array_equal(serial, forked), (which, threads)
    want = _oracle(lambda *_: sc, w, h)
    mx, n0, n1 = diff_stats(serial, want)
    # (the "wide" scenes are 400-node random scenes: held to the north star's tolerance like the fuzz sweep -- an elliptical clip
    # corner with a large radius can put one pixel 2 LSB off)
    assert mx <= 2 and n1 <= 4 and n0 <= 0.005 * w * h, (which, mx, n0, n1)


def test_a_folded_clear_in_a_consolidated_frame_keeps_the_record_digest(hip):
    """A frame whose first draw is a full-frame one-colour rectangle (its clear is folded: the draw's bin record travels with empty
    bounds) AND whose pieces outnumber the upload's run table (consolidated into one lane): after the GPU frame the recorded frame
    must still be what the calls produced -- fdh_debug_record_digest equal to the serial walk's and to a record-only context's
    (the fold used to empty the box before the consolidation copied it)."""
    from figdraw_amd import scene as S
    from figdraw_amd.context import HipContext

    w, h = 800, 600
    lst = S.RenderList()
    lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(0, 0, w, h), fill=S.rgba(240, 244, 250, 255)))
    for g in range(14):
        parent = lst.addRoot(S.Fig(kind=S.FigKind.nkFrame, screenBox=S.rect(0, 40.0 * g, w, 40)))
        for k in range(60):
            lst.addChild(parent, S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(12.0 * k, 40.0 * g + 4, 10, 30), corners=[2] * 4,
                                       fill=S.rgba((k * 37) & 255, (g * 53) & 255, 90, 255)))
    sc = S.Renders()
    sc.setLayer(0, lst)
    rec = HipContext(record_only=True)
    rec.render_frame(sc, w, h)
    want = rec.record_digest()
    rec.close()
    import os

    folds = os.environ.get("FDH_FOLD_CLEAR", "1") != "0"  # (tools/suite_off_defaults.sh runs the suite with the fold off as well)
    hip.set_walk_threads(0)
    hip.render_frame(sc, w, h)
    hip.sync()
    assert hip.frame_stats().clear_folded == (1.0 if folds else 0.0)
    serial_px = hip.read_pixels()
    assert hip.record_digest() == want
    hip.set_walk_threads(3)
    hip.render_frame(sc, w, h)
    hip.sync()
    assert hip.walk_stats()[1] == 14 and hip.frame_stats().clear_folded == (1.0 if folds else 0.0)
    assert hip.record_digest() == want
    assert np.array_equal(hip.read_pixels(), serial_px)
    hip.set_walk_threads(-1)


def test_fault_hunting_probes_and_the_staging_store_by_device():
    import os

    """Round 5's probes on a healthy frame, and the staging store's keying.  fdh_debug_verify_upload: the device's frame block equals the
    host lanes it was gathered from (but for bin record 0's box when the clear was folded: 4 bytes, by design); fdh_debug_bin_digest: a
    replay of the resident records leaves the same counts and lists; fdh_debug_staging_store_bytes: blocks a closed context released
    are held under ITS device ordinal and under no other (ADVICE r4: the store used to be process-wide)."""
    import ctypes as C
    import os

    from figdraw_amd import context as ctx_mod
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import make_render_tree_100

    L = ctx_mod.load()

    def held(dev):
        out = C.c_int64(-1)
        assert L.fdh_debug_staging_store_bytes(dev, C.byref(out)) == 0
        return out.value

    w, h = 1280, 720
    c = HipContext(device=0)
    c.set_walk_threads(3)
    c.render_frame(make_render_tree_100(w, h, 3, full_frame_blur=True), w, h)
    c.sync()
    v = c.verify_upload()
    assert v[0] == 0 and v[2] == 0 and v[1] in (0, 4) and v[3] > 0 and v[12] == 0 and v[17] == 0, v
    d0 = c.bin_digest()
    assert d0[1] > 0 and d0[4] == 0
    c.replay(1)
    c.sync()
    assert c.bin_digest() == d0
    before = held(0)
    c.close()
    after = held(0)
    if os.environ.get("FDH_VRAM_STAGING", "1") != "0" and os.environ.get("FDH_VRAM_STORE", "1") == "1":
        assert after > before, (before, after)  # the context's staging blocks went to device 0's store ...
    assert held(1) == 0 and held(5) == 0      # ... and to no other ordinal's


def test_draw_image_adj_and_the_lcd_flag_through_the_seam():
    """drawImageAdj (glcontext.nim:1369-1381: the uv rect pulled in by two texels) against the oracle, upright, scaled and under a
    rotation; and setTextLcdFilteringEnabled / textLcdFilteringEnabled (figbackend.nim:663-667): a glyph uploaded with
    FDH_GLYPH_LCD_CONTEXT is filtered exactly when the context's flag is on."""
    import os

    from conftest import GOLDEN
    from figdraw_amd.context import HipContext
    from figdraw_amd.scenes import load_glyph_fixture
    from oracle import oracle as O

    imgs = load_glyph_fixture(os.path.join(GOLDEN, "glyphs_ubuntu20.npz"))
    w, h = 240, 180
    ctx, o = HipContext(atlas_size=256, device=0), O.Oracle(atlas_size=256)
    for k in (3000, 2065):
        assert ctx.put_image(k, imgs[k]) == o.put_image(k, imgs[k])
    calls = [["begin_frame", 1, [0.2, 0.25, 0.3, 1.0]],
             ["draw_image_adj", 3000, [10, 12], [255, 255, 255, 255], [100, 100]],
             ["draw_image_adj", 3000, [120.5, 8.25], [255, 200, 160, 200], [70, 45]],
             ["save_transform"], ["translate", 60, 120], ["rotate", 0.3],
             ["draw_image_adj", 2065, [0, 0], [90, 255, 120, 255], [64, 40]],
             ["restore_transform"], ["end_frame"]]
    for be in (ctx, o):
        be.W, be.H = w, h
    ctx.replay_calls(calls)
    o.replay(calls)
    mx, n0, n1 = diff_stats(ctx.read_pixels(), o.read_pixels())
    assert mx <= 1 and n0 <= 0.005 * w * h, (mx, n0, n1)
    # the LCD flag
    assert ctx.text_lcd_filtering() is False
    g = imgs[1000 + ord("W")]
    frames = {}
    for name, flag_on, how in (("ctx_on", True, "context"), ("ctx_off", False, "context"), ("forced", False, True), ("plain", True, False)):
        c2 = HipContext(atlas_size=256, device=0)
        c2.set_text_lcd_filtering(flag_on)
        assert c2.text_lcd_filtering() is flag_on
        c2.put_glyph_image(7, g, lcd_filter=how)
        c2.begin_frame(64, 48, True, (0, 0, 0, 1))
        c2.draw_image(7, (5, 5), [(255, 255, 255, 255)] * 4)
        c2.end_frame()
        frames[name] = c2.read_pixels()
        c2.close()
    assert np.array_equal(frames["ctx_on"], frames["forced"]) and np.array_equal(frames["ctx_off"], frames["plain"])
    assert not np.array_equal(frames["ctx_on"], frames["ctx_off"])
    ctx.close()


def test_clear_folding_changes_no_pixel():
    """A cleared frame whose first draw is one colour at full coverage over the whole frame starts, in effect, from
    blend(clear, colour): Context::fold_clear folds that draw into the clear colour (FDH_FOLD_CLEAR=0 turns it off; read once per
    process, hence the child processes).  Same frames bit for bit -- translucent and opaque backgrounds over several clear colours,
    and backgrounds that must NOT be folded (rounded corners, a gradient, smaller than the frame, a clip opened first)."""
    import os
    import subprocess
    import sys
    import tempfile

    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from figdraw_amd import scene as S\n"
        "from figdraw_amd.context import HipContext\n"
        "from figdraw_amd.scenes import make_render_tree_100\n"
        "import ref_scenes as RS\n"
        "ctx = HipContext(device=0)\n"
        "out, folded = [], []\n"
        "def frame(sc, w, h, color=(1.0, 1.0, 1.0, 1.0)):\n"
        "    ctx.render_frame(sc, w, h, color=color); out.append(ctx.read_pixels().copy()); folded.append(ctx.frame_stats().clear_folded)\n"
        "frame(make_render_tree_100(1920, 1080, 2, full_frame_blur=True), 1920, 1080)\n"
        "for k, (bg, clear, corners, grad, inset) in enumerate([((255, 255, 255, 155), (0.2, 0.4, 0.9, 1.0), 0, False, 0), ((10, 200, 90, 255), (1, 1, 1, 1), 0, False, 0),\n"
        "        ((90, 20, 200, 1), (0.5, 0.5, 0.5, 0.5), 0, False, 0), ((255, 0, 0, 128), (0, 0, 0, 0), 0, False, 0), ((30, 30, 30, 200), (1, 1, 1, 1), 9, False, 0),\n"
        "        ((30, 30, 30, 200), (1, 1, 1, 1), 0, True, 0), ((30, 30, 30, 200), (1, 1, 1, 1), 0, False, 3)]):\n"
        "    w, h = 333, 217\n"
        "    sc = RS.random_scene(40 + k, float(w), float(h), n=25, clips=(k %% 2 == 0), blur=(k %% 3 == 0))\n"
        "    lst = sc.layers[0]\n"
        "    fill = S.linear(S.rgba(*bg), S.rgba(5, 5, 5, 255)) if grad else S.rgba(*bg)\n"
        "    node = S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(inset, inset, w - 2 * inset, h - 2 * inset), fill=fill, corners=[corners] * 4)\n"
        "    node.parent = -1\n"
        "    lst.nodes.insert(0, node)\n"
        "    for f in lst.nodes[1:]:\n"
        "        if f.parent >= 0: f.parent += 1\n"
        "    lst.rootIds = [0] + [r + 1 for r in lst.rootIds]\n"
        "    frame(sc, w, h, color=clear)\n"
        "np.savez(sys.argv[1], *out, folded=np.array(folded))\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for on in ("1", "0"):
            path = os.path.join(td, f"fold{on}.npz")
            subprocess.check_call([sys.executable, "-c", code, path], env=dict(os.environ, FDH_FOLD_CLEAR=on))
            z = np.load(path)
            res[on] = ([z[f"arr_{i}"] for i in range(8)], z["folded"].tolist())
    assert res["0"][1] == [0.0] * 8
    assert res["1"][1] == [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0], res["1"][1]  # the last three must not fold
    for a, b in zip(res["0"][0], res["1"][0]):
        assert np.array_equal(a, b)


def test_staging_in_device_memory_changes_no_pixel():
    """Where the recording threads put a frame's records for the gather kernel: device memory written through the PCIe BAR (the
    default on a large-BAR device) or pinned host memory (FDH_VRAM_STAGING=0; read once per process, hence the child processes).
    Same frames bit for bit: the bench frame with the walk pool on, a frame recorded through more pieces than the run table
    holds (consolidated), a retained scene's diff upload after an edit, and a frame that grows the mirrors mid-way."""
    import os
    import subprocess
    import sys
    import tempfile

    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from figdraw_amd import scene as S\n"
        "from figdraw_amd.context import HipContext\n"
        "from figdraw_amd.scenes import make_render_tree_100, make_non_clip_benchmark\n"
        "import ref_scenes as RS\n"
        "ctx = HipContext(device=0)\n"
        "out = []\n"
        "ctx.set_walk_threads(5)\n"
        "for k in (0, 3): ctx.render_frame(make_render_tree_100(1920, 1080, k, full_frame_blur=True), 1920, 1080); out.append(ctx.read_pixels().copy())\n"
        "lst = S.RenderList()\n"
        "for g in range(14):\n"
        "    parent = lst.addRoot(S.Fig(kind=S.FigKind.nkFrame, screenBox=S.rect(0, 40.0 * g, 800, 40)))\n"
        "    for k in range(60):\n"
        "        lst.addChild(parent, S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(12.0 * k, 40.0 * g + 4, 10, 30), corners=[2] * 4, fill=S.rgba((k * 37) & 255, (g * 53) & 255, 90, 255)))\n"
        "sc = S.Renders(); sc.setLayer(0, lst)\n"
        "ctx.render_frame(sc, 800, 600); out.append(ctx.read_pixels().copy())\n"
        "ctx.render_frame(make_non_clip_benchmark(), 1200, 800); out.append(ctx.read_pixels().copy())\n"
        "sc = RS.random_scene(5, 640.0, 480.0, n=40)\n"
        "ctx.scene_retain(sc, 640, 480); out.append(ctx.read_pixels().copy())\n"
        "n = sc.layers[0].nodes[3]; n.screenBox = S.rect(33, 44, 120, 80)\n"
        "ctx.scene_update_nodes(0, 3, [n]); ctx.scene_render(); out.append(ctx.read_pixels().copy())\n"
        "np.savez(sys.argv[1], *out)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for on in ("1", "0"):
            path = os.path.join(td, f"st{on}.npz")
            subprocess.check_call([sys.executable, "-c", code, path], env=dict(os.environ, FDH_VRAM_STAGING=on))
            z = np.load(path)
            res[on] = [z[f"arr_{i}"] for i in range(6)]
    for a, b in zip(res["0"], res["1"]):
        assert np.array_equal(a, b)


def test_launch_chain_switches_change_no_pixel():
    """Round 4's change to the bin launch is speed only: which bins a later phase's part of it covers (the phase's own box -- or the
    whole grid, FDH_BIN_SUBGRIDS=0; read once per process, hence the child processes).  (Its other change -- the bin launch's first
    wave, not an event behind the upload, tells the host that a staging set is free again -- had a switch too until round 5 pruned
    it; a frame without a bin launch still takes the event.)  A burst of animation frames through one context (the staging sets rotate and are waited for), a frame of
    four phases with blur nodes of different footprints, a clipped tree and a stripe: same frames bit for bit."""
    import os
    import subprocess
    import sys
    import tempfile

    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from figdraw_amd import scene as S\n"
        "from figdraw_amd.context import HipContext\n"
        "from figdraw_amd.scenes import make_render_tree_100, make_clip_mask_benchmark\n"
        "ctx = HipContext(device=0)\n"
        "out = []\n"
        "for k in range(12): ctx.render_frame(make_render_tree_100(1280, 720, k, full_frame_blur=(k %% 2 == 0)), 1280, 720)\n"
        "out.append(ctx.read_pixels().copy())\n"
        "sc = make_render_tree_100(1920, 1080, 5, full_frame_blur=True)\n"
        "lst = sc.layers[0]\n"
        "lst.addRoot(S.Fig(kind=S.FigKind.nkBackdropBlur, corners=[12] * 4, screenBox=S.rect(1500, 40, 300, 200), fill=S.rgba(0, 0, 0, 0), blur=7.0))\n"
        "lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, corners=[12] * 4, screenBox=S.rect(1480, 30, 200, 120), fill=S.rgba(40, 200, 90, 130)))\n"
        "ctx.render_frame(sc, 1920, 1080); out.append(ctx.read_pixels().copy())\n"
        "ctx.render_frame(make_clip_mask_benchmark('sub_clip'), 1200, 800); out.append(ctx.read_pixels().copy())\n"
        "ctx.set_stripe(270, 540)\n"
        "ctx.render_frame(make_render_tree_100(1920, 1080, 2, full_frame_blur=True), 1920, 1080); out.append(ctx.read_pixels()[270:540].copy())\n"
        "np.savez(sys.argv[1], *out)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for name, env in (("default", {}), ("whole_grid", {"FDH_BIN_SUBGRIDS": "0"})):
            path = os.path.join(td, f"{name}.npz")
            subprocess.check_call([sys.executable, "-c", code, path], env=dict(os.environ, **env))
            z = np.load(path)
            res[name] = [z[f"arr_{i}"] for i in range(4)]
    for name in ("whole_grid",):
        for a, b in zip(res["default"], res[name]):
            assert np.array_equal(a, b), name


def test_small_blur_in_one_kernel_equals_the_two_pass_route():
    """k_blur_small (a small region's two passes in one kernel, snapshot to the backdrop surface, composited by the phase's launch)
    against the two small-region passes with the composite fused into the vertical one (FDH_BLUR_FUSED=0: the two-pass routes for
    every node; read once per process): regions at the frame's edges (clamped taps), a stripe, several radii, a rounded translucent quad.  The blurred
    snapshot is the same sum in the same order; the frames must agree bit for bit -- and with the oracle."""
    import os
    import subprocess
    import sys
    import tempfile

    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from figdraw_amd import scene as S\n"
        "from figdraw_amd.context import HipContext\n"
        "import ref_scenes as RS\n"
        "ctx = HipContext(device=0)\n"
        "out = []\n"
        "for k, (w, h, box, radius, corner, fill, stripe) in enumerate([(640, 360, (100, 60, 360, 240), 18.0, 20, (255, 225, 55, 0), None), (333, 217, (-20, -10, 200, 120), 6.0, 0, (0, 0, 0, 60), None),\n"
        "        (400, 300, (250, 180, 200, 150), 22.0, 40, (20, 20, 20, 0), None), (512, 512, (30, 40, 300, 400), 9.0, 8, (255, 255, 255, 30), (96, 288)), (300, 200, (10, 10, 280, 180), 3.0, 12, (0, 0, 0, 0), None)]):\n"
        "    sc = RS.random_scene(70 + k, float(w), float(h), n=30, clips=False, blur=False)\n"
        "    lst = sc.layers[0]\n"
        "    lst.addRoot(S.Fig(kind=S.FigKind.nkBackdropBlur, screenBox=S.rect(*box), corners=[corner] * 4, fill=S.rgba(*fill), blur=radius))\n"
        "    lst.addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(box[0] + 10, box[1] + 10, 60, 40), fill=S.rgba(200, 30, 30, 180), corners=[6] * 4))\n"
        "    if stripe: ctx.set_stripe(*stripe)\n"
        "    ctx.render_frame(sc, w, h)\n"
        "    px = ctx.read_pixels()\n"
        "    out.append(px[stripe[0]:stripe[1]].copy() if stripe else px.copy())\n"
        "    ctx.set_stripe(0, 0)\n"
        "np.savez(sys.argv[1], *out)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for on in ("1", "0"):
            path = os.path.join(td, f"one{on}.npz")
            subprocess.check_call([sys.executable, "-c", code, path], env=dict(os.environ, FDH_BLUR_FUSED=on))
            z = np.load(path)
            res[on] = [z[f"arr_{i}"] for i in range(5)]
    for a, b in zip(res["0"], res["1"]):
        assert np.array_equal(a, b)
    # the first scene against the oracle
    from figdraw_amd import scene as S

    w, h = 640, 360
    sc = RS.random_scene(70, float(w), float(h), n=30, clips=False, blur=False)
    sc.layers[0].addRoot(S.Fig(kind=S.FigKind.nkBackdropBlur, screenBox=S.rect(100, 60, 360, 240), corners=[20] * 4, fill=S.rgba(255, 225, 55, 0), blur=18.0))
    sc.layers[0].addRoot(S.Fig(kind=S.FigKind.nkRectangle, screenBox=S.rect(110, 70, 60, 40), fill=S.rgba(200, 30, 30, 180), corners=[6] * 4))
    mx, n0, n1 = diff_stats(res["1"][0], _oracle(lambda *_: sc, w, h))
    assert mx <= 1 and n0 <= 0.005 * w * h, (mx, n0, n1)
