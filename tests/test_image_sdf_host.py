"""Distance fields from coverage images (fdh_put_image_sdf, fdh_put_image_sdf_of; include_glyphs/figdraw_hip_image_sdf.h), what a CPU can
check: known answers for the reference tests/image_sdf_ref.py itself; the calls' rules on a record-only context and through C99; and the
source of k_image_sdf.hip under the host shim of tests/emu (tests/image_sdf_emu) against that reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_build
import image_sdf_cases as IC
import image_sdf_ref as REF
from figdraw_amd import context
from figdraw_amd.context import HipContext

ROOT = IC.ROOT
INVALID = -1
MTSDF = 4


def RANGE(r):
    return r << 8


# ------------------------------------------------------------------------------------------------------------------ 1. the reference
def test_half_plane_reads_the_edge_position():
    """x_edge - x_centre in every row and column away from the image's ends (nearer than the edge: the plane outside is an edge too)"""
    cov = IC.half_plane()
    h, w = cov.shape
    d = REF.distances(cov, 0, 16)
    x_edge = 5.0 + cov[0, 5] / 255.0
    assert abs(x_edge - IC.HALF_PLANE_EDGE) < 0.5 / 255
    cols = np.arange(3, 14)  # column 2's centre is 2.5 from the image's left end and 2.8 from the edge
    want = x_edge - (cols + 0.5)
    assert np.abs(d[6:h - 6, 3:14] - want[None, :]).max() < 1e-12
    assert (d[6:h - 6, :5] > 0).all() and (d[6:h - 6, 5:] < 0).all()


def test_fully_covered_image_reads_the_distance_to_its_border():
    for w, h in ((17, 17), (9, 5), (1, 1)):
        d = REF.distances(np.full((h, w), 255, np.uint8), 0, 64)
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        assert np.array_equal(d, np.minimum(np.minimum(x, w - 1 - x), np.minimum(y, h - 1 - y)) + 0.5)


def test_lone_texel_is_its_own_edge():
    for v in (128, 200, 254, 255):
        d = REF.distances(np.full((1, 1), v, np.uint8), 3, 4)
        assert d[3, 3] == v / 255.0 - 0.5
    for v in (1, 127):  # below one half the texel is outside, and still its own nearest edge
        assert REF.distances(np.full((1, 1), v, np.uint8), 3, 4)[3, 3] == v / 255.0 - 0.5
    assert np.isneginf(REF.distances(np.zeros((1, 1), np.uint8), 3, 4)).all()
    assert not REF.field(np.zeros((1, 1), np.uint8), 3, 4).any()


def test_complement_negates_the_distance():
    """an image in a frame of zeros wider than the window, and its complement in a frame of 255: the plane outside plays no part"""
    rng = np.random.default_rng(5)
    R, frame = 8, REF.reach(8) + 1
    inner = rng.integers(0, 256, size=(19, 23)).astype(np.uint8)
    a = np.zeros((19 + 2 * frame, 23 + 2 * frame), np.uint8)
    a[frame:-frame, frame:-frame] = inner
    da, db = REF.distances(a, 0, R), REF.distances(255 - a, 0, R)
    core = (slice(frame, -frame), slice(frame, -frame))
    both = np.isfinite(da[core]) & np.isfinite(db[core])
    assert both.sum() > 400
    assert np.abs(da[core][both] + db[core][both]).max() < 1e-12


SMALL = ("byte noise", "binary noise", "disc", "half plane", "65 x 9", "covered 17 x 17", "1 x 1 at 128", "empty 9 x 9")


def test_the_bounded_window_gives_the_unbounded_bytes():
    cases = {c[0]: c for c in IC.hostile()}
    for name in SMALL:
        _, rgba, channel, pad, _ = cases[name]
        whole = REF.distances(rgba[..., channel], pad, None)
        for R in (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 63, 64):
            assert np.array_equal(REF.encode(whole, R), REF.field(rgba[..., channel], pad, R)), (name, R)


def test_the_rule_on_the_disc():
    """against the analytic distance where that is below 8 texels.  Measured: mean 0.028, max 0.236"""
    D = IC.DISC
    d = REF.distances(IC.disc(**D), 0, 64)
    x, y = np.meshgrid(np.arange(D["w"]) + 0.5, np.arange(D["h"]) + 0.5)
    true = D["radius"] - np.hypot(x - D["cx"], y - D["cy"])
    near = np.abs(true) < 8.0
    err = np.abs(d - true)[near]
    print(f"disc: mean abs error {err.mean():.3f}, max {err.max():.3f} texels over {int(near.sum())} texels")
    assert err.mean() < 0.05 and err.max() < 0.25


# ------------------------------------------------------------------------------------------------------------------ 2. the calls
def packed_area(ctx):
    area = C.c_int64()
    assert ctx.L.fdh_atlas_packed_area(ctx.h, C.byref(area)) == 0
    return area.value


def _retained_text_context():
    """a record-only context with a retained scene whose text root caches atlas positions: it is walked again when the atlas's epoch moved"""
    from figdraw_amd.scene import Fig, FigKind, Glyph, Renders, rect, rgba

    ctx = HipContext(atlas_size=256, record_only=True)
    ctx.put_image(7, np.zeros((10, 8, 4), np.uint8))
    r = Renders()
    r.addRoot(0, Fig(kind=FigKind.nkRectangle, screenBox=rect(0, 0, 256, 128), fill=rgba(240, 240, 240, 255)))
    r.addRoot(0, Fig(kind=FigKind.nkText, screenBox=rect(20, 30, 200, 30), glyphs=[Glyph(image_id=7, x=10.3 + 9.37 * i, y=2.0, subpixel_shift=-1.0) for i in range(4)]))
    ctx.scene_retain(r, 256, 128)
    ctx.scene_render()
    assert ctx.scene_stats()[0] == 0
    return ctx


def test_refusals_leave_directory_packer_and_epoch_untouched():
    ctx = _retained_text_context()
    L = ctx.L
    img = np.full((5, 7, 4), 200, np.uint8)
    p, out = img.ctypes.data, (C.c_int * 4)()
    before = (ctx.atlas_size(), packed_area(ctx))
    refused = [
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 0, 5, p, 3, 0, 0, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 0, p, 3, 0, 0, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, -3, 5, p, 3, 0, 0, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, None, 3, 0, 0, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, p, -1, 0, 0, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, p, 4, 0, 0, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, p, 3, -1, 0, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, p, 3, 65, 0, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, p, 3, 0, 1, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, p, 3, 0, MTSDF | RANGE(4), out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, p, 3, 0, 1 << 16, out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, p, 3, 0, RANGE(65), out),
        lambda: L.fdh_put_image_sdf(ctx.h, 9, 7, 5, p, 3, 0, RANGE(255), out),
        lambda: L.fdh_put_image_sdf_of(ctx.h, 8, 9, 3, 0, 0, out),          # an unknown source
        lambda: L.fdh_put_image_sdf_of(ctx.h, 7, 7, 3, 0, 0, out),          # the source's own key
        lambda: L.fdh_put_image_sdf_of(ctx.h, 7, 9, 4, 0, 0, out),
        lambda: L.fdh_put_image_sdf_of(ctx.h, 7, 9, 3, 65, 0, out),
        lambda: L.fdh_put_image_sdf_of(ctx.h, 7, 9, 3, 0, MTSDF, out),
        lambda: L.fdh_put_image_sdf_of(ctx.h, 7, 9, 3, 0, RANGE(65), out),
    ]
    for i, call in enumerate(refused):
        assert call() == INVALID, i
        assert "put_image_sdf" in L.fdh_last_error().decode()
        assert (ctx.atlas_size(), packed_area(ctx)) == before and not ctx.has_image(9) and ctx.has_image(7)
        ctx.scene_render()
        assert ctx.scene_stats()[0] == 0, i  # the epoch stood still: no root was walked again
    # and a call that goes through moves all three
    assert ctx.put_image_sdf(9, img, pad=2)[2:] == (11, 9)
    assert ctx.has_image(9) and packed_area(ctx) > before[1]
    ctx.scene_render()
    assert ctx.scene_stats()[0] > 0
    ctx.close()


def test_rectangles_have_the_padded_size_and_pack_like_plain_images():
    """on a record-only context: every put through both calls against fdh_put_glyph_image of an image of the output's size on a second
    context -- the same rectangles, an existing key, growth that drops every entry -- and a size no atlas takes"""
    from figdraw_amd.context import FigdrawHipError

    a, b = HipContext(atlas_size=64, record_only=True), HipContext(atlas_size=64, record_only=True)
    rng = np.random.default_rng(3)
    sizes = [(7, 5, 0), (1, 1, 0), (1, 9, 3), (20, 11, 4), (7, 5, 2), (30, 30, 8), (40, 3, 64), (9, 9, 1)]  # (w, h, pad): the atlas grows on the way
    for key, (w, h, pad) in enumerate(sizes, start=1):
        if key == 5:
            key = 1  # an existing key
        img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        got = a.put_image_sdf(key, img, channel=key % 4, pad=pad, sdf_range=key)
        assert got == b.put_glyph_image(key, np.zeros((h + 2 * pad, w + 2 * pad, 4), np.uint8)), (w, h, pad)
        assert got[2:] == (w + 2 * pad, h + 2 * pad)
        assert (a.atlas_size(), packed_area(a)) == (b.atlas_size(), packed_area(b))
        assert [a.has_image(k) for k in range(1, 10)] == [b.has_image(k) for k in range(1, 10)]
    assert a.atlas_size() > 64
    # the source's size comes from the directory; a source that the growth drops is gone like every other key
    a.reset_atlas(0), b.reset_atlas(0)
    assert a.atlas_size() == 64
    a.put_image(20, np.zeros((9, 13, 4), np.uint8)), b.put_image(20, np.zeros((9, 13, 4), np.uint8))
    assert a.put_image_sdf_of(20, 21, pad=3) == b.put_glyph_image(21, np.zeros((15, 19, 4), np.uint8))
    assert a.has_image(20) and a.has_image(21)
    got = a.put_image_sdf_of(20, 22, pad=40, sdf_range=64)
    assert got == b.put_glyph_image(22, np.zeros((89, 93, 4), np.uint8)) and got[2:] == (93, 89)
    assert a.atlas_size() == b.atlas_size() > 64
    assert [a.has_image(k) for k in (20, 21, 22)] == [b.has_image(k) for k in (20, 21, 22)] == [False, False, True]
    # an output no atlas takes: what fdh_put_glyph_image answers for that size
    codes = []
    for ctx, call in ((a, lambda: a.put_image_sdf(30, np.zeros((1, 16400, 4), np.uint8), pad=1)), (b, lambda: b.put_glyph_image(30, np.zeros((3, 16402, 4), np.uint8)))):
        with pytest.raises(FigdrawHipError) as e:
            call()
        codes.append((e.value.code, ctx.atlas_size(), packed_area(ctx), ctx.has_image(22)))
    assert codes[0] == codes[1] and codes[0][0] == -4
    a.close(), b.close()


def test_image_sdf_abi_smoke_in_c99(tmp_path):
    context.build()
    exe = tmp_path / "image_sdf_abi_smoke"
    lib_dir = os.path.dirname(context.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include_glyphs"),
                           os.path.join(ROOT, "tests", "image_sdf_abi_smoke.c"), "-o", str(exe), "-L", lib_dir, "-l:libfigdraw_hip.so",
                           "-Wl,-rpath," + lib_dir])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "image_sdf_abi_smoke: OK" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ 3. the kernel's source
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """k_image_sdf.hip compiled as plain C++ under the sequential shim of tests/emu with the driver of tests/image_sdf_emu -> the directory
    of ./emu, ./emu_nocull (no exit from the walk, no shortcut) and ./emu_san: the same stand-alone program under AddressSanitizer and UBSan"""
    return emu_build.build(tmp_path_factory, "image_sdf_emu", ("k_image_sdf.hip",), {"emu": (), "emu_nocull": ("-DFDH_IMAGE_SDF_NO_CULL=1",), "emu_san": emu_build.SAN},
                           opt="-O2")


def through_the_shim(tmp, cases, exe="./emu"):
    """-> [(oh, ow, 4) uint8 per case], what the program printed"""
    with open(os.path.join(tmp, "cases.bin"), "wb") as f:
        for _, rgba, channel, pad, R in cases:
            h, w = rgba.shape[:2]
            f.write(np.array([w, h, channel, pad, R], np.int32).tobytes())
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
    r = subprocess.run([exe, "cases.bin", "fields.bin"], cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (exe, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = np.fromfile(os.path.join(tmp, "fields.bin"), np.uint8)
    out, at = [], 0
    for _, rgba, _, pad, _ in cases:
        oh, ow = rgba.shape[0] + 2 * pad, rgba.shape[1] + 2 * pad
        out.append(raw[at:at + oh * ow * 4].reshape(oh, ow, 4))
        at += oh * ow * 4
    assert at == len(raw)
    return out, r.stdout


@pytest.fixture(scope="module")
def emulated(shim):
    cases = IC.glyphs() + IC.hostile()
    fields, said = through_the_shim(shim, cases)
    print(said.strip())
    return cases, fields


def test_the_kernel_source_against_the_reference(emulated):
    """every case within 1 LSB on every texel, no exceptions; all four bytes of a texel equal"""
    cases, fields = emulated
    differ = texels = 0
    for case, got in zip(cases, fields):
        want = IC.reference(case)
        assert got.shape[:2] == want.shape, case[0]
        assert (got == got[..., :1]).all(), case[0]
        n_any, n_over = IC.compare(got, want)
        assert n_over == 0, f"{case[0]}: {n_over} texels are more than 1 LSB from the reference"
        differ += n_any
        texels += want.size
    print(f"float32 kernel source against the float64 reference: {differ} of {texels} texels differ at all")


def test_known_fields(emulated):
    cases, fields = emulated
    by_name = {c[0]: f for c, f in zip(cases, fields)}
    assert not by_name["empty 9 x 9"].any() and not by_name["1 x 1 at 0"].any()
    wide = by_name["wide disc"][..., 0]
    assert (wide[:16, :16] == 0).all() and (wide[96:112, 128:144] == 255).all()  # a tile of each shortcut
    assert 0 < wide[32 + 74, 32 + 29] < 255  # and the ramp at the disc's left end


def test_exit_and_shortcuts_change_no_byte(shim, emulated):
    cases, fields = emulated
    plain, _ = through_the_shim(shim, cases, exe="./emu_nocull")
    for case, a, b in zip(cases, fields, plain):
        assert np.array_equal(a, b), case[0]


def test_the_shim_under_sanitizers(shim, emulated):
    """the stand-alone program built with -fsanitize=address,undefined, on the small and hostile cases and a few glyphs"""
    cases, fields = emulated
    pick = [i for i, c in enumerate(cases) if not c[0].startswith("glyph")] + list(range(0, 4 * 94, 37))
    got, _ = through_the_shim(shim, [cases[i] for i in pick], exe="./emu_san")
    for i, g in zip(pick, got):
        assert np.array_equal(g, fields[i]), cases[i][0]
