"""Distance fields from coverage images on the device (fdh_put_image_sdf, fdh_put_image_sdf_of; k_image_sdf_generate): the texels against
the float64 reference tests/image_sdf_ref.py, the atlas-to-atlas call against the host-to-atlas one, rendering with those texels against
the oracle, and the atlas's other users undisturbed."""
import math
import os

import numpy as np
import pytest

import image_sdf_cases as IC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def generated():
    """every case through fdh_put_image_sdf into one 2048 atlas -> the cases, {name: (rect, texels)}, and level 0 itself"""
    from figdraw_amd.context import HipContext

    cases = IC.glyphs() + IC.hostile()
    ctx = HipContext(atlas_size=2048, device=0)
    rects = {}
    for i, (name, rgba, channel, pad, R) in enumerate(cases):
        rects[name] = ctx.put_image_sdf(5000 + i, rgba, channel=channel, pad=pad, sdf_range=R)
        assert rects[name][2:] == (rgba.shape[1] + 2 * pad, rgba.shape[0] + 2 * pad), name
    assert ctx.atlas_size() == 2048
    atlas = ctx.debug_read_surface(4)
    ctx.close()
    assert atlas.shape == (2048, 2048, 4)
    return cases, {name: (r, atlas[r[1]:r[1] + r[3], r[0]:r[0] + r[2]].copy()) for name, r in rects.items()}, atlas


def test_texels_against_the_reference(generated):
    """within 1 LSB on every texel, all four bytes of a texel equal, and nothing written outside the rectangles"""
    cases, texels, atlas = generated
    differ = total = 0
    written = np.zeros(atlas.shape[:2], bool)
    for case in cases:
        (x, y, w, h), got = texels[case[0]]
        want = IC.reference(case)
        assert got.shape[:2] == want.shape, case[0]
        assert (got == got[..., :1]).all(), f"{case[0]}: the four bytes of a texel differ"
        n_any, n_over = IC.compare(got, want)
        assert n_over == 0, f"{case[0]}: {n_over} texels are more than 1 LSB from the reference"
        differ += n_any
        total += want.size
        written[y:y + h, x:x + w] = True
    print(f"device against the float64 reference: {differ} of {total} texels differ at all")
    for name, ((x, y, w, h), _) in texels.items():
        ring = atlas[max(y - 4, 0):y + h + 4, max(x - 4, 0):x + w + 4].copy()
        ring[y - max(y - 4, 0):y - max(y - 4, 0) + h, x - max(x - 4, 0):x - max(x - 4, 0) + w] = 0
        assert not ring.any(), f"{name}: the margin was written"
    assert not atlas[~written].any()


def _cut(atlas, r):
    return atlas[r[1]:r[1] + r[3], r[0]:r[0] + r[2]].copy()


CODES = [33, 38, 48, 56, 64, 65, 81, 87, 103, 109, 119, 126]  # a dozen glyphs


def test_field_of_an_atlas_entry_is_the_field_of_its_texels():
    """sources the device rasterised itself and sources that were uploaded: fdh_put_image_sdf_of leaves, byte for byte, what
    fdh_put_image_sdf leaves when handed the source's texels as they were read back"""
    from conftest import GOLDEN
    from figdraw_amd.context import HipContext

    z = np.load(os.path.join(GOLDEN, "outlines_ubuntu20.npz"))
    imgs = IC.glyph_images()
    ctx, other = HipContext(atlas_size=1024, device=0), HipContext(atlas_size=1024, device=0)
    src = {}
    for code in CODES:
        src[1000 + code] = ctx.put_glyph_outline(1000 + code, z[f"segs_{code}"], *(int(v) for v in z[f"size_{code}"]))
        src[2000 + code] = ctx.put_image(2000 + code, imgs[code])
    before = ctx.debug_read_surface(4)
    settings = {}
    for i, key in enumerate(src):
        settings[key] = dict(channel=(3, 0)[i % 2], pad=(2, 4, 0, 7)[i % 4], sdf_range=(4, 8, 1, 13)[i % 4])
        assert ctx.has_image(key)
    fields = {key: ctx.put_image_sdf_of(key, 10000 + key, **settings[key]) for key in src}
    after = ctx.debug_read_surface(4)
    ink, host_rects = 0, {}
    for key, r in src.items():
        texels = _cut(before, r)
        assert np.array_equal(texels, _cut(after, r)) and ctx.has_image(key)  # the source stays what it was
        ink += int((texels[..., 3] > 0).sum())
        host_rects[key] = other.put_image_sdf(key, texels, **settings[key])
        pad = settings[key]["pad"]
        assert fields[key][2:] == host_rects[key][2:] == (r[2] + 2 * pad, r[3] + 2 * pad)
    host = other.debug_read_surface(4)
    for key in src:
        got = _cut(after, fields[key])
        assert np.array_equal(got, _cut(host, host_rects[key])), key
        n_over = IC.compare(got, IC.REF.field(_cut(before, src[key])[..., settings[key]["channel"]], settings[key]["pad"], settings[key]["sdf_range"]))[1]
        assert n_over == 0, key
    assert ink > 2000  # the sources held glyphs
    ctx.close(), other.close()


def test_field_of_an_entry_that_the_growing_atlas_drops():
    """a 64-texel atlas that must grow during the call: the field is made of what was there, out_rect is valid, the source key is gone"""
    from figdraw_amd.context import HipContext

    img = IC.glyph_images()[ord("g")]
    h, w = img.shape[:2]
    ctx = HipContext(atlas_size=64, device=0)
    r = ctx.put_image(1, img)
    ctx.put_image(2, img[:5, :5])
    texels = _cut(ctx.debug_read_surface(4), r)
    pad, R = 26, 8
    f = ctx.put_image_sdf_of(1, 3, channel=3, pad=pad, sdf_range=R)
    assert ctx.atlas_size() == 128 and f[2:] == (w + 2 * pad, h + 2 * pad)
    assert f[0] >= 4 and f[1] >= 4 and f[0] + f[2] <= 124 and f[1] + f[3] <= 124
    assert not ctx.has_image(1) and not ctx.has_image(2) and ctx.has_image(3)
    atlas = ctx.debug_read_surface(4)
    got = _cut(atlas, f)
    outside = atlas.copy()
    outside[f[1]:f[1] + f[3], f[0]:f[0] + f[2]] = 0
    assert not outside.any()  # the new atlas holds the field and nothing else
    ctx.close()
    want = IC.REF.field(texels[..., 3], pad, R)
    n_any, n_over = IC.compare(got, want)
    print(f"grown atlas: {n_any} of {want.size} texels differ from the reference at all")
    assert n_over == 0 and (got == got[..., :1]).all() and got.max() > 128 and got.min() == 0
    host = HipContext(atlas_size=128, device=0)
    assert host.put_image_sdf(3, texels, channel=3, pad=pad, sdf_range=R) == f
    assert np.array_equal(_cut(host.debug_read_surface(4), f), got)
    host.close()


def _scene(ctx, keys, sizes, px_range, threshold):
    """fields at scales 0.75, 1, 2.5, row after row, and under a 7 degree rotation; the four modes, flip_y"""
    W, H = 1280, 900
    ctx.begin_frame(W, H, True, (0.92, 0.94, 0.98, 1.0))
    y = 6.0
    i = 0
    for scale, count in ((0.75, 80), (1.0, 70), (2.5, 60)):
        x, row_h = 6.0, 0.0
        for k in range(count):
            key = keys[i % len(keys)]
            w, h = sizes[key]
            if x + w * scale > W - 6.0:
                x, y, row_h = 6.0, y + row_h + 6.0, 0.0
            mtsdf, stroke, flip = bool(i & 1), 1.5 if i & 2 else 0.0, i % 5 == 4
            ctx.draw_msdf(key, (x + 0.25 * (k % 3), y + 0.5 * (k % 2)), (20 + 15 * (k % 14), 40, 200 - 12 * (k % 14), 255 - 9 * (k % 4)), (w * scale, h * scale), px_range, threshold, stroke, mtsdf, flip)
            x += w * scale + 5.0
            row_h = max(row_h, h * scale)
            i += 1
        y += row_h + 6.0
    ctx.save_transform()
    ctx.translate(40.0, y + 20.0)
    ctx.rotate(math.radians(7.0))
    x = 0.0
    for k in range(24):
        key = keys[i % len(keys)]
        w, h = sizes[key]
        ctx.draw_msdf(key, (x, 0.0), (200, 30 + 15 * (k % 12), 40, 255), (w * 1.6, h * 1.6), px_range, threshold, 1.5 if k & 2 else 0.0, bool(k & 1), k % 4 == 3)
        x += w * 1.6 + 6.0
        i += 1
    ctx.restore_transform()
    ctx.end_frame()
    return ctx.read_pixels()


# (R and pad of the fields, px_range and threshold of the draws): the field as it is meant, the glow, the fattened shape
RENDERINGS = {"as generated": (4, 2, 4.0, 0.5), "glow": (8, 4, 1.0, 0.5), "threshold 0.3": (4, 2, 4.0, 0.3)}


@pytest.mark.parametrize("what", list(RENDERINGS))
def test_rendering_with_the_generated_texels(generated, what):
    """HIP and oracle, both holding the texels the device generated, agree within the suite's bar of 1 LSB"""
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    R, pad, px_range, threshold = RENDERINGS[what]
    _, texels, _ = generated
    imgs = IC.glyph_images()
    codes = list(range(35, 127, 4))[:22]
    ctx, orc = HipContext(atlas_size=2048, device=0), O.Oracle(atlas_size=2048, threads=8)
    keys, sizes = [], {}
    for i, code in enumerate(codes):
        field = texels[f"glyph {code} R={R} pad={pad}"][1]
        assert ctx.put_image_sdf(6000 + i, imgs[code], channel=3, pad=pad, sdf_range=R) == orc.put_image(6000 + i, field)
        keys.append(6000 + i)
        sizes[6000 + i] = (field.shape[1], field.shape[0])
    got, want = _scene(ctx, keys, sizes, px_range, threshold), _scene(orc, keys, sizes, px_range, threshold)
    ctx.close()
    d = np.abs(got.astype(int) - want.astype(int))
    drawn = int((want != want[0, 0]).any(axis=2).sum())
    print(f"{what}: max |hip - oracle| = {d.max()} LSB on {int((d > 0).any(axis=2).sum())} pixels, {drawn} drawn")
    assert drawn > 20000
    assert d.max() <= 1


def test_the_atlas_other_users_are_undisturbed():
    """Coverage glyphs put before and after an image's field render bit-identically to a context that put a plain image of the output's
    size instead (both atlases pack alike), and a frame in flight while the field is generated is unharmed: the call synchronises, like
    every atlas put."""
    from conftest import GOLDEN
    from figdraw_amd.context import HipContext

    z = np.load(os.path.join(GOLDEN, "outlines_ubuntu20.npz"))
    gw, gh = (int(v) for v in z[f"size_{ord('G')}"])  # the atlas-to-atlas call takes the glyph G as its source: every variant makes an image of that size
    img = IC.white(IC.disc(gw, gh, gw / 2.0, gh / 2.0, min(gw, gh) / 3.0))
    pad, R = 5, 9
    W, H = 640, 96

    def frame(ctx, codes):
        ctx.begin_frame(W, H, True, (0.0, 0.0, 0.0, 1.0))
        x = 3
        for code in codes:
            gw, gh = (int(v) for v in z[f"size_{code}"])
            ctx.draw_image(7000 + code, (float(x), 5.0), [(255, 255, 255, 255)] * 4)
            x += gw + 2
        ctx.end_frame()

    before, after = list(range(65, 85)), list(range(97, 117))
    frames = []
    for field in ("host", "atlas", None):
        ctx = HipContext(atlas_size=512, device=0)
        for code in before:
            ctx.put_glyph_outline(7000 + code, z[f"segs_{code}"], *(int(v) for v in z[f"size_{code}"]))
        frame(ctx, before)  # in flight: nothing has waited for it yet
        if field == "host":
            ctx.put_image_sdf(9000, img, channel=3, pad=pad, sdf_range=R)
        elif field == "atlas":
            ctx.put_image_sdf_of(7000 + ord("G"), 9000, channel=3, pad=pad, sdf_range=R)
        else:
            ctx.put_image(9000, np.full((img.shape[0] + 2 * pad, img.shape[1] + 2 * pad, 4), 77, np.uint8))
        first = ctx.read_pixels()
        for code in after:
            ctx.put_glyph_outline(7000 + code, z[f"segs_{code}"], *(int(v) for v in z[f"size_{code}"]))
        frame(ctx, before[::2] + after)
        frames.append((first, ctx.read_pixels()))
        ctx.close()
    assert frames[2][0].max() == 255 and frames[2][1].max() == 255
    for k in (0, 1):
        assert np.array_equal(frames[k][0], frames[2][0]), "the frame in flight"
        assert np.array_equal(frames[k][1], frames[2][1]), "coverage glyphs before and after"
