"""The distance-field correction pass on the device (fdh_put_glyph_outline with FDH_GLYPH_MTSDF | FDH_GLYPH_MTSDF_CORRECT, k_msdf_correct):
every shape is put twice, without and with the flag, and the corrected texels are held to tests/msdf_correct_ref.py applied to the
device's own uncorrected texels; drawing with the corrected texels against the oracle; another context's frame undisturbed; the largest
outline the call accepts.  Every field is read back through fdh_debug_read_surface(ctx, 4)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import msdf_cases as MC
import msdf_correct_ref as CR
import msdf_ref as M

pytestmark = pytest.mark.gpu

CAP = 1  # texels per image whose bytes may differ from correct(device's F, float64): see test_msdf_correct_host.py
SQUARE = MC.poly([(2, 2), (10, 2), (10, 9), (2, 9)])
XY = [1, 0, 3, 2, 5, 4]  # an outline mirrored in the diagonal


def shapes():
    """-> [(name, segs, w, h, R)]: widths and heights that are no multiples of 8 ('*' has artefacts), the smallest and the largest range, the
    hostile cases that are thin, tiny, 1 texel wide or high, mostly outside or empty, a single tile, and a tile edge one texel inside the image"""
    font = {c[0]: c for c in MC.inputs()}
    hostile = {c[0]: c[:5] for c in MC.hostile_inputs()}
    out = [font[f"{ch} x2"] for ch in "*g&R8"]
    out += [hostile[n] for n in ("R x2 R=1", "8 x2 R=64", "spike 0.05 wide", "sliver triangle 0.04 high", "sub-texel square", "9 x 1 image",
                                 "outside the image on three sides")]
    name, segs, w, h, R = hostile["9 x 1 image"]
    out.append(("1 x 9 image", np.ascontiguousarray(segs[:, XY]), h, w, R))
    out.append(("0 segments", np.zeros((0, 6), np.float32), 12, 11, 4))
    out.append(("8 x 8 image", MC.poly([(1.5, 1.25), (6.5, 2), (4, 6.75)]), 8, 8, 2))
    out.append(("17 x 9 image", MC.poly([(3.3, 2.2), (14.1, 1.7), (12.6, 7.4), (2.9, 6.8)]), 17, 9, 2))
    return out


@pytest.fixture(scope="module")
def put_twice():
    """every shape without and with the flag into one 1024 atlas -> {name: (rect, F, rect, G)}, level 0 itself, and each shape's reference
    correct(F of the device, float64) -> {name: (corrected, marked)}; all made once, here"""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=1024, device=0)
    rects = {}
    for i, (name, segs, w, h, R) in enumerate(shapes()):
        plain = ctx.put_glyph_outline(4000 + 2 * i, segs, w, h, mtsdf=True, sdf_range=R)
        fixed = ctx.put_glyph_outline(4001 + 2 * i, segs, w, h, mtsdf=True, sdf_range=R, correct=True)
        assert plain[2:] == (w, h) and fixed[2:] == (w, h)
        rects[name] = (plain, fixed)
    assert ctx.atlas_size() == 1024
    atlas = ctx.debug_read_surface(4)
    ctx.close()
    cut = lambda r: atlas[r[1]:r[1] + r[3], r[0]:r[0] + r[2]].copy()
    fields = {name: (p, cut(p), f, cut(f)) for name, (p, f) in rects.items()}
    want = {name: CR.correct(fields[name][1], segs, R)[:2] for name, segs, w, h, R in shapes()}
    return fields, atlas, want


def test_corrected_texels_against_the_reference(put_twice):
    fields, atlas, want = put_twice
    over, changed = {}, {}
    for name, segs, w, h, R in shapes():
        _, F, _, G = fields[name]
        ref, marked = want[name]
        n = int((G != ref).any(axis=2).sum())
        if n:
            over[name] = n
        assert n <= CAP, f"{name}: {n} texels differ from the reference's correction of the device's own field"
        got_marked = (G != F).any(axis=2)
        assert int((got_marked != marked).sum()) <= CAP, f"{name}: the marked set"
        changed[name] = int(got_marked.sum())
        # the invariants, exactly
        assert np.array_equal(G[..., 3], F[..., 3]), f"{name}: alpha was touched"
        assert np.array_equal(MC.median3(G), MC.median3(F)), f"{name}: a median moved"
        gm = G[got_marked]
        assert (gm[:, 0] == gm[:, 1]).all() and (gm[:, 1] == gm[:, 2]).all(), f"{name}: a corrected texel's channels disagree"
    print(f"texels that differ from correct(F of the device) per image (cap {CAP}): {over or 'none in any image'}; texels corrected: {changed}")
    assert changed["* x2"] > 0, "nothing was corrected in '*': the pass did no work"
    assert not fields["0 segments"][3].any()


def test_the_atlas_around_both_rectangles_is_unwritten(put_twice):
    fields, atlas, _ = put_twice
    written = np.zeros(atlas.shape[:2], bool)
    for name, (p, _, f, _) in fields.items():
        for x, y, w, h in (p, f):
            written[y:y + h, x:x + w] = True
            ring = atlas[max(y - 4, 0):y + h + 4, max(x - 4, 0):x + w + 4].copy()
            ring[y - max(y - 4, 0):y - max(y - 4, 0) + h, x - max(x - 4, 0):x - max(x - 4, 0) + w] = 0
            assert not ring.any(), f"{name}: the margin was written"
    assert not atlas[~written].any()


def test_flag_off_is_the_field_of_before(put_twice):
    """without the flag nothing moved: the same bytes, within the tolerance of test_msdf.py, as the float64 reference of steps 1 to 4"""
    fields, _, _ = put_twice
    for name, segs, w, h, R in shapes():
        n = MC.over_tolerance(fields[name][1], M.generate(segs, w, h, R))
        assert n <= MC.CAP, f"{name}: {n} texels are more than 1 LSB from the reference"


def _draw(ctx, key, w, h, scale=3.0):
    W, H = int(w * scale) + 8, 2 * (int(h * scale) + 8)
    ctx.begin_frame(W, H, True, (0.0, 0.0, 0.0, 1.0))
    ctx.draw_msdf(key, (4.0, 4.0), (255, 255, 255, 255), (w * scale, h * scale), 4.0, 0.5, 0.0, False, False)
    ctx.draw_msdf(key, (4.0, H / 2 + 4.0), (255, 255, 255, 255), (w * scale, h * scale), 4.0, 0.5, 0.0, True, False)
    ctx.end_frame()
    return ctx.read_pixels()


def test_drawing_with_the_corrected_texels(put_twice):
    """HIP and oracle, both holding the device's corrected texels of '*', agree within 1 LSB at scale 3, in MSDF and in MTSDF mode"""
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    name, segs, w, h, R = shapes()[0]
    G = put_twice[0][name][3]
    ctx, orc = HipContext(atlas_size=512, device=0), O.Oracle(atlas_size=512, threads=4)
    assert ctx.put_glyph_outline(1, segs, w, h, mtsdf=True, sdf_range=R, correct=True) == orc.put_image(1, G)
    got, want = _draw(ctx, 1, w, h), _draw(orc, 1, w, h)
    ctx.close()
    d = np.abs(got.astype(int) - want.astype(int))
    assert (want[..., 0] > 0).sum() > 2000  # something was drawn
    print(f"max |hip - oracle| = {d.max()} LSB on {int((d > 0).any(axis=2).sum())} pixels")
    assert d.max() <= 1


def test_another_context_frame_is_undisturbed():
    """a corrected put of one context between two frames of another, the first still in flight: that context's frames are bit-identical to
    those of a run in which the put never happened"""
    from conftest import GOLDEN
    from figdraw_amd.context import HipContext

    z = np.load(os.path.join(GOLDEN, "outlines_ubuntu20.npz"))
    name, fsegs, fw, fh, R = shapes()[0]
    W, H = 640, 96
    codes = list(range(65, 85))

    def frame(ctx, codes):
        ctx.begin_frame(W, H, True, (0.0, 0.0, 0.0, 1.0))
        x = 3
        for code in codes:
            ctx.draw_image(7000 + code, (float(x), 5.0), [(255, 255, 255, 255)] * 4)
            x += int(z[f"size_{code}"][0]) + 2
        ctx.end_frame()

    frames = []
    for with_put in (True, False):
        a, b = HipContext(atlas_size=512, device=0), HipContext(atlas_size=512, device=0)
        for code in codes:
            a.put_glyph_outline(7000 + code, z[f"segs_{code}"], *(int(v) for v in z[f"size_{code}"]))
        frame(a, codes)  # in flight: nothing has waited for it yet
        if with_put:
            b.put_glyph_outline(9000, fsegs, fw, fh, mtsdf=True, sdf_range=R, correct=True)
        first = a.read_pixels()
        frame(a, codes[::2])
        frames.append((first, a.read_pixels()))
        if with_put:
            r = b.put_glyph_outline(9001, fsegs, fw, fh, mtsdf=True, sdf_range=R)
            atlas = b.debug_read_surface(4)
            assert (atlas[r[1]:r[1] + r[3], r[0]:r[0] + r[2]] != 0).any()  # and b's put did happen
        a.close()
        b.close()
    assert frames[0][0].max() == 255 and frames[0][1].max() == 255
    assert np.array_equal(frames[0][0], frames[1][0]), "the frame in flight"
    assert np.array_equal(frames[0][1], frames[1][1]), "the frame after"


BIG = """
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import msdf_cases as MC
from figdraw_amd.context import HipContext
many = np.tile(MC.poly([(2, 2), (10, 2), (10, 9), (2, 9)]), (16383, 1))
ctx = HipContext(atlas_size=256, device=0)
p = ctx.put_glyph_outline(1, many, 12, 11, mtsdf=True, sdf_range=4)
f = ctx.put_glyph_outline(2, many, 12, 11, mtsdf=True, sdf_range=4, correct=True)
atlas = ctx.debug_read_surface(4)
ctx.close()
np.save(sys.argv[2], np.stack([atlas[r[1]:r[1] + r[3], r[0]:r[0] + r[2]] for r in (p, f)]))
"""


def test_the_largest_outline(tmp_path):
    """16 383 copies of one square, 65 532 segments, with the flag: the same bytes as without it (a square's field has no artefact).  The
    only large input; it runs in a process of its own, which is what gives it a time limit of its own."""
    out = tmp_path / "big.npy"
    r = subprocess.run([sys.executable, "-c", BIG, MC.ROOT, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    plain, fixed = np.load(out)
    assert plain.shape == (11, 12, 4) and plain.any()
    assert np.array_equal(fixed, plain)
    assert MC.over_tolerance(plain, M.generate(SQUARE, 12, 11, 4)) <= MC.CAP  # (duplicates change no texel: test_msdf.py)
