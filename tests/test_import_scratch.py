"""Glyph making (fdh_glyphs.h, class GlyphMaker) and image and video import (fdh_import.h, class Importer) each own their scratch: on one
context, glyph puts, single imports, import batches, an update and a compaction interleaved; neither needs what the other reserved.  The
yardstick of every call is the same call on a fresh context of its own, in an atlas of the same size: the entry's texels at every level it
stores, and its ink boxes, are identical.

How the two are compared.  The draw records carry an entry's ink boxes and its place, so the fresh context gives the call the place it has on
the interleaved one: the other entries are put there as transparent images of their sizes through fdh_put_image, in the same order, and the
atlas is compacted at the same point (one packer places every kind of put: tests/test_atlas_host.py).  From the level on at which the
rounded rectangles of neighbours meet, single puts overwrite one another's shared texels (fdh_glyphs.cpp, "the batches"): a texel of a
level that lies in another entry's rectangle of that level too is the later put's on either context and is left out; level 0 is compared
whole."""
import numpy as np
import pytest

from test_video_frame import WHITE, Memory

pytestmark = pytest.mark.gpu

SIZE = 4096  # (the last two images are 2080 wide)
NV12, A420, BT709, LIMITED = 1, 11, 1, 0
NAN = float("nan")


def box(x0, y0, x1, y1):
    """a closed rectangle of four lines"""
    return np.array([[x0, y0, NAN, NAN, x1, y0], [x1, y0, NAN, NAN, x1, y1], [x1, y1, NAN, NAN, x0, y1], [x0, y1, NAN, NAN, x0, y0]], np.float32)


def rgba(rng, w, h, border):
    """premultiplied noise with a transparent border: ink boxes that are not the rectangle"""
    img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
    img[..., :3] = (img[..., :3].astype(np.uint16) * img[..., 3:] // 255).astype(np.uint8)
    if border:
        keep = np.zeros((h, w), bool)
        keep[border:h - border, 2 * border:w - border] = True
        img[~keep] = 0
    return img


class Sources:
    """every call's source, uploaded once; the calls themselves, each on whatever context it is given"""

    def __init__(self, memory):
        rng = np.random.default_rng(64)
        up = lambda a: memory.upload(np.ascontiguousarray(a).tobytes())
        luma = rng.integers(0, 256, size=(33, 33)).astype(np.uint8)
        luma[:6], luma[:, 29:] = 16, 16  # black rows and columns: the colour's ink boxes are not the rectangle
        chroma = np.full((17, 17, 2), 128, np.uint8)
        chroma[8:, :9] = rng.integers(0, 256, size=(9, 9, 2))
        self.nv12 = (up(luma), up(chroma))
        self.a420 = [up(rng.integers(0, 256, size=s).astype(np.uint8)) for s in ((33, 33), (17, 17), (17, 17))]
        alpha = rng.integers(0, 256, size=(33, 33)).astype(np.uint8)
        alpha[27:], alpha[:, :3] = 0, 0
        self.a420.append(up(alpha))
        self.images = {6: (65, 40, up(rgba(rng, 65, 40, 5))), 7: (1, 7, up(rgba(rng, 1, 7, 0))),
                       8: (2080, 20, up(rgba(rng, 2080, 20, 3))), 9: (2080, 130, up(rgba(rng, 2080, 130, 9)))}
        self.fields = [(3, box(2.5, 2.0, 9.25, 10.0), 12, 12), (4, box(1.5, 3.0, 7.0, 11.5), 9, 14), (5, box(3.0, 1.5, 13.5, 6.0), 16, 8)]

    def image_item(self, key):
        w, h, ptr = self.images[key]
        return (key, ptr, w, h, 4 * w)

    # (name, the entries it makes or remakes: key -> (w, h), the call)
    def steps(self):
        return [
            ("glyph outline", {1: (20, 20)}, lambda c: c.put_glyph_outline(1, box(3.25, 2.5, 16.5, 17.75), 20, 20)),
            ("video frame", {2: (33, 33)}, lambda c: c.put_video_frame(2, *self.nv12, 33, 33, 33, 34, format=NV12, matrix=BT709, range=LIMITED)),
            ("glyph fields", {3: (12, 12), 4: (9, 14), 5: (16, 8)}, lambda c: c.put_glyph_outlines(self.fields)),
            ("image batch", {6: (65, 40), 7: (1, 7)}, lambda c: c.put_images_device([self.image_item(6), self.image_item(7)])),
            ("alpha update", {2: (33, 33)}, lambda c: c.update_video_alpha(2, self.a420, 33, 33, (33, 17, 17, 33), format=A420, matrix=BT709, range=LIMITED)),
            ("compaction", {}, lambda c: c.compact_atlas()),
            # one tile high: the first kernel stores every level it has (20 -> 10 -> 5 -> 3 -> 2), nothing is left for the chain behind it
            ("wide image, one tile high", {8: (2080, 20)}, lambda c: c.put_image_device(*self.image_item(8))),
            # 65 x 5 tiles, levels 0 .. 7: the level-5 image is minified once into the second buffer (level 6), the tail works from there (level 7)
            ("wide image, five tiles high", {9: (2080, 130)}, lambda c: c.put_image_device(*self.image_item(9))),
        ]


def level_rects(w, h, x, y, n_levels):
    """the chain an entry stores: (level, x, y, w, h) while both extents exceed 1"""
    out, l = [], 0
    while w > 1 and h > 1 and l < n_levels:
        out.append((l, x, y, w, h))
        l, x, y, w, h = l + 1, x // 2, y // 2, (w + 1) // 2, (h + 1) // 2
    return out


class Snapshot:
    """what a context shows of its entries at one moment: the rectangles, every level, per group of keys the digest of their draw records"""

    def __init__(self, ctx, sizes, groups):
        self.n_levels = ctx.atlas_size().bit_length()
        self.rects = {k: ctx.image_rect(k) for k in sizes}
        assert all(self.rects[k][2:] == sizes[k] for k in sizes)
        levels = [ctx.read_atlas_level(l) for l in range(self.n_levels)]
        self.texels = {k: self.own_texels(levels, k) for k in sizes}  # (cut out here: a level of this atlas is up to 64 MB)
        self.digests = {}
        for keys in groups:
            ctx.begin_frame(1200, 600, True, (0.1, 0.2, 0.3, 1.0))
            x = 4.0
            for k in keys:  # magnified where small (the draws shrink to the ink boxes), minified where large
                w, h = sizes[k]
                s = 2.5 if w <= 128 else 0.25
                ctx.draw_image(k, (x + 0.25, 6.0), WHITE, (w * s, h * s))
                x += w * s + 3.0
            ctx.end_frame()
            self.digests[keys] = ctx.record_digest()

    def own_texels(self, levels, key):
        """per stored level of `key`: the texels of its rectangle, and which of them lie in no other entry's rectangle of that level"""
        x, y, w, h = self.rects[key]
        out = []
        for l, lx, ly, lw, lh in level_rects(w, h, x, y, self.n_levels):
            own = np.ones((lh, lw), bool)
            for other, (ox, oy, ow, oh) in self.rects.items():
                for ol, px, py, pw, ph in level_rects(ow, oh, ox, oy, self.n_levels):
                    if other != key and ol == l:
                        own[max(py - ly, 0):max(py + ph - ly, 0), max(px - lx, 0):max(px + pw - lx, 0)] = False
            out.append((l, levels[l][ly:ly + lh, lx:lx + lw].copy(), own))
        return out


@pytest.fixture(scope="module")
def runs():
    """the interleaved context's two snapshots -- before the update, which replaces the video frame's texels, and at the end -- and per call
    the snapshot of its fresh context at the same moment"""
    from figdraw_amd.context import HipContext

    memory = Memory()
    steps = Sources(memory).steps()
    moments = {"video frame": 4}  # the snapshot behind this many steps; every other call: at the end
    groups = lambda upto: [tuple(made) for _, made, _ in steps[:upto] if made]

    def play(real):
        """the steps on a fresh context, all of them as they are (real = None) or step `real` alone with transparent images around it"""
        ctx = HipContext(atlas_size=SIZE, device=0)
        sizes, shots = {}, {}
        for i, (name, made, call) in enumerate(steps):
            if real is None or i == real or name == "compaction":
                call(ctx)
            else:
                for k, (w, h) in made.items():
                    if k not in sizes:  # (an update of a transparent image: nothing to do)
                        ctx.put_image(k, np.zeros((h, w, 4), np.uint8))
            sizes.update(made)
            for n, upto in list(moments.items()) + [("end", len(steps))]:
                if i + 1 == upto and (real is None or (steps[real][0] == n if n != "end" else steps[real][0] not in moments)):
                    shots[n] = Snapshot(ctx, dict(sizes), groups(upto) if real is None else [tuple(steps[real][1])])
            if real is not None and shots:
                break
        assert ctx.atlas_size() == SIZE
        ctx.close()
        return shots

    interleaved = play(None)
    fresh = {name: play(i) for i, (name, made, _) in enumerate(steps) if made}
    memory.free()
    return interleaved, fresh


CALLS = ["glyph outline", "video frame", "glyph fields", "image batch", "alpha update", "wide image, one tile high", "wide image, five tiles high"]


def test_every_call_is_compared(runs):
    interleaved, fresh = runs
    assert sorted(fresh) == sorted(CALLS) and set(interleaved) == {"video frame", "end"}
    assert all(len(shots) == 1 for shots in fresh.values())


@pytest.mark.parametrize("name", CALLS)
def test_the_call_alone_leaves_the_same_entry(runs, name):
    interleaved, fresh = runs
    (moment, alone), = fresh[name].items()
    among = interleaved[moment]
    assert among.rects == alone.rects  # the same places: what follows compares like with like
    (keys, digest), = alone.digests.items()
    compared = 0
    for key in keys:
        a, b = among.texels[key], alone.texels[key]
        assert [l for l, _, _ in a] == [l for l, _, _ in b]
        assert a or 1 in among.rects[key][2:]  # (an image 1 texel wide or high stores nothing)
        for (l, ta, own), (_, tb, own_b) in zip(a, b):
            assert np.array_equal(own, own_b) and (l > 0 or own.all())
            assert np.array_equal(ta[own], tb[own]), f"{name}: key {key}, level {l}: {int((ta[own] != tb[own]).any(axis=1).sum())} texels differ"
            compared += int(own.sum())
            if l == 0:
                assert ta.any(), f"{name}: key {key} has no texels at all"
    assert compared > 0
    assert among.digests[keys] == digest, f"{name}: the draw records (the ink boxes) differ"
