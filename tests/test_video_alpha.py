"""Video with an alpha plane in and out on the device (fdh_put_video_alpha, fdh_update_video_alpha, fdh_read_video_alpha;
k_video_alpha_import, k_video_alpha_export; include_video/figdraw_hip_video_alpha.h).  The bar is identity both ways.  The way in: a
context that gets A420, A444, A410 and UYVA frames from device memory against one that gets, through fdh_put_image, the bytes the
reference tests/video_alpha_ref.py makes of them -- every level of the atlases, the draw records (the ink boxes shrink the draws) and a
rendered frame --, and frames with an opaque alpha plane against the sibling calls.  The way out: the planes against the reference
applied to what fdh_read_pixels returns of the same frame, from each plane's pointer to its last row's end, the padding untouched; the
premultiplied planes 0 .. 2 also against the sibling calls' planes on the device, and plane 3 against fdh_read_pixels' alpha."""
import ctypes as C

import numpy as np
import pytest

import video_alpha_cases as VC
import video_alpha_ref as REF

pytestmark = pytest.mark.gpu

WHITE = [(255, 255, 255, 255)] * 4
OPAQUE, TRANSPARENT = (0.1, 0.2, 0.3, 1.0), (0.0, 0.0, 0.0, 0.0)
L, S = REF.CHROMA_LINEAR, REF.STRAIGHT_ALPHA


class Memory:
    """device memory through the runtime the library runs on"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.blocks, self.pinned = [], []

    def device(self, n):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
        self.blocks.append(p)
        return p.value

    def filled(self, n, align=0):
        """n bytes of VC.FILL in device memory at an address `align` past a 256-byte boundary, in a block that ends with them"""
        base = self.device(n + align)
        assert self.hip.hipMemset(C.c_void_p(base), VC.FILL, C.c_size_t(n + align)) == 0
        return base + align

    def upload(self, data: bytes, align=0):
        """`data` in device memory at an address `align` past a 256-byte boundary, in a block that ends with it"""
        base = self.device(len(data) + align)
        assert self.hip.hipMemcpy(C.c_void_p(base + align), data, C.c_size_t(len(data)), 1) == 0  # host -> device
        return base + align

    def download(self, ptr, n):
        out = np.empty(n, np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(n), 2) == 0  # device -> host
        return out

    def page_locked(self, n, data: bytes = None):
        p = C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(p), C.c_size_t(n), 0) == 0
        self.pinned.append(p)
        if data is None:
            C.memset(p.value, VC.FILL, n)
        else:
            C.memmove(p.value, data, n)
        return p.value

    def free(self):
        for p in self.blocks:
            self.hip.hipFree(p)
        for p in self.pinned:
            self.hip.hipHostFree(p)
        self.blocks, self.pinned = [], []


@pytest.fixture(scope="module")
def memory():
    m = Memory()
    yield m
    m.free()


# ------------------------------------------------------------------------------------------------------------------ the way in
def put_case(ctx, memory, key, case, update=False, place=None):
    """`place`: how a plane's bytes get an address (memory.upload by default)"""
    w, h = VC.size_of(case)
    place = place or memory.upload
    packed = VC.pack(case)
    ptrs = VC.four_of(case[1], [place(data, align) for data, align, _ in packed])
    pitches = VC.four_of(case[1], [pitch for _, _, pitch in packed])
    call = ctx.update_video_alpha if update else ctx.put_video_alpha
    return call(key, ptrs, w, h, pitches, format=case[1], matrix=case[2], range=case[3], flags=case[4])


def put_sibling(ctx, memory, key, case):
    """the case's first three planes (or its UYVY plane) through the sibling call: fdh_put_video_planes or fdh_put_video_422"""
    w, h = VC.size_of(case)
    packed = VC.pack(case)[:-1]
    ptrs, pitches = [memory.upload(data, align) for data, align, _ in packed], [pitch for _, _, pitch in packed]
    _, base = REF.BASE[case[1]]
    if REF.packed(case[1]):
        return ctx.put_video_422(key, ptrs + [0, 0], w, h, pitches + [0, 0], format=base, matrix=case[2], range=case[3], flags=case[4] & L)
    return ctx.put_video_planes(key, ptrs, w, h, pitches, format=base, matrix=case[2], range=case[3], flags=case[4] & L)


def levels_of(ctx):
    return [ctx.read_atlas_level(l) for l in range(ctx.atlas_size().bit_length())]


def against_oracle(got, want, what):
    """test_video_frame.py's bar: within 1 LSB, on at most 0.5 % of the pixels"""
    d = np.abs(got.astype(int) - want.astype(int)).max(axis=2)
    print(f"{what}: max |hip - oracle| = {d.max()} LSB on {int((d > 0).sum())} of {d.size} pixels")
    assert d.max() <= 1 and (d > 0).sum() <= 0.005 * d.size, what


def same_atlases(a, b, what=""):
    """usage and every level, byte for byte"""
    assert a.atlas_usage() == b.atlas_usage(), what
    for l, (x, y) in enumerate(zip(levels_of(a), levels_of(b))):
        assert x.shape == y.shape, (what, l)
        if not np.array_equal(x, y):
            ys, xs = np.nonzero((x != y).any(axis=2))
            raise AssertionError(f"{what}: level {l} differs in {len(xs)} texels, the first at ({xs[0]}, {ys[0]}): {x[ys[0], xs[0]]} != {y[ys[0], xs[0]]}")


@pytest.fixture(scope="module")
def two(memory):
    """every case into one atlas of 2048 on two fresh contexts -- the alpha call, and fdh_put_image of the reference's texels -- and into
    the oracle's -> cases, contexts, the oracle, the rectangles"""
    from figdraw_amd.context import HipContext
    from oracle import oracle as O

    cases = VC.in_cases()
    dev, host = (HipContext(atlas_size=2048, device=0) for _ in range(2))
    orc = O.Oracle(atlas_size=2048, threads=8)
    rects = []
    for i, case in enumerate(cases):
        r = put_case(dev, memory, 100 + i, case)
        assert r == host.put_image(100 + i, VC.texels(case)) == tuple(orc.put_image(100 + i, VC.texels(case))), case[0]
        assert r[2:] == VC.size_of(case) and dev.image_rect(100 + i) == r
        rects.append(r)
    assert dev.atlas_size() == 2048
    yield cases, dev, host, orc, rects
    dev.close(), host.close()


def test_rectangles_usage_and_every_level(two):
    cases, dev, host, _, rects = two
    assert {(c[1], c[4]) for c in cases} == set(VC.KINDS)
    same_atlases(dev, host, "all cases, against fdh_put_image")
    level0 = dev.read_atlas_level(0)
    for case, (x, y, w, h) in zip(cases, rects):  # and level 0 is the reference's conversion (nothing of a line)
        want = VC.texels(case) if w > 1 and h > 1 else np.zeros((h, w, 4), np.uint8)
        assert np.array_equal(level0[y:y + h, x:x + w], want), case[0]


def _frame(ctx, rects):
    """every image up to 128 x 128 at 1:1 and magnified 2.5 times (the draws shrink to the ink boxes), the larger ones minified"""
    W, H = 2000, 1800
    ctx.begin_frame(W, H, True, (0.1, 0.2, 0.3, 1.0))
    x, y, row, n = 4.0, 4.0, 0.0, 0
    for i, r in enumerate(rects):
        w, h = r[2:]
        for s in ((0.25,) if w > 128 or h > 128 else (1.0, 2.5)):
            if x + w * s > W - 4:
                x, y, row = 4.0, y + row + 3.0, 0.0
            ctx.draw_image(100 + i, (x + 0.25 * (i % 3), y), WHITE, (w * s, h * s), i % 7 == 3)
            x += w * s + 3.0
            row = max(row, h * s)
            n += 1
    assert y + row < H
    ctx.end_frame()
    return n


def test_draw_records_and_frames(two):
    """the ink boxes: the draw records are those of the host path (a draw shrinks to its image's ink box), and so is the rendered frame:
    what the library draws of the converted image given through fdh_put_image -- and the frame matches the oracle of the converted
    images, every alpha and the ink-shrunk boxes among them (two contexts share a compositor; the oracle does not)"""
    cases, dev, host, orc, rects = two
    for ctx in (dev, host, orc):
        n = _frame(ctx, rects)
    assert n > 60
    assert dev.record_digest() == host.record_digest()
    got = dev.read_pixels()
    assert np.array_equal(got, host.read_pixels())
    against_oracle(got, orc.read_pixels(), "all cases")


def test_updates_of_every_case(two, memory):
    """(behind the tests of the puts: it changes the fixture's atlases) every entry gets the next frame on both paths"""
    from oracle import oracle as O

    cases, dev, host, _, rects = two
    nxt = VC.in_cases(again=True)
    orc = O.Oracle(atlas_size=2048, threads=8)  # (the oracle has no update: a fresh one takes the new texels into the same rectangles)
    for i, case in enumerate(nxt):
        texels = VC.texels(case)
        assert not np.array_equal(texels, VC.texels(cases[i])), case[0]
        put_case(dev, memory, 100 + i, case, update=True)
        host.update_image(100 + i, texels)
        assert tuple(orc.put_image(100 + i, texels)) == rects[i]
    same_atlases(dev, host, "all cases updated, against fdh_update_image")
    for ctx in (dev, host, orc):
        _frame(ctx, rects)
    assert dev.record_digest() == host.record_digest()
    got = dev.read_pixels()
    assert np.array_equal(got, host.read_pixels())
    against_oracle(got, orc.read_pixels(), "all cases updated")
    memory.free()


def test_opaque_alpha_planes_leave_the_sibling_calls_atlas(memory):
    """every case but the largest with its alpha plane all 255 (1023 for A410), under the case's flags -- FDH_VIDEO_STRAIGHT_ALPHA among
    them --: what fdh_put_video_planes (I420, I444, I410) or fdh_put_video_422 (UYVY) leaves of the first three planes"""
    from figdraw_amd.context import HipContext

    dev, sib = HipContext(atlas_size=2048, device=0), HipContext(atlas_size=2048, device=0)
    cases = [VC.opaque(c) for c in VC.in_cases(largest=False)]
    assert {(c[1], c[4]) for c in cases} == set(VC.KINDS)
    for i, case in enumerate(cases):
        assert put_case(dev, memory, 100 + i, case) == put_sibling(sib, memory, 100 + i, case), case[0]
    same_atlases(dev, sib, "opaque alpha planes, against the sibling calls")
    dev.close(), sib.close()
    memory.free()


def small_case(fmt, flags, w, h, seed, layout="padded", matrix=REF.BT601, rng=REF.FULL):
    return (f"{REF.NAMES[fmt]} {w} x {h} seed {seed}", fmt, matrix, rng, flags, VC.noise_stored(np.random.default_rng(seed), fmt, w, h), layout, w)


def test_page_locked_host_memory_is_a_source(memory):
    from figdraw_amd.context import HipContext

    dev, host = HipContext(atlas_size=256, device=0), HipContext(atlas_size=256, device=0)
    for key, (fmt, flags) in enumerate(((REF.A410, S), (REF.UYVA, L), (REF.A420, L | S), (REF.A444, 0)), start=1):
        case = small_case(fmt, flags, 71, 45, 30 + key, layout="tight", matrix=REF.BT2020, rng=REF.LIMITED)
        assert put_case(dev, memory, key, case, place=lambda data, align: memory.page_locked(len(data), data)) == host.put_image(key, VC.texels(case))
        put_case(dev, memory, key, case, update=True, place=lambda data, align: memory.page_locked(len(data), data))
        host.update_image(key, VC.texels(case))
    same_atlases(dev, host, "page-locked")
    dev.close(), host.close()


def test_pageable_host_memory_is_refused_for_each_of_the_four_planes(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    host_planes = [np.zeros((9, 16), np.uint8) for _ in range(4)]
    good = [memory.upload(p.tobytes()) for p in host_planes]
    packed_host = np.zeros((9, 32), np.uint8)
    packed_good = memory.upload(packed_host.tobytes())
    pitches = (16, 16, 16, 16)
    assert ctx.put_video_alpha(1, good, 16, 9, pitches, format=REF.A444)[2:] == (16, 9)
    before = ctx.atlas_usage()
    attempts = []
    for p in range(4):
        ptrs = list(good)
        ptrs[p] = host_planes[p].ctypes.data
        attempts.append((ptrs, pitches, REF.A444))
    attempts.append(([packed_host.ctypes.data, 0, 0, good[3]], (32, 0, 0, 16), REF.UYVA))
    attempts.append(([packed_good, 0, 0, host_planes[3].ctypes.data], (32, 0, 0, 16), REF.UYVA))
    for ptrs, pt, fmt in attempts:
        for call in (lambda: ctx.put_video_alpha(2, ptrs, 16, 9, pt, format=fmt), lambda: ctx.update_video_alpha(1, ptrs, 16, 9, pt, format=fmt)):
            with pytest.raises(FigdrawHipError) as e:
                call()
            assert e.value.code == -1 and "neither device memory of the context's device nor page-locked host memory" in str(e.value)
            assert ctx.atlas_usage() == before and not ctx.has_image(2)
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    assert ctx.put_video_alpha(2, good, 16, 9, pitches, format=REF.A444, flags=S)[2:] == (16, 9)  # and the context works on
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the way out
def noise(w, h, seed=0):
    """premultiplied noise with every alpha: a quarter of the texels transparent, a quarter opaque"""
    rng = np.random.default_rng(1000 * w + h + seed)
    img = rng.integers(0, 256, size=(h, w, 4)).astype(np.uint16)
    kind = rng.integers(0, 4, size=(h, w))
    img[kind == 0, 3], img[kind == 1, 3] = 0, 255
    img[..., :3] = img[..., :3] * img[..., 3:] // 255
    return img.astype(np.uint8)


def render(ctx, w, h, clear, seed=0):
    """a few shapes, then the noise image 1:1 over them: neighbouring pixels differ in every channel, alpha among them over a transparent
    clear"""
    ctx.put_image(1, noise(w, h, seed))
    ctx.begin_frame(w, h, True, clear)
    ctx.draw_rect((0.0, 0.0, w * 0.6, h * 0.5), (200, 40, 90, 255))
    ctx.draw_rect((w * 0.3, h * 0.25, w * 0.7, h * 0.75), (10, 220, 160, 180))
    ctx.draw_image(1, (0.0, 0.0), WHITE, (float(w), float(h)))
    ctx.end_frame()
    return ctx.read_pixels()


def export(ctx, memory, frame, fmt, m, r, flags, layout, rect=None, alloc=None, ptrs=None):
    """one fdh_read_video_alpha into fresh blocks of VC.FILL (or at `ptrs`) and its comparison with the reference applied to `frame`
    -> the pointers, the layout, the stored planes"""
    h, w = frame.shape[:2]
    case = (f"{w} x {h} rect {rect} {REF.NAMES[fmt]} m{m} r{r} f{flags} {layout}", w, h, rect, fmt, m, r, flags, layout)
    lay = VC.layouts(case)
    alloc = alloc or memory.filled
    sizes = [VC.plane_bytes(pitch, rows, row_bytes) for _, pitch, rows, row_bytes in lay]
    ptrs = ptrs or [alloc(n, align) for n, (align, _, _, _) in zip(sizes, lay)]
    ctx.read_video_alpha(VC.four_of(fmt, ptrs), VC.four_of(fmt, [l[1] for l in lay]), format=fmt, matrix=m, range=r, flags=flags, rect=rect)
    want = VC.expected_planes(case, frame)
    got = [memory.download(ptr, n) for ptr, n in zip(ptrs, sizes)]
    for p, (a, b) in enumerate(zip(got, want)):
        if not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            raise AssertionError(f"{case[0]}: plane {VC.plane_ids(fmt)[p]} differs in {int((a != b).sum())} bytes, the first at {at} (pitch {lay[p][1]}): {a[at]} != {b[at]}")
    return ptrs, lay, VC.stored_of(got, case)


def sibling_planes(ctx, memory, frame, fmt, m, r, flags, rect=None):
    """the sibling call's planes of the same frame, matrix, range and chroma rule, tightly packed: fdh_read_video_planes, fdh_read_video_422"""
    _, base = REF.BASE[fmt]
    _, _, w, h = rect or (0, 0, frame.shape[1], frame.shape[0])
    ids = VC.plane_ids(fmt)[:-1]
    sizes = [VC.plane_size(fmt, p, w, h) for p in ids]
    ptrs = [memory.filled(row * rows) for row, rows in sizes]
    pad = [0] * (3 - len(ids))
    call = ctx.read_video_422 if REF.packed(fmt) else ctx.read_video_planes
    call(ptrs + pad, [row for row, _ in sizes] + pad, format=base, matrix=m, range=r, flags=flags & L, rect=rect)
    return [memory.download(ptr, row * rows).view(REF.dtype_of(fmt)).reshape(rows, -1) for ptr, (row, rows) in zip(ptrs, sizes)]


CLEARS = (OPAQUE, TRANSPARENT)
# the smallest that still break a kernel, and the tile's width +- 1 by its height +- 1: 8 rows for the one-row builds, 16 for A420 (`t`)
OUT_SIZES = [(1, 1, 0), (2, 1, 0), (7, 3, 0), (9, 2, 0)] + [(w, 8 + d, 1) for w in (255, 256, 257) for d in (-1, 0, 1)]


@pytest.mark.parametrize("w,h,tile", OUT_SIZES, ids=[f"{w}x{h}" for w, h, _ in OUT_SIZES])
def test_every_kind_and_layout_against_the_reference(memory, w, h, tile):
    """every format x chroma rule x straight x layout against the reference applied to fdh_read_pixels, the six rows of the coefficient
    table dealt out over them, over an opaque and over a transparent clear; the premultiplied planes 0 .. 2 are the sibling call's planes
    on the device, plane 3 is fdh_read_pixels' alpha (its a10 for A410); the frame is untouched and the padding still holds the fill
    (export compares every byte from a plane's pointer to its last row's end)"""
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=512, device=0)
    n = 0
    for fmt in REF.FORMATS:
        hh = h + 8 if tile and fmt == REF.A420 else h  # 15 / 16 / 17 rows for A420's tile
        frame = render(ctx, w, hh, CLEARS[(w + h + fmt) & 1])
        if w * hh >= 64:
            assert (frame[..., 3] == 255).any() and ((frame[..., 3] < 255).any() == (CLEARS[(w + h + fmt) & 1] is TRANSPARENT))
        for li, layout in enumerate(VC.LAYOUTS):
            for ki, flags in enumerate(fl for f, fl in VC.KINDS if f == fmt):
                m, r = VC.MATRIX_RANGE[(ki + li + w + fmt) % 6]
                _, _, stored = export(ctx, memory, frame, fmt, m, r, flags, layout)
                assert np.array_equal(stored[-1], REF.alpha_out(frame[..., 3], fmt)), (fmt, flags, layout)
                if not flags & S and layout == "tight":
                    want = sibling_planes(ctx, memory, frame, fmt, m, r, flags)
                    assert len(want) == len(stored) - 1 and all(np.array_equal(a, b) for a, b in zip(stored, want)), (fmt, flags)
                n += 1
        assert np.array_equal(ctx.read_pixels(), frame)  # the frame is untouched
    assert n == 36
    ctx.close()
    memory.free()


def test_rectangles_are_the_export_of_the_cropped_frame(memory):
    """the odd-y rectangles that UYVA allows and A420 refuses among them, and odd x for A444 / A410"""
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, *VC.RECT_SOURCE, TRANSPARENT)
    for ki, (fmt, flags) in enumerate(VC.KINDS):
        for k, rect in enumerate(VC.rects(fmt)):
            m, r = VC.MATRIX_RANGE[(k + ki) % 6]
            export(ctx, memory, frame, fmt, m, r, flags, VC.LAYOUTS[(k + ki) % 3], rect=rect)
    rect = VC.rects(REF.UYVA)[-1]
    assert rect[1] & 1 and np.array_equal(ctx.read_pixels(*rect), VC.cropped(frame, rect))
    with pytest.raises(FigdrawHipError) as e:
        export(ctx, memory, frame, REF.A420, 0, 0, 0, "tight", rect=rect)
    assert "the rectangle's x and y must be even for A420" in str(e.value)
    assert np.array_equal(ctx.read_pixels(), frame)
    ctx.close()
    memory.free()


def test_a_page_locked_destination_and_ndis_one_block(memory):
    from figdraw_amd.context import HipContext

    ctx = HipContext(atlas_size=256, device=0)
    frame = render(ctx, 71, 45, TRANSPARENT)
    pinned = Memory()
    pinned.download = lambda ptr, n: np.ctypeslib.as_array((C.c_uint8 * n).from_address(ptr)).copy()
    try:
        for fmt, flags, layout in ((REF.A420, L | S, "tight"), (REF.UYVA, 0, "padded"), (REF.A410, S, "aligned"), (REF.A444, 0, "aligned"), (REF.UYVA, L | S, "aligned")):
            export(ctx, pinned, frame, fmt, REF.BT2020, REF.LIMITED, flags, layout, alloc=lambda n, align: pinned.page_locked(n + align) + align)
    finally:
        pinned.free()
    # NDI's layout: one contiguous block, the UYVY plane and the alpha plane right behind it
    uyvy, alpha = 4 * 36 * 45, 71 * 45
    block = memory.filled(uyvy + alpha + 16)
    export(ctx, memory, frame, REF.UYVA, REF.BT709, REF.LIMITED, 0, "tight", ptrs=[block, block + uyvy])
    assert (memory.download(block + uyvy + alpha, 16) == VC.FILL).all()
    ctx.close()
    memory.free()


def colour_movement():
    """how far a colour byte may move through A444 full range and back, from the two references on the CPU alone: every colour of a lattice
    of step 3 and a million random ones, per matrix the largest |back - colour|.  The colours are opaque here, and the figure holds for the
    premultiplied bytes of a texel of any alpha all the same: premultiplied A444 is N = 1 without FDH_VIDEO_STRAIGHT_ALPHA both ways, every
    sample is made of the texel's three colour bytes as stored and every colour byte of those three samples -- the alpha byte enters
    neither conversion, it travels in its own plane unchanged"""
    g = np.arange(0, 256, 3)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 1, 3)
    rnd = np.random.default_rng(99).integers(0, 256, size=(1_000_000, 1, 3))
    img = np.concatenate([lattice, rnd]).astype(np.uint8)
    img = np.concatenate([img, np.full(img.shape[:2] + (1,), 255, np.uint8)], axis=2)
    out = {}
    for m in (REF.BT601, REF.BT709, REF.BT2020):
        back = REF.convert(REF.export(img, REF.A444, m, REF.FULL), REF.A444, m, REF.FULL)
        out[m] = int(np.abs(back.astype(int) - img.astype(int))[..., :3].max())
    return out


def test_round_trip_through_a444(memory):
    """export premultiplied A444 full range, put it back, draw it 1:1 over a transparent clear.  How far a texel may move is computed
    first, on the CPU, from the two references (colour_movement; the figure is in profiles/video_alpha.txt): alpha not at all, a colour
    byte of the entry by what the 8-bit YCbCr grid loses, whatever the alpha beside it -- the premultiplied bytes go through as they are.
    The compositor is no identity on an image with alpha (draw_image weighs the sampled colour with the sampled alpha, for an image
    given through fdh_put_image just the same), so the frame drawn from the entry is held against the frame drawn the same way from
    the exported frame itself as an fdh_put_image image: a draw maps a colour byte monotonically with a slope of at most 1, alpha given,
    so two drawn texels lie no further apart than the two colour bytes they were drawn from."""
    from figdraw_amd.context import HipContext

    bound = colour_movement()
    print(f"A444 full range there and back, the references on the CPU: max |back - colour| = {bound}")
    assert all(0 < v <= 3 for v in bound.values())  # (the 8-bit grid: a sanity bracket of the figure, not the assertion below)
    a, b, plain = (HipContext(atlas_size=256, device=0) for _ in range(3))
    frame = render(a, 71, 45, TRANSPARENT)

    def drawn(ctx, key):
        ctx.begin_frame(71, 45, True, TRANSPARENT)
        ctx.draw_image(key, (0.0, 0.0), WHITE, (71.0, 45.0))
        ctx.end_frame()
        return ctx.read_pixels()

    plain.put_image(1, frame)
    base = drawn(plain, 1)
    assert np.array_equal(base[..., 3], frame[..., 3])
    for key, m in enumerate((REF.BT601, REF.BT709, REF.BT2020), start=1):
        ptrs, lay, _ = export(a, memory, frame, REF.A444, m, REF.FULL, 0, "padded")
        x, y, w, h = b.put_video_alpha(key, ptrs, 71, 45, [l[1] for l in lay], format=REF.A444, matrix=m, range=REF.FULL)
        want = REF.convert(REF.export(frame, REF.A444, m, REF.FULL), REF.A444, m, REF.FULL)
        entry = b.read_atlas_level(0)[y:y + h, x:x + w]
        assert np.array_equal(entry, want), m
        moved = np.abs(entry.astype(int) - frame.astype(int))
        assert moved[..., 3].max() == 0 and moved[..., :3].max() <= bound[m], (m, int(moved[..., :3].max()), bound[m])
        back = drawn(b, key)
        d = np.abs(back.astype(int) - base.astype(int))
        # the slope claim itself, texel by texel and channel by channel: drawn from bytes that differ by k, under the same alpha, two drawn
        # bytes differ by at most k -- so by nothing where the entry holds the frame's byte
        assert (d[..., :3] <= moved[..., :3]).all(), (m, int((d[..., :3] > moved[..., :3]).sum()))
        print(f"m{m}: the entry against the frame: max colour {int(moved[..., :3].max())}; drawn 1:1, against the frame drawn 1:1: max colour {int(d[..., :3].max())}, alpha {int(d[..., 3].max())}")
        assert d[..., 3].max() == 0 and d[..., :3].max() <= bound[m], (m, int(d[..., :3].max()), bound[m])
    a.close(), b.close(), plain.close()
    memory.free()


# ------------------------------------------------------------------------------------------------------------------ refusals: each in front of any launch
def test_refusals_on_a_device_context(memory):
    from figdraw_amd.context import FigdrawHipError, HipContext

    ctx = HipContext(atlas_size=256, device=0)
    sizes = (16 * 9,) * 4
    good = [memory.filled(n) for n in sizes]
    pitches = (16, 16, 16, 16)

    def refused(text, ptrs, pitches=pitches, format=REF.A444, **kw):
        with pytest.raises(FigdrawHipError) as e:
            ctx.read_video_alpha(ptrs, pitches, format=format, **kw)
        assert e.value.code == -1 and str(e.value).split("] ", 1)[1].startswith("read_video_alpha: ") and text in str(e.value), str(e.value)
        assert all((memory.download(p, n) == VC.FILL).all() for p, n in zip(good, sizes))

    def with_plane(p, ptr):
        ptrs = list(good)
        ptrs[p] = ptr
        return ptrs

    refused("no frame has been submitted", good)
    frame = render(ctx, 16, 9, TRANSPARENT)
    # pageable host memory, for each of the four planes and for UYVA's two
    pageable = [np.full(n, VC.FILL, np.uint8) for n in sizes]
    for p in range(4):
        refused("neither device memory of the context's device nor page-locked host memory", with_plane(p, pageable[p].ctypes.data))
    packed_host, packed_good = np.full(32 * 9, VC.FILL, np.uint8), memory.filled(32 * 9)
    refused("neither device memory of the context's device nor page-locked host memory", [packed_host.ctypes.data, 0, 0, good[3]], (32, 0, 0, 16), format=REF.UYVA)
    refused("neither device memory of the context's device nor page-locked host memory", [packed_good, 0, 0, pageable[3].ctypes.data], (32, 0, 0, 16), format=REF.UYVA)
    assert all((a == VC.FILL).all() for a in pageable) and (packed_host == VC.FILL).all() and (memory.download(packed_good, 32 * 9) == VC.FILL).all()
    assert memory.hip.hipGetLastError() == 0  # the sticky error was cleared
    # a plane inside the context's own surface (the atlas's address is not handed out: its rule is read_video_422's loop, untested there too)
    surface = ctx.frame_device_ptr()[0]
    for p in range(4):
        refused("a plane overlaps the context's own frame surface", with_plane(p, surface + 16 * 9 * 4 - 2))
    refused("a plane overlaps the context's own frame surface", [surface + 16, 0, 0, good[3]], (32, 0, 0, 16), format=REF.UYVA)
    # two planes in one block, one inside the other's bytes
    refused("planes 2 and 3 overlap", with_plane(3, good[2] + 16 * 9 - 1))
    # the rules that need no device hold here too
    refused("the rectangle's x and y must be even for A420", good, (16, 8, 8, 16), format=REF.A420, rect=(0, 1, 4, 4))
    refused("the rectangle's x must be even for UYVA", [packed_good, 0, 0, good[3]], (32, 0, 0, 16), format=REF.UYVA, rect=(1, 0, 4, 4))
    refused("rectangle outside the frame", good, rect=(2, 0, 16, 9))
    refused("unknown format", good, format=5)
    refused("FDH_VIDEO_IGNORE_ALPHA is the sibling call", good, flags=REF.IGNORE_ALPHA)
    refused("planes[1], planes[2] and their pitches must be 0", good, format=REF.UYVA)
    # under a row stripe
    ctx.set_stripe(0, 4)
    refused("not under fdh_set_stripe", good)
    ctx.set_stripe(0, 0)
    assert np.array_equal(ctx.read_pixels(), frame)
    # and the context works on: an odd x and y are fine for 4:4:4
    ctx.read_video_alpha(good, pitches, format=REF.A444, flags=S, rect=(3, 3, 13, 5))
    want = REF.export(frame[3:8, 3:16], REF.A444, REF.BT709, REF.LIMITED, S)
    for ptr, pitch, plane in zip(good, pitches, want):
        got = memory.download(ptr, pitch * 5).reshape(5, pitch)
        assert np.array_equal(got[:, :plane.shape[1]], plane) and (got[:, plane.shape[1]:] == VC.FILL).all()
    ctx.close()
