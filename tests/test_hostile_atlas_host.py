"""CPU suite: the hostile atlas frames of tests/hostile_atlas_cases.py where no GPU is needed -- the reference side and the host logic.

  * the oracle against every golden the reference's shaders wrote for the direct forms (tests/golden/ss_hostile_atlas_<name>.png): equal to
    the manifest's record, the listed pixels exactly those beyond 1 LSB, at most MAX_GOLDEN_OUTLIERS of them per frame
  * the frames without a golden (ORACLE_ONLY): the oracle within 1 LSB of tests/atlas_sample_ref.py, a float64 restatement of the
    shader's atlas modes, on every quad drawn alone
  * the record-only front-end and the oracle give the same call stream for the node-level frames; their set_cull(2) stream, rendered by
    the oracle, is the oracle's frame bit for bit
  * the frames test what they claim: a deliberately wrong variant of each family's calls or images moves the oracle's frame
  * every rectangle the packer hands out keeps margin_ texels from all four atlas edges (below: why the kernels need that)
  * record counts and drawn pixels

THE PACKER INVARIANT THE KERNELS' 16-BYTE RUNS REST ON (k_composite_strip.inc, build <2>, level 0 of an atlas S wide).

  The 1:1 route (:361-405).  A lane owns pixels px0 .. px0 + 3, px0 a multiple of 4, and reads ONE run of four texels at
  (px0 + tdx, py + tdy), tdx = e.x - q.x0, tdy = e.y - q.y0 (fdh_record.cpp, Recorder::draw_image; q the ceil-snapped quad, as large
  as the entry e).  It reads only if a pixel of it is inside the draw's bounds (:369: py in [by0, by1), px0 + 3 >= bx0, px0 < bx1;
  other lanes read offset 0, :373), and the bounds are inside the quad, so px0 is in [q.x0 - 3, q.x0 + e.w - 1] and py in
  [q.y0, q.y0 + e.h - 1]: the run covers texel columns e.x - 3 .. e.x + e.w + 2 of rows e.y .. e.y + e.h - 1.  Inside the level iff
  e.x >= 3, e.x + e.w + 2 <= S - 1 and the rows exist: margin_ = 4 on every side gives e.x >= 4 and e.x + e.w <= S - 4, one texel to
  spare on each side.  With a smaller margin the run of a quad whose x is 1, 2 or 3 (mod 4) would start in the row above's last texels
  (harmless) or, for an entry in row 0 / the last row, before / after the level (a fault).

  The window (:433-459).  Staged only if wx0 >= 0, wy0 >= 0, wx1 + 3 < S, wy1 < S (:436).  The staging loop reads rows wy0 .. wy1 (:445,
  row <= wy1 - wy0) and per row the runs at wx0 + cc, cc <= (wx1 - wx0) & ~3 <= wx1 - wx0 (:441), i.e. columns up to wx1 + 3 < S: inside
  the level by the condition itself, margin or not.  It then reads LDS at lx <= kWinCols - 2 (+ 1) and ly <= kWinRows - 2 (+ 1 row):
  inside the kWinRows x kWinStride words it staged or left from the last draw -- and a lane INSIDE the quad has fxi in [wx0, wx1 - 1],
  because u is a monotone float function of the pixel column, so its clamp is the identity.

  The gather (:460-472) wraps with & (S - 1): inside the level whatever the coordinates.

So the only address that rests on the packer is the 1:1 run, and it rests on margin_ >= 3 on the left and right; the test below holds the
packer to its margin_ = 4 on all four sides for every way an entry gets its rectangle."""
import numpy as np
import pytest

import atlas_sample_ref as F64
import hostile_atlas_cases as HA
from conftest import diff_stats, load_png
from figdraw_amd.context import HipContext
from oracle import oracle as O
from test_frontend_calls import _same

_ORACLE = {}
_FRAMES = {}


def _oracle(mutant=None):
    if mutant not in _ORACLE:
        o = O.Oracle(atlas_size=HA.ATLAS, threads=8)
        rects = HA.put_images(o, None if mutant is None else HA.mutate_images(mutant))
        _ORACLE[mutant] = (o, rects)
    return _ORACLE[mutant]


def oracle_frame(name, form="direct"):
    if (name, form) not in _FRAMES:
        o, _ = _oracle()
        HA.render(o, name, form)
        _FRAMES[name, form] = o.read_pixels().copy()
        _FRAMES[name, form].setflags(write=False)
    return _FRAMES[name, form]


def _recorder(**kw):
    ctx = HipContext(atlas_size=HA.ATLAS, record_only=True)
    rects = HA.put_images(ctx)
    assert rects == _oracle()[1]  # the same packer, the same rectangles
    return ctx


def test_the_frames_are_what_they_claim():
    """every direct form leaves at most 64 records, every lists form more; every frame is drawn on"""
    ctx = _recorder()
    ctx.set_pick(True)
    for name in HA.FRAMES:
        n = {}
        for form in HA.FORMS:
            HA.render(ctx, name, form)
            n[form] = len(ctx.pick_draw_tags())
            clear = np.floor(np.array(HA.clear_of(name)) * 255 + 0.5).astype(np.uint8)
            assert int((oracle_frame(name, form) != clear).any(axis=2).sum()) > 2000, (name, form)
        assert 0 < n["direct"] <= 64 < n["lists"], (name, n)
    ctx.close()


def test_edge_entries_sit_against_the_atlas_edges():
    r = _oracle()[1]
    S = HA.ATLAS
    assert r[HA.K_NOISE][:2] == (4, 4)
    assert r[HA.K_TALL][1] + r[HA.K_TALL][3] == S - 4
    assert r[HA.K_DISC][0] + r[HA.K_DISC][2] == S - 5 and r[HA.K_ROW][0] + r[HA.K_ROW][2] == S - 6


@pytest.mark.parametrize("name", HA.GOLDEN_FRAMES)
def test_oracle_matches_the_shaders_golden(name, golden_manifest):
    entry = golden_manifest[f"hostile_atlas_{name}"]
    assert (entry["width"], entry["height"], entry["atlas_size"]) == (HA.W, HA.H, HA.ATLAS)
    got, gold = oracle_frame(name), load_png(f"ss_hostile_atlas_{name}.png")
    mx, n0, n1 = diff_stats(got, gold)
    assert {"max": mx, "n_gt0": n0, "n_gt1": n1} == entry["oracle_vs_swiftshader"]
    ys, xs = np.nonzero(np.abs(got.astype(int) - gold.astype(int)).max(axis=2) > 1)
    assert sorted(zip(xs.tolist(), ys.tolist())) == sorted(map(tuple, entry["oracle_gt1"])), name
    assert len(entry["oracle_gt1"]) <= HA.MAX_GOLDEN_OUTLIERS, name


@pytest.mark.parametrize("name", sorted(HA.ORACLE_ONLY))
def test_oracle_matches_the_float64_restatement(name, capsys):
    """the second witness of the frames without a golden: every quad of the family drawn alone, at most 1 LSB"""
    o, rects = _oracle()
    levels = F64.build_atlas(HA.images(), rects, HA.ATLAS)
    _, clear, subpixel = HA.FAMILIES[name]
    worst, differ, drawn = 0, 0, 0
    for i, (call, xf) in enumerate(HA.quads(name)):
        o.W, o.H = HA.W, HA.H
        o.replay(HA.wrap(HA.quad_calls(call, xf), clear, subpixel))
        got = o.read_pixels()
        want = F64.render_quad(call, levels, rects, HA.W, HA.H, clear, xf)
        mx, n0, n1 = diff_stats(got, want)
        worst, differ = max(worst, mx), differ + n0
        drawn += int((want != want[HA.H - 1, 0]).any(axis=2).sum()) if (call[2][0] > 0 and call[2][1] > 0) else 0
        assert mx <= 1, (name, i, call, xf, mx, n0, n1)
    with capsys.disabled():
        print(f"\n  hostile atlas {name}: {len(HA.quads(name))} quads alone, oracle vs float64 max {worst} LSB, {differ} px differ in all", end="")
    assert drawn > 2000, (name, drawn)


def _recorded(name, form, cull=None):
    ctx = _recorder()
    if cull is not None:
        ctx.set_cull(cull)
    ctx.record_begin()
    HA.render(ctx, name, form)
    calls, n = ctx.record_calls(), ctx.culled_draws()
    ctx.close()
    return calls, n


@pytest.mark.parametrize("name", HA.NODE_FRAMES)
def test_front_end_call_streams_are_the_oracles(name):
    for form in HA.FORMS:
        o, _ = _oracle()
        o.record_begin()
        HA.render(o, name, form)
        got, _ = _recorded(name, form)
        _same(o.record_calls(), got)


@pytest.mark.parametrize("name", HA.NODE_FRAMES)
def test_culled_streams_give_the_oracles_frame(name):
    for form in HA.FORMS:
        calls, n = _recorded(name, form, cull=2)
        assert n > 0, (name, form)
        o, _ = _oracle()
        o.W, o.H = HA.W, HA.H
        o.replay(calls)
        assert np.array_equal(o.read_pixels(), oracle_frame(name, form)), (name, form)


# family -> the wrong variants that must show in it (a variant a family has no parameter for is not listed: `shift` needs the sub-pixel
# switch, `mips` a minified or 1:1 draw of the flat-level entry, px_range and threshold a distance field whose slope is not clamped away)
MUTANTS = {
    "window": ("px_range", "threshold", "size", "roll"), "one_to_one": ("shift", "size", "mips", "roll"), "ranges": ("px_range", "threshold", "size", "roll"),
    "minified": ("size", "mips", "roll"), "rotated": ("px_range", "threshold", "size", "mips", "roll"), "rotated_mix": ("px_range", "threshold", "size", "roll"),
    "far_atlas": ("size", "roll"), "far_fields": ("px_range", "threshold", "size", "roll"), "minified_msdf": ("px_range", "threshold", "size", "roll"),
    "steep": ("px_range", "threshold", "size", "mips", "roll"),
}


def test_a_wrong_variant_moves_every_family(capsys):
    """px_range x 1.05, sd_threshold + 1 / 255, the sub-pixel shift dropped, the size + 1 px, the mip levels swapped, the texels rolled by one
    column: each moves the oracle's frame by more than 1 LSB on at least 50 pixels -- a frame that a wrong kernel parameter does not
    move would not catch a kernel that has it wrong"""
    assert set(MUTANTS) == set(HA.FAMILIES)
    lines = []
    for name, kinds in MUTANTS.items():
        base, counts = oracle_frame(name), {}
        for kind in kinds:
            o, _ = _oracle(kind if kind in ("mips", "roll") else None)
            o.W, o.H = HA.W, HA.H
            o.replay(HA.calls(name) if kind in ("mips", "roll") else HA.mutate_calls(HA.calls(name), kind))
            counts[kind] = diff_stats(o.read_pixels(), base)[2]
        lines.append(f"\n  hostile atlas {name:13s} pixels moved by > 1 LSB: " + ", ".join(f"{k} {v}" for k, v in counts.items()))
        assert all(v >= 50 for v in counts.values()), (name, counts)
    with capsys.disabled():
        print("".join(lines), end="")


# ---------------------------------------------------------------- the packer's margin
def _inside(rect, size, margin=4):
    x, y, w, h = rect
    return x >= margin and y >= margin and x + w <= size - margin and y + h <= size - margin


def test_every_rectangle_keeps_the_margin():
    """put_image, put_image_mips, a glyph batch, a growth and fdh_compact_atlas, on a record-only context whose atlas is filled until the
    next put grows it (keep mode: the entries survive the growth and get new rectangles)"""
    rng = np.random.default_rng(HA.SEED)
    ctx = HipContext(atlas_size=64, record_only=True)
    ctx.set_atlas_keep(True)
    keys, grown = [], 0
    nan = float("nan")
    square = np.array([[1, 1, nan, nan, 9, 1], [9, 1, nan, nan, 9, 9], [9, 9, nan, nan, 1, 9], [1, 9, nan, nan, 1, 1]], np.float32)  # four lines, closed
    for i in range(400):
        size = ctx.atlas_size()
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        kind = i % 4
        if kind == 0:
            rect = ctx.put_image(i, np.zeros((h, w, 4), np.uint8))
        elif kind == 1:
            rect = ctx.put_image_mips(i, [np.full((max(h >> l, 1), max(w >> l, 1), 4), 255, np.uint8) for l in range(3)])
        elif kind == 2:
            rect = ctx.put_glyph_coverage_batch([(i, square, w, h)])[0]
        else:
            rect = ctx.put_glyph_outlines([(i, square, w, h)])[0]
        keys.append(i)
        grown += ctx.atlas_size() != size
        assert _inside(tuple(rect)[:4], ctx.atlas_size()), (i, kind, rect, ctx.atlas_size())
        if ctx.atlas_size() != size or i % 97 == 96:  # after a growth, and now and then after a compaction: every entry again
            if ctx.atlas_size() == size:
                ctx.compact_atlas()
            for k in keys:
                assert _inside(ctx.image_rect(k), ctx.atlas_size()), (i, k, ctx.image_rect(k), ctx.atlas_size())
        if grown >= 3:
            break
    assert grown >= 3 and ctx.atlas_size() >= 512
    ctx.compact_atlas(ctx.atlas_size() * 2)
    for k in keys:
        assert _inside(ctx.image_rect(k), ctx.atlas_size()), (k, ctx.image_rect(k))
    ctx.close()
    # the reference's own packer rule, on the frames' atlas: the same rectangles as the oracle's (asserted by _recorder) and inside the margin
    for k, r in _oracle()[1].items():
        assert _inside(r, HA.ATLAS), (k, r)
