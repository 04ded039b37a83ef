"""Glyph coverage on the device against exact pixel areas (k_rasterize_lines, k_coverage_cells_batch, k_coverage_sum_batch): the outlines of
tests/coverage_hostile_cases.py through every route that rasterises coverage -- fdh_put_glyph_outline, fdh_put_glyph_coverage_batch in the
given and in the reversed order, fdh_put_glyph_outline_cubic, fdh_put_glyph_coverage_batch_cubic --, one context per route, and every texel
of level 0 held DIRECTLY to tests/coverage_exact_ref.py's float64 polygon clipping of the route's flattened lines:
|texel - 255 c| <= 0.5 + e, e per family from coverage_hostile_cases.E.  Then, as everywhere else, the oracle's bytes, and all routes the same
texels.  Unfiltered coverage only: the LCD routes stay with their byte-equality tests."""
import numpy as np
import pytest

import coverage_cases as CC
import coverage_hostile_cases as H
import msdf_cubic_cases as MCC
from test_coverage_exact_host import REF_EPS

pytestmark = pytest.mark.gpu
ROUTES = ("outline", "batch", "batch reversed", "outline cubic", "batch cubic")
ATLAS = 512


def put(ctx, route, cases):
    """-> the rectangles, in the order of `cases`"""
    quadratic = [(1000 + i, H.as6(segs), w, h) for i, (_, _, segs, w, h) in enumerate(cases)]
    cubic = [(1000 + i, H.as8(segs), w, h) for i, (_, _, segs, w, h) in enumerate(cases)]
    if route == "outline":
        return [ctx.put_glyph_outline(*g) for g in quadratic]
    if route == "batch":
        return ctx.put_glyph_coverage_batch(quadratic)
    if route == "batch reversed":
        return ctx.put_glyph_coverage_batch(quadratic[::-1])[::-1]
    if route == "outline cubic":
        return [ctx.put_glyph_outline_cubic(*g) for g in cubic]
    return ctx.put_glyph_coverage_batch_cubic(cubic)


@pytest.fixture(scope="module")
def filled():
    """-> the cases, {route: (level 0 (512, 512, 4), the rectangles in the cases' order)}"""
    from figdraw_amd.context import HipContext

    cases = H.cases()
    out = {}
    for route in ROUTES:
        ctx = HipContext(atlas_size=ATLAS, device=0)
        rects = put(ctx, route, cases)
        assert ctx.atlas_size() == ATLAS and all(ctx.has_image(1000 + i) for i in range(len(cases))), route
        assert [tuple(r[2:]) for r in rects] == [(w, h) for _, _, _, w, h in cases]
        out[route] = (ctx.debug_read_surface(4), rects)
        ctx.close()
    return cases, out


@pytest.fixture(scope="module")
def lines():
    """{cubic route or not: the flattened lines of every case}: coverage_cases.flatten's (the oracle's fo_flatten_outline) for the quadratic routes,
    msdf_cubic_cases.flatten_lines' for the cubic ones"""
    from oracle import oracle as O

    return {False: [CC.flatten(O, H.as6(segs)) for _, _, segs, _, _ in H.cases()], True: [MCC.flatten_lines(H.as8(segs)) for _, _, segs, _, _ in H.cases()]}


@pytest.mark.parametrize("route", ROUTES)
def test_device_against_exact_areas(filled, lines, route):
    """every texel of every rectangle: |texel - 255 c| <= 0.5 + e, c the exact coverage of the lines this route rasterises"""
    from oracle import oracle as O

    cases, out = filled
    level0, rects = out[route]
    worst, failed = {}, []
    for (family, name, segs, w, h), (x, y, _, _), own in zip(cases, rects, lines["cubic" in route]):
        got = level0[y:y + h, x:x + w]
        if w == 1 or h == 1:  # placed and unwritten: the level chain stores nothing of such an image
            assert not got.any(), name
            continue
        # the reference of this route's own lines: made once for all routes where the lines are the same, which they are
        assert np.array_equal(own, H.lines6(O, segs)), f"{name}: the route's lines are not the quadratic route's"
        c = H.exact(O, family, name)
        assert (got == got[..., :1]).all(), name  # premultiplied white
        e = H.E[family][1] + REF_EPS
        ex, at, n = H.hold(got[..., 0], c, e)
        if ex > worst.get(family, (-1.0, ""))[0]:
            worst[family] = (ex, f"{name}: texel (x {at[1]}, y {at[0]}) reads {int(got[at][0])}, exact {255.0 * c[at]:.6f}")
        if n:
            failed.append(f"{family}, {name}: {n} of {w * h} texels, the worst by {ex:.6f}")
    for family, (ex, what) in worst.items():
        print(f"{route}, {family}: largest |texel - 255 c| - 0.5 = {ex:.6f} LSB, {what}; e = {H.E[family][1]:.6f}")
    assert set(worst) == set(H.E) and not failed, failed


@pytest.mark.parametrize("route", ROUTES)
def test_device_is_the_oracle(filled, lines, route):
    """byte equality with the oracle's image of the same lines, the whole of level 0"""
    from oracle import oracle as O

    cases, out = filled
    level0, rects = out[route]
    want = np.zeros_like(level0)
    for (_, name, segs, w, h), (x, y, _, _), own in zip(cases, rects, lines["cubic" in route]):
        if w > 1 and h > 1:
            want[y:y + h, x:x + w] = O.rasterize_outline(MCC.lines_as_outline(own), w, h)
    assert want.any() and np.array_equal(level0, want), f"{int((level0 != want).any(axis=2).sum())} texels differ from the oracle's"


def test_all_routes_give_the_same_texels(filled):
    cases, out = filled
    first, rects = out["outline"]
    for route in ("batch", "outline cubic", "batch cubic"):  # the same order: the same rectangles, whole arrays
        assert out[route][1] == rects and np.array_equal(out[route][0], first), route
    other, back = out["batch reversed"]
    assert back != rects
    for (_, name, _, w, h), (x, y, _, _), (u, v, _, _) in zip(cases, rects, back):
        assert np.array_equal(other[v:v + h, u:u + w], first[y:y + h, x:x + w]), name
