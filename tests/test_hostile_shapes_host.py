"""CPU suite: the hostile frames of tests/hostile_cases.py where no GPU is needed -- the reference pair and the host logic.

  * the oracle against every golden the reference's shaders wrote for the direct forms (tests/golden/ss_hostile_<name>.png): at most 1 LSB,
    except the pixels tests/golden/manifest.json lists, which must be exactly the pixels where the oracle IS more than 1 LSB away, at most
    hostile_cases.MAX_GOLDEN_OUTLIERS per frame (the GPU test may leave out of its 2-LSB bar those and no others)
  * the library's record-only front-end and the oracle's give the same call stream for every node-level frame, both forms
  * the set_cull(2) stream of every node-level frame, rendered by the oracle, is the oracle's own frame bit for bit
  * fdh_saturated_core_union over a hostile sweep (half extents 0.15 .. 300, radii 0 .. 1000 and elliptical, AA factors 0.05 .. 50, modes
    3, 7, 9, 11, 12, spread -500 .. 40, weights -3 .. 500): every rectangle saturated and inside the quad, with the formulas of
    tests/test_core_union_host.py"""
import ctypes as C

import numpy as np
import pytest

import hostile_cases as HC
import test_core_union_host as CU
from conftest import diff_stats, load_png
from figdraw_amd.context import HipContext
from oracle import oracle as O
from test_frontend_calls import _same

_FRAMES = {}


def oracle_frame(name, form="direct"):
    if (name, form) not in _FRAMES:
        o = O.Oracle(threads=8)
        HC.render(o, name, form)
        _FRAMES[name, form] = o.read_pixels().copy()
        _FRAMES[name, form].setflags(write=False)
    return _FRAMES[name, form]


def _records(name, form):
    """the draw records the library makes of a frame (culling as on a rendering context), counted by their pick tags"""
    ctx = HipContext(record_only=True)
    ctx.set_pick(True)
    HC.render(ctx, name, form)
    n = len(ctx.pick_draw_tags())
    ctx.close()
    return n


def test_the_frames_are_what_they_claim():
    """every direct form leaves at most 64 records (`stack` apart), every lists form more (no frame here has a second phase); every frame
    is drawn on"""
    for name in HC.FRAMES:
        d, l = _records(name, "direct"), _records(name, "lists")
        assert (0 < d <= 64 or name == "stack") and l > 64, (name, d, l)
        clear = np.round(np.array(HC.clear_of(name)) * 255).astype(np.uint8)
        for form in HC.FORMS:
            assert int((oracle_frame(name, form) != clear).any(axis=2).sum()) > 2000, (name, form)


@pytest.mark.parametrize("name", HC.FRAMES)
def test_oracle_matches_the_shaders_golden(name, golden_manifest):
    entry = golden_manifest[f"hostile_{name}"]
    assert (entry["width"], entry["height"]) == (HC.W, HC.H)
    got, gold = oracle_frame(name), load_png(f"ss_hostile_{name}.png")
    mx, n0, n1 = diff_stats(got, gold)
    assert {"max": mx, "n_gt0": n0, "n_gt1": n1} == entry["oracle_vs_swiftshader"]
    ys, xs = np.nonzero(np.abs(got.astype(int) - gold.astype(int)).max(axis=2) > 1)
    assert sorted(zip(xs.tolist(), ys.tolist())) == sorted(map(tuple, entry["oracle_gt1"])), name
    assert len(entry["oracle_gt1"]) <= HC.MAX_GOLDEN_OUTLIERS, name


def _recorded(name, form, cull=None):
    ctx = HipContext(record_only=True)
    if cull is not None:
        ctx.set_cull(cull)
    ctx.record_begin()
    HC.render(ctx, name, form)
    calls, n = ctx.record_calls(), ctx.culled_draws()
    ctx.close()
    return calls, n


@pytest.mark.parametrize("name", HC.NODE_FRAMES)
def test_front_end_call_streams_are_the_oracles(name):
    for form in HC.FORMS:
        o = O.Oracle(threads=8)
        o.record_begin()
        HC.render(o, name, form)
        got, _ = _recorded(name, form)
        _same(o.record_calls(), got)
        d = HC.n_draws(got)
        assert d <= 64 if form == "direct" else d > 64, (name, form, d)


@pytest.mark.parametrize("name", HC.NODE_FRAMES)
def test_culled_streams_give_the_oracles_frame(name):
    for form in HC.FORMS:
        calls, n = _recorded(name, form, cull=2)
        assert n > 0, (name, form)
        o = O.Oracle(threads=8)
        o.W, o.H = HC.W, HC.H
        o.replay(calls)
        assert np.array_equal(o.read_pixels(), oracle_frame(name, form)), (name, form)


# ---------------------------------------------------------------- the core rule on a hostile sweep
SWEEP_HALF_EXTENTS = [(0.15, 0.15), (0.4, 20.3), (2.5, 300.0), (20.3, 7.5), (48.75, 130.0), (300.0, 48.75)]
SWEEP_RADII = [((0, 0, 0, 0), None), ((0.4, 0.4, 0.4, 0.4), None), ((7.5, 7.5, 7.5, 7.5), None), ((1000, 1000, 1000, 1000), None), ((0, 1, 7.5, 30), None),
               ((4, 8, 100, 1), (8, 1, 1, 100))]
SWEEP_AA = [0.05, 0.3, 1.2, 4.0, 50.0]
SWEEP_MODES = [3, 7, 9, 11, 12]
# (factor = blur or stroke weight, spread, inner-shadow offset)
SWEEP_PARAMS = [(-3.0, 0.0, (3.0, -2.0)), (0.0, -500.0, (-4.5, 6.0)), (0.2, -8.0, (0.0, 0.0)), (1.0, 0.0, (50.0, -40.0)), (5.0, 4.0, (3.0, -2.0)),
                (5.0, 40.0, (-4.5, 6.0)), (8.0, -3.0, (0.3, 0.3)), (60.0, 0.0, (3.0, -2.0)), (500.0, -500.0, (0.0, 0.0)), (500.0, 40.0, (3.0, -2.0))]


def sweep():
    k = 0
    for aa in SWEEP_AA:
        for mode in SWEEP_MODES:
            for hx, hy in SWEEP_HALF_EXTENTS:
                for rx, ry in SWEEP_RADII:
                    for factor, spread, off in SWEEP_PARAMS:
                        ox, oy = CU.ORIGINS[k % len(CU.ORIGINS)]
                        k += 1
                        w, h = 2.0 * hx, 2.0 * hy
                        rect, shape, push = (ox, oy, w, h), (0.0, 0.0), 0
                        if mode == 3:
                            push = k % 2
                        if mode == 7:  # the padded quad around the shape (fdh_frontend.cpp: drop_shadows)
                            pad = max(float(CU.CS.nim_round(spread) + CU.CS.nim_round(1.5 * factor)), 0.0)
                            rect, shape = (ox, oy, w + 2 * pad, h + 2 * pad), (w, h)
                        if mode == 9:
                            shape = off
                        yield aa, (rect, rx, (ry if ry is not None else rx), mode, factor, spread, shape, push)


def test_core_union_is_saturated_on_the_hostile_sweep():
    L = CU._lib()
    n_cases = n_rects = 0
    for aa, case in sweep():
        rect, rx, ry, mode, factor, spread, shape, push = case
        out, n = CU.I12(), C.c_int()
        assert L.fdh_saturated_core_union(CU.F4(*rect), CU.F4(*rx), CU.F4(*ry), mode, factor, spread, CU.F2(*shape), aa, push, out, C.byref(n)) == 0
        rec = CU.CS.Rec(rect, rx, ry, mode, factor, spread, shape, aa, bool(push))
        n_cases += 1
        for k in range(3):
            x0, y0, x1, y1 = out[4 * k:4 * k + 4]
            if not (x1 > x0 and y1 > y0) or (x1 - x0) * (y1 - y0) > 4 << 20:
                continue
            assert x0 >= rec.ox and y0 >= rec.oy and x1 <= rec.ox + rec.w_px and y1 <= rec.oy + rec.h_px, (aa, case, k, tuple(out))
            bad = CU.saturated(rec, x0, y0, x1, y1)
            assert bad == 0, (aa, case, k, tuple(out), bad)
            n_rects += 1
    assert n_cases == 9000
    assert n_rects > n_cases // 2  # the sweep does reach the rule
