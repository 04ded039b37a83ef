"""Host logic, no GPU: the float64 blur reference of tests/blur_ref.py against the library's own taps and against the oracle, and the
comparator (check_pass) against mutants of the reference's own output -- the kind of error a rewritten blur kernel makes (a tap dropped,
a window one texel off, an edge not clamped, an intermediate not rounded, two channels swapped).  tests/test_blur_exact.py holds the
kernels with the same comparator; this file shows that it has teeth and that its excuse for rounding ties stays small."""
import numpy as np
import pytest

import blur_exact_child as BC
import blur_ref as BR
from conftest import diff_stats, load_png

RADII = [0.8, 1, 3, 6.5, 9, 12, 18, 24, 30, 40, 50, 58, 63.5, 64, 100]
MUTANT_RADII = [6.5, 18, 64]
W, H = 264, 200


@pytest.fixture(scope="module")
def src():
    return BR.noise(W, H, 20261, "premul")


@pytest.fixture(scope="module")
def passes(src):
    """radius -> (reach, weights, exact horizontal sums, its bytes, exact vertical sums of those bytes): computed once, never modified"""
    out = {}
    for radius in MUTANT_RADII:
        reach, dense = BR.taps(radius)
        w = dense.astype(np.float64)
        hx = BR.fir(src, w, reach, 1)
        h8 = BR.to_u8(hx)
        vx = BR.fir(h8, w, reach, 0)
        for a in (hx, h8, vx):
            a.setflags(write=False)
        out[radius] = (reach, w, hx, h8, vx)
    return out


@pytest.mark.parametrize("radius", RADII)
def test_taps_equal_the_librarys_element_for_element(radius):
    """blur_ref.taps restates make_taps in float32; the library's dense array (fdh_blur_weight_fragments) must be the same floats, and
    the matrix-pipe weights read off its f16 fragments must sum to 1 and stay within an f16 step of them."""
    reach, dense = BR.taps(radius)
    for vertical in (False, True):
        r, nk, lib_dense, _ = BR.lib_taps(radius, vertical)
        assert r == reach, (radius, reach, r)
        assert nk == (32 + 2 * reach + (0 if vertical else 3) + 15) // 16
        assert lib_dense.shape == dense.shape and np.array_equal(lib_dense.view(np.uint32), dense.view(np.uint32)), (radius, np.abs(lib_dense - dense).max())
        r2, nk2, mw = BR.mx_taps(radius, vertical)
        assert (r2, nk2) == (reach, nk) and abs(mw.sum() - 1.0) < 1e-6
        # (half an f16 step of its own rounding + the error carried over from the tap before it, at most half a step of the centre tap's)
        assert np.abs(mw - dense).max() <= 2.0 ** -10 * dense.max(), (radius, np.abs(mw - dense).max())
    assert reach <= 66 and dense[0] != 0.0 and dense[-1] != 0.0
    if radius >= 64:
        assert np.array_equal(dense, BR.taps(64)[1])  # the radius clamp


@pytest.mark.parametrize("radius", [0.8, 6.5, 18, 64])
@pytest.mark.parametrize("content", ["blur_src", "noise"])
def test_two_reference_passes_match_the_oracle(radius, content, src):
    """fir, rint, fir, rint in float64 against the oracle's float32 blur (oracle.blur_image): the suite's usual bar, at most 1 LSB and at
    most 0.5 % of the pixels."""
    from oracle import oracle as O

    img = load_png("blur_src.png") if content == "blur_src" else src
    reach, dense = BR.taps(radius)
    w = dense.astype(np.float64)
    got = BR.to_u8(BR.fir(BR.to_u8(BR.fir(img, w, reach, 1)), w, reach, 0))
    mx, n0, n1 = diff_stats(got, O.blur_image(img, radius))
    assert mx <= 1 and n0 <= 0.005 * img.shape[0] * img.shape[1], (radius, content, mx, n0, n1)


def _eps(reach):
    return BR.eps_for(2 * reach + 1)


@pytest.mark.parametrize("radius", MUTANT_RADII)
def test_check_pass_accepts_the_reference_with_few_excused(radius, passes):
    """The condition behind the 2 % cap: on noise the fractional parts of the exact sums are uniform, so the share within eps of a tie is
    2 * eps -- for the VALU kernels' eps and for the widest matrix-pipe one (n = 16 * 11 products)."""
    reach, w, hx, h8, vx = passes[radius]
    v8 = BR.to_u8(vx)
    for eps in (_eps(reach), BR.eps_for(16 * 11)):
        for got, exact in ((h8, hx), (v8, vx)):
            st = {}
            share = BR.check_pass(got, exact, eps, stats=st)
            assert st["differ"] == 0 and share < BR.EXCUSED_CAP
            assert share < 2 * eps * 1.5 + 1e-4, (radius, eps, share)


def _rejected(got, exact, eps, **kw):
    try:
        BR.check_pass(got, exact, eps, **kw)
    except BR.PassMismatch as e:
        return str(e)
    return None


@pytest.mark.parametrize("radius", MUTANT_RADII)
@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("mutant", ["outer_taps_dropped", "window_shifted", "zero_padding", "channels_swapped"])
def test_check_pass_rejects_one_pass_mutants(radius, axis, mutant, passes, src):
    reach, w, hx, h8, vx = passes[radius]
    source, exact = (src, hx) if axis == 1 else (h8, vx)
    if mutant == "outer_taps_dropped":
        wm = w.copy()
        wm[0] = wm[-1] = 0.0
        got = BR.to_u8(BR.fir(source, wm, reach, axis))
    elif mutant == "window_shifted":
        n = source.shape[axis]
        got = BR.to_u8(BR.fir(np.take(source, np.clip(np.arange(n) + 1, 0, n - 1), axis=axis), w, reach, axis))
    elif mutant == "zero_padding":
        got = BR.to_u8(BR.fir(source, w, reach, axis, mode="constant"))
    else:
        got = np.ascontiguousarray(BR.to_u8(exact)[:, :, [1, 0, 2, 3]])
    msg = _rejected(got, exact, _eps(reach), label=mutant, source=source, axis=axis, reach=reach)
    assert msg is not None, (radius, axis, mutant, "accepted")
    assert "first at x=" in msg and "tap window" in msg, msg
    # (also with the widest eps any kernel is given)
    assert _rejected(got, exact, BR.eps_for(16 * 11)) is not None


@pytest.mark.parametrize("radius", MUTANT_RADII)
def test_check_pass_rejects_an_intermediate_that_was_not_rounded(radius, passes):
    """the vertical pass fed the horizontal sums as floats, not the RGBA8 texture the reference stores between the passes"""
    reach, w, hx, h8, vx = passes[radius]
    got = BR.to_u8(BR.fir(hx, w, reach, 0))
    assert _rejected(got, vx, _eps(reach)) is not None
    assert _rejected(got, vx, BR.eps_for(16 * 11)) is not None


def test_check_pass_masks_and_excuses():
    """the mask limits what is looked at; a value within eps of a tie may be floor or ceil and nothing else"""
    exact = np.full((4, 4, 4), 10.25)
    exact[1, 1, 2] = 20.5 + 1e-4
    got = BR.to_u8(exact)
    assert BR.check_pass(got, exact, 1e-3, cap=1.0) == 1 / 64
    got[1, 1, 2] = 20
    assert BR.check_pass(got, exact, 1e-3, cap=1.0) == 1 / 64
    assert _rejected(got, exact, 1e-5) is not None
    got[1, 1, 2] = 22
    assert _rejected(got, exact, 1e-3, cap=1.0) is not None
    where = np.ones((4, 4), dtype=bool)
    where[1, 1] = False
    assert BR.check_pass(got, exact, 1e-3, where) == 0.0
    assert _rejected(BR.to_u8(exact), exact, 1e-3, cap=0.01) is not None  # 1 of 64 excused: over a 1 % cap


def test_the_radii_reach_every_k_step_count_a_radius_can_select():
    """Host logic: the radii of shapes 1 and 2 select every NK a radius in (0.5, 64] can -- horizontal 4 - 11, vertical 3 - 10 -- and every
    fused pair k_blur_fx is built for but (3, 3).  (NK = 3 horizontal, NK = 11 vertical, FDH_FX(3, 3) and case 16 of the NOUT switches are
    instantiations no radius reaches.)"""
    nkh, nkv, fused = set(), set(), set()
    for r in BC.RADII_ALL:
        reach, h, _, _ = BR.lib_taps(r, False)
        _, v, _, _ = BR.lib_taps(r, True)
        nkh.add(h); nkv.add(v)
        if BC.fused_supported(reach):
            fused.add((h, v))
    assert nkh == set(range(4, 12)) and nkv == set(range(3, 11)), (sorted(nkh), sorted(nkv))
    assert fused == {(4, 3), (4, 4), (5, 4), (5, 5), (6, 5), (6, 6)}, sorted(fused)
    every = np.arange(0.55, 64.01, 0.05)
    assert {BR.taps(r)[0] for r in every} <= set(range(1, 65))
    reaches = {BR.taps(r)[0] for r in every}
    assert {(32 + 2 * x + 18) // 16 for x in reaches} == nkh and {(32 + 2 * x + 15) // 16 for x in reaches} == nkv


def test_the_nout_cases_select_every_build():
    """Host logic: blur_pick_nout's cost model restated (blur_exact_child.pick_nout): the node widths 300 / 600 / 700 select the 8 / 10 / 12
    outputs-per-thread build of k_blur_h and the heights 32 / 40 / 48 those of k_blur_v, at every radius of the cases."""
    for r in BC.RADII_FEW:
        reach = BR.lib_taps(r)[0]
        assert [BC.pick_nout(w, 64, reach) for w in BC.NOUT_WIDTHS] == [8, 10, 12], r
        assert [BC.pick_nout(h, 4, reach) for h in BC.NOUT_HEIGHTS] == [8, 10, 12], r
    names = [c.name for c in BC.cases("valu8", lambda r: BR.lib_taps(r)[0]) if c.shape == "nout"]
    assert {n.split("-")[1] for n in names} == {f"h{a}v{b}" for a in (8, 10, 12) for b in (8, 10, 12)}
