"""Every blur kernel held to an exact float64 filter on noise (tests/blur_ref.py).

A blur pass is a fixed FIR whose result is rounded to RGBA8, so a float64 evaluation gives the one correct byte wherever the exact sum
lies further than the kernel's float32 accumulation error (eps, derived from the number of products of an output) from a rounding tie.
On noise a dropped tap or a window one texel off moves most bytes, so the comparison is sharp where the suite's scene tests (UI content,
"1 LSB on 0.5 % of the frame") are not.  The cases -- shapes, radii, sources -- are in tests/blur_exact_child.py; one child process per
route renders them (the children set their own FDH_FORCE_BLUR_PATH and FDH_BLUR_FUSED, whatever tools/suite_off_defaults.sh or the caller
has exported), the reference runs here.  Two-pass routes: the horizontal output (debug_read_surface(1)) against fir(source), the final
output against fir of the device's OWN horizontal output -- each kernel on its own.  One-kernel routes (k_blur_small, k_blur_fx) keep no
intermediate: they are held by bit-for-bit equality with the two-pass route of the same sums.  Every final frame also lies within 1 LSB of
the oracle's frame of the same calls, and equals its source outside the node.  The counts are printed (profiles/blur_exact.txt)."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import blur_exact_child as BC
import blur_ref as BR
from conftest import diff_stats

pytestmark = pytest.mark.gpu
ORACLE_ROW = "frame vs the oracle's"
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _reach(radius):
    return BR.lib_taps(radius)[0]


_children = {}  # route -> what its child rendered, or the message of its failure: a route's child is started ONCE per session


def _rendered(route):
    """one child process (a fresh interpreter with the route's switches) renders all of the route's cases.  A child that faulted, failed
    or ran into its time limit ends the session: nothing more is started on the GPU, and the same child is never started again."""
    if route not in _children:
        env = {k: v for k, v in os.environ.items() if k not in BC.REMOVED_ENV}
        env.update(BC.ROUTES[route][0])
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, route + ".npz")
            try:
                r = subprocess.run([sys.executable, os.path.join(HERE, "blur_exact_child.py"), route, path], env=env, capture_output=True, text=True, timeout=300)
                failure = None if r.returncode == 0 else f"blur_exact_child.py {route} ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
            except subprocess.TimeoutExpired as e:  # (subprocess.run has killed the child)
                failure = f"blur_exact_child.py {route} did not end within {e.timeout:g} s and was killed"
            if failure is None:
                with np.load(path) as z:
                    _children[route] = {k: z[k] for k in z.files}
            else:
                _children[route] = failure
    if isinstance(_children[route], str):
        pytest.exit(_children[route], returncode=1)
    return _children[route]


@functools.lru_cache(maxsize=None)
def _cases(route):
    return {c.name: c for c in BC.cases(route, _reach)}


def _shapes(route):
    seen = []
    for c in BC.cases(route, _reach):
        if c.shape not in seen:
            seen.append(c.shape)
    return seen


@functools.lru_cache(maxsize=None)
def _weights(radius, matrix_pipe):
    """-> reach, ((horizontal weights, products per output), (vertical ...)): the float taps for the VALU kernels, the f16 fragments'
    effective weights and 16 * k_steps products for the matrix-pipe ones"""
    if matrix_pipe:
        rh, nkh, wh = BR.mx_taps(radius, False)
        rv, nkv, wv = BR.mx_taps(radius, True)
        assert rh == rv
        return rh, ((wh, 16 * nkh), (wv, 16 * nkv))
    reach, dense = BR.taps(radius)
    assert reach == _reach(radius)
    w = dense.astype(np.float64)
    return reach, ((w, 2 * reach + 1), (w, 2 * reach + 1))


_oracle_state = {}


def _oracle_frame(c):
    """the oracle's frame of the case's calls (an oracle per image, so that each image sits at the same place of its atlas)"""
    from oracle import oracle as O

    key = BC.image_key(c)
    if key not in _oracle_state:
        o = O.Oracle(atlas_size=2048, threads=8)
        o.put_image(key, BR.noise(c.w, c.h, BC.image_seed(c), c.kind))
        _oracle_state[key] = (o, {})
    o, frames = _oracle_state[key]
    fk = (c.clip, c.rect, c.radius)  # (stripes and routes are the same calls)
    if fk not in frames:
        o.W, o.H = c.w, c.h
        o.replay(BC.calls(c, True))
        frames[fk] = o.read_pixels()
    return frames[fk]


def _geometry(c, reach):
    """the node's box in the frame, the rows its final pass produces (a stripe cuts them) and the rows the horizontal pass produces"""
    x, y, w, h = c.rect
    x0, y0, x1, y1 = max(0, x), max(0, y), min(c.w, x + w), min(c.h, y + h)
    s0, s1 = c.stripe if c.stripe else (0, c.h)
    vy0, vy1 = max(y0, s0), min(y1, s1)
    node = np.zeros((c.h, c.w), dtype=bool)
    node[vy0:vy1, x0:x1] = True
    hrows = np.zeros((c.h, c.w), dtype=bool)
    hrows[max(0, vy0 - reach):min(c.h, vy1 + reach), x0:x1] = True
    rows = np.zeros((c.h, c.w), dtype=bool)
    rows[s0:s1] = True
    return (x0, y0, x1, y1, vy0, vy1), node, hrows, rows


def _source(data, c):
    src = data[f"src|{c.w}x{c.h}-{c.kind}{'-clip' if c.clip else ''}"]
    if c.kind != "premul":  # the opaque image drawn 1:1 REPLACES the frame: the source is the upload
        assert np.array_equal(src, BR.noise(c.w, c.h, BC.image_seed(c), c.kind)), (c.name, "the source frame is not the uploaded image")
    return src


def _final(route, data, c):
    """the case's raw vertical-filter output: the blurred snapshot where the route writes one (a node under a clip, k_blur_small), else the
    frame itself -- an opaque snapshot under full coverage replaces the surface"""
    return data[c.name + ("|snap" if c.clip or route == "small" else "|frame")]


def _common_checks(route, data, c, node, rows, table):
    src, frame = _source(data, c), data[c.name + "|frame"]
    outside = rows & ~node
    assert np.array_equal(frame[outside], src[outside]), (route, c.name, "pixels outside the node differ from the source", int((frame[outside] != src[outside]).any(axis=1).sum()))
    want = _oracle_frame(c)
    r3 = np.broadcast_to(rows[:, :, None], frame.shape)
    mx, n0, n1 = diff_stats(np.where(r3, frame, 0), np.where(r3, want, 0))
    assert mx <= 1, (route, c.name, "vs oracle", mx, n0, n1)
    t = table.setdefault((ORACLE_ROW, c.radius), [0, 0, 0])
    t[0] += int(rows.sum()); t[2] += n0


def _tally(table, kernel, radius, st):
    t = table.setdefault((kernel, radius), [0, 0, 0])
    t[0] += st["n"]; t[1] += st["excused"]; t[2] += st["differ"]


def _print_table(title, table, capsys):
    with capsys.disabled():
        print(f"\n  blur-exact {title}")
        for (kernel, radius), (n, exc, dif) in sorted(table.items(), key=lambda kv: (kv[0][0], kv[0][1])):
            if kernel == ORACLE_ROW:
                print(f"  blur-exact   {kernel:44s} r={radius:<4g} pixels {n:9d}  differing by 1 LSB {dif:6d}")
            elif " == " in kernel:
                print(f"  blur-exact   {kernel:44s} r={radius:<4g} values {n:9d}  all equal")
            else:
                print(f"  blur-exact   {kernel:44s} r={radius:<4g} values {n:9d}  excused {exc:6d} ({exc / max(n, 1):.3%})  not rint(exact) {dif:6d}")


def _kernel_names(route, c, geo, reach):
    x0, y0, x1, y1, vy0, vy1 = geo
    if route == "valu2":
        return "k_blur_h<2>", "k_blur_v<2,4>"
    if route == "valu8":
        return f"k_blur_h<{BC.pick_nout(x1 - x0, 64, reach)}>", f"k_blur_v<{BC.pick_nout(vy1 - vy0, 4, reach)},4>"
    form = "rgba" if c.kind == "premul" else "opaque"
    nkh, nkv = (32 + 2 * reach + 3 + 15) // 16, (32 + 2 * reach + 15) // 16
    return f"k_blur_mx<{nkh},H,{form}>", f"k_blur_mx<{nkv},V,{form}>"


def _check_two_pass(route, data, c, table, evidence=None):
    """horizontal output against fir(source); final output against fir of the device's own horizontal output"""
    matrix_pipe = route in ("mx", "native")
    reach, ((wh, nh), (wv, nv)) = _weights(c.radius, matrix_pipe)
    geo, node, hrows, rows = _geometry(c, reach)
    ms = data[c.name + "|ms"]
    assert ms[5] == 1 and ms[0] == 0 and ms[1] > 0 and ms[2] > 0, (route, c.name, "the frame did not take a two-pass route", ms.tolist())
    kh, kv = _kernel_names(route, c, geo, reach)
    src, hdev = _source(data, c), data[c.name + "|h"]
    st = {}
    BR.check_pass(hdev, BR.fir(src, wh, reach, 1), BR.eps_for(nh), hrows, label=f"{route} {c.name} {kh}", source=src, axis=1, reach=reach, stats=st)
    if evidence is not None and matrix_pipe and c.kind != "checker":  # bytes that the float taps (what a VALU pass multiplies) would not give
        as_valu = BR.to_u8(BR.fir(src, BR.taps(c.radius)[1].astype(np.float64), reach, 1))
        evidence["not_the_float_taps"] = evidence.get("not_the_float_taps", 0) + int(((hdev != as_valu) & hrows[:, :, None]).sum())
    tag = " on the checkerboard" if c.kind == "checker" else ""
    _tally(table, kh + tag, c.radius, st)
    if c.clip or c.kind != "premul":  # (a translucent snapshot composited by the pass itself is a blend: held by the oracle bar, and k_blur_fx's partner)
        hin = np.where(np.broadcast_to(hrows[:, :, None], hdev.shape), hdev, 0)
        # The 2 % cap on excused values is a statement about noise, whose sums have uniform fractional parts.  The checkerboard's horizontal
        # output is two bytes a, b alternating (a + b = 255 or so), so every vertical sum is b + (a - b) x (the weights of every other tap,
        # which sum to a half): with a - b odd it SITS on a tie by construction (radii 3 and 18: 54 - 70 % of the values).  There, and only
        # there, "floor or ceil" is all that can be asked; the horizontal pass of the checkerboard keeps the cap.
        cap = 1.0 if c.kind == "checker" else BR.EXCUSED_CAP
        BR.check_pass(_final(route, data, c), BR.fir(hin, wv, reach, 0), BR.eps_for(nv), node, label=f"{route} {c.name} {kv}", source=hin, axis=0, reach=reach, stats=st, cap=cap)
        _tally(table, kv + tag, c.radius, st)
    _common_checks(route, data, c, node, rows, table)
    return node


def _check_stripe_rows(route, data, c, node):
    if c.stripe:  # the stripe's rows equal the full frame's rows bit for bit
        full = c.name.replace("stripe-", "full-", 1)
        for what in ("|frame", "|snap") if (c.clip or route == "small") else ("|frame",):
            a, b = data[c.name + what], data[full + what]
            assert np.array_equal(a[node], b[node]), (route, c.name, what, "the stripe's rows differ from the full frame's")


TWO_PASS = [(r, s) for r in ("valu2", "valu8", "mx") for s in ("full", "fullodd", "tiny", "stripe", "inner", "cornerA", "cornerB", "tinynode", "col", "row", "nout")
            if not (s == "fullodd" and r == "mx") and not (s == "nout" and r != "valu8")]


@pytest.mark.parametrize("route,shape", TWO_PASS)
def test_two_pass_kernels_are_exact(route, shape, capsys):
    """k_blur_h<2|8|10|12>, k_blur_v<2|8|10|12, 4> and k_blur_mx (horizontal and vertical, three- and four-channel forms): each OBSERVED
    DIRECTLY -- the horizontal pass through debug_read_surface(1), the vertical one through the blurred snapshot (a node under a clip) or
    the frame (an opaque snapshot under full coverage replaces the surface) -- and held to the float64 filter by check_pass, with eps from
    the reach (VALU) or the k-steps (matrix pipe) of fdh_blur_weight_fragments.  frame_stats must show two blur passes and no fused kernel.
    frame_stats cannot tell a matrix-pipe pass from a VALU one, and the kernel names in the table are worked out here, not reported by the
    library.  That the mx route ran k_blur_mx is shown by its bytes: they are held to the f16 weights of the fragments, which a VALU pass
    (float taps) does not reproduce on noise -- and on the large shapes some bytes must differ from what the float taps give."""
    assert shape in _shapes(route)
    data, table, evidence = _rendered(route), {}, {}
    for c in _cases(route).values():
        if c.shape == shape:
            node = _check_two_pass(route, data, c, table, evidence)
            _check_stripe_rows(route, data, c, node)
    if route == "mx" and shape in ("full", "inner", "stripe"):
        assert evidence["not_the_float_taps"] > 0, "every byte of the mx route is what the float taps give: did a VALU pass run?"
    _print_table(f"route {route} ({BC.ROUTES[route][2]}), shape {shape}", table, capsys)


@pytest.mark.parametrize("route,partner,shape", [("small", "valu2", s) for s in ("full", "fullodd", "tiny", "stripe", "inner", "cornerA", "cornerB", "tinynode", "col", "row")] +
                         [("fx", "mx", s) for s in ("full", "tiny", "stripe")])
def test_one_kernel_routes_equal_their_two_pass_partner(route, partner, shape, capsys):
    """k_blur_small and k_blur_fx keep no intermediate in memory: each is TIED BIT FOR BIT to the two-pass route of the same sums on the same
    noise source -- k_blur_h<2> / k_blur_v<2,4> for k_blur_small (its snapshot, debug_read_surface(2)), the k_blur_mx pair for k_blur_fx
    (the frame it composites into) -- whose outputs test_two_pass_kernels_are_exact observes directly.  For the translucent source the tie
    of k_blur_fx takes a second step: its partner is the mx route's COMPOSITED frame (no clip), a blend that is held to the oracle's 1 LSB
    and not to the filter; the four-channel vertical k_blur_mx that made it is observed directly in the clip cases of the same image and
    radius (debug_read_surface(2)), and its horizontal pass in both.  frame_stats must show the one-kernel route: ms_blur_fused for
    k_blur_fx; a vertical span and no horizontal one for k_blur_small."""
    assert shape in _shapes(route)
    data, pdata, table = _rendered(route), _rendered(partner), {}
    n_cases = 0
    for c in _cases(route).values():
        if c.shape != shape:
            continue
        assert c.name in _cases(partner), (c.name, "has no partner case")
        reach = _reach(c.radius)
        geo, node, hrows, rows = _geometry(c, reach)
        ms = data[c.name + "|ms"]
        if route == "fx":
            assert ms[5] == 1 and ms[0] > 0 and ms[1] == 0, (c.name, "the frame did not take k_blur_fx", ms.tolist())
        else:
            assert ms[5] == 1 and ms[0] == 0 and ms[1] == 0 and ms[2] > 0, (c.name, "the frame did not take k_blur_small", ms.tolist())
        assert np.array_equal(_source(data, c), _source(pdata, c))
        a, b = _final(route, data, c), _final(partner, pdata, c)
        differ = int((a[node] != b[node]).any(axis=1).sum())
        assert differ == 0, (route, c.name, f"{differ} pixels differ from the {partner} route's", np.argwhere((a != b).any(axis=2) & node)[:4].tolist())
        if route == "fx" or c.kind != "premul":  # the frames too
            assert np.array_equal(data[c.name + "|frame"][rows], pdata[c.name + "|frame"][rows]), (route, c.name, "frames differ")
        t = table.setdefault((f"{'k_blur_fx' if route == 'fx' else 'k_blur_small'} == {partner} route, {c.kind}", c.radius), [0, 0, 0])
        t[0] += int(node.sum()) * 4
        _common_checks(route, data, c, node, rows, table)
        _check_stripe_rows(route, data, c, node)
        n_cases += 1
    assert n_cases > 0
    _print_table(f"route {route} ({BC.ROUTES[route][2]}) tied bit for bit to route {partner}, shape {shape}", table, capsys)


def test_the_matrix_pipe_taken_natively_is_exact(capsys):
    """1024 x 384, the smallest frame that is not "small" to blur_small, no FDH_FORCE_BLUR_PATH: set_blur_route(0) runs the k_blur_mx pair,
    OBSERVED DIRECTLY as in test_two_pass_kernels_are_exact; set_blur_route(1) runs k_blur_fx (radii whose filter it is built for), TIED BIT
    FOR BIT to the pair's frame (the composited frame: for the translucent source see test_one_kernel_routes_equal_their_two_pass_partner).
    That the pair is the matrix pipe's and not a quiet VALU fallback is shown as in test_two_pass_kernels_are_exact: by its bytes."""
    data, table, evidence = _rendered("native"), {}, {}
    by_name = _cases("native")
    for c in by_name.values():
        reach = _reach(c.radius)
        if c.blur_route == 0 or not BC.fused_supported(reach):
            _check_two_pass("native", data, c, table, evidence)
            continue
        geo, node, hrows, rows = _geometry(c, reach)
        ms = data[c.name + "|ms"]
        assert ms[5] == 1 and ms[0] > 0 and ms[1] == 0, (c.name, "the frame did not take k_blur_fx", ms.tolist())
        partner = c.name.replace("-route1-", "-route0-")
        assert np.array_equal(data[c.name + "|frame"], data[partner + "|frame"]), (c.name, "k_blur_fx differs from the k_blur_mx pair")
        table.setdefault((f"k_blur_fx == k_blur_mx pair, {c.kind}", c.radius), [0, 0, 0])[0] += int(node.sum()) * 4
        _common_checks("native", data, c, node, rows, table)
    assert evidence["not_the_float_taps"] > 0, "every byte of the two-pass frames is what the float taps give: did a VALU pass run?"
    _print_table("native 1024 x 384", table, capsys)
