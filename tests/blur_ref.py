"""The backdrop blur as an exact filter: a float64 reference for ONE pass of the separable blur (glsl/blur.frag:11-32 as the merged FIR
of make_taps, glcontext.nim:1743-1786 for the RGBA8 intermediate) and the comparator that holds a kernel's bytes to it.

A pass is a fixed FIR over integer offsets whose result is rounded to RGBA8 (round to nearest even).  Evaluated in float64 it gives the
one correct byte everywhere except where the exact sum lies within the kernel's float32 accumulation error of a rounding tie: check_pass
demands that byte wherever the sum is further than `eps` from a tie and floor or ceil where it is nearer.  Plain numpy; used by
tests/test_blur_ref_host.py (no GPU) and tests/test_blur_exact.py (the kernels)."""
import ctypes as C
import math

import numpy as np

EXCUSED_CAP = 0.02  # share of values check_pass may excuse: on noise the fractional parts are uniform, so the reference alone excuses 2 * eps


def taps(radius):
    """make_taps (figdraw_amd/csrc/fdh_record.cpp) restated: radius clamp 64, sigma = max(radius / 2, 0.5), step = max(radius / 8, 1),
    17 bilinear taps merged over integer offsets, every operation in float32 in the library's order.  -> (reach, dense[2 reach + 1] float32)"""
    f = np.float32
    r = f(min(max(float(radius), 0.0), 64.0))
    sigma = max(f(0.5) * r, f(0.5))
    step = max(r / f(8.0), f(1.0))
    w, wsum = [], f(0.0)
    for i in range(-8, 9):
        x = f(i) * step
        arg = f(-0.5) * (x * x) / (sigma * sigma)
        w.append(f(math.exp(float(arg))))  # (expf of glibc is correctly rounded for these arguments: so is exp in double, rounded once)
        wsum = wsum + w[-1]
    inv = f(1.0) / max(wsum, f(1e-5))
    offs, coef = [], []

    def add(off, c):
        if c == 0.0:
            return
        if off in offs:
            k = offs.index(off)
            coef[k] = coef[k] + c
        else:
            offs.append(off)
            coef.append(c)

    for i in range(-8, 9):
        x = f(i) * step
        fl = f(math.floor(float(x)))
        a = x - fl
        add(int(fl), w[i + 8] * (f(1.0) - a) * inv)
        add(int(fl) + 1, w[i + 8] * a * inv)
    reach = max(abs(o) for o in offs)
    dense = np.zeros(2 * reach + 1, dtype=np.float32)
    for o, c in zip(offs, coef):
        dense[reach + o] = c
    return reach, dense


def _lib():
    from figdraw_amd import context as ctx_mod

    L = ctx_mod.load()
    L.fdh_blur_weight_fragments.argtypes = [C.c_float, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def lib_taps(radius, vertical=False):
    """what the library itself builds (fdh_blur_weight_fragments): (reach, k_steps, dense float32, fragments float64 [k_steps][2][64][8])"""
    dense = (C.c_float * 160)()
    bits = (C.c_uint16 * (11 * 2 * 64 * 8))()
    reach, nk = C.c_int(), C.c_int()
    rc = _lib().fdh_blur_weight_fragments(float(radius), int(bool(vertical)), dense, bits, C.byref(reach), C.byref(nk))
    assert rc == 0, ("fdh_blur_weight_fragments", radius, rc)
    r, n = reach.value, nk.value
    frag = np.frombuffer(bits, dtype=np.float16)[: n * 2 * 64 * 8].astype(np.float64).reshape(n, 2, 64, 8)
    return r, n, np.array(dense[: 2 * r + 1], dtype=np.float32), frag


def _krow(g, t, vertical):
    """row of a 16-texel k-step that element t of lane group g carries (mx_krow, figdraw_amd/csrc/fdh_types.h)"""
    return (t & 3) + 8 * (t >> 2) + 4 * g if vertical else 8 * g + t


def mx_taps(radius, vertical):
    """The effective weights of a matrix-pipe pass (k_blur_mx / k_blur_fx): the f16 weight fragments the library builds, read off at output
    0 of a block (lane j = 0: window texel 16 m + krow meets tap k = that - delta), both halves summed, at scale 2^-10.
    -> (reach, k_steps, weights[2 reach + 1] float64)"""
    r, n, _, frag = lib_taps(radius, vertical)
    delta = 0 if vertical else (-r) % 4
    out = np.zeros(2 * r + 1)
    for m in range(n):
        for g in range(2):
            for t in range(8):
                k = 16 * m + _krow(g, t, vertical) - delta
                if 0 <= k <= 2 * r:
                    out[k] = frag[m, 0, 32 * g, t] + frag[m, 1, 32 * g, t]
    return r, n, out / 1024.0


def fir(img, weights, reach, axis, mode="edge"):
    """One pass: out[p] = sum_k weights[k] * img[clamp(p + k - reach)] along `axis` (0: vertical, 1: horizontal) of an (h, w, c) array,
    clamp-to-edge at the frame's edges (glcontext.nim:214-215), float64 sums, NOT rounded."""
    img = np.asarray(img, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.float64)
    assert weights.shape == (2 * reach + 1,) and img.ndim == 3 and axis in (0, 1)
    n = img.shape[axis]
    # the pass as a matrix: row p holds, for every texel of the line, the sum of the taps that the clamp sends to it
    m = np.zeros((n, n))
    p = np.arange(n)
    for k in range(2 * reach + 1):
        q = p + k - reach
        if mode == "edge":
            np.add.at(m, (p, np.clip(q, 0, n - 1)), weights[k])
        elif mode == "constant":  # zero padding: what a kernel that does not clamp its taps computes (a mutant for the comparator's own test)
            ok = (q >= 0) & (q < n)
            np.add.at(m, (p[ok], q[ok]), weights[k])
        else:
            raise ValueError(mode)
    out = np.tensordot(m, img, axes=(1, axis))  # (p, other axis, channel)
    return out if axis == 0 else np.ascontiguousarray(out.transpose(1, 0, 2))


def to_u8(exact):
    """the byte a pass stores: round to nearest even (v_cvt_pk_u8_f32), saturated"""
    return np.clip(np.rint(exact), 0, 255).astype(np.uint8)


def eps_for(n_products):
    """how near a rounding tie an exact sum must lie before float32 accumulation may land on either side: n accumulated products, each add
    rounding a running sum of at most 255 by 2^-24 relative; the factor 2 covers an accumulation order or rounding inside an MFMA that is
    not round-to-nearest per add (and a multiply that is not fused into its add)"""
    return 2.0 * n_products * 2.0 ** -24 * 255.0


class PassMismatch(AssertionError):
    pass


def check_pass(got_u8, exact_f64, eps, where=None, label="", source=None, axis=None, reach=None, stats=None, cap=EXCUSED_CAP):
    """Every channel value of `got_u8` inside the boolean (h, w) mask `where` against the exact sums: further than eps from a rounding tie it
    must be rint(exact); nearer it is excused but must still be floor(exact) or ceil(exact).  Returns the excused share and fails if that
    exceeds `cap`.  A mismatch reports `label` (the kernel), the first wrong pixel and, given `source` / `axis` / `reach`, the source
    values of its tap window.  `stats`, a dict, receives n, excused and differ (values that are not rint(exact))."""
    got = np.asarray(got_u8)
    exact = np.asarray(exact_f64, dtype=np.float64)
    assert got.shape == exact.shape and got.dtype == np.uint8, (label, got.shape, exact.shape, got.dtype)
    if where is None:
        where = np.ones(got.shape[:2], dtype=bool)
    m = np.broadcast_to(np.asarray(where, dtype=bool)[:, :, None], got.shape)
    n = int(m.sum())
    assert n > 0, (label, "empty mask")
    ex = np.clip(exact, 0.0, 255.0)
    lo = np.floor(ex)
    near = np.abs(ex - lo - 0.5) < eps
    g = got.astype(np.float64)
    want = np.rint(ex)
    bad = m & np.where(near, (g != lo) & (g != np.ceil(ex)), g != want)
    excused = int((m & near).sum())
    differ = int((m & (g != want)).sum())
    if stats is not None:
        stats.update(n=n, excused=excused, differ=differ)
    if bad.any():
        y, x, c = (int(v[0]) for v in np.nonzero(bad))
        msg = f"{label}: {int(bad.sum())} of {n} values wrong; first at x={x} y={y} channel {c}: got {int(got[y, x, c])}, exact {exact[y, x, c]:.6f} (eps {eps:.2e})"
        if source is not None and axis is not None and reach is not None:
            src = np.asarray(source)
            idx = np.clip(np.arange(-reach, reach + 1) + (y if axis == 0 else x), 0, src.shape[axis] - 1)
            win = src[idx, x, c] if axis == 0 else src[y, idx, c]
            msg += f"; tap window ({'rows' if axis == 0 else 'columns'} {int(idx[0])}..{int(idx[-1])}, clamped): {win.tolist()}"
        raise PassMismatch(msg)
    share = excused / n
    if share > cap:
        raise PassMismatch(f"{label}: {share:.4%} of the values lie within eps = {eps:.2e} of a rounding tie -- more than the {cap:.0%} a comparison may excuse")
    return share


def noise(w, h, seed, kind="opaque"):
    """the sources of the exact tests, by recipe: 'opaque' white noise with alpha 255; 'premul' premultiplied noise with random alpha;
    'checker' the 1-pixel 0 / 255 checkerboard (opaque)"""
    rng = np.random.default_rng(seed)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 4, axis=2)
        img[:, :, 3] = 255
        return np.ascontiguousarray(img)
    img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    if kind == "opaque":
        img[:, :, 3] = 255
    elif kind == "premul":
        a = img[:, :, 3:4].astype(np.uint32)
        img[:, :, :3] = ((img[:, :, :3].astype(np.uint32) * a + 127) // 255).astype(np.uint8)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(img)
