"""Host-side proofs behind the opaque-surface kernels (Context::decide_opaque, k_composite_tiles<4 | 32>, the kOpaque forms of
k_blur_mx / k_blur_fx).  No GPU.

1. The blend keeps an opaque texel opaque: A' = rint(fma(A, 1 - sa, 255 sa)) with A = 255 is 255 for EVERY float sa in
   [-2^-10, 1 + 2^-10] -- about 2.05 G values, tried one by one by a small C program (IEEE single, no contraction: the operations the
   kernels run).  The range is wider than what shading produces (coverage x colour alpha x masks, each in [0, 1]).
2. The blur keeps it: the f16 weight fragments the library builds for the matrix-pipe passes sum, per output, so close to the scale
   (1024) that an all-255 plane filters to a value inside (254.5, 255.5), i.e. rounds to 255 -- radii 1, 5, 18, 64, both passes."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

BLEND_C = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t as_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
/* every float whose bit pattern lies in [lo, hi]: how many give something else than 255 */
static unsigned long long sweep(uint32_t lo, uint32_t hi, unsigned long long* tried) {
  unsigned long long bad = 0;
  const long long n = (long long)hi - (long long)lo + 1;
#pragma omp parallel for reduction(+ : bad) schedule(static)
  for (long long i = 0; i < n; i++) {
    const float sa = as_float(lo + (uint32_t)i);
    const float ia = 1.0f - sa, A = 255.0f * sa;       /* blend(): fdh_device.h */
    const float out = rintf(fmaf(255.0f, ia, A));      /* round to nearest even, like v_rndne_f32 */
    bad += out != 255.0f;
  }
  *tried += (unsigned long long)n;
  return bad;
}
int main(void) {
  const float eps = 0.0009765625f; /* 2^-10 */
  unsigned long long tried = 0, bad = 0;
  bad += sweep(as_bits(0.0f), as_bits(1.0f + eps), &tried);    /* +0 .. 1 + 2^-10: the positive floats in bit order */
  bad += sweep(as_bits(-0.0f), as_bits(-eps), &tried);         /* -0 .. -2^-10 */
  printf("%llu %llu\n", tried, bad);
  return bad != 0;
}
"""


def _compile(src_path, exe_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on this machine (the suite's other host tests need one too)")
    base = [cc, "-O2", "-ffp-contract=off", src_path, "-o", exe_path, "-lm"]
    # fastest first: hardware FMA / rounding instructions and OpenMP; every form computes the same IEEE operations
    for extra in (["-march=native", "-fopenmp"], ["-fopenmp"], ["-march=native"], []):
        r = subprocess.run(base[:3] + extra + base[3:], capture_output=True, text=True)
        if r.returncode == 0:
            return
    pytest.fail("could not compile the blend sweep: " + r.stderr[-400:])


def test_the_blend_keeps_an_opaque_texel_opaque_for_every_source_alpha():
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "blend_sweep.c"), os.path.join(td, "blend_sweep")
        with open(src, "w") as f:
            f.write(BLEND_C)
        _compile(src, exe)
        r = subprocess.run([exe], capture_output=True, text=True)
    tried, bad = (int(v) for v in r.stdout.split())
    # +0 .. 1 + 2^-10 is 0x3F802000 + 1 patterns, -0 .. -2^-10 is 0x3A800000 + 1
    assert tried == (0x3F802000 + 1) + (0x3A800000 + 1), tried
    assert bad == 0 and r.returncode == 0, f"{bad} of {tried} source alphas move an opaque texel's alpha off 255"


def _krow(g, t, vertical):
    return (t & 3) + 8 * (t >> 2) + 4 * g if vertical else 8 * g + t


@pytest.mark.parametrize("radius", [1.0, 5.0, 18.0, 64.0])
def test_the_blur_weight_fragments_keep_an_opaque_plane_opaque(radius):
    from figdraw_amd import context as ctx_mod

    L = ctx_mod.load()
    L.fdh_blur_weight_fragments.argtypes = [C.c_float, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    for vertical in (0, 1):
        dense = (C.c_float * 160)()
        bits = (C.c_uint16 * (11 * 2 * 64 * 8))()
        reach, nk = C.c_int(), C.c_int()
        assert L.fdh_blur_weight_fragments(radius, vertical, dense, bits, C.byref(reach), C.byref(nk)) == 0
        n = nk.value
        frag = np.frombuffer(bits, dtype=np.float16)[: n * 2 * 64 * 8].astype(np.float64).reshape(n, 2, 64, 8)
        # what output j of a block meets: every element of its two lanes (j, g = 0, 1) over all k-steps, both halves -- a texel
        # outside the band carries weight 0, so the sum over the whole window is the sum the kernels form
        per_output = np.zeros(32)
        rows = set()
        for m in range(n):
            for lane in range(64):
                per_output[lane & 31] += frag[m, :, lane, :].sum()
                if lane & 31 == 0:
                    rows.update(16 * m + _krow(lane >> 5, t, vertical) for t in range(8))
        assert rows == set(range(16 * n))  # (every window texel exactly once per output)
        out = 255.0 * per_output / 1024.0  # an all-255 plane: texel 255 at every tap
        assert (out > 254.5).all() and (out < 255.5).all(), (radius, vertical, out.min(), out.max())
        # ... and with the margin the library asks of itself (kMxOpaqueSumBound, fdh_types.h): |sum - 1024| <= 1
        assert np.abs(per_output - 1024.0).max() <= 1.0, (radius, vertical, np.abs(per_output - 1024.0).max())
