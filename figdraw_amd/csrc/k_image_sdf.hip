// k_image_sdf.hip -- distance fields from coverage images: fdh_put_image_sdf and fdh_put_image_sdf_of (the specification is the comment of
// include_glyphs/figdraw_hip_image_sdf.h; this file is its rule).  One workgroup owns a 16 x 16 tile of the output, one lane a texel.  The
// coverage of the tile and of a halo as wide as the search window reaches is staged into LDS once, as the floats e = byte / 255 - 0.5 the
// rule adds, so a candidate costs one LDS read, an add, a compare and a min, and nothing in the walk depends on a load but the min.  Every
// lane of a wave walks the same Chebyshev ring of candidates at the same time -- the offsets are wave-uniform -- and the wave leaves the
// walk when no lane's best term can still be beaten: ring k holds terms of k - 0.5 at the least.  Two shortcuts ahead of the walk: a
// staged region of zeros makes a tile of zeros, a staged region of 255 that lies inside the source a tile of 255.  Neither they nor the
// exit change a byte; a build with FDH_IMAGE_SDF_NO_CULL=1 has none of the three and shows it (tests/test_image_sdf_host.py,
// tools/image_sdf_bench.py).
#include "fdh_device.h"

namespace fdh {

#ifndef FDH_IMAGE_SDF_NO_CULL
#define FDH_IMAGE_SDF_NO_CULL 0  // the second build of tests and tools/image_sdf_bench.py: every texel walks the whole window
#endif

// The two cross-lane operations of this file.  On the device a wave's ballot and the workgroup's voting barrier; a host build that runs
// the lanes of a workgroup one after the other brings its own (tests/image_sdf_emu/fdh_device.h).
#ifndef FDH_IMAGE_SDF_WAVE_ANY
#define FDH_IMAGE_SDF_WAVE_ANY(p) (__ballot(p) != 0)
#define FDH_IMAGE_SDF_GROUP_ANY(p) (__syncthreads_or(p) != 0)
#endif
// Six loaded words pinned in registers at one point: the loads behind them are issued before any is waited for.  (Left alone the
// compiler sinks each load into the branch that uses it, a round trip to memory at a time.)
#ifndef FDH_IMAGE_SDF_TOGETHER
#define FDH_IMAGE_SDF_TOGETHER(a, b, c, d, e, f) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f))
#endif

constexpr int kSdfTile = 16;  // the tile's side; the workgroup has kSdfTile^2 lanes

// how far the search looks along each axis for the range R (1 .. 64): floor(R / 2 + 0.5) + 1, at most 33.  A candidate farther than
// R / 2 + 0.5 from the texel has a term above R / 2, which only a saturated byte can come from.
__host__ __device__ inline int image_sdf_reach(int range) { return (range + 1) / 2 + 1; }
// the staged region's side and the dynamic LDS of a launch: at most 82 texels, 26 896 bytes
__host__ __device__ inline int image_sdf_side(int reach) { return kSdfTile + 2 * reach; }

// src: the source, sw x sh RGBA8 texels, `src_pitch` texels from row to row; byte `channel` of a texel is its coverage.  out: the field,
// (sw + 2 pad) x (sh + 2 pad) texels, rows packed, all four bytes of a texel the encoded distance.
__global__ __launch_bounds__(kSdfTile * kSdfTile) void k_image_sdf_generate(const uint32_t* __restrict__ src, int sw, int sh, int src_pitch, int channel, int pad, int reach,
                                                                            float range, uint32_t* __restrict__ out) {
#pragma clang fp contract(off)
  HIP_DYNAMIC_SHARED(float, e_at)  // side x side: e = c - 0.5 of every texel of the staged region
  const int ow = sw + 2 * pad, oh = sh + 2 * pad;
  const int lane = (int)threadIdx.x;
  const int side = image_sdf_side(reach);
  // the staged region's first texel, in source coordinates
  const int rx0 = (int)blockIdx.x * kSdfTile - pad - reach, ry0 = (int)blockIdx.y * kSdfTile - pad - reach;
  // ---- staging: 16 rows of the region at a time, a lane up to three texels of each of its two rows.  Every load has a valid address --
  // the texel's coordinates clamped into the source -- and what lies outside is replaced behind it: no branch around a load, and the
  // six go out together.
  int any_set = 0, any_clear = 0;
  const int tx = lane & 31, ty = lane >> 5;
  for (int ry = ty; ry < side; ry += 16) {
    uint32_t texel[2][3];
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int sy = ry0 + ry + 8 * i;
      const int cy = sy < 0 ? 0 : (sy >= sh ? sh - 1 : sy);
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int sx = rx0 + tx + 32 * j;
        const int cx = sx < 0 ? 0 : (sx >= sw ? sw - 1 : sx);
        texel[i][j] = src[(size_t)cy * src_pitch + cx];
      }
    }
    FDH_IMAGE_SDF_TOGETHER(texel[0][0], texel[0][1], texel[0][2], texel[1][0], texel[1][1], texel[1][2]);
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int sy = ry0 + ry + 8 * i;
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int rx = tx + 32 * j, sx = rx0 + rx;
        if (rx >= side || ry + 8 * i >= side) continue;
        const bool in_source = sy >= 0 && sy < sh && sx >= 0 && sx < sw;
        const uint32_t b = in_source ? (texel[i][j] >> (8 * channel)) & 255u : 0u;  // (the plane outside the source: coverage 0)
        e_at[(ry + 8 * i) * side + rx] = (float)b / 255.0f - 0.5f;
        any_set |= (int)(b != 0u);
        any_clear |= (int)(b != 255u);
      }
    }
  }
#if FDH_IMAGE_SDF_NO_CULL
  __syncthreads();
#else
  // (each of the two votes is a barrier as well: the staged values are visible behind the first)
  const bool some_set = FDH_IMAGE_SDF_GROUP_ANY(any_set), some_clear = FDH_IMAGE_SDF_GROUP_ANY(any_clear);
#endif
  // a wave owns an 8 x 8 quarter of the tile: its lanes' best terms are close to one another, and so are the rings at which they are done
  const int wave = lane >> 6, in_wave = lane & 63;
  const int lx = (wave & 1) * 8 + (in_wave & 7), ly = (wave >> 1) * 8 + (in_wave >> 3);
  const int x = (int)blockIdx.x * kSdfTile + lx, y = (int)blockIdx.y * kSdfTile + ly;
  const bool live = x < ow && y < oh;  // (a lane beyond the image walks with its wave -- every read stays inside the staged region -- and stores nothing)
#if !FDH_IMAGE_SDF_NO_CULL
  if (!some_set || !some_clear) {  // workgroup-uniform.  (All 255 with a part of the region outside the source cannot be: that part is 0.)
    if (live) out[(size_t)y * ow + x] = some_set ? 0xFFFFFFFFu : 0u;
    return;
  }
#endif
  const float* __restrict__ centre = e_at + (ly + reach) * side + (lx + reach);
  const bool inside = centre[0] >= 0.0f;  // 2 c_p >= 1: byte 128 and above
  // inside: the minimum of |p - q| + e_q over q with c_q < 1; outside: of |p - q| - e_q over q with c_q > 0.  Of the 256 values of e only
  // 255 / 255 - 0.5 is 0.5 and only 0 / 255 - 0.5 is -0.5: the candidate a rule bars is known by its e.
  const float sign = inside ? 1.0f : -1.0f, barred = inside ? 0.5f : -0.5f;
  float best = 3.0e38f;  // no candidate: saturated
  auto offer = [&](int dx, int dy, float apart) {  // apart = |p - q|
    const float e = centre[dy * side + dx];
    const float term = apart + sign * e;
    best = __builtin_fminf(best, e != barred ? term : 3.0e38f);
  };
  for (int k = 0; k <= reach; k++) {
#if !FDH_IMAGE_SDF_NO_CULL
    // ring k has terms of k - 0.5 at the least: a lane whose best is no larger is done, and so is the wave when all its lanes are
    if (!FDH_IMAGE_SDF_WAVE_ANY(live && best > (float)k - 0.5f)) break;  // wave-uniform
#endif
    if (k == 0) { offer(0, 0, 0.0f); continue; }
    for (int d = -k; d <= k; d++) {
      const float apart = __builtin_sqrtf((float)(d * d + k * k));  // (of an exact integer, and the same for the ring's four candidates at d)
      offer(d, -k, apart); offer(d, k, apart);                      // the ring's two rows
      if (d > -k && d < k) { offer(-k, d, apart); offer(k, d, apart); }  // and what is left of its two columns
    }
  }
  const float dist = inside ? best : -best;
  const float v = clamp01(0.5f + dist / range);
  const uint32_t byte = (uint32_t)__builtin_floorf(255.0f * v + 0.5f);
  if (live) out[(size_t)y * ow + x] = byte * 0x01010101u;
}

void launch_image_sdf_generate(hipStream_t s, const uint32_t* src, int sw, int sh, int src_pitch, int channel, int pad, int range, uint32_t* out) {
  const int ow = sw + 2 * pad, oh = sh + 2 * pad;
  if (sw <= 0 || sh <= 0 || range < 1 || range > 64) return;
  const int reach = image_sdf_reach(range), side = image_sdf_side(reach);
  FDH_LAUNCH(k_image_sdf_generate, dim3((ow + kSdfTile - 1) / kSdfTile, (oh + kSdfTile - 1) / kSdfTile), dim3(kSdfTile * kSdfTile), (size_t)side * side * sizeof(float), s, src, sw, sh,
             src_pitch, channel, pad, reach, (float)range, out);
}

}  // namespace fdh
