// k_video_export.hip -- the rendered frame on its way out as NV12, P010 or BGRA8: fdh_read_video_frame (the specification is the comment
// of include_video/figdraw_hip_video_out.h; the parameter block is fdh_video_export.h's).  One launch per call.  A workgroup of 256 takes
// a tile of 128 x 16 texels of the rectangle, a lane a run of four texels by two rows: two 16-byte loads of the surface, the two luma
// runs as one 4-byte (NV12) or 8-byte (P010) store each, and the two chroma pairs under the run as one store of the same size -- a wave
// stores 128 contiguous luma bytes per row where it read 512.  BGRA8 is the same run with the bytes swapped, two 16-byte stores.  The
// FDH_VIDEO_CHROMA_LINEAR builds take the texel left of the run by one more 4-byte load per row (the neighbouring lane's lines: no LDS,
// no barrier, no cross-lane traffic).  Wide loads and stores only where the host found pointer and pitch aligned (Params::wide_*) and the
// run lies whole inside the row; element by element elsewhere.  Nothing is stored outside w x h samples, cw x ch pairs: the bytes
// between a row's end and the pitch stay.  No float arithmetic anywhere in this unit.
#include "fdh_device.h"
#include "fdh_video_export.h"

namespace fdh {
namespace ve = video_export;

namespace video_export {

struct Rgb { int r, g, b; };
__device__ __forceinline__ Rgb rgb_of(uint32_t t) { return Rgb{(int)(t & 255u), (int)((t >> 8) & 255u), (int)((t >> 16) & 255u)}; }
__device__ __forceinline__ Rgb operator+(Rgb a, Rgb b) { return Rgb{a.r + b.r, a.g + b.g, a.b + b.b}; }
// ---- the conversion, once.  int32 throughout; >> of a negative sum is an arithmetic shift (floor).
__device__ __forceinline__ int luma_of(const Params& P, uint32_t t) {
  const Rgb c = rgb_of(t);
  return P.yoff + ((P.ky[0] * c.r + P.ky[1] * c.g + P.ky[2] * c.b + 8192) >> 14);
}
// clamp(Coff + ((k . s + (N << 13)) >> (14 + log2 N)), 0, 2^b - 1) with kShift = 14 + log2 N, written as the clamp of the sum, Coff << kShift
// in it, in front of the shift, which is the same number (k_video_import.hip, shift_clamp, says why the clamp comes first).  The largest
// sum of absolute terms is 134 085 120 (the specification); Coff << kShift is at most 2^26: no sum reaches 2^31.
template <int kShift, int kBits>
__device__ __forceinline__ uint32_t chroma_of(const int32_t k[3], int coff, Rgb s) {
  const int sum = k[0] * s.r + k[1] * s.g + k[2] * s.b + (1 << (kShift - 1)) + coff * (1 << kShift);
  return (uint32_t)min(max(sum, 0), (1 << (kBits + kShift)) - 1) >> kShift;
}
// B, G, R, A from R, G, B, A
__device__ __forceinline__ uint32_t bgra_of(uint32_t t, uint32_t flags) {
  const uint32_t o = (t & 0xFF00FF00u) | ((t >> 16) & 255u) | ((t & 255u) << 16);
  return (flags & kIgnoreAlpha) ? o | 0xFF000000u : o;
}
// the run's four texels of the surface row at `row`: one load, or the columns xc[] (clamped into the rectangle) one by one
__device__ __forceinline__ void load_run(const uint32_t* row, int x0, const int xc[4], bool wide, uint32_t out[4]) {
  if (wide) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + x0);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = row[xc[i]];
  }
}
// n (1 .. 4) luma samples of b bits to columns x0 .. of the plane row at `row`; wide: all four as one store
template <uint32_t kFormat>
__device__ __forceinline__ void store_luma(char* row, int x0, const int Y[4], int n, bool wide) {
  if (kFormat == kNv12) {
    if (wide) *reinterpret_cast<uint32_t*>(row + (size_t)x0) = (uint32_t)Y[0] | ((uint32_t)Y[1] << 8) | ((uint32_t)Y[2] << 16) | ((uint32_t)Y[3] << 24);
    else
      for (int i = 0; i < n; i++) *reinterpret_cast<uint8_t*>(row + (size_t)(x0 + i)) = (uint8_t)Y[i];
  } else {
    if (wide) {
      uint2 v;
      v.x = ((uint32_t)Y[0] << 6) | ((uint32_t)Y[1] << 22); v.y = ((uint32_t)Y[2] << 6) | ((uint32_t)Y[3] << 22);
      *reinterpret_cast<uint2*>(row + (size_t)x0 * 2) = v;
    } else
      for (int i = 0; i < n; i++) *reinterpret_cast<uint16_t*>(row + (size_t)(x0 + i) * 2) = (uint16_t)(Y[i] << 6);
  }
}
// n (1 or 2) pairs Cb, Cr to pairs i0 .. of the chroma row at `row`; wide: both as one store
template <uint32_t kFormat>
__device__ __forceinline__ void store_chroma(char* row, int i0, const uint32_t cb[2], const uint32_t cr[2], int n, bool wide) {
  if (kFormat == kNv12) {
    if (wide) *reinterpret_cast<uint32_t*>(row + (size_t)i0 * 2) = cb[0] | (cr[0] << 8) | (cb[1] << 16) | (cr[1] << 24);
    else
      for (int k = 0; k < n; k++) *reinterpret_cast<uint16_t*>(row + (size_t)(i0 + k) * 2) = (uint16_t)(cb[k] | (cr[k] << 8));
  } else {
    if (wide) {
      uint2 v;
      v.x = (cb[0] << 6) | (cr[0] << 22); v.y = (cb[1] << 6) | (cr[1] << 22);
      *reinterpret_cast<uint2*>(row + (size_t)i0 * 4) = v;
    } else
      for (int k = 0; k < n; k++) *reinterpret_cast<uint32_t*>(row + (size_t)(i0 + k) * 4) = (cb[k] << 6) | (cr[k] << 22);
  }
}

}  // namespace video_export

template <uint32_t kFormat, bool kLinear>
__global__ __launch_bounds__(ve::kGroup) void k_video_export(const ve::Params P) {
  const int lane = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * ve::kTileW + (lane & 31) * ve::kRun, y0 = (int)blockIdx.y * ve::kTileH + (lane >> 5) * 2;
  if (x0 >= P.w || y0 >= P.h) return;  // (no barrier below: a lane without a texel just leaves)
  // ---- the loads, all in front of the first conversion.  Rows y0 and min(y0 + 1, h - 1), columns clamped into the rectangle: a run cut
  // by the right edge holds the last column again, an odd height's last pair the last row twice -- the clamps of the specification.
  const bool two = y0 + 1 < P.h, whole = x0 + ve::kRun <= P.w;
  const int n = whole ? ve::kRun : P.w - x0;  // texels of the run inside the rectangle
  int xc[4];
#pragma unroll
  for (int i = 0; i < 4; i++) xc[i] = min(x0 + i, P.w - 1);
  const uint32_t* ra = P.src + (int64_t)y0 * P.src_pitch;
  const uint32_t* rb = P.src + (int64_t)(two ? y0 + 1 : y0) * P.src_pitch;
  uint32_t a[4], b[4], la = 0u, lb = 0u;
  ve::load_run(ra, x0, xc, P.wide_src != 0 && whole, a);
  ve::load_run(rb, x0, xc, P.wide_src != 0 && whole, b);
  if (kLinear) { const int xl = max(x0 - 1, 0); la = ra[xl]; lb = rb[xl]; }
  char* const luma = static_cast<char*>(P.luma);
  const bool wide_y = P.wide_y != 0 && whole;
  if (kFormat == ve::kBgra8) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
      if (r == 1 && !two) break;
      const uint32_t* t = r ? b : a;
      char* row = luma + (int64_t)(y0 + r) * P.pitch_y + (int64_t)x0 * 4;
      if (wide_y) {
        uint4 v;
        v.x = ve::bgra_of(t[0], P.flags); v.y = ve::bgra_of(t[1], P.flags); v.z = ve::bgra_of(t[2], P.flags); v.w = ve::bgra_of(t[3], P.flags);
        *reinterpret_cast<uint4*>(row) = v;
      } else
        for (int i = 0; i < n; i++) reinterpret_cast<uint32_t*>(row)[i] = ve::bgra_of(t[i], P.flags);
    }
    return;
  }
  constexpr int kBits = kFormat == ve::kP010 ? 10 : 8;
  // ---- luma: a sample per texel
#pragma unroll
  for (int r = 0; r < 2; r++) {
    if (r == 1 && !two) break;
    const uint32_t* t = r ? b : a;
    int Y[4];
#pragma unroll
    for (int i = 0; i < 4; i++) Y[i] = ve::luma_of(P, t[i]);
    ve::store_luma<kFormat>(luma + (int64_t)(y0 + r) * P.pitch_y, x0, Y, n, wide_y);
  }
  // ---- chroma: pairs i0 = x0 / 2 and i0 + 1 of chroma row y0 / 2, from the run's columns 2 k, 2 k + 1 of both rows; kLinear also
  // takes the column to the left -- the lane's extra load for k = 0 (the rectangle's first column: itself), the run's second texel for k = 1
  uint32_t cb[2], cr[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    ve::Rgb s;
    if (!kLinear) {
      s = ve::rgb_of(a[2 * k]) + ve::rgb_of(a[2 * k + 1]) + ve::rgb_of(b[2 * k]) + ve::rgb_of(b[2 * k + 1]);
      cb[k] = ve::chroma_of<16, kBits>(P.ku, P.coff, s); cr[k] = ve::chroma_of<16, kBits>(P.kv, P.coff, s);
    } else {
      const ve::Rgb l = ve::rgb_of(k ? a[1] : la) + ve::rgb_of(k ? b[1] : lb), c = ve::rgb_of(a[2 * k]) + ve::rgb_of(b[2 * k]),
                    rr = ve::rgb_of(a[2 * k + 1]) + ve::rgb_of(b[2 * k + 1]);
      s = l + c + c + rr;
      cb[k] = ve::chroma_of<17, kBits>(P.ku, P.coff, s); cr[k] = ve::chroma_of<17, kBits>(P.kv, P.coff, s);
    }
  }
  const int n_pairs = x0 + 2 < P.w ? 2 : 1;
  ve::store_chroma<kFormat>(static_cast<char*>(P.chroma) + (int64_t)(y0 >> 1) * P.pitch_c, x0 >> 1, cb, cr, n_pairs, P.wide_c != 0 && n_pairs == 2);
}

void launch_video_export(hipStream_t s, const ve::Params& P) {
  if (P.w <= 0 || P.h <= 0) return;
  const dim3 grid((P.w + ve::kTileW - 1) / ve::kTileW, (P.h + ve::kTileH - 1) / ve::kTileH), block(ve::kGroup);
  const bool linear = (P.flags & ve::kChromaLinear) != 0;
  if (P.format == ve::kBgra8) FDH_LAUNCH((k_video_export<ve::kBgra8, false>), grid, block, 0, s, P);
  else if (P.format == ve::kNv12 && !linear) FDH_LAUNCH((k_video_export<ve::kNv12, false>), grid, block, 0, s, P);
  else if (P.format == ve::kNv12) FDH_LAUNCH((k_video_export<ve::kNv12, true>), grid, block, 0, s, P);
  else if (!linear) FDH_LAUNCH((k_video_export<ve::kP010, false>), grid, block, 0, s, P);
  else FDH_LAUNCH((k_video_export<ve::kP010, true>), grid, block, 0, s, P);
}

}  // namespace fdh
