// k_video_alpha_export.hip -- the rendered frame on its way out as video with an alpha plane, A420, A444, A410 (three planes and A) or
// UYVA (a UYVY plane and A): fdh_read_video_alpha (the specification is the comment of include_video/figdraw_hip_video_alpha.h; the
// parameter block is fdh_video_alpha.h's OutParams).  One launch per call, a workgroup of 256, a lane a run of EIGHT texels.  A420 pairs
// rows, a chroma sample averages both: a lane takes its run in TWO rows of a 256 x 16 tile, k_video_planar_export's shape.  A444, A410
// and UYVA pair none: a lane takes ONE row of a 256 x 8 tile, k_video_422_export's shape, which DESIGN.md section 8 found the faster
// where no rows pair.  A lane makes two 16-byte loads of the surface per row; luma, chroma and the UYVY groups are stored as the base
// format's kernel stores them, and the run's alpha samples, packed from the texels already in registers, are one 8-byte store (16 bytes
// for A410) per row.  The FDH_VIDEO_CHROMA_LINEAR builds take the texel left of the run by one more 4-byte load per row.  Wide loads
// and stores only where the host found pointer and pitch aligned (OutParams::wide*) and the run lies whole inside the row; element by
// element elsewhere, the UYVY plane group by group.  Without FDH_VIDEO_STRAIGHT_ALPHA the surface's premultiplied colour bytes go out as
// stored; with it every sample is made of the un-premultiplied colour: s = min(255 N, (510 N sc + sa) / (2 sa)) per channel, sc and sa
// the sample's weighted sums of colour and of alpha, 0 where sa is 0 -- the language's unsigned `/`, an exact quotient (the largest
// numerator, 510 * 8 * 2040 + 2040, is below 2^24).  Nothing is stored outside a row's samples: the bytes between a row's end and the
// pitch stay.  No float arithmetic anywhere in this unit.
#include "fdh_device.h"
#include "fdh_video_alpha.h"

namespace fdh {
namespace va = video_alpha;

namespace video_alpha {

// a texel's, or a sample's weighted sum of texels', four channels
struct OutRgba { int r, g, b, a; };
__device__ __forceinline__ OutRgba out_rgba(uint32_t t) { return OutRgba{(int)(t & 255u), (int)((t >> 8) & 255u), (int)((t >> 16) & 255u), (int)(t >> 24)}; }
__device__ __forceinline__ OutRgba operator+(OutRgba a, OutRgba b) { return OutRgba{a.r + b.r, a.g + b.g, a.b + b.b, a.a + b.a}; }
// N times the alpha-weighted average straight colour of a sample whose weights sum to kN, rounded half up: per channel
// min(255 N, (510 N sc + sa) / (2 sa)), 0 where sa is 0.  kN = 1: the texel's straight byte.  Not kStraight: the sums as they are.
template <bool kStraight, int kN>
__device__ __forceinline__ OutRgba out_colour(OutRgba s) {
  if (!kStraight) return s;
  if (s.a == 0) return OutRgba{0, 0, 0, 0};
  const uint32_t sa = (uint32_t)s.a, d = 2u * sa;
  return OutRgba{(int)min(255u * kN, (510u * kN * (uint32_t)s.r + sa) / d), (int)min(255u * kN, (510u * kN * (uint32_t)s.g + sa) / d),
                 (int)min(255u * kN, (510u * kN * (uint32_t)s.b + sa) / d), s.a};
}
// ---- the conversion, once.  int32 throughout; >> of a negative sum is an arithmetic shift (floor).
__device__ __forceinline__ int out_luma(const OutParams& P, OutRgba c) { return P.yoff + ((P.ky[0] * c.r + P.ky[1] * c.g + P.ky[2] * c.b + 8192) >> 14); }
// clamp(Coff + ((k . s + (N << 13)) >> (14 + log2 N)), 0, 2^b - 1) with kShift = 14 + log2 N, written as the clamp of the sum, Coff << kShift
// in it, in front of the shift, which is the same number (k_video_import.hip, shift_clamp, says why the clamp comes first).  N <= 8 and
// every operand is at most 255 N, straight or not: figdraw_hip_video_out.h proved that no sum reaches 2^31; Coff << kShift is at most 2^26.
template <int kShift, int kBits>
__device__ __forceinline__ uint32_t out_chroma(const int32_t k[3], int coff, OutRgba s) {
  const int sum = k[0] * s.r + k[1] * s.g + k[2] * s.b + (1 << (kShift - 1)) + coff * (1 << kShift);
  return (uint32_t)min(max(sum, 0), (1 << (kBits + kShift)) - 1) >> kShift;
}
// the alpha sample of an alpha byte: the byte, or for A410 the exact rational 1023 A / 255 to nearest (no tie: 255 and 1023 are odd)
template <bool kTen>
__device__ __forceinline__ uint32_t out_alpha(uint32_t texel) { return kTen ? (1023u * (texel >> 24) + 127u) / 255u : texel >> 24; }
// the run's eight texels of the surface row at `row`: two loads, or the columns xc[] (clamped into the rectangle) one by one
__device__ __forceinline__ void load_run(const uint32_t* row, int x0, const int xc[kRun], bool wide, uint32_t out[kRun]) {
  if (wide) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + x0), u = *reinterpret_cast<const uint4*>(row + x0 + 4);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    out[4] = u.x; out[5] = u.y; out[6] = u.z; out[7] = u.w;
  } else {
#pragma unroll
    for (int i = 0; i < kRun; i++) out[i] = row[xc[i]];
  }
}
// n (1 .. kN) samples of b bits, the high bits of a 10-bit word zero, to columns c0 .. of the plane row at `row`; wide: all kN (4 or 8) as
// one store
template <bool kTen, int kN>
__device__ __forceinline__ void store_samples(char* row, int c0, const uint32_t v[kN], int n, bool wide) {
  if (wide) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < kN; i++) {
      if (kTen) w[i >> 1] |= v[i] << (16 * (i & 1));
      else w[i >> 2] |= v[i] << (8 * (i & 3));
    }
    char* at = row + (size_t)c0 * (kTen ? 2 : 1);
    if (kN * (kTen ? 2 : 1) == 4) *reinterpret_cast<uint32_t*>(at) = w[0];
    else if (kN * (kTen ? 2 : 1) == 8) { uint2 t; t.x = w[0]; t.y = w[1]; *reinterpret_cast<uint2*>(at) = t; }
    else { uint4 t; t.x = w[0]; t.y = w[1]; t.z = w[2]; t.w = w[3]; *reinterpret_cast<uint4*>(at) = t; }
  } else {
    for (int i = 0; i < n; i++) {
      if (kTen) *reinterpret_cast<uint16_t*>(row + (size_t)(c0 + i) * 2) = (uint16_t)v[i];
      else *reinterpret_cast<uint8_t*>(row + (size_t)(c0 + i)) = (uint8_t)v[i];
    }
  }
}
// n (1 .. 4) groups of the UYVY plane, a group a 32-bit word, to groups g0 .. of the row at `row`; wide: all four as one store
__device__ __forceinline__ void store_groups(char* row, int g0, const uint32_t g[kRun / 2], int n, bool wide) {
  if (wide) {
    uint4 t; t.x = g[0]; t.y = g[1]; t.z = g[2]; t.w = g[3];
    *reinterpret_cast<uint4*>(row + (size_t)g0 * 4) = t;
  } else {
    for (int k = 0; k < n; k++) *reinterpret_cast<uint32_t*>(row + (size_t)(g0 + k) * 4) = g[k];
  }
}

}  // namespace video_alpha

// kFormat: kA420 .. kUYVA; kLinear: FDH_VIDEO_CHROMA_LINEAR (A420 and UYVA alone); kStraight: FDH_VIDEO_STRAIGHT_ALPHA
template <uint32_t kFormat, bool kLinear, bool kStraight>
__global__ __launch_bounds__(va::kOutGroup) void k_video_alpha_export(const va::OutParams P) {
  constexpr bool kTen = va::ten_bit(kFormat), kFull = va::full_chroma(kFormat), kPacked = va::packed(kFormat);
  static_assert(!(kLinear && kFull), "a 4:4:4 frame has a chroma sample per texel");
  constexpr int kRun = va::kRun, kC = kRun / 2, kBits = kTen ? 10 : 8, kRows = va::out_rows(kFormat);
  const int lane = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * va::kOutTileW + (lane & 31) * kRun, y0 = (int)blockIdx.y * va::out_tile_h(kFormat) + (lane >> 5) * kRows;
  if (x0 >= P.w || y0 >= P.h) return;  // (no barrier below: a lane without a texel just leaves)
  // ---- the loads, all in front of the first conversion.  Columns clamped into the rectangle: a run cut by the right edge holds the last
  // column again, an odd height's last row pair (A420) the last row twice -- the clamps of the specification, and the second luma of an odd
  // width's last UYVY group.
  const bool two = kRows == 2 && y0 + 1 < P.h, whole = x0 + kRun <= P.w;
  const int n = whole ? kRun : P.w - x0;  // texels of the run inside the rectangle
  const int n_c = (n + 1) >> 1;           // its 4:2:0 / 4:2:2 chroma samples, its groups
  int xc[kRun];
#pragma unroll
  for (int i = 0; i < kRun; i++) xc[i] = min(x0 + i, P.w - 1);
  uint32_t t[kRows][kRun], left[kRows];
#pragma unroll
  for (int r = 0; r < kRows; r++) {
    const uint32_t* row = P.src + (int64_t)(r && two ? y0 + 1 : y0) * P.src_pitch;
    va::load_run(row, x0, xc, P.wide_src != 0 && whole, t[r]);
    left[r] = kLinear ? row[max(x0 - 1, 0)] : 0u;
  }
  // ---- alpha and luma: a sample per texel; 4:4:4 chroma too (N = 1: of the texel's straight colour, or of its bytes as stored)
  uint32_t Y[kRows][kRun];
#pragma unroll
  for (int r = 0; r < kRows; r++) {
    if (r == 1 && !two) break;
    uint32_t A[kRun], cb[kRun], cr[kRun];
#pragma unroll
    for (int i = 0; i < kRun; i++) {
      const va::OutRgba c = va::out_colour<kStraight, 1>(va::out_rgba(t[r][i]));
      A[i] = va::out_alpha<kTen>(t[r][i]);
      Y[r][i] = (uint32_t)va::out_luma(P, c);
      if (kFull) { cb[i] = va::out_chroma<14, kBits>(P.ku, P.coff, c); cr[i] = va::out_chroma<14, kBits>(P.kv, P.coff, c); }
    }
    va::store_samples<kTen, kRun>(static_cast<char*>(P.plane[va::kAlpha]) + (int64_t)(y0 + r) * P.pitch[va::kAlpha], x0, A, n, P.wide[va::kAlpha] != 0 && whole);
    if (!kPacked) va::store_samples<kTen, kRun>(static_cast<char*>(P.plane[0]) + (int64_t)(y0 + r) * P.pitch[0], x0, Y[r], n, P.wide[0] != 0 && whole);
    if (kFull) {
      va::store_samples<kTen, kRun>(static_cast<char*>(P.plane[1]) + (int64_t)(y0 + r) * P.pitch[1], x0, cb, n, P.wide[1] != 0 && whole);
      va::store_samples<kTen, kRun>(static_cast<char*>(P.plane[2]) + (int64_t)(y0 + r) * P.pitch[2], x0, cr, n, P.wide[2] != 0 && whole);
    }
  }
  if (kFull) return;
  // ---- subsampled chroma: samples i0 = x0 / 2 .. i0 + 3, from the run's columns 2 k and 2 k + 1 of the lane's rows (an odd height's last
  // row twice, as loaded); kLinear also takes the column to the left -- the lane's extra load for k = 0 (the rectangle's first column:
  // itself), the run's texel 2 k - 1 else -- with weights 1 2 1.  N = 2 kRows, or 4 kRows with kLinear.
  constexpr int kLog2N = (kRows == 2 ? 2 : 1) + (kLinear ? 1 : 0);
  uint32_t cb[kC], cr[kC];
#pragma unroll
  for (int k = 0; k < kC; k++) {
    va::OutRgba c = va::out_rgba(t[0][2 * k]), rr = va::out_rgba(t[0][2 * k + 1]), l = va::out_rgba(k ? t[0][2 * k - 1] : left[0]);
    if (kRows == 2) {
      c = c + va::out_rgba(t[kRows - 1][2 * k]); rr = rr + va::out_rgba(t[kRows - 1][2 * k + 1]);
      l = l + va::out_rgba(k ? t[kRows - 1][2 * k - 1] : left[kRows - 1]);
    }
    const va::OutRgba s = va::out_colour<kStraight, 1 << kLog2N>(kLinear ? l + c + c + rr : c + rr);
    cb[k] = va::out_chroma<14 + kLog2N, kBits>(P.ku, P.coff, s); cr[k] = va::out_chroma<14 + kLog2N, kBits>(P.kv, P.coff, s);
  }
  if (kPacked) {
    uint32_t g[kC];
#pragma unroll
    for (int k = 0; k < kC; k++) g[k] = cb[k] | (Y[0][2 * k] << 8) | (cr[k] << 16) | (Y[0][2 * k + 1] << 24);  // Cb Y0 Cr Y1
    va::store_groups(static_cast<char*>(P.plane[0]) + (int64_t)y0 * P.pitch[0], x0 >> 1, g, n_c, P.wide[0] != 0 && whole);
    return;
  }
  va::store_samples<kTen, kC>(static_cast<char*>(P.plane[1]) + (int64_t)(y0 >> 1) * P.pitch[1], x0 >> 1, cb, n_c, P.wide[1] != 0 && whole);
  va::store_samples<kTen, kC>(static_cast<char*>(P.plane[2]) + (int64_t)(y0 >> 1) * P.pitch[2], x0 >> 1, cr, n_c, P.wide[2] != 0 && whole);
}

namespace video_alpha {
template <uint32_t kFormat, bool kLinear>
void launch_out(hipStream_t s, const OutParams& P) {
  const dim3 grid((P.w + kOutTileW - 1) / kOutTileW, (P.h + out_tile_h(kFormat) - 1) / out_tile_h(kFormat)), block(kOutGroup);
  if (P.flags & kStraightAlpha) FDH_LAUNCH((k_video_alpha_export<kFormat, kLinear, true>), grid, block, 0, s, P);
  else FDH_LAUNCH((k_video_alpha_export<kFormat, kLinear, false>), grid, block, 0, s, P);
}
}  // namespace video_alpha

void launch_video_alpha_export(hipStream_t s, const va::OutParams& P) {
  if (P.w <= 0 || P.h <= 0) return;
  const bool linear = (P.flags & va::kChromaLinear) != 0;
  if (P.format == va::kA420 && !linear) va::launch_out<va::kA420, false>(s, P);
  else if (P.format == va::kA420) va::launch_out<va::kA420, true>(s, P);
  else if (P.format == va::kA444) va::launch_out<va::kA444, false>(s, P);
  else if (P.format == va::kA410) va::launch_out<va::kA410, false>(s, P);
  else if (!linear) va::launch_out<va::kUYVA, false>(s, P);
  else va::launch_out<va::kUYVA, true>(s, P);
}

}  // namespace fdh
