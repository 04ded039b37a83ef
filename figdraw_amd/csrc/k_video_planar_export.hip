// k_video_planar_export.hip -- the rendered frame on its way out as three planes, I420, I010 (4:2:0), I444 or I410 (4:4:4):
// fdh_read_video_planes (the specification is the comment of include_video/figdraw_hip_video_planar.h; the parameter block is
// fdh_video_planar.h's OutParams).  One launch per call.  A workgroup of 256 takes a tile of 256 x 16 texels of the rectangle, a lane a
// run of EIGHT texels by two rows: four 16-byte loads of the surface, the two luma runs as one 8-byte (8 bit) or 16-byte (10 bit) store
// each, and for 4:2:0 the four Cb and the four Cr samples under the run as one 4-byte or 8-byte store per plane -- with
// k_video_export's run of four a lane would store two bytes into either chroma plane.  For 4:4:4 the run's eight chroma samples of
// either row are a store of the luma run's size per plane.  The FDH_VIDEO_CHROMA_LINEAR builds take the texel left of the run by one
// more 4-byte load per row (the neighbouring lane's lines: no LDS, no barrier, no cross-lane traffic).  Wide loads and stores only where
// the host found pointer and pitch aligned (OutParams::wide*) and the run lies whole inside the row; element by element elsewhere.
// Nothing is stored outside w x h luma samples and cw x ch samples of either chroma plane: the bytes between a row's end and the pitch
// stay.  No float arithmetic anywhere in this unit.
#include "fdh_device.h"
#include "fdh_video_planar.h"

namespace fdh {
namespace vp = video_planar;

namespace video_planar {

struct OutRgb { int r, g, b; };
__device__ __forceinline__ OutRgb out_rgb(uint32_t t) { return OutRgb{(int)(t & 255u), (int)((t >> 8) & 255u), (int)((t >> 16) & 255u)}; }
__device__ __forceinline__ OutRgb operator+(OutRgb a, OutRgb b) { return OutRgb{a.r + b.r, a.g + b.g, a.b + b.b}; }
// ---- the conversion, once.  int32 throughout; >> of a negative sum is an arithmetic shift (floor).
__device__ __forceinline__ int out_luma(const OutParams& P, uint32_t t) {
  const OutRgb c = out_rgb(t);
  return P.yoff + ((P.ky[0] * c.r + P.ky[1] * c.g + P.ky[2] * c.b + 8192) >> 14);
}
// clamp(Coff + ((k . s + (N << 13)) >> (14 + log2 N)), 0, 2^b - 1) with kShift = 14 + log2 N, written as the clamp of the sum, Coff << kShift
// in it, in front of the shift, which is the same number (k_video_import.hip, shift_clamp, says why the clamp comes first).  The largest
// sum of absolute terms is 134 085 120 (the specification of figdraw_hip_video_out.h); Coff << kShift is at most 2^26: no sum reaches 2^31.
template <int kShift, int kBits>
__device__ __forceinline__ uint32_t out_chroma(const int32_t k[3], int coff, OutRgb s) {
  const int sum = k[0] * s.r + k[1] * s.g + k[2] * s.b + (1 << (kShift - 1)) + coff * (1 << kShift);
  return (uint32_t)min(max(sum, 0), (1 << (kBits + kShift)) - 1) >> kShift;
}
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

}  // namespace video_planar

// kTen: I010 / I410; kFull: I444 / I410 (a chroma sample per texel; kLinear is the 4:2:0 formats')
template <bool kTen, bool kFull, bool kLinear>
__global__ __launch_bounds__(vp::kOutGroup) void k_video_planar_export(const vp::OutParams P) {
  constexpr int kRun = vp::kRun, kBits = kTen ? 10 : 8;
  const int lane = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * vp::kOutTileW + (lane & 31) * kRun, y0 = (int)blockIdx.y * vp::kOutTileH + (lane >> 5) * 2;
  if (x0 >= P.w || y0 >= P.h) return;  // (no barrier below: a lane without a texel just leaves)
  // ---- the loads, all in front of the first conversion.  Rows y0 and min(y0 + 1, h - 1), columns clamped into the rectangle: a run cut
  // by the right edge holds the last column again, an odd height's last row pair the last row twice -- the clamps of the specification.
  const bool two = y0 + 1 < P.h, whole = x0 + kRun <= P.w;
  const int n = whole ? kRun : P.w - x0;  // texels of the run inside the rectangle
  int xc[kRun];
#pragma unroll
  for (int i = 0; i < kRun; i++) xc[i] = min(x0 + i, P.w - 1);
  const uint32_t* ra = P.src + (int64_t)y0 * P.src_pitch;
  const uint32_t* rb = P.src + (int64_t)(two ? y0 + 1 : y0) * P.src_pitch;
  uint32_t a[kRun], b[kRun], la = 0u, lb = 0u;
  vp::load_run(ra, x0, xc, P.wide_src != 0 && whole, a);
  vp::load_run(rb, x0, xc, P.wide_src != 0 && whole, b);
  if (kLinear) { const int xl = max(x0 - 1, 0); la = ra[xl]; lb = rb[xl]; }
  // ---- luma: a sample per texel
#pragma unroll
  for (int r = 0; r < 2; r++) {
    if (r == 1 && !two) break;
    const uint32_t* t = r ? b : a;
    uint32_t Y[kRun];
#pragma unroll
    for (int i = 0; i < kRun; i++) Y[i] = (uint32_t)vp::out_luma(P, t[i]);
    vp::store_samples<kTen, kRun>(static_cast<char*>(P.plane[0]) + (int64_t)(y0 + r) * P.pitch[0], x0, Y, n, P.wide[0] != 0 && whole);
  }
  if (kFull) {
    // ---- 4:4:4 chroma: a sample per texel, N = 1
#pragma unroll
    for (int r = 0; r < 2; r++) {
      if (r == 1 && !two) break;
      const uint32_t* t = r ? b : a;
      uint32_t cb[kRun], cr[kRun];
#pragma unroll
      for (int i = 0; i < kRun; i++) {
        const vp::OutRgb s = vp::out_rgb(t[i]);
        cb[i] = vp::out_chroma<14, kBits>(P.ku, P.coff, s); cr[i] = vp::out_chroma<14, kBits>(P.kv, P.coff, s);
      }
      vp::store_samples<kTen, kRun>(static_cast<char*>(P.plane[1]) + (int64_t)(y0 + r) * P.pitch[1], x0, cb, n, P.wide[1] != 0 && whole);
      vp::store_samples<kTen, kRun>(static_cast<char*>(P.plane[2]) + (int64_t)(y0 + r) * P.pitch[2], x0, cr, n, P.wide[2] != 0 && whole);
    }
    return;
  }
  // ---- 4:2:0 chroma: samples i0 = x0 / 2 .. i0 + 3 of chroma row y0 / 2, from the run's columns 2 k, 2 k + 1 of both rows; kLinear also
  // takes the column to the left -- the lane's extra load for k = 0 (the rectangle's first column: itself), the run's texel 2 k - 1 else
  uint32_t cb[kRun / 2], cr[kRun / 2];
#pragma unroll
  for (int k = 0; k < kRun / 2; k++) {
    vp::OutRgb s;
    if (!kLinear) {
      s = vp::out_rgb(a[2 * k]) + vp::out_rgb(a[2 * k + 1]) + vp::out_rgb(b[2 * k]) + vp::out_rgb(b[2 * k + 1]);
      cb[k] = vp::out_chroma<16, kBits>(P.ku, P.coff, s); cr[k] = vp::out_chroma<16, kBits>(P.kv, P.coff, s);
    } else {
      const vp::OutRgb l = vp::out_rgb(k ? a[2 * k - 1] : la) + vp::out_rgb(k ? b[2 * k - 1] : lb), c = vp::out_rgb(a[2 * k]) + vp::out_rgb(b[2 * k]),
                       rr = vp::out_rgb(a[2 * k + 1]) + vp::out_rgb(b[2 * k + 1]);
      s = l + c + c + rr;
      cb[k] = vp::out_chroma<17, kBits>(P.ku, P.coff, s); cr[k] = vp::out_chroma<17, kBits>(P.kv, P.coff, s);
    }
  }
  const int n_c = (n + 1) >> 1;  // chroma samples of the run inside the rectangle
  vp::store_samples<kTen, kRun / 2>(static_cast<char*>(P.plane[1]) + (int64_t)(y0 >> 1) * P.pitch[1], x0 >> 1, cb, n_c, P.wide[1] != 0 && whole);
  vp::store_samples<kTen, kRun / 2>(static_cast<char*>(P.plane[2]) + (int64_t)(y0 >> 1) * P.pitch[2], x0 >> 1, cr, n_c, P.wide[2] != 0 && whole);
}

void launch_video_planar_export(hipStream_t s, const vp::OutParams& P) {
  if (P.w <= 0 || P.h <= 0) return;
  const dim3 grid((P.w + vp::kOutTileW - 1) / vp::kOutTileW, (P.h + vp::kOutTileH - 1) / vp::kOutTileH), block(vp::kOutGroup);
  const bool linear = (P.flags & vp::kChromaLinear) != 0;
  if (P.format == vp::kI420 && !linear) FDH_LAUNCH((k_video_planar_export<false, false, false>), grid, block, 0, s, P);
  else if (P.format == vp::kI420) FDH_LAUNCH((k_video_planar_export<false, false, true>), grid, block, 0, s, P);
  else if (P.format == vp::kI010 && !linear) FDH_LAUNCH((k_video_planar_export<true, false, false>), grid, block, 0, s, P);
  else if (P.format == vp::kI010) FDH_LAUNCH((k_video_planar_export<true, false, true>), grid, block, 0, s, P);
  else if (P.format == vp::kI444) FDH_LAUNCH((k_video_planar_export<false, true, false>), grid, block, 0, s, P);
  else FDH_LAUNCH((k_video_planar_export<true, true, false>), grid, block, 0, s, P);
}

}  // namespace fdh
