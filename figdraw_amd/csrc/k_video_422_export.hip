// k_video_422_export.hip -- the rendered frame on its way out as 4:2:2 video, I422, I210 (three planes) or YUY2, UYVY (one plane of
// four-byte groups): fdh_read_video_422 (the specification is the comment of include_video/figdraw_hip_video_422.h; the parameter block
// is fdh_video_422.h's OutParams).  One launch per call.  A workgroup of 256 takes a tile of 256 x 8 texels of the rectangle, a lane a
// run of EIGHT texels of ONE row.  One row, not k_video_planar_export's two: 4:2:0 pairs rows because a chroma sample averages both, and
// a 4:2:2 sample averages along its own row alone -- a second row would share no load, no sum and no store with the first, it would
// double the eight texel registers a lane holds in front of its first conversion and halve the lanes a small frame gives the device.
// With one row a wave covers two whole rows of the tile's width, every store of a plane 32 lanes' worth of contiguous bytes.  A lane
// makes two 16-byte loads of the surface; the luma run is one 8-byte (8 bit) or 16-byte (10 bit) store, the four Cb and the four Cr
// samples under it one 4-byte or 8-byte store per plane; a packed run, four groups, is one 16-byte store.  The FDH_VIDEO_CHROMA_LINEAR
// builds take the texel left of the run by one more 4-byte load (the neighbouring lane's line: no LDS, no barrier, no cross-lane
// traffic).  Wide loads and stores only where the host found pointer and pitch aligned (OutParams::wide*) and the run lies whole inside
// the row; element by element elsewhere, a packed row group by group.  Nothing is stored outside w luma and cw chroma samples of a row,
// or 4 cw bytes of a packed row: the bytes between a row's end and the pitch stay.  No float arithmetic anywhere in this unit.
#include "fdh_device.h"
#include "fdh_video_422.h"

namespace fdh {
namespace v2 = video_422;

namespace video_422 {

struct OutRgb { int r, g, b; };
__device__ __forceinline__ OutRgb out_rgb(uint32_t t) { return OutRgb{(int)(t & 255u), (int)((t >> 8) & 255u), (int)((t >> 16) & 255u)}; }
__device__ __forceinline__ OutRgb operator+(OutRgb a, OutRgb b) { return OutRgb{a.r + b.r, a.g + b.g, a.b + b.b}; }
// ---- the conversion, once.  int32 throughout; >> of a negative sum is an arithmetic shift (floor).
__device__ __forceinline__ int out_luma(const OutParams& P, uint32_t t) {
  const OutRgb c = out_rgb(t);
  return P.yoff + ((P.ky[0] * c.r + P.ky[1] * c.g + P.ky[2] * c.b + 8192) >> 14);
}
// clamp(Coff + ((k . s + (N << 13)) >> (14 + log2 N)), 0, 2^b - 1) with kShift = 14 + log2 N, written as the clamp of the sum, Coff << kShift
// in it, in front of the shift, which is the same number (k_video_import.hip, shift_clamp, says why the clamp comes first).  N is 2 or 4
// here; figdraw_hip_video_out.h proved for N <= 8 that no sum reaches 2^31, and Coff << kShift is at most 2^25.
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
// n (1 .. 4) groups of a packed row, a group a 32-bit word, to groups g0 .. of the row at `row`; wide: all four as one store
__device__ __forceinline__ void store_groups(char* row, int g0, const uint32_t g[kRun / 2], int n, bool wide) {
  if (wide) {
    uint4 t; t.x = g[0]; t.y = g[1]; t.z = g[2]; t.w = g[3];
    *reinterpret_cast<uint4*>(row + (size_t)g0 * 4) = t;
  } else {
    for (int k = 0; k < n; k++) *reinterpret_cast<uint32_t*>(row + (size_t)(g0 + k) * 4) = g[k];
  }
}

}  // namespace video_422

// kTen: I210; kPacked: YUY2 / UYVY (P.order says which); kLinear: FDH_VIDEO_CHROMA_LINEAR
template <bool kTen, bool kPacked, bool kLinear>
__global__ __launch_bounds__(v2::kOutGroup) void k_video_422_export(const v2::OutParams P) {
  static_assert(!(kTen && kPacked), "the packed formats are 8 bit");
  constexpr int kRun = v2::kRun, kC = kRun / 2, kBits = kTen ? 10 : 8;
  const int lane = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * v2::kOutTileW + (lane & 31) * kRun, y = (int)blockIdx.y * v2::kOutTileH + (lane >> 5);
  if (x0 >= P.w || y >= P.h) return;  // (no barrier below: a lane without a texel just leaves)
  // ---- the loads, all in front of the first conversion.  Columns clamped into the rectangle: a run cut by the right edge holds the last
  // column again -- the clamp of the specification's xb and xr, and the second luma of an odd width's last group.
  const bool whole = x0 + kRun <= P.w;
  const int n = whole ? kRun : P.w - x0;  // texels of the run inside the rectangle
  const int n_c = (n + 1) >> 1;           // its chroma samples, its groups
  int xc[kRun];
#pragma unroll
  for (int i = 0; i < kRun; i++) xc[i] = min(x0 + i, P.w - 1);
  const uint32_t* ra = P.src + (int64_t)y * P.src_pitch;
  uint32_t a[kRun], la = 0u;
  v2::load_run(ra, x0, xc, P.wide_src != 0 && whole, a);
  if (kLinear) la = ra[max(x0 - 1, 0)];
  // ---- luma: a sample per texel (a cut run: the last column's again behind it, for the packed group)
  uint32_t Y[kRun];
#pragma unroll
  for (int i = 0; i < kRun; i++) Y[i] = (uint32_t)v2::out_luma(P, a[i]);
  // ---- chroma: samples i0 = x0 / 2 .. i0 + 3 of the row, from the run's columns 2 k and 2 k + 1; kLinear also takes the column to the
  // left -- the lane's extra load for k = 0 (the rectangle's first column: itself), the run's texel 2 k - 1 else
  uint32_t cb[kC], cr[kC];
#pragma unroll
  for (int k = 0; k < kC; k++) {
    const v2::OutRgb c = v2::out_rgb(a[2 * k]), rr = v2::out_rgb(a[2 * k + 1]);
    if (!kLinear) {
      const v2::OutRgb s = c + rr;
      cb[k] = v2::out_chroma<15, kBits>(P.ku, P.coff, s); cr[k] = v2::out_chroma<15, kBits>(P.kv, P.coff, s);
    } else {
      const v2::OutRgb s = v2::out_rgb(k ? a[2 * k - 1] : la) + c + c + rr;
      cb[k] = v2::out_chroma<16, kBits>(P.ku, P.coff, s); cr[k] = v2::out_chroma<16, kBits>(P.kv, P.coff, s);
    }
  }
  if (kPacked) {
    const int s = P.order ? 8 : 0;
    uint32_t g[kC];
#pragma unroll
    for (int k = 0; k < kC; k++) g[k] = (Y[2 * k] << s) | (Y[2 * k + 1] << (16 + s)) | (cb[k] << (8 - s)) | (cr[k] << (24 - s));
    v2::store_groups(static_cast<char*>(P.plane[0]) + (int64_t)y * P.pitch[0], x0 >> 1, g, n_c, P.wide[0] != 0 && whole);
    return;
  }
  v2::store_samples<kTen, kRun>(static_cast<char*>(P.plane[0]) + (int64_t)y * P.pitch[0], x0, Y, n, P.wide[0] != 0 && whole);
  v2::store_samples<kTen, kC>(static_cast<char*>(P.plane[1]) + (int64_t)y * P.pitch[1], x0 >> 1, cb, n_c, P.wide[1] != 0 && whole);
  v2::store_samples<kTen, kC>(static_cast<char*>(P.plane[2]) + (int64_t)y * P.pitch[2], x0 >> 1, cr, n_c, P.wide[2] != 0 && whole);
}

void launch_video_422_export(hipStream_t s, const v2::OutParams& P) {
  if (P.w <= 0 || P.h <= 0) return;
  const dim3 grid((P.w + v2::kOutTileW - 1) / v2::kOutTileW, (P.h + v2::kOutTileH - 1) / v2::kOutTileH), block(v2::kOutGroup);
  const bool linear = (P.flags & v2::kChromaLinear) != 0;
  if (P.format == v2::kI422 && !linear) FDH_LAUNCH((k_video_422_export<false, false, false>), grid, block, 0, s, P);
  else if (P.format == v2::kI422) FDH_LAUNCH((k_video_422_export<false, false, true>), grid, block, 0, s, P);
  else if (P.format == v2::kI210 && !linear) FDH_LAUNCH((k_video_422_export<true, false, false>), grid, block, 0, s, P);
  else if (P.format == v2::kI210) FDH_LAUNCH((k_video_422_export<true, false, true>), grid, block, 0, s, P);
  else if (!linear) FDH_LAUNCH((k_video_422_export<false, true, false>), grid, block, 0, s, P);
  else FDH_LAUNCH((k_video_422_export<false, true, true>), grid, block, 0, s, P);
}

}  // namespace fdh
