// k_video_alpha_import.hip -- video frames with an alpha plane on their way into the atlas: fdh_put_video_alpha and
// fdh_update_video_alpha (the specification is the comment of include_video/figdraw_hip_video_alpha.h; the parameter block is
// fdh_video_alpha.h's InParams).  A420 (I420's planes and an alpha plane), A444, A410 (I444's, I410's) and UYVA (a UYVY plane and an
// alpha plane).  k_video_alpha_import has k_image_import's tile (k_image_import.hip), which takes any alpha through its level chain and
// its ink block: a 32 x 32 tile of the IMAGE per workgroup of 128, a lane per run of EIGHT texels of one row, four runs across the tile
// and 32 rows down; level 0 into the atlas, levels 1 .. 5 through LDS, the last texel into the compact level-5 image, the ink block;
// k_image_import_tail finishes the chain.  A lane's colour loads are its base format's -- I420's (k_video_planar_import.hip: 8 + 4 + 4
// bytes, with FDH_VIDEO_CHROMA_LINEAR a second chroma row and one sample more), I444's / I410's (8 or 16 bytes a plane) or UYVY's
// (k_video_422_import.hip: four groups, 16 bytes, with FDH_VIDEO_CHROMA_LINEAR one group more) -- and one more load: the run's eight
// alpha samples, 8 bytes, or 16 for A410.  Alpha is the sample of the texel itself, never interpolated.  With FDH_VIDEO_STRAIGHT_ALPHA a
// colour byte becomes (c * A) / 255 behind the conversion, import_texel's rule; without it the converted colour is stored as converted.
// The tile body and the conversion are restated here, not shared: the existing kernel units and their code objects stay as they are.
// No float arithmetic anywhere in this unit.
#include "fdh_device.h"
#include "fdh_video_alpha.h"

namespace fdh {
namespace va = video_alpha;
namespace ii = image_import;

namespace video_alpha {

// ---- the conversion, once.  int32 throughout; >> of a negative sum is an arithmetic shift (floor).
// clamp(sum >> 14, 0, 255), written as the clamp of the sum in front of the shift, which is the same number.  In the other order the
// compiler packs two channels with an instruction that takes the upper half of its destination for zero where the MI355X keeps what the
// register held (k_video_import.hip, shift_clamp, has the whole story); tools/lint_isa.py refuses the opcode.
__device__ __forceinline__ uint32_t in_shift_clamp(int sum) { return (uint32_t)min(max(sum, 0), (256 << 14) - 1) >> 14; }
// Y, Cb, Cr samples (b bits each) and the alpha byte -> the texel R | G << 8 | B << 16 | A << 24; kStraight: a colour byte becomes
// (c * A) / 255 first (k_image_import.hip, import_texel)
template <bool kStraight>
__device__ __forceinline__ uint32_t in_texel(const InParams& P, int Y, int cb, int cr, uint32_t a) {
  const int y = P.cy * (Y - P.yoff) + 8192, u = cb - P.coff, v = cr - P.coff;
  uint32_t r = in_shift_clamp(y + P.crv * v);
  uint32_t g = in_shift_clamp(y - P.cgu * u - P.cgv * v);
  uint32_t b = in_shift_clamp(y + P.cbu * u);
  if (kStraight) { r = r * a / 255u; g = g * a / 255u; b = b * a / 255u; }
  return r | (g << 8) | (b << 16) | (a << 24);
}
// the alpha byte of a 10-bit alpha sample: the exact rational 255 a10 / 1023 to nearest (no tie: 255 and 1023 are odd)
__device__ __forceinline__ uint32_t in_alpha10(int a10) { return (255u * (uint32_t)a10 + 511u) / 1023u; }
// FDH_VIDEO_CHROMA_LINEAR of A420 (I420's rule), one component: near / far = sample i of chroma rows j / jn, near1 / far1 sample
// min(i + 1, cw - 1).  Even luma columns lie on sample i, odd ones midway to the next.
__device__ __forceinline__ int in_chroma_even(int near, int far) { return (3 * near + far + 2) >> 2; }
__device__ __forceinline__ int in_chroma_odd(int near, int far, int near1, int far1) { return (3 * near + far + 3 * near1 + far1 + 4) >> 3; }
// ... of UYVA (UYVY's rule), an odd luma column: midway between sample i and sample min(i + 1, cw - 1) of its own row
__device__ __forceinline__ int in_chroma_odd_row(int near, int next) { return (near + next + 1) >> 1; }

// ---- the loads.  As in k_image_import: `wide` -- pointer and pitch allow one load of the run, and the row has a whole run --, every
// lane issues that one load, its own run where that lies inside the row (`whole`), the row's first where it does not; such a lane then
// loads element by element at clamped columns, as every lane does without `wide`.
// kN (4 or 8) samples at columns c0 .. c0 + kN - 1 (cc[]: clamped) of the row at `row`; a 10-bit sample is word & 1023
template <bool kTen, int kN>
__device__ __forceinline__ void load_samples(const char* row, int c0, const int cc[kN], bool wide, bool whole, int out[kN]) {
  uint32_t v[4] = {0u, 0u, 0u, 0u};  // the run as it lies in memory: kN bytes or kN words
  const char* at = row + (size_t)(whole ? c0 : 0) * (kTen ? 2 : 1);
  if (wide) {
    if (kN * (kTen ? 2 : 1) == 4) v[0] = *reinterpret_cast<const uint32_t*>(at);
    else if (kN * (kTen ? 2 : 1) == 8) { const uint2 t = *reinterpret_cast<const uint2*>(at); v[0] = t.x; v[1] = t.y; }
    else { const uint4 t = *reinterpret_cast<const uint4*>(at); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  }
#pragma unroll
  for (int i = 0; i < kN; i++) {
    if (kTen) out[i] = (int)((v[i >> 1] >> (16 * (i & 1))) & 1023u);
    else out[i] = (int)((v[i >> 2] >> (8 * (i & 3))) & 255u);
  }
  if (!whole) {
#pragma unroll
    for (int i = 0; i < kN; i++) {
      if (kTen) out[i] = (int)(*reinterpret_cast<const uint16_t*>(row + (size_t)cc[i] * 2) & 1023u);
      else out[i] = (int)*reinterpret_cast<const uint8_t*>(row + (size_t)cc[i]);
    }
  }
}
// one sample more, at the clamped column c (FDH_VIDEO_CHROMA_LINEAR of A420: the sample right of the run's four)
__device__ __forceinline__ int load_sample(const char* row, int c) { return (int)*reinterpret_cast<const uint8_t*>(row + (size_t)c); }
// the UYVY plane's four groups g0 .. g0 + 3 of a row (gc[]: clamped), a group a 32-bit word: one 16-byte load, or four 4-byte loads
__device__ __forceinline__ void load_groups(const char* row, int g0, const int gc[kRun / 2], bool wide, bool whole, uint32_t out[kRun / 2]) {
  if (wide) {
    const uint4 t = *reinterpret_cast<const uint4*>(row + (size_t)(whole ? g0 : 0) * 4);
    out[0] = t.x; out[1] = t.y; out[2] = t.z; out[3] = t.w;
  }
  if (!whole) {
#pragma unroll
    for (int k = 0; k < kRun / 2; k++) out[k] = *reinterpret_cast<const uint32_t*>(row + (size_t)gc[k] * 4);
  }
}
// a group's four bytes: Cb Y0 Cr Y1
__device__ __forceinline__ int group_cb(uint32_t g) { return (int)(g & 255u); }
__device__ __forceinline__ int group_y0(uint32_t g) { return (int)((g >> 8) & 255u); }
__device__ __forceinline__ int group_cr(uint32_t g) { return (int)((g >> 16) & 255u); }
__device__ __forceinline__ int group_y1(uint32_t g) { return (int)(g >> 24); }

// ---- the tile body's two steps, as k_image_import.hip has them (import_minify, import_store).
// One texel of minify_by2_host: a, b = the texels (2x, 2y), (2x + 1, 2y), c, d = those of the row below; col_pair / row_pair: the source
// has column 2x + 1 / row 2y + 1.  Where it has not, `a` is its last column / row.
__device__ __forceinline__ uint32_t in_minify(uint32_t a, uint32_t b, uint32_t c, uint32_t d, bool col_pair, bool row_pair) {
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const uint32_t ca = (a >> k) & 255u, cb = (b >> k) & 255u, cc = (c >> k) & 255u, cd = (d >> k) & 255u;
    uint32_t v;
    if (col_pair && row_pair) v = (ca + cb + cc + cd) >> 2;
    else if (row_pair) v = ((ca * 127u + cc * 128u) / 255u) * 128u / 255u;  // last column: rows 2y, 2y + 1
    else if (col_pair) v = ((ca * 127u + cb * 128u) / 255u) * 128u / 255u;  // last row: columns 2x, 2x + 1
    else v = ca * 64u / 255u;
    o |= v << k;
  }
  return o;
}
// texel (i, j) of the image at level l -> its place in the atlas; a texel outside the level is dropped
__device__ __forceinline__ void in_store(uint32_t* const* level, int size, int x, int y, int l, int i, int j, uint32_t texel) {
  const int LS = size >> l, tx = (x >> l) + i, ty = (y >> l) + j;
  if (tx >= 0 && ty >= 0 && tx < LS && ty < LS) level[l][(size_t)ty * LS + tx] = texel;
}

// LDS of a tile: the levels one after the other, 32 x 32, 16 x 16, .. 1 (no level is written twice)
constexpr int kInTileWords = 1024 + 256 + 64 + 16 + 4 + 1;

}  // namespace video_alpha

// kFormat: kA420 .. kUYVA; kLinear: FDH_VIDEO_CHROMA_LINEAR (A420 and UYVA alone); kStraight: FDH_VIDEO_STRAIGHT_ALPHA
template <uint32_t kFormat, bool kLinear, bool kStraight>
__global__ __launch_bounds__(va::kInGroup) void k_video_alpha_import(const va::InParams P) {
  constexpr bool kTen = va::ten_bit(kFormat), kFull = va::full_chroma(kFormat), kPacked = va::packed(kFormat);
  static_assert(!(kLinear && kFull), "a 4:4:4 frame has a chroma sample per texel");
  __shared__ __attribute__((aligned(16))) uint32_t tile[va::kInTileWords + 3];
  __shared__ uint32_t lines[2 * ii::kTile];  // per row of the tile, then per column: the largest alpha | the largest colour byte << 8
  constexpr int kRun = va::kRun, kC = kFull ? kRun : kRun / 2;  // chroma samples of either kind, or groups, that go with a run
  const int lane = (int)threadIdx.x;
  const int r = lane >> 2, c0 = (lane & 3) * kRun;  // a wave covers sixteen whole rows of the tile
  const int X0 = (int)blockIdx.x * ii::kTile + c0, Y = (int)blockIdx.y * ii::kTile + r;
  // ---- the loads.  Every address is valid -- rows, columns, samples and groups clamped into their plane -- and what lies outside the
  // image is replaced behind the conversion: no load waits for a branch on the texel's place, and all of a lane's loads go out before
  // the first conversion.  The run's luma columns X0 .. X0 + 7 lie over the chroma samples (the groups) i0 .. i0 + kC - 1.
  const int yc = min(Y, P.h - 1);
  int xc[kRun];
#pragma unroll
  for (int i = 0; i < kRun; i++) xc[i] = min(X0 + i, P.w - 1);
  const int i0 = kFull ? X0 : X0 >> 1, last = min(i0 + kC, P.cw - 1);
  int pc[kC];
#pragma unroll
  for (int k = 0; k < kC; k++) pc[k] = min(i0 + k, P.cw - 1);
  const char* row = static_cast<const char*>(P.plane[0]) + (int64_t)yc * P.pitch[0];
  const char* arow = static_cast<const char*>(P.plane[va::kAlpha]) + (int64_t)yc * P.pitch[va::kAlpha];
  int Ys[kRun], As[kRun], cu[kRun], cv[kRun];  // per texel: luma, alpha sample, Cb, Cr
  const bool wide_a = P.wide[va::kAlpha] != 0, whole_a = wide_a && X0 + kRun <= P.w;
  va::load_samples<kTen, kRun>(arow, X0, xc, wide_a, whole_a, As);
  if (kPacked) {
    // UYVY's groups of row yc; kLinear also reads group min(i0 + 4, cw - 1)
    const bool wide = P.wide[0] != 0, whole = wide && i0 + kC <= P.cw;
    uint32_t g[kRun / 2 + 1];
    va::load_groups(row, i0, pc, wide, whole, g);
    g[kRun / 2] = kLinear ? *reinterpret_cast<const uint32_t*>(row + (size_t)last * 4) : 0u;
#pragma unroll
    for (int i = 0; i < kRun; i++) {
      const int k = i >> 1;
      Ys[i] = (i & 1) ? va::group_y1(g[k]) : va::group_y0(g[k]);
      cu[i] = kLinear && (i & 1) ? va::in_chroma_odd_row(va::group_cb(g[k]), va::group_cb(g[k + 1])) : va::group_cb(g[k]);
      cv[i] = kLinear && (i & 1) ? va::in_chroma_odd_row(va::group_cr(g[k]), va::group_cr(g[k + 1])) : va::group_cr(g[k]);
    }
  } else {
    const int j = kFull ? yc : yc >> 1;
    const bool wide_y = P.wide[0] != 0, whole_y = wide_y && X0 + kRun <= P.w;
    const bool wide_b = P.wide[1] != 0, whole_b = wide_b && i0 + kC <= P.cw;
    const bool wide_r = P.wide[2] != 0, whole_r = wide_r && i0 + kC <= P.cw;
    const char* brow = static_cast<const char*>(P.plane[1]) + (int64_t)j * P.pitch[1];
    const char* rrow = static_cast<const char*>(P.plane[2]) + (int64_t)j * P.pitch[2];
    int cb[kC + 1], cr[kC + 1];
    va::load_samples<kTen, kRun>(row, X0, xc, wide_y, whole_y, Ys);
    va::load_samples<kTen, kC>(brow, i0, pc, wide_b, whole_b, cb);
    va::load_samples<kTen, kC>(rrow, i0, pc, wide_r, whole_r, cr);
    if (!kLinear) {
#pragma unroll
      for (int i = 0; i < kRun; i++) { cu[i] = cb[kFull ? i : i >> 1]; cv[i] = cr[kFull ? i : i >> 1]; }
    } else {
      // A420: a second chroma row, the one nearer to the luma row, and one sample more of all four rows
      const int jn = (yc & 1) ? min(j + 1, P.ch - 1) : max(j - 1, 0);
      const char* bfar = static_cast<const char*>(P.plane[1]) + (int64_t)jn * P.pitch[1];
      const char* rfar = static_cast<const char*>(P.plane[2]) + (int64_t)jn * P.pitch[2];
      int fb[kC + 1], fr[kC + 1];
      va::load_samples<kTen, kC>(bfar, i0, pc, wide_b, whole_b, fb);
      va::load_samples<kTen, kC>(rfar, i0, pc, wide_r, whole_r, fr);
      cb[kC] = va::load_sample(brow, last); fb[kC] = va::load_sample(bfar, last);
      cr[kC] = va::load_sample(rrow, last); fr[kC] = va::load_sample(rfar, last);
#pragma unroll
      for (int i = 0; i < kRun; i++) {
        const int k = i >> 1;
        cu[i] = (i & 1) ? va::in_chroma_odd(cb[k], fb[k], cb[k + 1], fb[k + 1]) : va::in_chroma_even(cb[k], fb[k]);
        cv[i] = (i & 1) ? va::in_chroma_odd(cr[k], fr[k], cr[k + 1], fr[k + 1]) : va::in_chroma_even(cr[k], fr[k]);
      }
    }
  }
  uint32_t px[kRun];
#pragma unroll
  for (int i = 0; i < kRun; i++) px[i] = va::in_texel<kStraight>(P, Ys[i], cu[i], cv[i], kTen ? va::in_alpha10(As[i]) : (uint32_t)As[i]);
  // ---- from here on the tile goes k_image_import's way.  Level 0 into the atlas (dword stores: the entry's x need not be a multiple of
  // four) and, as packed words, into LDS
  const bool row_in = Y < P.h;
#pragma unroll
  for (int i = 0; i < kRun; i++) {
    const bool in = row_in && X0 + i < P.w;
    if (in && P.n_store > 0) va::in_store(P.level, P.size, P.x, P.y, 0, X0 + i, Y, px[i]);
    if (!in) px[i] = 0u;
  }
  uint4 run;
  run.x = px[0]; run.y = px[1]; run.z = px[2]; run.w = px[3];
  *reinterpret_cast<uint4*>(tile + r * ii::kTile + c0) = run;
  run.x = px[4]; run.y = px[5]; run.z = px[6]; run.w = px[7];
  *reinterpret_cast<uint4*>(tile + r * ii::kTile + c0 + 4) = run;
  __syncthreads();
  // ---- the ink boxes, first half: 32 lanes take a row of the staged tile each (its words rotated by the row, so that the lanes read 32
  // banks), 32 a column: the largest alpha and the largest colour byte in it
  if (P.ink && lane < 2 * ii::kTile) {
    const int n = lane & (ii::kTile - 1);
    uint32_t a = 0u, c = 0u;
    for (int i = 0; i < ii::kTile; i++) {
      const uint32_t t = lane < ii::kTile ? tile[n * ii::kTile + ((i + n) & (ii::kTile - 1))] : tile[i * ii::kTile + n];
      a = max(a, t >> 24);
      c = max(c, max(t & 255u, max((t >> 8) & 255u, (t >> 16) & 255u)));
    }
    lines[lane] = a | (c << 8);
  }
  // ---- the chain in LDS.  Level l of the tile is (32 >> l)^2 texels at image texel (blockIdx * (32 >> l)); whether a texel has a full
  // 2 x 2 block under it is decided by the IMAGE's extent at level l - 1 (the host derived them), not by the tile.  Level 1 has 256
  // texels: two passes of the 128 lanes.
  int from = 0, side = ii::kTile;
#pragma unroll
  for (int l = 1; l < ii::kTileLevels; l++) {
    const int to = from + side * side, half = side >> 1;
    for (int t = lane; t < half * half; t += va::kInGroup) {
      const int i = t & (half - 1), jj = t / half;
      const int X = (int)blockIdx.x * half + i, Yl = (int)blockIdx.y * half + jj;
      uint32_t o = 0u;
      if (X < P.lw[l] && Yl < P.lh[l]) {
        const uint32_t* s = tile + from + (2 * jj) * side + 2 * i;
        o = va::in_minify(s[0], s[1], s[side], s[side + 1], 2 * X + 1 < P.lw[l - 1], 2 * Yl + 1 < P.lh[l - 1]);
        if (l < P.n_store) va::in_store(P.level, P.size, P.x, P.y, l, X, Yl, o);
        if (l == ii::kTileLevels - 1) P.scratch[(size_t)blockIdx.y * P.lw[l] + blockIdx.x] = o;
      }
      tile[to + jj * half + i] = o;
    }
    __syncthreads();
    // The ink boxes, second half (behind the barrier: `lines` is whole): lane = kind * 32 + k * 4 + {x0, y0, x1, y1} spans the columns or
    // the rows above level 16 k and stores its word of the tile's block -- plain stores into page-locked memory, the block whole.
    if (l == 1 && P.ink && lane < ii::kInkWords) {
      const int kind = lane >> 5, level = 16 * ((lane >> 2) & 7), xy = lane & 1, far = lane & 2;
      const uint32_t* line = lines + (xy ? 0 : ii::kTile);
      int lo = ii::kTile, hi = 0;
      for (int i = 0; i < ii::kTile; i++)
        if ((int)((line[i] >> (8 * kind)) & 255u) > level) { lo = min(lo, i); hi = i + 1; }
      const int origin = (int)(xy ? blockIdx.y : blockIdx.x) * ii::kTile;
      const int word = hi == 0 ? (far ? 0 : ii::kInkEmpty) : origin + (far ? hi : lo);
      P.ink_block[((size_t)blockIdx.y * P.lw[ii::kTileLevels - 1] + blockIdx.x) * ii::kInkWords + lane] = word;
    }
    from = to; side = half;
  }
}

namespace video_alpha {
template <uint32_t kFormat, bool kLinear>
void launch_in(hipStream_t s, dim3 grid, dim3 block, const InParams& P) {
  if (P.flags & kStraightAlpha) FDH_LAUNCH((k_video_alpha_import<kFormat, kLinear, true>), grid, block, 0, s, P);
  else FDH_LAUNCH((k_video_alpha_import<kFormat, kLinear, false>), grid, block, 0, s, P);
}
}  // namespace video_alpha

void launch_video_alpha_import(hipStream_t s, const va::InParams& P) {
  if (P.w <= 0 || P.h <= 0) return;
  const dim3 grid((P.w + ii::kTile - 1) / ii::kTile, (P.h + ii::kTile - 1) / ii::kTile), block(va::kInGroup);
  const bool linear = (P.flags & va::kChromaLinear) != 0;
  if (P.format == va::kA420 && !linear) va::launch_in<va::kA420, false>(s, grid, block, P);
  else if (P.format == va::kA420) va::launch_in<va::kA420, true>(s, grid, block, P);
  else if (P.format == va::kA444) va::launch_in<va::kA444, false>(s, grid, block, P);
  else if (P.format == va::kA410) va::launch_in<va::kA410, false>(s, grid, block, P);
  else if (!linear) va::launch_in<va::kUYVA, false>(s, grid, block, P);
  else va::launch_in<va::kUYVA, true>(s, grid, block, P);
}

}  // namespace fdh
