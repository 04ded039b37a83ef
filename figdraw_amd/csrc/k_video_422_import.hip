// k_video_422_import.hip -- 4:2:2 video frames on their way into the atlas: fdh_put_video_422 and fdh_update_video_422 (the specification
// is the comment of include_video/figdraw_hip_video_422.h; the parameter block is fdh_video_422.h's InParams).  I422 and I210 (three
// planes, a chroma row per luma row) and YUY2 and UYVY (one plane of four-byte groups).  k_video_422_import has k_video_planar_import's
// shape (k_video_planar_import.hip), which is k_image_import's tile (k_image_import.hip): a 32 x 32 tile of the IMAGE per workgroup of 128,
// a lane per run of EIGHT texels of one row, four runs across the tile and 32 rows down; level 0 into the atlas, levels 1 .. 5 through
// LDS, the last texel into the compact level-5 image, the ink block; k_image_import_tail finishes the chain.  A planar lane loads its
// eight luma samples and the four Cb and four Cr samples of the same row -- 8 + 4 + 4 bytes for I422, twice that for I210: its narrowest
// access is four bytes --, a packed lane its four groups as one 16-byte access.  The FDH_VIDEO_CHROMA_LINEAR builds take one more sample
// of either plane, or one more group, at min(i0 + 4, cw - 1): the neighbour to the right of the run's last chroma sample; there is no
// second chroma row, 4:2:2 interpolates along the row alone.  The tile body is restated here, not shared, as k_video_planar_import.hip
// restated it: the existing kernel units and their code objects stay as they are.  No float arithmetic anywhere in this unit.
#include "fdh_device.h"
#include "fdh_video_422.h"

namespace fdh {
namespace v2 = video_422;
namespace ii = image_import;

namespace video_422 {

// ---- the conversion, once.  int32 throughout; >> of a negative sum is an arithmetic shift (floor).
// clamp(sum >> 14, 0, 255), written as the clamp of the sum in front of the shift, which is the same number.  In the other order the
// compiler packs two channels with an instruction that takes the upper half of its destination for zero where the MI355X keeps what the
// register held (k_video_import.hip, shift_clamp, has the whole story); tools/lint_isa.py refuses the opcode.
__device__ __forceinline__ uint32_t in_shift_clamp(int sum) { return (uint32_t)min(max(sum, 0), (256 << 14) - 1) >> 14; }
// Y, Cb, Cr samples (b bits each) -> the texel R | G << 8 | B << 16 | 255 << 24
__device__ __forceinline__ uint32_t in_texel(const InParams& P, int Y, int cb, int cr) {
  const int y = P.cy * (Y - P.yoff) + 8192, u = cb - P.coff, v = cr - P.coff;
  const uint32_t r = in_shift_clamp(y + P.crv * v);
  const uint32_t g = in_shift_clamp(y - P.cgu * u - P.cgv * v);
  const uint32_t b = in_shift_clamp(y + P.cbu * u);
  return r | (g << 8) | (b << 16) | 0xFF000000u;
}
// FDH_VIDEO_CHROMA_LINEAR, an odd luma column: midway between sample i (`near`) and sample min(i + 1, cw - 1) (`next`) of its own row.
// Even columns lie on sample i.
__device__ __forceinline__ int in_chroma_odd(int near, int next) { return (near + next + 1) >> 1; }

// ---- the loads.  As in k_video_planar_import: `wide` -- pointer and pitch allow one load of the run, and the row has a whole run --,
// every lane issues that one load, its own run where that lies inside the row (`whole`), the row's first where it does not; such a lane
// then loads element by element at clamped columns, as every lane does without `wide`.
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
// one sample more, at the clamped column c (FDH_VIDEO_CHROMA_LINEAR: the sample right of the run's four)
template <bool kTen>
__device__ __forceinline__ int load_sample(const char* row, int c) {
  if (kTen) return (int)(*reinterpret_cast<const uint16_t*>(row + (size_t)c * 2) & 1023u);
  return (int)*reinterpret_cast<const uint8_t*>(row + (size_t)c);
}
// a packed row's four groups g0 .. g0 + 3 (gc[]: clamped), a group a 32-bit word: one 16-byte load, or four 4-byte loads
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
// a group's four bytes; order 0: Y0 Cb Y1 Cr, order 1: Cb Y0 Cr Y1 -- s = 8 * order
__device__ __forceinline__ int group_y0(uint32_t g, int s) { return (int)((g >> s) & 255u); }
__device__ __forceinline__ int group_y1(uint32_t g, int s) { return (int)((g >> (16 + s)) & 255u); }
__device__ __forceinline__ int group_cb(uint32_t g, int s) { return (int)((g >> (8 - s)) & 255u); }
__device__ __forceinline__ int group_cr(uint32_t g, int s) { return (int)((g >> (24 - s)) & 255u); }

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

}  // namespace video_422

// kTen: I210; kPacked: YUY2 / UYVY (P.order says which); kLinear: FDH_VIDEO_CHROMA_LINEAR
template <bool kTen, bool kPacked, bool kLinear>
__global__ __launch_bounds__(v2::kInGroup) void k_video_422_import(const v2::InParams P) {
  static_assert(!(kTen && kPacked), "the packed formats are 8 bit");
  __shared__ __attribute__((aligned(16))) uint32_t tile[v2::kInTileWords + 3];
  __shared__ uint32_t lines[2 * ii::kTile];  // per row of the tile, then per column: the largest alpha | the largest colour byte << 8
  constexpr int kRun = v2::kRun, kC = kRun / 2;  // chroma samples of either kind, and groups, that go with a run
  const int lane = (int)threadIdx.x;
  const int r = lane >> 2, c0 = (lane & 3) * kRun;  // a wave covers sixteen whole rows of the tile
  const int X0 = (int)blockIdx.x * ii::kTile + c0, Y = (int)blockIdx.y * ii::kTile + r;
  // ---- the loads.  Every address is valid -- the row, columns, samples and groups clamped into their plane -- and what lies outside the
  // image is replaced behind the conversion: no load waits for a branch on the texel's place, and all of a lane's loads go out before
  // the first conversion.  The run's luma columns X0 .. X0 + 7 lie over the chroma samples (the groups) i0 .. i0 + 3 of the SAME row;
  // kLinear also reads min(i0 + 4, cw - 1).
  const int yc = min(Y, P.h - 1), i0 = X0 >> 1, last = min(i0 + kC, P.cw - 1);
  int pc[kC];
#pragma unroll
  for (int k = 0; k < kC; k++) pc[k] = min(i0 + k, P.cw - 1);
  int Ys[kRun], cb[kC + 1], cr[kC + 1];
  uint32_t px[kRun];
  const char* row = static_cast<const char*>(P.plane[0]) + (int64_t)yc * P.pitch[0];
  if (kPacked) {
    const bool wide = P.wide[0] != 0, whole = wide && i0 + kC <= P.cw;
    uint32_t g[kC + 1];
    v2::load_groups(row, i0, pc, wide, whole, g);
    g[kC] = kLinear ? *reinterpret_cast<const uint32_t*>(row + (size_t)last * 4) : 0u;
    const int s = P.order ? 8 : 0;
#pragma unroll
    for (int k = 0; k < kC; k++) { Ys[2 * k] = v2::group_y0(g[k], s); Ys[2 * k + 1] = v2::group_y1(g[k], s); }
#pragma unroll
    for (int k = 0; k <= kC; k++) { cb[k] = v2::group_cb(g[k], s); cr[k] = v2::group_cr(g[k], s); }
  } else {
    int xc[kRun];
#pragma unroll
    for (int i = 0; i < kRun; i++) xc[i] = min(X0 + i, P.w - 1);
    const bool wide_y = P.wide[0] != 0, whole_y = wide_y && X0 + kRun <= P.w;
    const bool wide_b = P.wide[1] != 0, whole_b = wide_b && i0 + kC <= P.cw;
    const bool wide_r = P.wide[2] != 0, whole_r = wide_r && i0 + kC <= P.cw;
    const char* brow = static_cast<const char*>(P.plane[1]) + (int64_t)yc * P.pitch[1];
    const char* rrow = static_cast<const char*>(P.plane[2]) + (int64_t)yc * P.pitch[2];
    v2::load_samples<kTen, kRun>(row, X0, xc, wide_y, whole_y, Ys);
    v2::load_samples<kTen, kC>(brow, i0, pc, wide_b, whole_b, cb);
    v2::load_samples<kTen, kC>(rrow, i0, pc, wide_r, whole_r, cr);
    cb[kC] = kLinear ? v2::load_sample<kTen>(brow, last) : 0;
    cr[kC] = kLinear ? v2::load_sample<kTen>(rrow, last) : 0;
  }
#pragma unroll
  for (int i = 0; i < kRun; i++) {
    const int k = i >> 1;
    const int u = kLinear && (i & 1) ? v2::in_chroma_odd(cb[k], cb[k + 1]) : cb[k];
    const int v = kLinear && (i & 1) ? v2::in_chroma_odd(cr[k], cr[k + 1]) : cr[k];
    px[i] = v2::in_texel(P, Ys[i], u, v);
  }
  // ---- from here on the tile goes k_image_import's way.  Level 0 into the atlas (dword stores: the entry's x need not be a multiple of
  // four) and, as packed words, into LDS
  const bool row_in = Y < P.h;
#pragma unroll
  for (int i = 0; i < kRun; i++) {
    const bool in = row_in && X0 + i < P.w;
    if (in && P.n_store > 0) v2::in_store(P.level, P.size, P.x, P.y, 0, X0 + i, Y, px[i]);
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
    for (int t = lane; t < half * half; t += v2::kInGroup) {
      const int i = t & (half - 1), jj = t / half;
      const int X = (int)blockIdx.x * half + i, Yl = (int)blockIdx.y * half + jj;
      uint32_t o = 0u;
      if (X < P.lw[l] && Yl < P.lh[l]) {
        const uint32_t* s = tile + from + (2 * jj) * side + 2 * i;
        o = v2::in_minify(s[0], s[1], s[side], s[side + 1], 2 * X + 1 < P.lw[l - 1], 2 * Yl + 1 < P.lh[l - 1]);
        if (l < P.n_store) v2::in_store(P.level, P.size, P.x, P.y, l, X, Yl, o);
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

void launch_video_422_import(hipStream_t s, const v2::InParams& P) {
  if (P.w <= 0 || P.h <= 0) return;
  const dim3 grid((P.w + ii::kTile - 1) / ii::kTile, (P.h + ii::kTile - 1) / ii::kTile), block(v2::kInGroup);
  const bool linear = (P.flags & v2::kChromaLinear) != 0;
  if (P.format == v2::kI422 && !linear) FDH_LAUNCH((k_video_422_import<false, false, false>), grid, block, 0, s, P);
  else if (P.format == v2::kI422) FDH_LAUNCH((k_video_422_import<false, false, true>), grid, block, 0, s, P);
  else if (P.format == v2::kI210 && !linear) FDH_LAUNCH((k_video_422_import<true, false, false>), grid, block, 0, s, P);
  else if (P.format == v2::kI210) FDH_LAUNCH((k_video_422_import<true, false, true>), grid, block, 0, s, P);
  else if (!linear) FDH_LAUNCH((k_video_422_import<false, true, false>), grid, block, 0, s, P);
  else FDH_LAUNCH((k_video_422_import<false, true, true>), grid, block, 0, s, P);
}

}  // namespace fdh
