// k_video_import.hip -- decoded video frames on their way into the atlas: fdh_put_video_frame and fdh_update_video_frame (the
// specification is the comment of include_glyphs/figdraw_hip_video_frame.h; the parameter block is fdh_video_import.h's).  k_video_import
// has k_image_import's tile shape (k_image_import.hip): a workgroup of 256 per 32 x 32 tile of the IMAGE, a lane per run of four texels.
// Only its front is its own: the lane loads its run of the decoder's planes -- four luma samples and the two or three chroma pairs over
// them, or four BGRA texels --, makes the premultiplied RGBA8 texels with the specification's integer expressions, and from there the
// tile goes the way k_image_import's goes: level 0 into the atlas, levels 1 .. 5 through LDS, the last texel into the compact level-5
// image, the ink block.  k_image_import_tail finishes the chain.  The tile body is restated here, not shared: k_image_import.hip and its
// code objects stay as they are.  No float arithmetic anywhere in this unit.
// The batches (fdh_put_video_frames, fdh_update_video_frames; include_glyphs/figdraw_hip_video_frames.h): k_video_import_batch<format, linear>
// runs video_batch_tile over a table of tiles and a record per frame (vi::BatchFrame), and stores into level ii::kOwnerLevel or deeper only
// where the frame's owner bit is set; k_image_import_tail_batch finishes the chains.
#include "fdh_device.h"
#include "fdh_video_import.h"

namespace fdh {
namespace vi = video_import;
namespace ii = image_import;

namespace video_import {

// ---- the conversion, once.  int32 throughout; >> of a negative sum is an arithmetic shift (floor).
// clamp(sum >> 14, 0, 255), written as the clamp of the sum in front of the shift, which is the same number.  In the other order the
// compiler packs two channels with v_ashr_pk_u8_i32 and takes the upper half of its destination for zero; on the MI355X that half keeps
// what the register held (here: bits 16 .. 31 of the green sum, which then were ORed into blue).  tools/lint_isa.py refuses the opcode.
__device__ __forceinline__ uint32_t shift_clamp(int sum) { return (uint32_t)min(max(sum, 0), (256 << 14) - 1) >> 14; }
// Y, Cb, Cr samples (b bits each) -> the texel R | G << 8 | B << 16 | 255 << 24
__device__ __forceinline__ uint32_t yuv_texel(const Params& P, int Y, int cb, int cr) {
  const int y = P.cy * (Y - P.yoff) + 8192, u = cb - P.coff, v = cr - P.coff;
  const uint32_t r = shift_clamp(y + P.crv * v);
  const uint32_t g = shift_clamp(y - P.cgu * u - P.cgv * v);
  const uint32_t b = shift_clamp(y + P.cbu * u);
  return r | (g << 8) | (b << 16) | 0xFF000000u;
}
// FDH_VIDEO_CHROMA_LINEAR, one component: near / far = the samples of pair i in chroma rows j / jn, near1 / far1 those of pair
// min(i + 1, cw - 1).  Even luma columns lie on pair i, odd ones midway to the next.
__device__ __forceinline__ int chroma_even(int near, int far) { return (3 * near + far + 2) >> 2; }
__device__ __forceinline__ int chroma_odd(int near, int far, int near1, int far1) { return (3 * near + far + 3 * near1 + far1 + 4) >> 3; }
// the bytes B, G, R, A -> the texel; kIgnoreAlpha: A = 255; kStraightAlpha: each colour byte becomes (c * a) / 255 (put_flippy's rule)
__device__ __forceinline__ uint32_t bgra_texel(uint32_t t, uint32_t flags) {
  uint32_t b = t & 255u, g = (t >> 8) & 255u, r = (t >> 16) & 255u, a = t >> 24;
  if (flags & kIgnoreAlpha) a = 255u;
  if (flags & kStraightAlpha) { r = r * a / 255u; g = g * a / 255u; b = b * a / 255u; }
  return r | (g << 8) | (b << 16) | (a << 24);
}

// ---- the loads.  As in k_image_import: `wide` -- pointer and pitch allow one load of the run, and the plane has a whole run --, every
// lane issues that one load, its own run where that lies inside the plane (`whole`), the row's first where it does not; such a lane then
// loads element by element at clamped columns, as every lane does without `wide`.
// Four luma samples at columns x0 .. x0 + 3 (xc[]: clamped) of the row at `row`
template <uint32_t kFormat>
__device__ __forceinline__ void load_luma(const char* row, int x0, const int xc[4], bool wide, bool whole, int out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  if (kFormat == kNv12) {
    if (wide) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(row + (size_t)(whole ? x0 : 0));
      out[0] = (int)(v & 255u); out[1] = (int)((v >> 8) & 255u); out[2] = (int)((v >> 16) & 255u); out[3] = (int)(v >> 24);
    }
    if (!whole) {
#pragma unroll
      for (int i = 0; i < 4; i++) out[i] = (int)*reinterpret_cast<const uint8_t*>(row + (size_t)xc[i]);
    }
  } else {
    if (wide) {
      const uint2 v = *reinterpret_cast<const uint2*>(row + (size_t)(whole ? x0 : 0) * 2);
      out[0] = (int)((v.x & 0xFFFFu) >> 6); out[1] = (int)(v.x >> 22); out[2] = (int)((v.y & 0xFFFFu) >> 6); out[3] = (int)(v.y >> 22);
    }
    if (!whole) {
#pragma unroll
      for (int i = 0; i < 4; i++) out[i] = (int)(*reinterpret_cast<const uint16_t*>(row + (size_t)xc[i] * 2) >> 6);
    }
  }
}
// kPairs (2 or 3) chroma pairs of the row at `row`: pairs i0 and i0 + 1 are the wide load, a third (FDH_VIDEO_CHROMA_LINEAR) is a load
// of its own; pc[]: the pairs' columns, clamped
template <uint32_t kFormat, int kPairs>
__device__ __forceinline__ void load_chroma(const char* row, int i0, const int pc[3], bool wide, bool whole, int cb[3], int cr[3]) {
  uint32_t p[3] = {0u, 0u, 0u};  // a pair as Cb | Cr << 16, samples of b bits
  if (kFormat == kNv12) {
    if (wide) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(row + (size_t)(whole ? i0 : 0) * 2);
      p[0] = (v & 255u) | ((v & 0xFF00u) << 8); p[1] = ((v >> 16) & 255u) | ((v >> 24) << 16);
    }
#pragma unroll
    for (int k = 0; k < kPairs; k++)
      if (k == 2 || !whole) {
        const uint32_t v = *reinterpret_cast<const uint16_t*>(row + (size_t)pc[k] * 2);
        p[k] = (v & 255u) | ((v >> 8) << 16);
      }
  } else {
    if (wide) {
      const uint2 v = *reinterpret_cast<const uint2*>(row + (size_t)(whole ? i0 : 0) * 4);
      p[0] = (v.x >> 6) & 0x03FF03FFu; p[1] = (v.y >> 6) & 0x03FF03FFu;
    }
#pragma unroll
    for (int k = 0; k < kPairs; k++)
      if (k == 2 || !whole) p[k] = (*reinterpret_cast<const uint32_t*>(row + (size_t)pc[k] * 4) >> 6) & 0x03FF03FFu;
  }
#pragma unroll
  for (int k = 0; k < kPairs; k++) { cb[k] = (int)(p[k] & 0xFFFFu); cr[k] = (int)(p[k] >> 16); }
}
__device__ __forceinline__ void load_bgra(const char* row, int x0, const int xc[4], bool wide, bool whole, uint32_t out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0u;
  if (wide) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + (size_t)(whole ? x0 : 0) * 4);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  }
  if (!whole) {
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = *reinterpret_cast<const uint32_t*>(row + (size_t)xc[i] * 4);
  }
}

// ---- the tile body's two steps, as k_image_import.hip has them (import_minify, import_store).
// One texel of minify_by2_host: a, b = the texels (2x, 2y), (2x + 1, 2y), c, d = those of the row below; col_pair / row_pair: the source
// has column 2x + 1 / row 2y + 1.  Where it has not, `a` is its last column / row.
__device__ __forceinline__ uint32_t minify(uint32_t a, uint32_t b, uint32_t c, uint32_t d, bool col_pair, bool row_pair) {
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
__device__ __forceinline__ void store(uint32_t* const* level, int size, int x, int y, int l, int i, int j, uint32_t texel) {
  const int LS = size >> l, tx = (x >> l) + i, ty = (y >> l) + j;
  if (tx >= 0 && ty >= 0 && tx < LS && ty < LS) level[l][(size_t)ty * LS + tx] = texel;
}

// LDS of a tile: the levels one after the other, 32 x 32, 16 x 16, .. 1 (no level is written twice)
constexpr int kTileWords = 1024 + 256 + 64 + 16 + 4 + 1;

}  // namespace video_import

template <uint32_t kFormat, bool kLinear>
__global__ __launch_bounds__(ii::kGroup) void k_video_import(const vi::Params P) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[vi::kTileWords + 3];
  __shared__ uint32_t lines[2 * ii::kTile];  // per row of the tile, then per column: the largest alpha | the largest colour byte << 8
  const int lane = (int)threadIdx.x;
  const int r = lane >> 3, c0 = (lane & 7) * 4;  // a wave covers eight whole rows of the tile
  const int X0 = (int)blockIdx.x * ii::kTile + c0, Y = (int)blockIdx.y * ii::kTile + r;
  // ---- the loads.  Every address is valid -- rows, columns and pairs clamped into their plane -- and what lies outside the image is
  // replaced behind the conversion: no load waits for a branch on the texel's place, and all of a lane's loads go out before the first
  // conversion.
  const int yc = min(Y, P.h - 1);
  int xc[4];
#pragma unroll
  for (int i = 0; i < 4; i++) xc[i] = min(X0 + i, P.w - 1);
  const bool wide = P.wide_y != 0, whole = wide && X0 + 4 <= P.w;
  const char* row = static_cast<const char*>(P.luma) + (int64_t)yc * P.pitch_y;
  uint32_t px[4];
  if (kFormat == vi::kBgra8) {
    uint32_t t[4];
    vi::load_bgra(row, X0, xc, wide, whole, t);
#pragma unroll
    for (int i = 0; i < 4; i++) px[i] = vi::bgra_texel(t[i], P.flags);
  } else {
    // the run's luma columns X0 .. X0 + 3 lie over the pairs i0 and i0 + 1; kLinear also reads min(i0 + 2, cw - 1), and a second row
    const int i0 = X0 >> 1, j = yc >> 1;
    int pc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) pc[k] = min(i0 + k, P.cw - 1);
    const bool wide_c = P.wide_c != 0, whole_c = wide_c && i0 + 2 <= P.cw;
    const char* crow = static_cast<const char*>(P.chroma) + (int64_t)j * P.pitch_c;
    int Ys[4], cb[3], cr[3];
    vi::load_luma<kFormat>(row, X0, xc, wide, whole, Ys);
    if (!kLinear) {
      vi::load_chroma<kFormat, 2>(crow, i0, pc, wide_c, whole_c, cb, cr);
#pragma unroll
      for (int i = 0; i < 4; i++) px[i] = vi::yuv_texel(P, Ys[i], cb[i >> 1], cr[i >> 1]);
    } else {
      const int jn = (yc & 1) ? min(j + 1, P.ch - 1) : max(j - 1, 0);
      const char* nrow = static_cast<const char*>(P.chroma) + (int64_t)jn * P.pitch_c;
      int fb[3], fr[3];
      vi::load_chroma<kFormat, 3>(crow, i0, pc, wide_c, whole_c, cb, cr);
      vi::load_chroma<kFormat, 3>(nrow, i0, pc, wide_c, whole_c, fb, fr);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int k = i >> 1;
        const int u = (i & 1) ? vi::chroma_odd(cb[k], fb[k], cb[k + 1], fb[k + 1]) : vi::chroma_even(cb[k], fb[k]);
        const int v = (i & 1) ? vi::chroma_odd(cr[k], fr[k], cr[k + 1], fr[k + 1]) : vi::chroma_even(cr[k], fr[k]);
        px[i] = vi::yuv_texel(P, Ys[i], u, v);
      }
    }
  }
  // ---- from here on the tile goes k_image_import's way.  Level 0 into the atlas (dword stores: the entry's x need not be a multiple of
  // four) and, as packed words, into LDS
  const bool row_in = Y < P.h;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const bool in = row_in && X0 + i < P.w;
    if (in && P.n_store > 0) vi::store(P.level, P.size, P.x, P.y, 0, X0 + i, Y, px[i]);
    if (!in) px[i] = 0u;
  }
  uint4 run;
  run.x = px[0]; run.y = px[1]; run.z = px[2]; run.w = px[3];
  *reinterpret_cast<uint4*>(tile + r * ii::kTile + c0) = run;
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
  // 2 x 2 block under it is decided by the IMAGE's extent at level l - 1 (the host derived them), not by the tile.
  int from = 0, side = ii::kTile;
#pragma unroll
  for (int l = 1; l < ii::kTileLevels; l++) {
    const int to = from + side * side, half = side >> 1;
    if (lane < half * half) {
      const int i = lane & (half - 1), jj = lane / half;
      const int X = (int)blockIdx.x * half + i, Yl = (int)blockIdx.y * half + jj;
      uint32_t o = 0u;
      if (X < P.lw[l] && Yl < P.lh[l]) {
        const uint32_t* s = tile + from + (2 * jj) * side + 2 * i;
        o = vi::minify(s[0], s[1], s[side], s[side + 1], 2 * X + 1 < P.lw[l - 1], 2 * Yl + 1 < P.lh[l - 1]);
        if (l < P.n_store) vi::store(P.level, P.size, P.x, P.y, l, X, Yl, o);
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

// ---- the batches (fdh_put_video_frames, fdh_update_video_frames; include_glyphs/figdraw_hip_video_frames.h).
// May level l's texel of a frame of a batch be stored?  k_image_import.hip's import_owns: `owner` holds, from bit `bit0` on, a bit per
// texel of the frame's levels ii::kOwnerLevel .., rows packed, set where the texel is still this frame's after the host painted the
// batch's rectangles in array order (fdh_video_batch.h).
__device__ __forceinline__ bool video_owns(const uint32_t* owner, uint32_t bit0, uint32_t bit) {
  bit += bit0;
  return (owner[bit >> 5] >> (bit & 31u)) & 1u;
}

// The body of a tile of a batch: tile (bx, by) of the frame P describes, staged in `tile` (vi::kTileWords + 3 words of LDS, 16-byte
// aligned) with `lines` (2 * ii::kTile words of LDS), with the owner bits of its frame.  It is k_video_import's body statement for
// statement -- the loads, the conversion, the chain and the ink block come from the functions above, which both call -- but for the tile's
// place, which is an argument here, and the owner bits in front of a store into level ii::kOwnerLevel or deeper.  It is a second statement
// and not a shared one because k_video_import, handed its own body as a function of its parameter block, is compiled to other code (20
// more SGPRs in all five builds; profiles/video_frame_batch.txt), and the single calls keep the code they were measured with.
template <uint32_t kFormat, bool kLinear>
__device__ __forceinline__ void video_batch_tile(const vi::Params& P, const int bx, const int by, const uint32_t* owner, const uint32_t owner_bit0, uint32_t* tile, uint32_t* lines) {
  const int lane = (int)threadIdx.x;
  const int r = lane >> 3, c0 = (lane & 7) * 4;  // a wave covers eight whole rows of the tile
  const int X0 = bx * ii::kTile + c0, Y = by * ii::kTile + r;
  // ---- the loads.  Every address is valid -- rows, columns and pairs clamped into their plane -- and what lies outside the image is
  // replaced behind the conversion: no load waits for a branch on the texel's place, and all of a lane's loads go out before the first
  // conversion.
  const int yc = min(Y, P.h - 1);
  int xc[4];
#pragma unroll
  for (int i = 0; i < 4; i++) xc[i] = min(X0 + i, P.w - 1);
  const bool wide = P.wide_y != 0, whole = wide && X0 + 4 <= P.w;
  const char* row = static_cast<const char*>(P.luma) + (int64_t)yc * P.pitch_y;
  uint32_t px[4];
  if (kFormat == vi::kBgra8) {
    uint32_t t[4];
    vi::load_bgra(row, X0, xc, wide, whole, t);
#pragma unroll
    for (int i = 0; i < 4; i++) px[i] = vi::bgra_texel(t[i], P.flags);
  } else {
    // the run's luma columns X0 .. X0 + 3 lie over the pairs i0 and i0 + 1; kLinear also reads min(i0 + 2, cw - 1), and a second row
    const int i0 = X0 >> 1, j = yc >> 1;
    int pc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) pc[k] = min(i0 + k, P.cw - 1);
    const bool wide_c = P.wide_c != 0, whole_c = wide_c && i0 + 2 <= P.cw;
    const char* crow = static_cast<const char*>(P.chroma) + (int64_t)j * P.pitch_c;
    int Ys[4], cb[3], cr[3];
    vi::load_luma<kFormat>(row, X0, xc, wide, whole, Ys);
    if (!kLinear) {
      vi::load_chroma<kFormat, 2>(crow, i0, pc, wide_c, whole_c, cb, cr);
#pragma unroll
      for (int i = 0; i < 4; i++) px[i] = vi::yuv_texel(P, Ys[i], cb[i >> 1], cr[i >> 1]);
    } else {
      const int jn = (yc & 1) ? min(j + 1, P.ch - 1) : max(j - 1, 0);
      const char* nrow = static_cast<const char*>(P.chroma) + (int64_t)jn * P.pitch_c;
      int fb[3], fr[3];
      vi::load_chroma<kFormat, 3>(crow, i0, pc, wide_c, whole_c, cb, cr);
      vi::load_chroma<kFormat, 3>(nrow, i0, pc, wide_c, whole_c, fb, fr);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int k = i >> 1;
        const int u = (i & 1) ? vi::chroma_odd(cb[k], fb[k], cb[k + 1], fb[k + 1]) : vi::chroma_even(cb[k], fb[k]);
        const int v = (i & 1) ? vi::chroma_odd(cr[k], fr[k], cr[k + 1], fr[k + 1]) : vi::chroma_even(cr[k], fr[k]);
        px[i] = vi::yuv_texel(P, Ys[i], u, v);
      }
    }
  }
  // ---- from here on the tile goes k_image_import's way.  Level 0 into the atlas (dword stores: the entry's x need not be a multiple of
  // four) and, as packed words, into LDS
  const bool row_in = Y < P.h;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const bool in = row_in && X0 + i < P.w;
    if (in && P.n_store > 0) vi::store(P.level, P.size, P.x, P.y, 0, X0 + i, Y, px[i]);
    if (!in) px[i] = 0u;
  }
  uint4 run;
  run.x = px[0]; run.y = px[1]; run.z = px[2]; run.w = px[3];
  *reinterpret_cast<uint4*>(tile + r * ii::kTile + c0) = run;
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
  // 2 x 2 block under it is decided by the IMAGE's extent at level l - 1 (the host derived them), not by the tile.
  int from = 0, side = ii::kTile;
  uint32_t level_bit = 0u;  // the first owner bit of level l, behind the frame's own first
#pragma unroll
  for (int l = 1; l < ii::kTileLevels; l++) {
    const int to = from + side * side, half = side >> 1;
    if (lane < half * half) {
      const int i = lane & (half - 1), jj = lane / half;
      const int X = bx * half + i, Yl = by * half + jj;
      uint32_t o = 0u;
      if (X < P.lw[l] && Yl < P.lh[l]) {
        const uint32_t* s = tile + from + (2 * jj) * side + 2 * i;
        o = vi::minify(s[0], s[1], s[side], s[side + 1], 2 * X + 1 < P.lw[l - 1], 2 * Yl + 1 < P.lh[l - 1]);
        if (l < P.n_store && (l < ii::kOwnerLevel || video_owns(owner, owner_bit0, level_bit + (uint32_t)(Yl * P.lw[l] + X)))) vi::store(P.level, P.size, P.x, P.y, l, X, Yl, o);
        if (l == ii::kTileLevels - 1) P.scratch[(size_t)by * P.lw[l] + bx] = o;
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
      const int origin = (xy ? by : bx) * ii::kTile;
      const int word = hi == 0 ? (far ? 0 : ii::kInkEmpty) : origin + (far ? hi : lo);
      P.ink_block[((size_t)by * P.lw[ii::kTileLevels - 1] + bx) * ii::kInkWords + lane] = word;
    }
    if (l >= ii::kOwnerLevel) level_bit += (uint32_t)(P.lw[l] * P.lh[l]);
    from = to; side = half;
  }
}

// The batch: a 1-D grid over the tile words of one group of a batch (vi::batch_group: BGRA8, or NV12 / P010 without or with
// FDH_VIDEO_CHROMA_LINEAR).  The frame's index comes from the block index alone, so every read of its record is wave-uniform and the body's
// branches on `wide_y`, `wide_c`, the flags and `ink` stay uniform.  The record is read whole before the first store, into the single
// kernel's parameter block.  A frame 1 texel wide or high has its tiles here (n_store == 0: nothing of it is stored, its ink blocks are).
template <uint32_t kFormat, bool kLinear>
__global__ __launch_bounds__(ii::kGroup) void k_video_import_batch(const vi::BatchFrame* __restrict__ frames, const uint32_t* __restrict__ tiles, const ii::BatchAtlas A,
                                                                   uint32_t* scratch, int32_t* ink_blocks, const uint32_t* __restrict__ owner) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[vi::kTileWords + 3];
  __shared__ uint32_t lines[2 * ii::kTile];
  const uint32_t word = tiles[blockIdx.x];
  const vi::BatchFrame& F = frames[word & 0xFFFFu];
  vi::Params P;
  P.luma = F.luma; P.chroma = F.chroma; P.pitch_y = F.pitch_y; P.pitch_c = F.pitch_c;
  P.w = F.w; P.h = F.h; P.cw = F.cw; P.ch = F.ch;
  P.format = kFormat; P.flags = F.flags; P.wide_y = F.wide_y; P.wide_c = F.wide_c;
  P.yoff = F.yoff; P.coff = F.coff; P.cy = F.cy; P.crv = F.crv; P.cgu = F.cgu; P.cgv = F.cgv; P.cbu = F.cbu;
  P.x = F.x; P.y = F.y; P.n_store = F.n_store; P.ink = F.ink;
#pragma unroll
  for (int l = 0; l < ii::kTileLevels; l++) { P.lw[l] = F.lw[l]; P.lh[l] = F.lh[l]; }
#pragma unroll
  for (int l = 0; l < ii::kLevels; l++) P.level[l] = A.level[l];
  P.size = A.size;
  P.scratch = scratch + F.scratch_off;
  P.ink_block = ink_blocks + (size_t)F.ink_off * ii::kInkWords;
  video_batch_tile<kFormat, kLinear>(P, (int)((word >> 16) & 63u), (int)(word >> 22), owner, F.owner_off, tile, lines);
}

void launch_video_import(hipStream_t s, const vi::Params& P) {
  if (P.w <= 0 || P.h <= 0) return;
  const dim3 grid((P.w + ii::kTile - 1) / ii::kTile, (P.h + ii::kTile - 1) / ii::kTile), block(ii::kGroup);
  const bool linear = (P.flags & vi::kChromaLinear) != 0;
  if (P.format == vi::kBgra8) FDH_LAUNCH((k_video_import<vi::kBgra8, false>), grid, block, 0, s, P);
  else if (P.format == vi::kNv12 && !linear) FDH_LAUNCH((k_video_import<vi::kNv12, false>), grid, block, 0, s, P);
  else if (P.format == vi::kNv12) FDH_LAUNCH((k_video_import<vi::kNv12, true>), grid, block, 0, s, P);
  else if (!linear) FDH_LAUNCH((k_video_import<vi::kP010, false>), grid, block, 0, s, P);
  else FDH_LAUNCH((k_video_import<vi::kP010, true>), grid, block, 0, s, P);
}

// the batch's launch of one group (vi::batch_group): n_tiles tiles, their words at `tiles`
void launch_video_import_batch(hipStream_t s, int group, const vi::BatchFrame* frames, const uint32_t* tiles, int n_tiles, const ii::BatchAtlas& A, uint32_t* scratch, int32_t* ink_blocks,
                               const uint32_t* owner) {
  if (n_tiles <= 0) return;
  const dim3 grid(n_tiles), block(ii::kGroup);
  if (group == 0) FDH_LAUNCH((k_video_import_batch<vi::kBgra8, false>), grid, block, 0, s, frames, tiles, A, scratch, ink_blocks, owner);
  else if (group == 1) FDH_LAUNCH((k_video_import_batch<vi::kNv12, false>), grid, block, 0, s, frames, tiles, A, scratch, ink_blocks, owner);
  else if (group == 2) FDH_LAUNCH((k_video_import_batch<vi::kNv12, true>), grid, block, 0, s, frames, tiles, A, scratch, ink_blocks, owner);
  else if (group == 3) FDH_LAUNCH((k_video_import_batch<vi::kP010, false>), grid, block, 0, s, frames, tiles, A, scratch, ink_blocks, owner);
  else FDH_LAUNCH((k_video_import_batch<vi::kP010, true>), grid, block, 0, s, frames, tiles, A, scratch, ink_blocks, owner);
}

}  // namespace fdh
