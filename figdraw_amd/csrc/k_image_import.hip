// k_image_import.hip -- images from device memory on their way into the atlas: fdh_put_image_device and fdh_update_image_device (the
// specification is the comment of include_glyphs/figdraw_hip_device_image.h; the parameter blocks are fdh_image_import.h's).  k_image_import:
// a workgroup of 256 per 32 x 32 tile of the IMAGE -- the tile grid starts at the image's own origin, so a tile owns whole 2^k blocks of
// the level chain.  A lane loads a run of four texels, converts them to the premultiplied RGBA8 texel, stores level 0 and stages the tile
// in LDS; the tile is then minified there to 16 x 16, 8 x 8, 4 x 4, 2 x 2 and one texel with minify_by2_host's integer rule (fdh_atlas.cpp),
// each block stored to its atlas level on the way, and the last texel goes into a compact level-5 image.  k_image_import_tail: one
// workgroup takes that image (at most 64 x 64) through the rest of the chain in LDS.  Two launches where glyph_to_atlas issues two a level.
// The batches (fdh_put_images_device, fdh_update_images_device; include_glyphs/figdraw_hip_device_images.h): k_image_import_batch<format> and
// k_image_import_tail_batch run the same two bodies -- import_tile, import_tail: one statement of the conversion and of the chain -- over a
// table of tiles and a record per image, and store into level kOwnerLevel or deeper only where the image's owner bit is set.
#include "fdh_device.h"
#include "fdh_image_import.h"

namespace fdh {
namespace ii = image_import;

// an IEEE half, as its 16 bits, widened to float (exact)
#ifndef FDH_IMPORT_HALF_TO_FLOAT
#define FDH_IMPORT_HALF_TO_FLOAT(bits) ((float)__builtin_bit_cast(_Float16, (uint16_t)(bits)))
#endif

// A planar value as the texel's byte: NaN gives 0, any other value rint(min(max(v, 0), 1) * 255) in float32, ties to even.
// The device build is compiled with -fno-honor-nans: `v != v` is false by decree there and the min / max may hand a NaN on or not.  So NaN
// is recognised on the bit pattern, with an integer compare, and the byte chosen behind the arithmetic.
__device__ __forceinline__ uint32_t import_byte(float v) {
#pragma clang fp contract(off)
  const uint32_t bits = __builtin_bit_cast(uint32_t, v);
  const bool nan = (bits & 0x7FFFFFFFu) > 0x7F800000u;
  const float c = fminf(fmaxf(nan ? 0.0f : v, 0.0f), 1.0f);
  return (uint32_t)rintf(c * 255.0f);
}
// R, G, B, A bytes -> the texel; FDH_IMAGE_STRAIGHT_ALPHA: each colour byte becomes (c * a) / 255 first (put_flippy's rule)
__device__ __forceinline__ uint32_t import_texel(uint32_t r, uint32_t g, uint32_t b, uint32_t a, bool straight) {
  if (straight) { r = r * a / 255u; g = g * a / 255u; b = b * a / 255u; }
  return r | (g << 8) | (b << 16) | (a << 24);
}
// One texel of minify_by2_host (k_minify2 is the same step from a dense image): a, b = the texels (2x, 2y), (2x + 1, 2y), c, d = those of
// the row below; col_pair / row_pair: the source has column 2x + 1 / row 2y + 1.  Where it has not, `a` is its last column / row.
__device__ __forceinline__ uint32_t import_minify(uint32_t a, uint32_t b, uint32_t c, uint32_t d, bool col_pair, bool row_pair) {
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
__device__ __forceinline__ void import_store(uint32_t* const* level, int size, int x, int y, int l, int i, int j, uint32_t texel) {
  const int LS = size >> l, tx = (x >> l) + i, ty = (y >> l) + j;
  if (tx >= 0 && ty >= 0 && tx < LS && ty < LS) level[l][(size_t)ty * LS + tx] = texel;
}

// A lane's run of one plane: four values at columns x0 .. x0 + 3 of the row at `row`.  `wide`: the plane's rows are 16-byte aligned and the
// image has a whole run -- every lane issues one load of a run, its own where that lies inside the image (`whole`), the row's first where it
// does not; such a lane then loads value by value at the columns xc[], which are clamped into the image, as every lane does without `wide`.
// (One unconditional wide load: left to choose between a wide load and four narrow ones the compiler shares the last dword between the two
// and issues three dwords and one.)
__device__ __forceinline__ void import_load_f32(const char* row, int x0, const int xc[4], bool wide, bool whole, float out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0.0f;
  if (wide) {
    const float4 v = *reinterpret_cast<const float4*>(row + (size_t)(whole ? x0 : 0) * 4);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  }
  if (!whole) {
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = *reinterpret_cast<const float*>(row + (size_t)xc[i] * 4);
  }
}
__device__ __forceinline__ void import_load_u32(const char* row, int x0, const int xc[4], bool wide, bool whole, uint32_t out[4]) {
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
__device__ __forceinline__ void import_load_f16(const char* row, int x0, const int xc[4], bool wide, bool whole, uint32_t out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0u;
  if (wide) {
    const uint2 v = *reinterpret_cast<const uint2*>(row + (size_t)(whole ? x0 : 0) * 2);
    out[0] = v.x & 0xFFFFu; out[1] = v.x >> 16; out[2] = v.y & 0xFFFFu; out[3] = v.y >> 16;
  }
  if (!whole) {
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = *reinterpret_cast<const uint16_t*>(row + (size_t)xc[i] * 2);
  }
}

// LDS of a tile: the levels one after the other, 32 x 32, 16 x 16, .. 1 (no level is written twice)
constexpr int kTileWords = 1024 + 256 + 64 + 16 + 4 + 1;

// May level l's texel (i, j) of an image of a batch be stored?  Single puts overwrite one another where two rectangles meet in a deep level;
// one launch has no order, so the host has painted the rectangles in array order (fdh_image_batch.h) and `owner` holds, from bit `bit0` on,
// a bit per texel of the image's levels kOwnerLevel .., rows packed: set where the texel is still this image's.  The single kernels
// (kBatch false) own every texel.
template <bool kBatch>
__device__ __forceinline__ bool import_owns(const uint32_t* owner, uint32_t bit0, uint32_t bit) {
  if (!kBatch) return true;
  bit += bit0;
  return (owner[bit >> 5] >> (bit & 31u)) & 1u;
}

// The body of a tile: tile (bx, by) of the image P describes, staged in `tile` (kTileWords + 3 words of LDS, 16-byte aligned) with `lines`
// (2 * kTile words of LDS).  k_image_import calls it for its own block, k_image_import_batch<format> for the tile its table word names, with
// the owner bits of its image: every read of P is wave-uniform in both.
template <uint32_t kFormat, bool kBatch>
__device__ __forceinline__ void import_tile(const ii::Params& P, const int bx, const int by, const uint32_t* owner, const uint32_t owner_bit0, uint32_t* tile, uint32_t* lines) {
  const int lane = (int)threadIdx.x;
  const int r = lane >> 3, c0 = (lane & 7) * 4;  // a wave covers eight whole rows of the tile
  const int X0 = bx * ii::kTile + c0, Y = by * ii::kTile + r;
  // ---- the loads.  Every address is valid -- row and columns clamped into the image -- and what lies outside is replaced behind the
  // conversion: no load waits for a branch on the texel's place, and all of a lane's loads go out before the first conversion.
  const int yc = min(Y, P.h - 1);
  int xc[4];
#pragma unroll
  for (int i = 0; i < 4; i++) xc[i] = min(X0 + i, P.w - 1);
  const bool wide = P.wide != 0, whole = wide && X0 + 4 <= P.w;
  const char* row = static_cast<const char*>(P.data) + (int64_t)yc * P.pitch_bytes;
  const bool straight = (P.flags & ii::kStraightAlpha) != 0;
  uint32_t px[4];
  if (kFormat == ii::kRgba8) {
    uint32_t t[4];
    import_load_u32(row, X0, xc, wide, whole, t);
#pragma unroll
    for (int i = 0; i < 4; i++) px[i] = import_texel(t[i] & 255u, (t[i] >> 8) & 255u, (t[i] >> 16) & 255u, t[i] >> 24, straight);
  } else {
    // (the plane count is the launch's: these branches are uniform)
    float f[4][4];
    if (kFormat == ii::kPlanarF32) {
      import_load_f32(row, X0, xc, wide, whole, f[0]);
      if (P.channels >= 3u) { import_load_f32(row + P.plane_bytes, X0, xc, wide, whole, f[1]); import_load_f32(row + 2 * P.plane_bytes, X0, xc, wide, whole, f[2]); }
      if (P.channels == 4u) import_load_f32(row + 3 * P.plane_bytes, X0, xc, wide, whole, f[3]);
    } else {
      uint32_t hb[4][4];
      import_load_f16(row, X0, xc, wide, whole, hb[0]);
      if (P.channels >= 3u) { import_load_f16(row + P.plane_bytes, X0, xc, wide, whole, hb[1]); import_load_f16(row + 2 * P.plane_bytes, X0, xc, wide, whole, hb[2]); }
      if (P.channels == 4u) import_load_f16(row + 3 * P.plane_bytes, X0, xc, wide, whole, hb[3]);
      const int planes = P.channels >= 3u ? (int)P.channels : 1;
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (k < planes) {
#pragma unroll
          for (int i = 0; i < 4; i++) f[k][i] = FDH_IMPORT_HALF_TO_FLOAT(hb[k][i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t b0 = import_byte(f[0][i]);
      uint32_t g = b0, b = b0, a = 255u;  // one channel: R = G = B = the byte, A = 255
      if (P.channels >= 3u) { g = import_byte(f[1][i]); b = import_byte(f[2][i]); }
      if (P.channels == 4u) a = import_byte(f[3][i]);
      px[i] = import_texel(b0, g, b, a, straight);
    }
  }
  // ---- level 0 into the atlas (dword stores: the entry's x need not be a multiple of four) and, as packed words, into LDS
  const bool row_in = Y < P.h;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const bool in = row_in && X0 + i < P.w;
    if (in && P.n_store > 0) import_store(P.level, P.size, P.x, P.y, 0, X0 + i, Y, px[i]);
    if (!in) px[i] = 0u;
  }
  uint4 run;
  run.x = px[0]; run.y = px[1]; run.z = px[2]; run.w = px[3];
  *reinterpret_cast<uint4*>(tile + r * ii::kTile + c0) = run;
  __syncthreads();
  // ---- the ink boxes (measure_ink), first half: a box is the span of the columns, and of the rows, that hold a texel above its level.
  // 32 lanes take a row of the staged tile each (its words rotated by the row, so that the lanes read 32 banks), 32 a column: the largest
  // alpha and the largest colour byte in it.  (Lanes folding their own texels into sixteen boxes with LDS atomics was the first build:
  // 64 atomics a lane on 64 words, every one of them 64 lanes deep -- 130 us for a workgroup.)
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
  uint32_t level_bit = 0u;  // (a batch) the first owner bit of level l, behind the image's own first
#pragma unroll
  for (int l = 1; l < ii::kTileLevels; l++) {
    const int to = from + side * side, half = side >> 1;
    if (lane < half * half) {
      const int i = lane & (half - 1), j = lane / half;
      const int X = bx * half + i, Yl = by * half + j;
      uint32_t o = 0u;
      if (X < P.lw[l] && Yl < P.lh[l]) {
        const uint32_t* s = tile + from + (2 * j) * side + 2 * i;
        o = import_minify(s[0], s[1], s[side], s[side + 1], 2 * X + 1 < P.lw[l - 1], 2 * Yl + 1 < P.lh[l - 1]);
        if (l < P.n_store && (l < ii::kOwnerLevel || import_owns<kBatch>(owner, owner_bit0, level_bit + (uint32_t)(Yl * P.lw[l] + X)))) import_store(P.level, P.size, P.x, P.y, l, X, Yl, o);
        if (l == ii::kTileLevels - 1) P.scratch[(size_t)by * P.lw[l] + bx] = o;
      }
      tile[to + j * half + i] = o;
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
    if (kBatch && l >= ii::kOwnerLevel) level_bit += (uint32_t)(P.lw[l] * P.lh[l]);
    from = to; side = half;
  }
}

template <uint32_t kFormat>
__global__ __launch_bounds__(ii::kGroup) void k_image_import(const ii::Params P) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[kTileWords + 3];
  __shared__ uint32_t lines[2 * ii::kTile];  // per row of the tile, then per column: the largest alpha | the largest colour byte << 8
  import_tile<kFormat, false>(P, (int)blockIdx.x, (int)blockIdx.y, nullptr, 0u, tile, lines);
}

// The batch: a 1-D grid over the tiles of all images of one format (tiles: this format's words, ii::batch_tile_word).  The image's index
// comes from the block index alone, so every read of its record is wave-uniform and the body's branches on channels, `wide` and `ink`
// stay uniform.  The record is read whole before the first store, into the single kernel's parameter block.
template <uint32_t kFormat>
__global__ __launch_bounds__(ii::kGroup) void k_image_import_batch(const ii::BatchImage* __restrict__ images, const uint32_t* __restrict__ tiles, const ii::BatchAtlas A,
                                                                   uint32_t* scratch, int32_t* ink_blocks, const uint32_t* __restrict__ owner) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[kTileWords + 3];
  __shared__ uint32_t lines[2 * ii::kTile];
  const uint32_t word = tiles[blockIdx.x];
  const ii::BatchImage& I = images[word & 0xFFFFu];
  ii::Params P;
  P.data = I.data; P.pitch_bytes = I.pitch_bytes; P.plane_bytes = I.plane_bytes;
  P.w = I.w; P.h = I.h; P.format = kFormat; P.channels = I.channels; P.flags = I.flags; P.wide = I.wide;
  P.x = I.x; P.y = I.y; P.n_store = I.n_store; P.ink = I.ink;
#pragma unroll
  for (int l = 0; l < ii::kTileLevels; l++) { P.lw[l] = I.lw[l]; P.lh[l] = I.lh[l]; }
#pragma unroll
  for (int l = 0; l < ii::kLevels; l++) P.level[l] = A.level[l];
  P.size = A.size;
  P.scratch = scratch + I.scratch_off;
  P.ink_block = ink_blocks + (size_t)I.ink_off * ii::kInkWords;
  import_tile<kFormat, true>(P, (int)((word >> 16) & 63u), (int)(word >> 22), owner, I.owner_off, tile, lines);
}

// LDS of the tail: the levels one after the other from 64 x 64 down
constexpr int kTailWords = 4096 + 1024 + 256 + 64 + 16 + 4 + 1;

// The body of the tail: `src` (sw x sh texels at level l0) through levels l0 + 1 .. n_store - 1 in `img` (kTailWords + 3 words of LDS); the
// entry at (x, y) of the atlas `level` of `size`.  kBatch: the owner bits as in import_tile; owner_bit0: the first bit of level l0 + 1.
// (`level` stays a pointer to the launch's arguments: the loop indexes it by a level that is no constant.)
template <bool kBatch>
__device__ __forceinline__ void import_tail(const uint32_t* src, int sw, int sh, const int l0, const int n_store, const int x, const int y, const int size, uint32_t* const* level,
                                            const uint32_t* owner, const uint32_t owner_bit0, uint32_t* img) {
  const int lane = (int)threadIdx.x;
  for (int t = lane; t < sw * sh; t += ii::kGroup) img[t] = src[t];
  __syncthreads();
  int from = 0;
  uint32_t level_bit = 0u;
  for (int l = l0 + 1; l < n_store; l++) {  // (n_store holds the chain's end: both extents of level l - 1 exceed 1)
    const int nw = (sw + 1) >> 1, nh = (sh + 1) >> 1, to = from + sw * sh;
    for (int t = lane; t < nw * nh; t += ii::kGroup) {
      const int j = t / nw, i = t - j * nw;
      const bool col_pair = 2 * i + 1 < sw, row_pair = 2 * j + 1 < sh;
      const uint32_t* s = img + from + (2 * j) * sw + 2 * i;
      const uint32_t o = import_minify(s[0], col_pair ? s[1] : 0u, row_pair ? s[sw] : 0u, col_pair && row_pair ? s[sw + 1] : 0u, col_pair, row_pair);
      if (import_owns<kBatch>(owner, owner_bit0, level_bit + (uint32_t)t)) import_store(level, size, x, y, l, i, j, o);
      img[to + t] = o;
    }
    __syncthreads();
    if (kBatch) level_bit += (uint32_t)(nw * nh);
    from = to; sw = nw; sh = nh;
  }
}

__global__ __launch_bounds__(ii::kGroup) void k_image_import_tail(const ii::TailParams P) {
  __shared__ uint32_t img[kTailWords + 3];
  import_tail<false>(P.src, P.sw, P.sh, P.l0, P.n_store, P.x, P.y, P.size, P.level, nullptr, 0u, img);
}

// The batch's tail: a workgroup per image whose chain goes beyond level 5 (tails: their indices in the records), on that image's level-5
// texels in the scratch.  (An image of a batch is at most kBatchMaxExtent each way: its level-5 image is at most kTailMax.)
__global__ __launch_bounds__(ii::kGroup) void k_image_import_tail_batch(const ii::BatchImage* __restrict__ images, const uint32_t* __restrict__ tails, const ii::BatchAtlas A,
                                                                        const uint32_t* scratch, const uint32_t* __restrict__ owner) {
  __shared__ uint32_t img[kTailWords + 3];
  const ii::BatchImage& I = images[tails[blockIdx.x]];
  uint32_t bit0 = I.owner_off;  // level 6's first bit lies behind levels kOwnerLevel .. 5
#pragma unroll
  for (int l = ii::kOwnerLevel; l < ii::kTileLevels; l++) bit0 += (uint32_t)(I.lw[l] * I.lh[l]);
  import_tail<true>(scratch + I.scratch_off, I.lw[ii::kTileLevels - 1], I.lh[ii::kTileLevels - 1], ii::kTileLevels - 1, I.n_store, I.x, I.y, A.size, A.level, owner, bit0, img);
}

void launch_image_import(hipStream_t s, const ii::Params& P) {
  if (P.w <= 0 || P.h <= 0) return;
  const dim3 grid((P.w + ii::kTile - 1) / ii::kTile, (P.h + ii::kTile - 1) / ii::kTile), block(ii::kGroup);
  if (P.format == ii::kRgba8) FDH_LAUNCH(k_image_import<ii::kRgba8>, grid, block, 0, s, P);
  else if (P.format == ii::kPlanarF32) FDH_LAUNCH(k_image_import<ii::kPlanarF32>, grid, block, 0, s, P);
  else FDH_LAUNCH(k_image_import<ii::kPlanarF16>, grid, block, 0, s, P);
}
void launch_image_import_tail(hipStream_t s, const ii::TailParams& P) {
  if (P.sw <= 0 || P.sh <= 0 || P.sw > ii::kTailMax || P.sh > ii::kTailMax || P.l0 + 1 >= P.n_store) return;
  FDH_LAUNCH(k_image_import_tail, dim3(1), dim3(ii::kGroup), 0, s, P);
}
// the batch's launches: n_tiles tiles of `format` (their words at `tiles`), and n_tails images with a tail
void launch_image_import_batch(hipStream_t s, uint32_t format, const ii::BatchImage* images, const uint32_t* tiles, int n_tiles, const ii::BatchAtlas& A, uint32_t* scratch,
                               int32_t* ink_blocks, const uint32_t* owner) {
  if (n_tiles <= 0) return;
  const dim3 grid(n_tiles), block(ii::kGroup);
  if (format == ii::kRgba8) FDH_LAUNCH(k_image_import_batch<ii::kRgba8>, grid, block, 0, s, images, tiles, A, scratch, ink_blocks, owner);
  else if (format == ii::kPlanarF32) FDH_LAUNCH(k_image_import_batch<ii::kPlanarF32>, grid, block, 0, s, images, tiles, A, scratch, ink_blocks, owner);
  else FDH_LAUNCH(k_image_import_batch<ii::kPlanarF16>, grid, block, 0, s, images, tiles, A, scratch, ink_blocks, owner);
}
void launch_image_import_tail_batch(hipStream_t s, const ii::BatchImage* images, const uint32_t* tails, int n_tails, const ii::BatchAtlas& A, const uint32_t* scratch, const uint32_t* owner) {
  if (n_tails <= 0) return;
  FDH_LAUNCH(k_image_import_tail_batch, dim3(n_tails), dim3(ii::kGroup), 0, s, images, tails, A, scratch, owner);
}

}  // namespace fdh
