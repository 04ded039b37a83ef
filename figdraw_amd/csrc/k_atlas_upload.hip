// k_atlas_upload.hip -- images on their way into the atlas: the LCD filter of glyph images (common/textrasters/pixie_raster.nim:12-43),
// pixie's minifyBy2 for the mip chain (opengl/textures.nim:106-119), the blit into a level, the coverage rasteriser of glyph outlines,
// and a fill.
#include "fdh_device.h"
#include "fdh_msdf_host.h"  // msdf::BatchGlyph: the batched blit and minify of fdh_put_glyph_outlines

namespace fdh {
// ------------------------------------------------------------------ glyph images on their way into the atlas
// FreeType's default 5-tap LCD filter as the reference applies it to a rasterised glyph before the upload
// (common/textrasters/pixie_raster.nim:12-43): weights 8, 77, 86, 77, 8 over x - 2 .. x + 2 with the column clamped to the image,
// per channel (sum + 128) >> 8.  Integer arithmetic: bit-exact with the oracle's restatement.
__global__ void k_lcd_filter(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int w, int h) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  const int wt[5] = {8, 77, 86, 77, 8};
  int sr = 0, sg = 0, sb = 0, sa = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const int sx = min(max(x + i - 2, 0), w - 1);
    const uint32_t p = src[(size_t)y * w + sx];
    sr += (int)(p & 255u) * wt[i]; sg += (int)((p >> 8) & 255u) * wt[i]; sb += (int)((p >> 16) & 255u) * wt[i]; sa += (int)(p >> 24) * wt[i];
  }
  dst[(size_t)y * w + x] = (uint32_t)(((sr + 128) >> 8) & 255) | ((uint32_t)(((sg + 128) >> 8) & 255) << 8) |
                           ((uint32_t)(((sb + 128) >> 8) & 255) << 16) | ((uint32_t)(((sa + 128) >> 8) & 255) << 24);
}
// one mip step of updateSubImage (textures.nim:106-119) = pixie's Image.minifyBy2 on premultiplied RGBA8: box sum div 4; an odd
// extent rounds the result size up and the extra column / row / corner carry half / half / quarter coverage (the arithmetic
// is pinned by the reference's data/img1.flippy: minify_by2_host in fdh_context.cpp spells it out)
__global__ void k_minify2(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int sw, int sh) {
  const int nw = (sw + 1) >> 1, nh = (sh + 1) >> 1;
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= nw || y >= nh) return;
  const bool col_pair = 2 * x + 1 < sw, row_pair = 2 * y + 1 < sh;
  const int x0 = col_pair ? 2 * x : sw - 1, x1 = col_pair ? 2 * x + 1 : sw - 1, y0 = row_pair ? 2 * y : sh - 1, y1 = row_pair ? 2 * y + 1 : sh - 1;
  const uint32_t a = src[(size_t)y0 * sw + x0], b = src[(size_t)y0 * sw + x1], c = src[(size_t)y1 * sw + x0], d = src[(size_t)y1 * sw + x1];
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
  dst[(size_t)y * nw + x] = o;
}
// (k_minify2 as a function of the texel, for k_minify2_batch; k_minify2 itself stays as it was compiled: profiles/msdf.txt section 6)
__device__ __forceinline__ void minify2_texel(const uint32_t* src, uint32_t* dst, int sw, int sh, int x, int y) {
  const int nw = (sw + 1) >> 1, nh = (sh + 1) >> 1;
  if (x >= nw || y >= nh) return;
  const bool col_pair = 2 * x + 1 < sw, row_pair = 2 * y + 1 < sh;
  const int x0 = col_pair ? 2 * x : sw - 1, x1 = col_pair ? 2 * x + 1 : sw - 1, y0 = row_pair ? 2 * y : sh - 1, y1 = row_pair ? 2 * y + 1 : sh - 1;
  const uint32_t a = src[(size_t)y0 * sw + x0], b = src[(size_t)y0 * sw + x1], c = src[(size_t)y1 * sw + x0], d = src[(size_t)y1 * sw + x1];
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
  dst[(size_t)y * nw + x] = o;
}
// a w x h image into the rectangle (x, y) of one atlas level (LS texels wide); texels outside the level are dropped
__device__ __forceinline__ void atlas_blit_texel(uint32_t* level, int LS, int x, int y, const uint32_t* src, int w, int h, int i, int j) {
  if (i >= w || j >= h) return;
  const int tx = x + i, ty = y + j;
  if (tx >= 0 && ty >= 0 && tx < LS && ty < LS) level[(size_t)ty * LS + tx] = src[(size_t)j * w + i];
}
__global__ void k_atlas_blit(uint32_t* __restrict__ level, int LS, int x, int y, const uint32_t* __restrict__ src, int w, int h) {
  atlas_blit_texel(level, LS, x, y, src, w, h, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y);
}
// fdh_put_glyph_outlines (include_glyphs/figdraw_hip_glyphs.h): level `l` of the chain for every glyph of a batch at once, over the tile table of the
// batched generator (k_msdf.hip): one workgroup per 8 x 8 tile of a glyph's LEVEL-0 tile grid -- the glyph minified l times has fewer, the
// rest leave.  A glyph's image at level l is ceil(w / 2^l) x ceil(h / 2^l), stored densely at the start of the glyph's own region of the
// two field buffers, which it goes back and forth between as a single put does between its two.  A glyph is in the chain while that image is
// more than 1 texel wide and high (Atlas::each_level); at level 0 a narrower one is stored all the same (Atlas::put_glyph_mtsdf).
// From msdf::kOwnerLevel on two glyphs' rectangles can meet, and single puts leave such a texel to the later one: the host has worked out
// which texels a glyph owns, one bit each, level after level from the glyph's owner_off.
struct BatchTile { msdf::BatchGlyph g; int cw, ch, i, j; };
__device__ __forceinline__ BatchTile batch_tile(const msdf::BatchGlyph* __restrict__ glyphs, const uint32_t* __restrict__ tile_glyph, int l) {
  BatchTile t;
  t.g = glyphs[tile_glyph[blockIdx.x]];
  const int tile = (int)(blockIdx.x - t.g.first_tile), tiles_x = (t.g.w + 7) / 8;
  t.cw = (t.g.w + (1 << l) - 1) >> l; t.ch = (t.g.h + (1 << l) - 1) >> l;
  t.j = tile / tiles_x * 8 + (int)(threadIdx.x >> 3); t.i = (tile - tile / tiles_x * tiles_x) * 8 + (int)(threadIdx.x & 7);
  return t;
}
__global__ __launch_bounds__(64) void k_atlas_blit_batch(uint32_t* __restrict__ level, int LS, int l, const msdf::BatchGlyph* __restrict__ glyphs,
                                                         const uint32_t* __restrict__ tile_glyph, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ src) {
  const BatchTile t = batch_tile(glyphs, tile_glyph, l);
  if (!((t.cw > 1 && t.ch > 1) || l == 0)) return;
  if (l >= msdf::kOwnerLevel) {
    if (t.i >= t.cw || t.j >= t.ch) return;
    uint32_t bit = t.g.owner_off;
    for (int k = msdf::kOwnerLevel; k < l; k++) bit += (uint32_t)(((t.g.w + (1 << k) - 1) >> k) * ((t.g.h + (1 << k) - 1) >> k));
    bit += (uint32_t)(t.j * t.cw + t.i);
    if (!((owner[bit >> 5] >> (bit & 31u)) & 1u)) return;
  }
  atlas_blit_texel(level, LS, t.g.x >> l, t.g.y >> l, src + t.g.field_off, t.cw, t.ch, t.i, t.j);
}
__global__ __launch_bounds__(64) void k_minify2_batch(int l, const msdf::BatchGlyph* __restrict__ glyphs, const uint32_t* __restrict__ tile_glyph,
                                                      const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
  const BatchTile t = batch_tile(glyphs, tile_glyph, l);
  if (!(t.cw > 1 && t.ch > 1)) return;
  minify2_texel(src + t.g.field_off, dst + t.g.field_off, t.cw, t.ch, t.i, t.j);
}
// Glyph outline -> coverage: exact-area scanline accumulation (oracle/figdraw_oracle.c, raster_row_line, operation for operation:
// no FMA contraction here so that both produce the same floats).  One lane owns one pixel row: it walks every line segment in
// order and adds the signed areas of the part inside its row to the row's accumulation cells (global scratch, w + 2 floats per
// row: nobody else touches them), then a running sum along the row turns areas into coverage.  Out: premultiplied white.
// The part of a line inside one row that lies left of the image (x < 0) has the whole row to its right: its share of the row piece's
// height goes to cell 0 as it is; the part right of the image (x > w) adds nothing; the part inside is accumulated with its own share.
__device__ __forceinline__ void raster_row_line(float* acc, int w, int y, float x0, float y0, float x1, float y1) {
#pragma clang fp contract(off)
  if (y0 == y1) return;
  float dir = 1.0f;
  if (y0 > y1) { float t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; dir = -1.0f; }
  const float ya = y0 > (float)y ? y0 : (float)y, yb = y1 < (float)(y + 1) ? y1 : (float)(y + 1);
  if (!(yb > ya)) return;
  const float dxdy = (x1 - x0) / (y1 - y0);
  const float xa = x0 + (ya - y0) * dxdy, xb = x0 + (yb - y0) * dxdy;
  float d = (yb - ya) * dir;
  float xl = xa < xb ? xa : xb, xr = xa < xb ? xb : xa;
  const float fw = (float)w;
  if (xl < 0.0f || xr > fw) {  // the row piece leaves the image: cut at x = 0 and x = w, d shared out in proportion to x
    if (!(xr > 0.0f)) { acc[0] += d; return; }  // wholly left of the image: everything at cell 0
    if (!(xl < fw)) return;                      // wholly right of it: nothing
    const float span = xr - xl;
    const float xli = xl < 0.0f ? 0.0f : xl, xri = xr > fw ? fw : xr;
    if (xl < 0.0f) acc[0] += d * ((0.0f - xl) / span);  // the outside share first, then what the inside part adds to cell 0
    d = d * ((xri - xli) / span);
    xl = xli; xr = xri;
  }
  const float x0floor = __builtin_floorf(xl);
  const int x0i = (int)x0floor;
  const float x1ceil = __builtin_ceilf(xr);
  const int x1i = (int)x1ceil;
  if (x1i <= x0i + 1) {
    const float xmf = 0.5f * (xl + xr) - x0floor;
    acc[x0i] += d - d * xmf;
    if (x0i + 1 <= w) acc[x0i + 1] += d * xmf;
  } else {
    const float s = 1.0f / (xr - xl);
    const float x0f = xl - x0floor;
    const float a0 = 0.5f * s * (1.0f - x0f) * (1.0f - x0f);
    const float x1f = xr - x1ceil + 1.0f;
    const float am = 0.5f * s * x1f * x1f;
    acc[x0i] += d * a0;
    if (x1i == x0i + 2) {
      acc[x0i + 1] += d * (1.0f - a0 - am);
    } else {
      const float a1 = s * (1.5f - x0f);
      acc[x0i + 1] += d * (a1 - a0);
      for (int xi = x0i + 2; xi < x1i - 1; xi++) acc[xi] += d * s;
      const float a2 = a1 + (float)(x1i - x0i - 3) * s;
      acc[x1i - 1] += d * (1.0f - a2 - am);
    }
    if (x1i <= w) acc[x1i] += d * am;
  }
}
__global__ __launch_bounds__(64) void k_rasterize_lines(const float4* __restrict__ lines, int n, int w, int h, float* __restrict__ scratch, uint32_t* __restrict__ out) {
#pragma clang fp contract(off)
  const int y = blockIdx.x * 64 + threadIdx.x;
  if (y >= h) return;
  float* acc = scratch + (size_t)y * (w + 2);
  for (int x = 0; x < w + 2; x++) acc[x] = 0.0f;
  for (int i = 0; i < n; i++) {
    const float4 l = lines[i];
    raster_row_line(acc, w, y, l.x, l.y, l.z, l.w);
  }
  float sum = 0.0f;
  for (int x = 0; x < w; x++) {
    sum += acc[x];
    float c = __builtin_fabsf(sum);
    if (c > 1.0f) c = 1.0f;
    const uint32_t v = (uint32_t)(c * 255.0f + 0.5f);
    out[(size_t)y * w + x] = v * 0x01010101u;
  }
}
void launch_rasterize_lines(hipStream_t s, const float4* lines, int n, int w, int h, float* scratch, uint32_t* out) {
  if (w > 0 && h > 0) hipLaunchKernelGGL(k_rasterize_lines, dim3((h + 63) / 64), dim3(64), 0, s, lines, n, w, h, scratch, out);
}
void launch_lcd_filter(hipStream_t s, const uint32_t* src, uint32_t* dst, int w, int h) {
  if (w > 0 && h > 0) hipLaunchKernelGGL(k_lcd_filter, dim3((w + 63) / 64, h), dim3(64), 0, s, src, dst, w, h);
}
void launch_minify2(hipStream_t s, const uint32_t* src, uint32_t* dst, int sw, int sh) {
  const int nw = (sw + 1) / 2, nh = (sh + 1) / 2;
  if (sw > 0 && sh > 0) hipLaunchKernelGGL(k_minify2, dim3((nw + 63) / 64, nh), dim3(64), 0, s, src, dst, sw, sh);
}
void launch_atlas_blit(hipStream_t s, uint32_t* level, int LS, int x, int y, const uint32_t* src, int w, int h) {
  if (w > 0 && h > 0) hipLaunchKernelGGL(k_atlas_blit, dim3((w + 63) / 64, h), dim3(64), 0, s, level, LS, x, y, src, w, h);
}
void launch_atlas_blit_batch(hipStream_t s, uint32_t* level, int LS, int l, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* owner,
                             const uint32_t* src) {
  if (n_tiles > 0) hipLaunchKernelGGL(k_atlas_blit_batch, dim3(n_tiles), dim3(64), 0, s, level, LS, l, glyphs, tile_glyph, owner, src);
}
void launch_minify2_batch(hipStream_t s, int l, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* src, uint32_t* dst) {
  if (n_tiles > 0) hipLaunchKernelGGL(k_minify2_batch, dim3(n_tiles), dim3(64), 0, s, l, glyphs, tile_glyph, src, dst);
}

// ------------------------------------------------------------------ fdh_put_glyph_coverage_batch: the coverage glyphs of a batch at once
// (the specification: include_glyphs/figdraw_hip_coverage.h).  The tables are the distance-field batch's: one msdf::BatchGlyph per glyph -- edge_off and
// n_edges are the glyph's first flattened line and its line count in `lines` --, one word per 8 x 8 tile naming the tile's glyph, the
// glyphs' w x h images one after the other in the two field buffers.  k_rasterize_lines SCATTERS: a lane owns a row and every line adds to
// the cells x0i .. x1i of that row.  Here a lane owns one accumulator cell (x, y) and GATHERS: it walks the glyph's lines in the same order
// and adds what raster_row_line would add to acc[x] of row y -- the same expressions, picked by where x lies in [x0i, x1i].  A line adds
// to a cell at most once -- but to cell 0 twice where its row piece crosses x = 0: the share left of the image first, then the inside
// part's, in raster_row_line's order -- so the cell's value is the same sequence of float additions and the same bits; it lives in a register and is
// stored once (as a float, into the glyph's region of the spare field buffer).  Cells x >= w are never read by the running sum: they do
// not exist here.  The line index is the loop counter, the tile and the glyph depend on blockIdx alone: scalar loads, wave-uniform culls.
__device__ __forceinline__ void coverage_cell_line(float& acc, int w, int x, int y, float x0, float y0, float x1, float y1) {
#pragma clang fp contract(off)
  if (y0 == y1) return;
  float dir = 1.0f;
  if (y0 > y1) { float t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; dir = -1.0f; }
  const float ya = y0 > (float)y ? y0 : (float)y, yb = y1 < (float)(y + 1) ? y1 : (float)(y + 1);
  if (!(yb > ya)) return;
  const float dxdy = (x1 - x0) / (y1 - y0);
  const float xa = x0 + (ya - y0) * dxdy, xb = x0 + (yb - y0) * dxdy;
  float d = (yb - ya) * dir;
  float xl = xa < xb ? xa : xb, xr = xa < xb ? xb : xa;
  const float fw = (float)w;
  if (xl < 0.0f || xr > fw) {  // raster_row_line's cut at x = 0 and x = w
    if (!(xr > 0.0f)) { if (x == 0) acc += d; return; }
    if (!(xl < fw)) return;
    const float span = xr - xl;
    const float xli = xl < 0.0f ? 0.0f : xl, xri = xr > fw ? fw : xr;
    if (xl < 0.0f && x == 0) acc += d * ((0.0f - xl) / span);  // cell 0's first addition of this line; the inside part's follows below
    d = d * ((xri - xli) / span);
    xl = xli; xr = xri;
  }
  const float x0floor = __builtin_floorf(xl);
  const int x0i = (int)x0floor;
  const float x1ceil = __builtin_ceilf(xr);
  const int x1i = (int)x1ceil;
  if (x < x0i) return;
  if (x1i <= x0i + 1) {  // narrow: cells x0i and x0i + 1
    if (x > x0i + 1) return;
    const float xmf = 0.5f * (xl + xr) - x0floor;
    if (x == x0i) acc += d - d * xmf;
    else acc += d * xmf;
  } else {               // wide: cells x0i .. x1i
    if (x > x1i) return;
    const float s = 1.0f / (xr - xl);
    const float x0f = xl - x0floor;
    const float a0 = 0.5f * s * (1.0f - x0f) * (1.0f - x0f);
    const float x1f = xr - x1ceil + 1.0f;
    const float am = 0.5f * s * x1f * x1f;
    if (x == x0i) acc += d * a0;
    else if (x == x1i) acc += d * am;
    else if (x1i == x0i + 2) acc += d * (1.0f - a0 - am);
    else {
      const float a1 = s * (1.5f - x0f);
      if (x == x0i + 1) acc += d * (a1 - a0);
      else if (x == x1i - 1) {
        const float a2 = a1 + (float)(x1i - x0i - 3) * s;
        acc += d * (1.0f - a2 - am);
      } else acc += d * s;
    }
  }
}
// One workgroup per tile, one lane per cell.  A line is skipped for the whole tile where no row of the tile can take anything from it:
// its y-range misses the tile's 8 rows (yb > ya fails in every row), or -- coordinates up to 2^16 in size -- its x-range, clamped to
// [0, w] as raster_row_line clamps, ends more than 2 cells left of the tile or starts 9 or more cells right of its first column.  (A row's xa and
// xb are x0 + (y - y0) * dxdy with 0 <= y - y0 <= y1 - y0: within [min(x0, x1), max(x0, x1)] but for rounding, which at that size stays below
// 0.06; the cells a row touches end at ceil(xr) or x0i + 1 and start at floor(xl): a whole cell of slack on either side.)  Lines left
// of a tile reach it through the running sum, not through its cells.  The share of a row piece that lies left of the image goes to cell
// 0, a cell of the row's first tile (tx0 = 0), and the cull keeps such a line for that tile: any line with a point at x < 0 -- or within
// the rounding above of it -- has a clamped range that starts at 0 (or 0.06 from it), which neither ends left of -2 nor starts at 9 or
// beyond; so does a line wholly left of the image, whose clamped range is [0, 0].  No other tile holds cell 0.  What lies right of the
// image adds nothing anywhere: a line wholly right of it clamps to [w, w] and may be skipped or not, to the same end.
__global__ __launch_bounds__(64) void k_coverage_cells_batch(const float4* __restrict__ lines, const msdf::BatchGlyph* __restrict__ glyphs,
                                                             const uint32_t* __restrict__ tile_glyph, float* __restrict__ acc) {
#pragma clang fp contract(off)
  const msdf::BatchGlyph g = glyphs[tile_glyph[blockIdx.x]];
  const int tile = (int)(blockIdx.x - g.first_tile), tiles_x = (g.w + 7) / 8;
  const int ty0 = tile / tiles_x * 8, tx0 = (tile - tile / tiles_x * tiles_x) * 8;
  const int x = tx0 + (int)(threadIdx.x & 7), y = ty0 + (int)(threadIdx.x >> 3);
  if (x >= g.w || y >= g.h) return;
  const float4* __restrict__ ln = lines + g.edge_off;
  const float fw = (float)g.w, left = (float)(tx0 - 2), right = (float)(tx0 + 9), top = (float)ty0, bottom = (float)(ty0 + 8);
  float a = 0.0f;
  for (int i = 0; i < g.n_edges; i++) {
    const float4 l = ln[i];
    const float ylo = l.y < l.w ? l.y : l.w, yhi = l.y < l.w ? l.w : l.y;
    if (!(yhi > top) || !(ylo < bottom)) continue;
    float xlo = l.x < l.z ? l.x : l.z, xhi = l.x < l.z ? l.z : l.x;
    if (xlo >= -65536.0f && xhi <= 65536.0f) {
      if (xlo < 0.0f) xlo = 0.0f;
      if (xhi < 0.0f) xhi = 0.0f;
      if (xlo > fw) xlo = fw;
      if (xhi > fw) xhi = fw;
      if (xhi < left || xlo >= right) continue;
    }
    coverage_cell_line(a, g.w, x, y, l.x, l.y, l.z, l.w);
  }
  acc[g.field_off + (size_t)y * g.w + x] = a;
}
// The second half of k_rasterize_lines, `sum += acc[x]` from left to right: a float recurrence that keeps its order.  The first tile of
// every 8-row band of a glyph does the band (the other workgroups leave at once): lane (row, column) walks the tiles from left to right
// and carries its row's sum across them; inside a tile every lane of a row makes the same 8 additions and keeps the sum as it stood after
// its own column -- cell x's coverage is (((a0 + a1) + a2) .. + ax), as in the single kernel, and a store covers 8 neighbouring texels.
__global__ __launch_bounds__(64) void k_coverage_sum_batch(const msdf::BatchGlyph* __restrict__ glyphs, const uint32_t* __restrict__ tile_glyph,
                                                           const float* __restrict__ acc, uint32_t* __restrict__ out) {
#pragma clang fp contract(off)
  const msdf::BatchGlyph g = glyphs[tile_glyph[blockIdx.x]];
  const int tile = (int)(blockIdx.x - g.first_tile), tiles_x = (g.w + 7) / 8;
  const int band = tile / tiles_x;
  if (tile != band * tiles_x) return;
  const int c = (int)(threadIdx.x & 7), y = band * 8 + (int)(threadIdx.x >> 3);
  if (y >= g.h) return;
  const float* __restrict__ row = acc + g.field_off + (size_t)y * g.w;
  uint32_t* __restrict__ orow = out + g.field_off + (size_t)y * g.w;
  float sum = 0.0f;
  for (int x0 = 0; x0 < g.w; x0 += 8) {
    float mine = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (x0 + k < g.w) {
        sum += row[x0 + k];
        if (k == c) mine = sum;
      }
    }
    if (x0 + c < g.w) {
      float cov = __builtin_fabsf(mine);
      if (cov > 1.0f) cov = 1.0f;
      const uint32_t v = (uint32_t)(cov * 255.0f + 0.5f);
      orow[x0 + c] = v * 0x01010101u;
    }
  }
}
// (k_lcd_filter as a function of the texel, for k_lcd_filter_batch; k_lcd_filter itself stays as it was compiled)
__device__ __forceinline__ void lcd_filter_texel(const uint32_t* src, uint32_t* dst, int w, int x, int y) {
  const int wt[5] = {8, 77, 86, 77, 8};
  int sr = 0, sg = 0, sb = 0, sa = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const int sx = min(max(x + i - 2, 0), w - 1);
    const uint32_t p = src[(size_t)y * w + sx];
    sr += (int)(p & 255u) * wt[i]; sg += (int)((p >> 8) & 255u) * wt[i]; sb += (int)((p >> 16) & 255u) * wt[i]; sa += (int)(p >> 24) * wt[i];
  }
  dst[(size_t)y * w + x] = (uint32_t)(((sr + 128) >> 8) & 255) | ((uint32_t)(((sg + 128) >> 8) & 255) << 8) |
                           ((uint32_t)(((sb + 128) >> 8) & 255) << 16) | ((uint32_t)(((sa + 128) >> 8) & 255) << 24);
}
// every glyph of the batch from one field buffer into the other, columns clamped to the glyph's own width
__global__ __launch_bounds__(64) void k_lcd_filter_batch(const msdf::BatchGlyph* __restrict__ glyphs, const uint32_t* __restrict__ tile_glyph,
                                                         const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
  const BatchTile t = batch_tile(glyphs, tile_glyph, 0);
  if (t.i >= t.g.w || t.j >= t.g.h) return;
  lcd_filter_texel(src + t.g.field_off, dst + t.g.field_off, t.g.w, t.i, t.j);
}
void launch_coverage_batch(hipStream_t s, const float4* lines, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, float* acc, uint32_t* out) {
  if (n_tiles <= 0) return;
  hipLaunchKernelGGL(k_coverage_cells_batch, dim3(n_tiles), dim3(64), 0, s, lines, glyphs, tile_glyph, acc);
  hipLaunchKernelGGL(k_coverage_sum_batch, dim3(n_tiles), dim3(64), 0, s, glyphs, tile_glyph, acc, out);
}
void launch_lcd_filter_batch(hipStream_t s, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* src, uint32_t* dst) {
  if (n_tiles > 0) hipLaunchKernelGGL(k_lcd_filter_batch, dim3(n_tiles), dim3(64), 0, s, glyphs, tile_glyph, src, dst);
}

__global__ void k_fill_u32(uint32_t* p, uint32_t v, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

void launch_fill(hipStream_t s, uint32_t* p, uint32_t v, size_t n) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_fill_u32, dim3(1024), dim3(256), 0, s, p, v, n);
}

#if FDH_STATS
void debug_wave_times(unsigned long long* out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_times), sizeof(unsigned long long) * 16 * 65536);
  void* p = nullptr;  // cleared after every read: the next read then holds exactly the launches in between
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_wave_times)) == hipSuccess) (void)hipMemset(p, 0, sizeof(unsigned long long) * 16 * 65536);
  (void)hipDeviceSynchronize();  // (the memset is asynchronous, the contexts' streams do not wait for the null stream: without this it clears rows of the NEXT launch)
}
void debug_counters(unsigned long long out[128], bool reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_counters), 128 * sizeof(unsigned long long));
  if (reset) { unsigned long long z[128] = {}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_counters), z, sizeof z); }
}
#endif

}  // namespace fdh
