// tests/video_alpha_in_emu/emu.cpp -- figdraw_amd/csrc/k_video_alpha_import.hip under the sequential host shim (tests/emu/fdh_device.h),
// with k_image_import.hip for the tail kernel; the kernels' sources and their parameter headers come from csrc, unmodified:
// tests/test_video_alpha_host.py copies them here.  Built twice: emu, and emu_san (the same stand-alone program under AddressSanitizer
// and UBSan, which also refuses a wide load at an address that is no multiple of its size).  The launches are
// Importer::import_one's for an AlphaSource (fdh_import.cpp) for a frame of up to 2048 x 2048.
// usage: emu cases.bin out.bin
//   cases.bin: per case twenty-four int32 -- w, h, format, matrix, range, flags, pitch[4], offset[4], bytes[4], x, y, atlas_size, n_levels,
//              0, 0 -- and bytes[0] + .. + bytes[3] bytes: the planes Y, Cb, Cr, A, or the UYVY plane and A (pitch, offset and bytes of
//              planes 1 and 2 are 0).  The kernel gets each plane at an address offset[p] past a 16-byte boundary, in a block of its own
//              that ends with the plane's last row's end (a read past either end is an error under AddressSanitizer)
//   out.bin:   per case every stored level's rectangle, ceil(w / 2^l) x ceil(h / 2^l) texels, level 0 first, then the 64 words of the ink
//              blocks as the host folds them (fold_ink; the start values where the image has no ink boxes), then the level-5 image,
//              ceil(w / 32) x ceil(h / 32) texels
// It prints, per build b = 2 * kind + straight (kind: A420 0, A420 linear 1, A444 2, A410 3, UYVA 4, UYVA linear 5), its cases and how
// many of them took the wide path per plane.
// exit 1: a texel outside the entry's rectangles was written; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_image_import.hip"
#include "k_video_alpha_import.hip"
#include "fdh_video_import.h"
#include <vector>
namespace ii = fdh::image_import;
namespace va = fdh::video_alpha;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const uint32_t kFill = 0xEEEEEEEEu;
  int32_t head[24];
  long cases = 0, per_build[12] = {}, wide[12][4] = {};
  while (fread(head, 4, 24, in) == 24) {
    const int w = head[0], h = head[1], x = head[18], y = head[19], size = head[20], n_levels = head[21];
    const uint32_t format = (uint32_t)head[2], matrix = (uint32_t)head[3], range = (uint32_t)head[4], flags = (uint32_t)head[5];
    if (w < 1 || h < 1 || w > 2048 || h > 2048 || !va::known(format) || matrix > 2 || range > 1 || (flags & ~3u) || n_levels < 1 || n_levels > ii::kLevels || x < 0 || y < 0 || x + w > size || y + h > size) return 2;
    if ((flags & va::kChromaLinear) && va::full_chroma(format)) return 2;
    const int kind = (format == va::kA420 ? 0 : format == va::kA444 ? 2 : format == va::kA410 ? 3 : 4) + (int)(flags & va::kChromaLinear);
    const int build = 2 * kind + ((flags & va::kStraightAlpha) ? 1 : 0);
    unsigned char* plane[4] = {nullptr, nullptr, nullptr, nullptr};
    va::InParams P{};
    P.w = w; P.h = h;
    P.cw = va::full_chroma(format) ? w : (w + 1) / 2; P.ch = (int)va::rows(format, 1, h);
    for (int p = 0; p < 4; p++) {
      const int offset = head[10 + p], bytes = head[14 + p];
      if (!va::has_plane(format, p)) { if (offset || bytes || head[6 + p]) return 2; continue; }
      const int64_t pitch = head[6 + p], row = va::row_bytes(format, p, w), run = va::run_bytes(format, p);
      if (offset < 0 || offset > 15 || pitch < row || bytes != (va::rows(format, p, h) - 1) * pitch + row) return 2;
      plane[p] = new unsigned char[(size_t)offset + bytes];
      if (fread(plane[p] + offset, 1, bytes, in) != (size_t)bytes) return 2;
      P.plane[p] = plane[p] + offset; P.pitch[p] = pitch;
      P.wide[p] = (uintptr_t)P.plane[p] % (uintptr_t)run == 0 && pitch % run == 0 && row >= run;
      wide[build][p] += P.wide[p];
    }
    per_build[build]++;
    P.format = format; P.flags = flags;
    const int32_t* c = fdh::video_import::kCoefficients[va::ten_bit(format)][matrix][range];
    P.yoff = c[0]; P.coff = c[1]; P.cy = c[2]; P.crv = c[3]; P.cgu = c[4]; P.cgv = c[5]; P.cbu = c[6];
    std::vector<std::vector<uint32_t>> levels;
    for (int l = 0; l < n_levels; l++) levels.emplace_back((size_t)(size >> l) * (size >> l), kFill);
    P.x = x; P.y = y; P.size = size;
    for (int cw = w, ch = h, l = 0; cw > 1 && ch > 1 && l < n_levels; l++, cw = (cw + 1) / 2, ch = (ch + 1) / 2) P.n_store++;
    P.ink = w <= ii::kInkMax && h <= ii::kInkMax;
    for (int l = 0; l < ii::kTileLevels; l++) { P.lw[l] = (w + (1 << l) - 1) >> l; P.lh[l] = (h + (1 << l) - 1) >> l; }
    for (int l = 0; l < n_levels; l++) P.level[l] = levels[(size_t)l].data();
    std::vector<uint32_t> scratch((size_t)P.lw[5] * P.lh[5], kFill);  // exactly the level-5 image
    P.scratch = scratch.data();
    const int tiles = P.ink ? P.lw[5] * P.lh[5] : 0;
    std::vector<int32_t> blocks((size_t)tiles * ii::kInkWords, -1);  // exactly the tiles' blocks; none where the image has no ink boxes
    P.ink_block = blocks.data();
    fdh::launch_video_alpha_import(nullptr, P);
    if (ii::kTileLevels < P.n_store) {
      ii::TailParams T{};
      T.src = scratch.data(); T.sw = P.lw[5]; T.sh = P.lh[5]; T.l0 = ii::kTileLevels - 1; T.n_store = P.n_store;
      T.x = x; T.y = y; T.size = size;
      for (int l = 0; l < n_levels; l++) T.level[l] = P.level[l];
      fdh::launch_image_import_tail(nullptr, T);
    }
    for (int p = 0; p < 4; p++) delete[] plane[p];
    for (int l = 0; l < n_levels; l++) {
      const int LS = size >> l, lx = x >> l, ly = y >> l, lw = (w + (1 << l) - 1) >> l, lh = (h + (1 << l) - 1) >> l;
      const bool stored = l < P.n_store;
      for (int j = 0; j < LS; j++)
        for (int i = 0; i < LS; i++) {
          const bool inside = stored && i >= lx && i < lx + lw && j >= ly && j < ly + lh;
          if (!inside && levels[(size_t)l][(size_t)j * LS + i] != kFill) { printf("case %ld: level %d written at (%d, %d)\n", cases, l, i, j); return 1; }
        }
      if (stored)
        for (int j = 0; j < lh; j++) fwrite(levels[(size_t)l].data() + (size_t)(ly + j) * LS + lx, 4, (size_t)lw, out);
    }
    int32_t ink[ii::kInkWords];
    ii::fold_ink(blocks.data(), tiles, ink);
    fwrite(ink, 4, ii::kInkWords, out);
    fwrite(scratch.data(), 4, scratch.size(), out);
    cases++;
  }
  fclose(in);
  fclose(out);
  printf("cases %ld workgroups %ld passes %ld", cases, emu::workgroups, emu::passes);
  for (int b = 0; b < 12; b++) printf(" b%d_cases %ld b%d_wide_0 %ld b%d_wide_1 %ld b%d_wide_2 %ld b%d_wide_3 %ld", b, per_build[b], b, wide[b][0], b, wide[b][1], b, wide[b][2], b, wide[b][3]);
  printf("\n");
  return 0;
}
