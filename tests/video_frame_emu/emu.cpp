// tests/video_frame_emu/emu.cpp -- figdraw_amd/csrc/k_video_import.hip under the sequential host shim (tests/emu/fdh_device.h), with k_image_import.hip for
// the tail kernel; the kernels' sources and their two parameter headers come from csrc, unmodified: tests/test_video_frame_host.py copies
// them here.  Built twice: emu, and emu_san (the same under AddressSanitizer and UBSan).  The launches are Importer::import_one's
// for a VideoSource (fdh_import.cpp) for a frame of up to 2048 x 2048.
// usage: emu cases.bin out.bin
//   cases.bin: per case sixteen int32 -- w, h, format, matrix, range, flags, pitch_y, pitch_c, offset_y, offset_c, bytes_y, bytes_c, x, y,
//              atlas_size, n_levels -- and bytes_y + bytes_c bytes: the luma plane, then the chroma plane (bytes_c = 0: none).  The kernel
//              gets each plane at an address offset_* past a 16-byte boundary, in a block of its own that ends with the plane's last
//              element (a read past either end is an error under AddressSanitizer)
//   out.bin:   per case every stored level's rectangle, ceil(w / 2^l) x ceil(h / 2^l) texels, level 0 first, then the 64 words of the ink
//              blocks as the host folds them (fold_ink; the start values where the image has no ink boxes), then the level-5 image, ceil(w / 32) x
//              ceil(h / 32) texels
// exit 1: a texel outside the entry's rectangles was written; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_image_import.hip"
#include "k_video_import.hip"
#include <vector>
namespace ii = fdh::image_import;
namespace vi = fdh::video_import;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const uint32_t kFill = 0xEEEEEEEEu;
  int32_t head[16];
  long cases = 0;
  while (fread(head, 4, 16, in) == 16) {
    const int w = head[0], h = head[1], x = head[12], y = head[13], size = head[14], n_levels = head[15];
    const uint32_t format = (uint32_t)head[2], matrix = (uint32_t)head[3], range = (uint32_t)head[4];
    if (w < 1 || h < 1 || w > 2048 || h > 2048 || format > vi::kP010 || matrix > 2 || range > 1 || n_levels < 1 || n_levels > ii::kLevels || x < 0 || y < 0 || x + w > size || y + h > size) return 2;
    unsigned char* plane[2] = {nullptr, nullptr};
    const unsigned char* data[2] = {nullptr, nullptr};
    for (int p = 0; p < 2; p++) {
      const int offset = head[8 + p], bytes = head[10 + p];
      if (offset < 0 || offset > 15 || bytes < 0 || (p == 0 && bytes < 1) || ((format != vi::kBgra8) != (bytes > 0) && p == 1)) return 2;
      if (!bytes) continue;
      plane[p] = new unsigned char[(size_t)offset + bytes];
      if (fread(plane[p] + offset, 1, bytes, in) != (size_t)bytes) return 2;
      data[p] = plane[p] + offset;
    }
    std::vector<std::vector<uint32_t>> levels;
    for (int l = 0; l < n_levels; l++) levels.emplace_back((size_t)(size >> l) * (size >> l), kFill);
    vi::Params P{};
    P.luma = data[0]; P.chroma = data[1]; P.pitch_y = head[6]; P.pitch_c = head[7];
    P.w = w; P.h = h; P.cw = (w + 1) / 2; P.ch = (h + 1) / 2;
    P.format = format; P.flags = (uint32_t)head[5];
    const uintptr_t run = format == vi::kBgra8 ? 16 : format == vi::kP010 ? 8 : 4;
    P.wide_y = (uintptr_t)P.luma % run == 0 && P.pitch_y % (int64_t)run == 0 && w >= 4;
    P.wide_c = format != vi::kBgra8 && (uintptr_t)P.chroma % run == 0 && P.pitch_c % (int64_t)run == 0 && P.cw >= 2;
    if (format != vi::kBgra8) {
      const int32_t* c = vi::kCoefficients[format == vi::kP010][matrix][range];
      P.yoff = c[0]; P.coff = c[1]; P.cy = c[2]; P.crv = c[3]; P.cgu = c[4]; P.cgv = c[5]; P.cbu = c[6];
    }
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
    fdh::launch_video_import(nullptr, P);
    if (ii::kTileLevels < P.n_store) {
      ii::TailParams T{};
      T.src = scratch.data(); T.sw = P.lw[5]; T.sh = P.lh[5]; T.l0 = ii::kTileLevels - 1; T.n_store = P.n_store;
      T.x = x; T.y = y; T.size = size;
      for (int l = 0; l < n_levels; l++) T.level[l] = P.level[l];
      fdh::launch_image_import_tail(nullptr, T);
    }
    delete[] plane[0];
    delete[] plane[1];
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
  printf("cases %ld workgroups %ld passes %ld\n", cases, emu::workgroups, emu::passes);
  return 0;
}
