// tests/device_image_emu/emu.cpp -- figdraw_amd/csrc/k_image_import.hip under the sequential host shim (tests/emu/fdh_device.h); the kernel's source and
// fdh_image_import.h come from csrc, unmodified: tests/test_device_image_host.py copies them here.  Built twice: emu, and emu_san (the same
// under AddressSanitizer and UBSan).  The launches are Importer::import_one's for an ImageSource (fdh_import.cpp) for a source of up to 2048 x 2048.
// usage: emu cases.bin out.bin
//   cases.bin: per case fourteen int32 -- w, h, format, channels, flags, pitch_bytes, plane_bytes, data_offset, source_bytes, x, y,
//              atlas_size, n_levels, 0 -- and source_bytes bytes: the source, which the kernel gets at an address data_offset past a
//              16-byte boundary, in a block that ends with it (a read past either end is an error under AddressSanitizer)
//   out.bin:   per case every stored level's rectangle, ceil(w / 2^l) x ceil(h / 2^l) texels, level 0 first, then the 64 words of the ink
//              blocks as the host folds them (fold_ink; the start values where the image has no ink boxes)
// exit 1: a texel outside the entry's rectangles was written; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_image_import.hip"
#include <vector>
namespace ii = fdh::image_import;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const uint32_t kFill = 0xEEEEEEEEu;
  int32_t head[14];
  long cases = 0;
  while (fread(head, 4, 14, in) == 14) {
    const int w = head[0], h = head[1], offset = head[7], bytes = head[8], x = head[9], y = head[10], size = head[11], n_levels = head[12];
    if (w < 1 || h < 1 || w > 2048 || h > 2048 || offset < 0 || offset > 15 || bytes < 1 || n_levels < 1 || n_levels > ii::kLevels || x < 0 || y < 0 || x + w > size || y + h > size) return 2;
    unsigned char* block = new unsigned char[(size_t)offset + bytes];
    if (fread(block + offset, 1, bytes, in) != (size_t)bytes) return 2;
    std::vector<std::vector<uint32_t>> levels;
    for (int l = 0; l < n_levels; l++) levels.emplace_back((size_t)(size >> l) * (size >> l), kFill);
    ii::Params P{};
    P.data = block + offset; P.pitch_bytes = head[5]; P.plane_bytes = head[6];
    P.w = w; P.h = h; P.format = (uint32_t)head[2]; P.channels = (uint32_t)head[3]; P.flags = (uint32_t)head[4];
    const bool planes = P.format != ii::kRgba8 && P.channels > 1;
    P.wide = (uintptr_t)P.data % 16 == 0 && P.pitch_bytes % 16 == 0 && (!planes || P.plane_bytes % 16 == 0) && w >= 4;
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
    fdh::launch_image_import(nullptr, P);
    if (ii::kTileLevels < P.n_store) {
      ii::TailParams T{};
      T.src = scratch.data(); T.sw = P.lw[5]; T.sh = P.lh[5]; T.l0 = ii::kTileLevels - 1; T.n_store = P.n_store;
      T.x = x; T.y = y; T.size = size;
      for (int l = 0; l < n_levels; l++) T.level[l] = P.level[l];
      fdh::launch_image_import_tail(nullptr, T);
    }
    delete[] block;
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
    cases++;
  }
  fclose(in);
  fclose(out);
  printf("cases %ld workgroups %ld passes %ld\n", cases, emu::workgroups, emu::passes);
  return 0;
}
