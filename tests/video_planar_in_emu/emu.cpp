// tests/video_planar_in_emu/emu.cpp -- figdraw_amd/csrc/k_video_planar_import.hip under the sequential host shim (tests/emu/fdh_device.h), with
// k_image_import.hip for the tail kernel; the kernels' sources and their parameter headers come from csrc, unmodified:
// tests/test_video_planar_host.py copies them here.  Built twice: emu, and emu_san (the same under AddressSanitizer and UBSan, which also
// refuses a wide load at an address that is no multiple of its size).  The launches are Importer::import_one's for a PlanarSource (fdh_import.cpp)
// for a frame of up to 2048 x 2048.
// usage: emu cases.bin out.bin
//   cases.bin: per case twenty int32 -- w, h, format, matrix, range, flags, pitch[3], offset[3], bytes[3], x, y, atlas_size, n_levels, 0 --
//              and bytes[0] + bytes[1] + bytes[2] bytes: the planes Y, Cb, Cr.  The kernel gets each plane at an address offset[p] past a
//              16-byte boundary, in a block of its own that ends with the plane's last sample (a read past either end is an error under
//              AddressSanitizer)
//   out.bin:   per case every stored level's rectangle, ceil(w / 2^l) x ceil(h / 2^l) texels, level 0 first, then the 64 words of the ink
//              blocks as the host folds them (fold_ink; the start values where the image has no ink boxes), then the level-5 image, ceil(w / 32) x
//              ceil(h / 32) texels
// exit 1: a texel outside the entry's rectangles was written; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_image_import.hip"
#include "k_video_planar_import.hip"
#include "fdh_video_import.h"
#include <vector>
namespace ii = fdh::image_import;
namespace vp = fdh::video_planar;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const uint32_t kFill = 0xEEEEEEEEu;
  int32_t head[20];
  long cases = 0, wide[3] = {0, 0, 0};
  while (fread(head, 4, 20, in) == 20) {
    const int w = head[0], h = head[1], x = head[15], y = head[16], size = head[17], n_levels = head[18];
    const uint32_t format = (uint32_t)head[2], matrix = (uint32_t)head[3], range = (uint32_t)head[4];
    if (w < 1 || h < 1 || w > 2048 || h > 2048 || format < vp::kI420 || format > vp::kI410 || matrix > 2 || range > 1 || n_levels < 1 || n_levels > ii::kLevels || x < 0 || y < 0 || x + w > size || y + h > size) return 2;
    const bool full = vp::full_chroma(format);
    const int es = vp::ten_bit(format) ? 2 : 1;
    unsigned char* plane[3] = {nullptr, nullptr, nullptr};
    vp::InParams P{};
    P.w = w; P.h = h; P.cw = full ? w : (w + 1) / 2; P.ch = full ? h : (h + 1) / 2;
    for (int p = 0; p < 3; p++) {
      const int offset = head[9 + p], bytes = head[12 + p];
      const int64_t pitch = head[6 + p], row = (int64_t)(p ? P.cw : w) * es, run = (p && !full ? vp::kRun / 2 : vp::kRun) * es;
      if (offset < 0 || offset > 15 || pitch < row || bytes != ((p ? P.ch : h) - 1) * pitch + row) return 2;
      plane[p] = new unsigned char[(size_t)offset + bytes];
      if (fread(plane[p] + offset, 1, bytes, in) != (size_t)bytes) return 2;
      P.plane[p] = plane[p] + offset; P.pitch[p] = pitch;
      P.wide[p] = (uintptr_t)P.plane[p] % (uintptr_t)run == 0 && pitch % run == 0 && row >= run;
      wide[p] += P.wide[p];
    }
    P.format = format; P.flags = (uint32_t)head[5];
    const int32_t* c = fdh::video_import::kCoefficients[vp::ten_bit(format)][matrix][range];
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
    fdh::launch_video_planar_import(nullptr, P);
    if (ii::kTileLevels < P.n_store) {
      ii::TailParams T{};
      T.src = scratch.data(); T.sw = P.lw[5]; T.sh = P.lh[5]; T.l0 = ii::kTileLevels - 1; T.n_store = P.n_store;
      T.x = x; T.y = y; T.size = size;
      for (int l = 0; l < n_levels; l++) T.level[l] = P.level[l];
      fdh::launch_image_import_tail(nullptr, T);
    }
    for (int p = 0; p < 3; p++) delete[] plane[p];
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
  printf("cases %ld wide_y %ld wide_cb %ld wide_cr %ld workgroups %ld passes %ld\n", cases, wide[0], wide[1], wide[2], emu::workgroups, emu::passes);
  return 0;
}
