// tests/device_images_emu/emu.cpp -- the batched kernels of figdraw_amd/csrc/k_image_import.hip under the sequential host shim (tests/emu/fdh_device.h),
// over the tables fdh_image_batch.h makes; the kernel's source and the headers come from csrc, unmodified: tests/test_device_images_host.py
// copies them here.  Built twice: emu, and emu_san (the same under AddressSanitizer and UBSan).  The launches are
// Importer::make's for an ImageBatch (fdh_import.cpp): one per format present, one for the tails.
// usage: emu batch.bin out.bin
//   batch.bin: four int32 -- n, atlas_size, n_levels, out_rows -- then per image twelve int32 -- w, h, format, channels, flags, pitch_bytes,
//              plane_bytes, data_offset, source_bytes, x, y, 0 -- and source_bytes bytes: the source, which the kernel gets at an address
//              data_offset past a 16-byte boundary, in a block that ends with it (a read past either end is an error under AddressSanitizer)
//   out.bin:   of every level l its first min(size >> l, (out_rows >> l) + 2) rows, whole, level 0 first (a texel nothing stored is
//              0xEEEEEEEE); then per image the 64 words of its ink blocks as the host folds them (fold_ink; the start values where the
//              batch measures no ink boxes of the image on the device)
// exit 1: a texel below the rows that are written out was stored; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_image_import.hip"
#include "fdh_image_batch.h"
#include <vector>
namespace ii = fdh::image_import;
namespace ib = fdh::image_batch;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const uint32_t kFill = 0xEEEEEEEEu;
  int32_t top[4];
  if (fread(top, 4, 4, in) != 4) return 2;
  const int n = top[0], size = top[1], n_levels = top[2], out_rows = top[3];
  if (n < 1 || n > ib::kMaxImages || size < 16 || (size & (size - 1)) || n_levels < 1 || n_levels > ii::kLevels || (size >> (n_levels - 1)) < 1) return 2;
  std::vector<unsigned char*> blocks((size_t)n);
  std::vector<ii::BatchImage> tab((size_t)n);
  for (int i = 0; i < n; i++) {
    int32_t head[12];
    if (fread(head, 4, 12, in) != 12) return 2;
    const int w = head[0], h = head[1], offset = head[7], bytes = head[8], x = head[9], y = head[10];
    if (w < 1 || h < 1 || w > ii::kBatchMaxExtent || h > ii::kBatchMaxExtent || offset < 0 || offset > 15 || bytes < 1 || x < 0 || y < 0 || x + w > size || y + h > size) return 2;
    blocks[(size_t)i] = new unsigned char[(size_t)offset + bytes];
    if (fread(blocks[(size_t)i] + offset, 1, bytes, in) != (size_t)bytes) return 2;
    ii::BatchImage& t = tab[(size_t)i];
    t = ii::BatchImage{};
    t.data = blocks[(size_t)i] + offset; t.pitch_bytes = head[5]; t.plane_bytes = head[6];
    t.w = w; t.h = h; t.format = (uint32_t)head[2]; t.channels = (uint32_t)head[3]; t.flags = (uint32_t)head[4];
    const bool planes = t.format != ii::kRgba8 && t.channels > 1;
    t.wide = (uintptr_t)t.data % 16 == 0 && t.pitch_bytes % 16 == 0 && (!planes || t.plane_bytes % 16 == 0) && w >= 4;
    t.x = x; t.y = y;
  }
  fclose(in);
  ib::Tables T;
  ib::tables(tab, 0, n, n_levels, &T);
  if (T.words.size() > ib::table_words(tab, ii::kLevels)) return 3;  // what was reserved holds what is copied
  // the buffers exactly as large as the tables say: the records and the words, a texel of scratch per tile, an ink block per tile with ink
  const std::vector<uint32_t> words(T.words);
  std::vector<uint32_t> scratch((size_t)T.n_tiles, kFill);
  std::vector<int32_t> ink((size_t)T.ink_blocks * ii::kInkWords, -1);
  std::vector<std::vector<uint32_t>> levels;
  for (int l = 0; l < n_levels; l++) levels.emplace_back((size_t)(size >> l) * (size >> l), kFill);
  ii::BatchAtlas A{};
  for (int l = 0; l < n_levels; l++) A.level[l] = levels[(size_t)l].data();
  A.size = size;
  const ii::BatchImage* images = reinterpret_cast<const ii::BatchImage*>(words.data());
  const uint32_t* owner = words.data() + T.owner_at;
  int launches = 0;
  for (int f = 0; f < ib::kFormats; f++) {
    if (!T.tile_count[f]) continue;
    fdh::launch_image_import_batch(nullptr, (uint32_t)f, images, words.data() + T.tiles_at + T.tile_first[f], (int)T.tile_count[f], A, scratch.data(), ink.data(), owner);
    launches++;
  }
  if (T.n_tails) { fdh::launch_image_import_tail_batch(nullptr, images, words.data() + T.tails_at, (int)T.n_tails, A, scratch.data(), owner); launches++; }
  for (unsigned char* b : blocks) delete[] b;
  for (int l = 0; l < n_levels; l++) {
    const int LS = size >> l, rows = LS < (out_rows >> l) + 2 ? LS : (out_rows >> l) + 2;
    fwrite(levels[(size_t)l].data(), 4, (size_t)rows * LS, out);
    for (size_t i = (size_t)rows * LS; i < levels[(size_t)l].size(); i++)
      if (levels[(size_t)l][i] != kFill) { printf("level %d written at (%zu, %zu)\n", l, i % LS, i / LS); return 1; }
  }
  for (int k = 0; k < n; k++) {
    int32_t got[ii::kInkWords];
    ii::fold_ink(ink.data() + (size_t)images[k].ink_off * ii::kInkWords, images[k].ink ? images[k].lw[ii::kTileLevels - 1] * images[k].lh[ii::kTileLevels - 1] : 0, got);
    fwrite(got, 4, ii::kInkWords, out);
  }
  fclose(out);
  printf("images %d tiles %u tails %u launches %d workgroups %ld passes %ld\n", n, T.n_tiles, T.n_tails, launches, emu::workgroups, emu::passes);
  return 0;
}
