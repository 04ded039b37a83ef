// tests/video_frames_emu/emu.cpp -- the batched kernels of figdraw_amd/csrc/k_video_import.hip, and k_image_import_tail_batch of k_image_import.hip,
// under the sequential host shim (tests/emu/fdh_device.h), over the tables fdh_video_batch.h makes; the kernels' sources and the headers
// come from csrc, unmodified: tests/test_video_frames_host.py copies them here.  Built twice: emu, and emu_san (the same under
// AddressSanitizer and UBSan).  The launches are Importer::make's for a VideoBatch (fdh_import.cpp): one per group present, one for the tails.
// usage: emu batch.bin out.bin
//   batch.bin: four int32 -- n, atlas_size, n_levels, out_rows -- then per frame sixteen int32 -- w, h, format, matrix, range, flags, pitch_y,
//              pitch_c, offset_y, offset_c, bytes_y, bytes_c, x, y, 0, 0 -- and bytes_y + bytes_c bytes: the luma plane, then the chroma plane
//              (bytes_c = 0: none).  The kernel gets each plane at an address offset_* past a 16-byte boundary, in a block of its own that
//              ends with the plane's last element (a read past either end is an error under AddressSanitizer)
//   out.bin:   of every level l its first min(size >> l, (out_rows >> l) + 2) rows, whole, level 0 first (a texel nothing stored is
//              0xEEEEEEEE); then per frame the 64 words of its ink blocks as the host folds them (fold_ink; the start values where the
//              frame has no ink boxes)
// exit 1: a texel below the rows that are written out was stored; exit 3: the tables outgrew what was reserved; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_image_import.hip"
#include "k_video_import.hip"
#include "fdh_video_batch.h"
#include <vector>
namespace ii = fdh::image_import;
namespace vi = fdh::video_import;
namespace vb = fdh::video_batch;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const uint32_t kFill = 0xEEEEEEEEu;
  int32_t top[4];
  if (fread(top, 4, 4, in) != 4) return 2;
  const int n = top[0], size = top[1], n_levels = top[2], out_rows = top[3];
  if (n < 1 || n > vb::kMaxFrames || size < 16 || (size & (size - 1)) || n_levels < 1 || n_levels > ii::kLevels || (size >> (n_levels - 1)) < 1) return 2;
  std::vector<unsigned char*> blocks;
  std::vector<vi::BatchFrame> tab((size_t)n);
  for (int i = 0; i < n; i++) {
    int32_t head[16];
    if (fread(head, 4, 16, in) != 16) return 2;
    const int w = head[0], h = head[1], x = head[12], y = head[13];
    const uint32_t format = (uint32_t)head[2], matrix = (uint32_t)head[3], range = (uint32_t)head[4];
    if (w < 1 || h < 1 || w > ii::kBatchMaxExtent || h > ii::kBatchMaxExtent || format > vi::kP010 || matrix > 2 || range > 1 || x < 0 || y < 0 || x + w > size || y + h > size) return 2;
    const unsigned char* data[2] = {nullptr, nullptr};
    for (int p = 0; p < 2; p++) {
      const int offset = head[8 + p], bytes = head[10 + p];
      if (offset < 0 || offset > 15 || bytes < 0 || (p == 0 && bytes < 1) || ((format != vi::kBgra8) != (bytes > 0) && p == 1)) return 2;
      if (!bytes) continue;
      blocks.push_back(new unsigned char[(size_t)offset + bytes]);
      if (fread(blocks.back() + offset, 1, bytes, in) != (size_t)bytes) return 2;
      data[p] = blocks.back() + offset;
    }
    vi::BatchFrame& t = tab[(size_t)i];
    t = vi::BatchFrame{};
    t.luma = data[0]; t.chroma = data[1]; t.pitch_y = head[6]; t.pitch_c = head[7];
    t.w = w; t.h = h; t.cw = (w + 1) / 2; t.ch = (h + 1) / 2;
    t.format = format; t.flags = (uint32_t)head[5];
    const uintptr_t run = format == vi::kBgra8 ? 16 : format == vi::kP010 ? 8 : 4;
    t.wide_y = (uintptr_t)t.luma % run == 0 && t.pitch_y % (int64_t)run == 0 && w >= 4;
    t.wide_c = format != vi::kBgra8 && (uintptr_t)t.chroma % run == 0 && t.pitch_c % (int64_t)run == 0 && t.cw >= 2;
    if (format != vi::kBgra8) {
      const int32_t* c = vi::kCoefficients[format == vi::kP010][matrix][range];
      t.yoff = c[0]; t.coff = c[1]; t.cy = c[2]; t.crv = c[3]; t.cgu = c[4]; t.cgv = c[5]; t.cbu = c[6];
    }
    t.x = x; t.y = y;
  }
  fclose(in);
  vb::Tables T;
  vb::tables(tab, 0, n, n_levels, &T);
  if (T.words.size() > vb::table_words(tab, ii::kLevels)) return 3;  // what was reserved holds what is copied
  // the buffers exactly as large as the tables say: the records and the words, a texel of scratch per tile, an ink block per tile with ink
  const std::vector<uint32_t> words(T.words);
  std::vector<uint32_t> scratch((size_t)T.n_tiles, kFill);
  std::vector<int32_t> ink((size_t)T.ink_blocks * ii::kInkWords, -1);
  std::vector<std::vector<uint32_t>> levels;
  for (int l = 0; l < n_levels; l++) levels.emplace_back((size_t)(size >> l) * (size >> l), kFill);
  ii::BatchAtlas A{};
  for (int l = 0; l < n_levels; l++) A.level[l] = levels[(size_t)l].data();
  A.size = size;
  const vi::BatchFrame* frames = reinterpret_cast<const vi::BatchFrame*>(words.data());
  const uint32_t* owner = words.data() + T.owner_at;
  int launches = 0;
  for (int g = 0; g < vb::kGroups; g++) {
    if (!T.tile_count[g]) continue;
    fdh::launch_video_import_batch(nullptr, g, frames, words.data() + T.tiles_at + T.tile_first[g], (int)T.tile_count[g], A, scratch.data(), ink.data(), owner);
    launches++;
  }
  if (T.n_tails) {
    fdh::launch_image_import_tail_batch(nullptr, reinterpret_cast<const ii::BatchImage*>(words.data() + T.tail_records_at), words.data() + T.tails_at, (int)T.n_tails, A, scratch.data(), owner);
    launches++;
  }
  for (unsigned char* b : blocks) delete[] b;
  for (int l = 0; l < n_levels; l++) {
    const int LS = size >> l, rows = LS < (out_rows >> l) + 2 ? LS : (out_rows >> l) + 2;
    fwrite(levels[(size_t)l].data(), 4, (size_t)rows * LS, out);
    for (size_t i = (size_t)rows * LS; i < levels[(size_t)l].size(); i++)
      if (levels[(size_t)l][i] != kFill) { printf("level %d written at (%zu, %zu)\n", l, i % LS, i / LS); return 1; }
  }
  for (int k = 0; k < n; k++) {
    int32_t got[ii::kInkWords];
    ii::fold_ink(ink.data() + (size_t)frames[k].ink_off * ii::kInkWords, frames[k].ink ? frames[k].lw[ii::kTileLevels - 1] * frames[k].lh[ii::kTileLevels - 1] : 0, got);
    fwrite(got, 4, ii::kInkWords, out);
  }
  fclose(out);
  printf("frames %d tiles %u tails %u launches %d workgroups %ld passes %ld\n", n, T.n_tiles, T.n_tails, launches, emu::workgroups, emu::passes);
  return 0;
}
