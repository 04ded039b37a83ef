// tests/atlas_move_emu/emu.cpp -- figdraw_amd/csrc/k_atlas_move.hip and the table builder fdh_atlas_move.h under the sequential host shim
// (tests/emu/fdh_device.h); tests/test_atlas_move_host.py copies it here, and both sources from csrc, unmodified.  Built twice: emu, and emu_san (the same
// stand-alone program under AddressSanitizer and UBSan).
// usage: emu case.bin out.bin
//   case.bin: int32 from_size, to_size, n_rects, buf_in_words, buf_out_words; the levels of the old atlas, level 0 first, down to 1 x 1 (or
//             fdh::move::kLevels of them), RGBA8; buf_in_words words; then per rectangle nine int32: src_level, sx, sy, dst_level, dx, dy,
//             w, h, copy -- in the painter's order of the destination
//   out.bin:  the levels of the new atlas (they start as zeros), then buf_out_words words (they start as 0xEEEEEEEE)
// Every level and both buffers are heap blocks of exactly their size: AddressSanitizer sees a texel read or written outside one.
// prints records, tiles, owner words, the lowest owner level and the workgroups run
#include "fdh_device.h"
#include "k_atlas_move.hip"
#include <cstring>
#include <memory>
static int levels_of(int size) {
  int n = 0;
  for (int ls = size; ls >= 1 && n < fdh::move::kLevels; ls >>= 1) n++;
  return n;
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[5];
  if (fread(head, 4, 5, in) != 5) return 2;
  const int from_size = head[0], to_size = head[1], n_rects = head[2], in_words = head[3], out_words = head[4];
  if (from_size < 1 || to_size < 1 || from_size > 16384 || to_size > 16384 || n_rects < 0 || in_words < 0 || out_words < 0) return 2;
  fdh::move::Views V{};
  V.from_size = from_size; V.from_levels = levels_of(from_size); V.to_size = to_size; V.to_levels = levels_of(to_size);
  std::unique_ptr<uint32_t[]> from[fdh::move::kLevels], to[fdh::move::kLevels];
  for (int l = 0; l < V.from_levels; l++) {
    const size_t n = (size_t)(from_size >> l) * (from_size >> l);
    from[l].reset(new uint32_t[n]);
    if (fread(from[l].get(), 4, n, in) != n) return 2;
    V.from[l] = from[l].get();
  }
  for (int l = 0; l < V.to_levels; l++) {
    const size_t n = (size_t)(to_size >> l) * (to_size >> l);
    to[l].reset(new uint32_t[n]());
    V.to[l] = to[l].get();
  }
  std::unique_ptr<uint32_t[]> buf_in(new uint32_t[in_words ? in_words : 1]), buf_out(new uint32_t[out_words ? out_words : 1]);
  if (in_words && fread(buf_in.get(), 4, (size_t)in_words, in) != (size_t)in_words) return 2;
  for (int i = 0; i < out_words; i++) buf_out[i] = 0xEEEEEEEEu;
  V.buf_in = buf_in.get(); V.buf_out = buf_out.get();
  std::vector<fdh::move::Rect> rects;
  for (int i = 0; i < n_rects; i++) {
    int32_t r[9];
    if (fread(r, 4, 9, in) != 9) return 2;
    rects.push_back(fdh::move::Rect{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8] != 0});
  }
  fclose(in);
  fdh::move::Tables T;
  fdh::move::build_tables(rects, &T);
  // the tables as the device holds them: one block of exactly their words
  std::unique_ptr<uint32_t[]> tab(new uint32_t[T.words.size()]);
  std::memcpy(tab.get(), T.words.data(), T.words.size() * 4);
  const uint32_t* tiles = tab.get() + (size_t)T.n_records * fdh::move::kRecordWords;
  fdh::launch_atlas_move(nullptr, V, reinterpret_cast<const fdh::move::Record*>(tab.get()), tiles, (int)T.n_tiles, tiles + T.n_tiles);
  for (int l = 0; l < V.to_levels; l++) fwrite(to[l].get(), 4, (size_t)(to_size >> l) * (to_size >> l), out);
  if (out_words) fwrite(buf_out.get(), 4, (size_t)out_words, out);
  fclose(out);
  printf("records %u tiles %u owner_words %u owner_level %d texels %lld workgroups %ld\n", T.n_records, T.n_tiles, T.owner_words, T.owner_level, (long long)T.texels,
         emu::workgroups);
  return 0;
}
