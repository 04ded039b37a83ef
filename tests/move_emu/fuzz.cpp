// tests/move_emu/fuzz.cpp -- the decoder of figdraw_amd/csrc/fdh_tile_decode.cpp over mutated version-2 streams, as a stand-alone program
// (built with -fsanitize=address,undefined: directory, payload and image live in heap blocks of their exact sizes, so a read or a write
// past any of them is reported).  usage: fuzz W H image.raw dir.bin payload.bin rounds
// Every round mutates a few bytes of a valid stream, or cuts the payload short, and decodes it into a copy of the image: a refused
// stream must leave the copy as it was; an accepted one may write what it likes, inside the image.  Prints "fuzz: OK <accepted> <refused>".
#include "fdh_tile_decode.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

static std::vector<uint8_t> slurp(const char* name) {
  std::vector<uint8_t> v;
  FILE* f = fopen(name, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", name); exit(2); }
  uint8_t buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const int W = atoi(argv[1]), H = atoi(argv[2]), rounds = atoi(argv[6]);
  const std::vector<uint8_t> image = slurp(argv[3]), dir = slurp(argv[4]), payload = slurp(argv[5]);
  if (image.size() != (size_t)W * H * 4 || dir.size() % sizeof(FdhCodedTile) != 0 || dir.empty()) return 2;
  const int n_tiles = (int)(dir.size() / sizeof(FdhCodedTile));
  std::string why;
  {  // the stream as it is decodes
    std::unique_ptr<uint8_t[]> img(new uint8_t[image.size()]);
    std::memcpy(img.get(), image.data(), image.size());
    if (!fdh::decode_tiles("fuzz", 2, img.get(), (int64_t)4 * W, W, H, reinterpret_cast<const FdhCodedTile*>(dir.data()), n_tiles, payload.data(),
                           (int64_t)payload.size(), &why)) { printf("the valid stream was refused: %s\n", why.c_str()); return 1; }
  }
  int accepted = 0, refused = 0;
  for (int round = 0; round < rounds; round++) {
    const size_t n_pay = (rnd() % 4 == 0 && !payload.empty()) ? rnd() % payload.size() : payload.size();  // a quarter of the rounds: cut short
    std::unique_ptr<FdhCodedTile[]> d(new FdhCodedTile[(size_t)n_tiles]);
    std::unique_ptr<uint8_t[]> p(new uint8_t[n_pay ? n_pay : 1]), img(new uint8_t[image.size()]);
    std::memcpy(d.get(), dir.data(), dir.size());
    std::memcpy(p.get(), payload.data(), n_pay);
    std::memcpy(img.get(), image.data(), image.size());
    uint8_t* const db = reinterpret_cast<uint8_t*>(d.get());
    for (int k = 1 + (int)(rnd() % 3); k > 0; k--) {
      const uint32_t how = rnd() % 5;
      if (how == 0 && n_pay) p[rnd() % n_pay] ^= (uint8_t)(1u << (rnd() % 8));
      else if (how == 1) db[rnd() % dir.size()] = (uint8_t)rnd();
      else if (how == 2) d[rnd() % (uint32_t)n_tiles].mode = (uint8_t)(rnd() % 6);
      else if (how == 3) d[rnd() % (uint32_t)n_tiles].solid = rnd() % 2 ? rnd() : (uint32_t)(uint16_t)(int16_t)((int)(rnd() % 300) - 150) | (uint32_t)(uint16_t)(int16_t)((int)(rnd() % 300) - 150) << 16;
      else db[rnd() % dir.size()] ^= (uint8_t)(1u << (rnd() % 8));
    }
    if (fdh::decode_tiles("fuzz", 2, img.get(), (int64_t)4 * W, W, H, d.get(), n_tiles, n_pay ? p.get() : nullptr, (int64_t)n_pay, &why)) accepted++;
    else {
      refused++;
      if (std::memcmp(img.get(), image.data(), image.size()) != 0) { printf("round %d: a refused stream wrote into the image (%s)\n", round, why.c_str()); return 1; }
    }
  }
  printf("fuzz: OK %d %d\n", accepted, refused);
  return 0;
}
