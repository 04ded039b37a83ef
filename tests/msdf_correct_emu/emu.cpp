// tests/msdf_correct_emu/emu.cpp -- figdraw_amd/csrc/k_msdf.hip and fdh_msdf_host.h under the sequential host shim (tests/emu/fdh_device.h;
// tests/test_msdf_correct_host.py copies it here, and the two from csrc, unmodified): k_msdf_generate, then k_msdf_correct on what it made.
// usage: emu W H RANGE segs.raw [field.raw]   (segs.raw: n x 6 float32, cx = NaN for a line; field.raw: W x H RGBA8 to correct in place of
//                                              the generated texels)
// -> writes texels.raw (W x H RGBA8, the uncorrected field) and corrected.raw, prints the workgroups, those that walked the edges and the
//    rounds they took; exit 3: an open contour; exit 1: a byte outside an image was written, or the input was; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_msdf.hip"
#include <cstring>
int main(int argc, char** argv) {
  if (argc != 5 && argc != 6) return 2;
  const int W = atoi(argv[1]), H = atoi(argv[2]), pad = 64;
  const float range = (float)atof(argv[3]);
  std::vector<float> segs;
  FILE* f = fopen(argv[4], "rb");
  if (!f) return 2;
  float v;
  while (fread(&v, 4, 1, f) == 1) segs.push_back(v);
  fclose(f);
  fdh::msdf::Shape shape;
  if (!fdh::msdf::build_shape(segs.data(), (int)(segs.size() / 6), &shape)) return 3;
  std::vector<float> rec;
  fdh::msdf::edge_records(shape, &rec);
  const size_t n = (size_t)W * H;
  // exactly-sized allocations: a read or a write past either end is an error under AddressSanitizer, a write also without it (the pads)
  std::vector<uint32_t> gen(n + 2 * pad, 0xEEEEEEEEu), out(n + 2 * pad, 0xEEEEEEEEu);
  fdh::launch_msdf_generate(nullptr, rec.data(), (int)shape.edges.size(), W, H, (float)shape.orient, range, gen.data() + pad);
  if (argc == 6) {
    f = fopen(argv[5], "rb");
    if (!f || fread(gen.data() + pad, 4, n, f) != n) return 2;
    fclose(f);
  }
  uint32_t* in = new uint32_t[n];  // no slack at all around what the correction reads
  memcpy(in, gen.data() + pad, n * 4);
  const std::vector<uint32_t> before(in, in + n);
  emu::ballots = emu::rounds = emu::workgroups = emu::workgroups_with_rounds = 0;
  fdh::launch_msdf_correct(nullptr, rec.data(), (int)shape.edges.size(), W, H, (float)shape.orient, range, in, out.data() + pad);
  const bool input_written = memcmp(in, before.data(), n * 4) != 0;
  delete[] in;
  if (input_written) { printf("the input was written\n"); return 1; }
  for (int i = 0; i < pad; i++)
    if (gen[i] != 0xEEEEEEEEu || gen[n + pad + i] != 0xEEEEEEEEu || out[i] != 0xEEEEEEEEu || out[n + pad + i] != 0xEEEEEEEEu) { printf("overrun\n"); return 1; }
  f = fopen("texels.raw", "wb"); fwrite(gen.data() + pad, 4, n, f); fclose(f);
  f = fopen("corrected.raw", "wb"); fwrite(out.data() + pad, 4, n, f); fclose(f);
  printf("workgroups %ld with_rounds %ld rounds %ld\n", emu::workgroups, emu::workgroups_with_rounds, emu::rounds);
  return 0;
}
