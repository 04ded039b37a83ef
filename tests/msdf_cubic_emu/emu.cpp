// tests/msdf_cubic_emu/emu.cpp -- figdraw_amd/csrc/k_msdf_cubic.hip and fdh_msdf_cubic_host.h (and k_msdf.hip with fdh_msdf_host.h, to compare
// with) under the sequential host shim (tests/emu/fdh_device.h); tests/test_msdf_cubic_host.py copies it here, and the four from csrc, unmodified.
// k_msdf_generate_cubic, then k_msdf_correct_cubic on what it made.
// usage: emu W H RANGE segs.raw   (segs.raw: n x 8 float32; c2x = NaN: a quadratic, c1x = NaN: a line)
//        emu flatten segs.raw     -> writes lines.raw, m x 4 float32: the coverage path's lines of the outline (msdf::cubic::flatten_outline)
// -> writes texels.raw (W x H RGBA8, the uncorrected field) and corrected.raw; where the outline holds no cubic also plain.raw, the field
//    k_msdf_generate makes of the same outline in the 6-float format; prints the workgroups, those that walked the edges for the
//    correction and the rounds they took, and the edges by kind.
//    exit 3: an open contour; exit 1: a byte outside an image was written, or the correction's input was; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_msdf.hip"
#include "k_msdf_cubic.hip"
#include <cstring>
static bool read_floats(const char* path, std::vector<float>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  float v;
  while (fread(&v, 4, 1, f) == 1) out->push_back(v);
  fclose(f);
  return true;
}
int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "flatten")) {
    std::vector<float> segs, lines;
    if (!read_floats(argv[2], &segs)) return 2;
    fdh::msdf::cubic::flatten_outline(segs.data(), (int)(segs.size() / 8), &lines);
    FILE* f = fopen("lines.raw", "wb"); fwrite(lines.data(), 4, lines.size(), f); fclose(f);
    return 0;
  }
  if (argc != 5) return 2;
  const int W = atoi(argv[1]), H = atoi(argv[2]), pad = 64;
  const float range = (float)atof(argv[3]);
  std::vector<float> segs;
  if (!read_floats(argv[4], &segs)) return 2;
  FILE* f;
  namespace mc = fdh::msdf::cubic;
  const int n_segs = (int)(segs.size() / 8);
  mc::Shape shape;
  if (!mc::build_shape(segs.data(), n_segs, &shape)) return 3;
  std::vector<float> rec;
  mc::edge_records(shape, &rec);
  const int n_edges = (int)shape.edges.size();
  const size_t n = (size_t)W * H;
  // exactly-sized allocations: a read or a write past either end is an error under AddressSanitizer, a write also without it (the pads)
  std::vector<uint32_t> gen(n + 2 * pad, 0xEEEEEEEEu), out(n + 2 * pad, 0xEEEEEEEEu), plain(n + 2 * pad, 0xEEEEEEEEu);
  fdh::launch_msdf_generate_cubic(nullptr, rec.data(), n_edges, W, H, (float)shape.orient, range, gen.data() + pad);
  uint32_t* in = new uint32_t[n];  // no slack at all around what the correction reads
  memcpy(in, gen.data() + pad, n * 4);
  const std::vector<uint32_t> before(in, in + n);
  emu::ballots = emu::rounds = emu::workgroups = emu::workgroups_with_rounds = 0;
  fdh::launch_msdf_correct_cubic(nullptr, rec.data(), n_edges, W, H, (float)shape.orient, range, in, out.data() + pad);
  const bool input_written = memcmp(in, before.data(), n * 4) != 0;
  delete[] in;
  if (input_written) { printf("the input was written\n"); return 1; }
  const bool cubic_free = !mc::holds_cubic(segs.data(), n_segs);
  if (cubic_free) {
    std::vector<float> six, rec6;
    mc::to_quadratic_format(segs.data(), n_segs, &six);
    fdh::msdf::Shape s6;
    if (!fdh::msdf::build_shape(six.data(), n_segs, &s6)) return 3;
    fdh::msdf::edge_records(s6, &rec6);
    fdh::launch_msdf_generate(nullptr, rec6.data(), (int)s6.edges.size(), W, H, (float)s6.orient, range, plain.data() + pad);
  }
  for (int i = 0; i < pad; i++)
    if (gen[i] != 0xEEEEEEEEu || gen[n + pad + i] != 0xEEEEEEEEu || out[i] != 0xEEEEEEEEu || out[n + pad + i] != 0xEEEEEEEEu || plain[i] != 0xEEEEEEEEu ||
        plain[n + pad + i] != 0xEEEEEEEEu) { printf("overrun\n"); return 1; }
  f = fopen("texels.raw", "wb"); fwrite(gen.data() + pad, 4, n, f); fclose(f);
  f = fopen("corrected.raw", "wb"); fwrite(out.data() + pad, 4, n, f); fclose(f);
  if (cubic_free) { f = fopen("plain.raw", "wb"); fwrite(plain.data() + pad, 4, n, f); fclose(f); }
  int kinds[3] = {0, 0, 0};
  for (const mc::Edge& e : shape.edges) kinds[e.kind]++;
  printf("workgroups %ld with_rounds %ld rounds %ld lines %d quadratics %d cubics %d\n", emu::workgroups, emu::workgroups_with_rounds, emu::rounds, kinds[0], kinds[1], kinds[2]);
  return 0;
}
