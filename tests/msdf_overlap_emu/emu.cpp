// tests/msdf_overlap_emu/emu.cpp -- figdraw_amd/csrc/k_msdf.hip and fdh_msdf_host.h (from csrc, unmodified: tests/test_msdf_overlap_host.py
// copies them here) under the sequential host shim, tests/emu/fdh_device.h, which the test copies here; built two ways:
//   as it is                              64 lanes of a wave together, with the ballot: k_msdf_generate, k_msdf_generate_union, k_msdf_correct_union
//   -DEMU_LANES_ALONE -DEMU_GENERATE_ONLY  a lane at a time: the two generators alone (the 16 383-contour outline,
//                                         and the -DFDH_MSDF_NO_CULL=1 build)
// usage: emu W H RANGE segs.raw     (segs.raw: n x 6 float32, cx = NaN for a line)
// -> writes plain.raw (k_msdf_generate), union.raw (k_msdf_generate_union) and, unless EMU_GENERATE_ONLY, corrected.raw (k_msdf_correct_union
//    on union.raw), each W x H RGBA8; prints the contours and how many are holes;
//    exit 3: an open contour; exit 1: a byte outside an image was written, or the correction's input was; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_msdf.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
static bool pads_intact(const std::vector<uint32_t>& v, size_t n, int pad) {
  for (int i = 0; i < pad; i++)
    if (v[i] != 0xEEEEEEEEu || v[n + pad + i] != 0xEEEEEEEEu) return false;
  return true;
}
static void save(const char* name, const uint32_t* p, size_t n) {
  FILE* f = fopen(name, "wb");
  fwrite(p, 4, n, f);
  fclose(f);
}
int main(int argc, char** argv) {
  if (argc != 5) return 2;
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
  std::vector<float> rec;  // exactly sized: a record read past the last one is an error under AddressSanitizer
  fdh::msdf::edge_records(shape, &rec);
  const int n_edges = (int)shape.edges.size();
  const size_t n = (size_t)W * H;
  std::vector<uint32_t> plain(n + 2 * pad, 0xEEEEEEEEu), uni(n + 2 * pad, 0xEEEEEEEEu), out(n + 2 * pad, 0xEEEEEEEEu);
  fdh::launch_msdf_generate(nullptr, rec.data(), n_edges, W, H, (float)shape.orient, range, plain.data() + pad);
  fdh::launch_msdf_generate_union(nullptr, rec.data(), n_edges, W, H, (float)shape.orient, range, uni.data() + pad);
  if (!pads_intact(plain, n, pad) || !pads_intact(uni, n, pad)) { printf("overrun\n"); return 1; }
  save("plain.raw", plain.data() + pad, n);
  save("union.raw", uni.data() + pad, n);
#ifndef EMU_GENERATE_ONLY
  uint32_t* in = new uint32_t[n];  // no slack at all around what the correction reads
  memcpy(in, uni.data() + pad, n * 4);
  fdh::launch_msdf_correct_union(nullptr, rec.data(), n_edges, W, H, (float)shape.orient, range, in, out.data() + pad);
  const bool input_written = memcmp(in, uni.data() + pad, n * 4) != 0;
  delete[] in;
  if (input_written) { printf("the input was written\n"); return 1; }
  if (!pads_intact(out, n, pad)) { printf("overrun\n"); return 1; }
  save("corrected.raw", out.data() + pad, n);
#endif
  int holes = 0;
  for (bool filled : shape.filled) holes += !filled;
  printf("contours %d holes %d\n", (int)shape.filled.size(), holes);
  return 0;
}
