// tests/msdf_emu/emu.cpp -- figdraw_amd/csrc/k_msdf.hip and fdh_msdf_host.h under the sequential host shim (tests/emu/fdh_device.h, built with
// -DEMU_LANES_ALONE: waves of one lane; tests/test_msdf_host.py copies it here, and the two from csrc, unmodified).
// usage: emu W H RANGE segs.raw          (segs.raw: n x 6 float32, cx = NaN for a line)
// -> writes texels.raw (W x H RGBA8) and edges.raw (the records, kEdgeFloats float32 each, then one float32: the orientation);
//    exit 3: an open contour; exit 1: a byte outside the image was written
#include "fdh_device.h"
#include "k_msdf.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>
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
  std::vector<float> rec;
  fdh::msdf::edge_records(shape, &rec);
  std::vector<uint32_t> out((size_t)W * H + 2 * pad, 0xEEEEEEEEu);
  fdh::launch_msdf_generate(nullptr, rec.data(), (int)shape.edges.size(), W, H, (float)shape.orient, range, out.data() + pad);
  for (int i = 0; i < pad; i++)
    if (out[i] != 0xEEEEEEEEu || out[(size_t)W * H + pad + i] != 0xEEEEEEEEu) { printf("overrun\n"); return 1; }
  f = fopen("texels.raw", "wb"); fwrite(out.data() + pad, 4, (size_t)W * H, f); fclose(f);
  const float orient = (float)shape.orient;
  f = fopen("edges.raw", "wb"); if (!rec.empty()) fwrite(rec.data(), 4, rec.size(), f); fwrite(&orient, 4, 1, f); fclose(f);
  return 0;
}
