// tests/video_planar_out_emu/emu.cpp -- figdraw_amd/csrc/k_video_planar_export.hip under the sequential host shim (tests/emu/fdh_device.h); the
// kernel's source and its parameter headers come from csrc, unmodified: tests/test_video_planar_host.py copies them here.  Built twice: emu,
// and emu_san (the same under AddressSanitizer and UBSan, which also refuses a wide load or store at an address that is no multiple of its
// size).  The parameter block is filled as video_out::read_planes fills it (fdh_video_out.cpp).
// usage: emu cases.bin out.bin
//   cases.bin: per case sixteen int32 -- W, H of the source, the rectangle x, y, w, h, format, matrix, range, flags, pitch[3], offset[3] --
//              and W * H * 4 bytes: the source's RGBA8 texels.  The kernel gets the source in a block of its own that ends with its last
//              texel, and each plane at an address offset[p] past a 16-byte boundary, in a block of its own that ends with the plane's last
//              sample (a read or a store past either end is an error under AddressSanitizer), filled with 0xEE bytes
//   out.bin:   per case each plane from its pointer to its last sample's end: Y, Cb, Cr
#include "fdh_device.h"
#include "k_video_planar_export.hip"
#include "fdh_video_export.h"
namespace vp = fdh::video_planar;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[16];
  long cases = 0, wide_src = 0, wide[3] = {0, 0, 0};
  while (fread(head, 4, 16, in) == 16) {
    const int W = head[0], H = head[1], x = head[2], y = head[3], w = head[4], h = head[5];
    const uint32_t format = (uint32_t)head[6], matrix = (uint32_t)head[7], range = (uint32_t)head[8], flags = (uint32_t)head[9];
    if (W < 1 || H < 1 || W > 4096 || H > 4096 || x < 0 || y < 0 || w < 1 || h < 1 || x + w > W || y + h > H || format < vp::kI420 || format > vp::kI410 || matrix > 2 || range > 1) return 2;
    const bool full = vp::full_chroma(format);
    if (!full && ((x | y) & 1)) return 2;
    uint32_t* src = new uint32_t[(size_t)W * H];
    if (fread(src, 4, (size_t)W * H, in) != (size_t)W * H) return 2;
    const int64_t es = vp::ten_bit(format) ? 2 : 1;
    vp::OutParams P{};
    P.src = src + (size_t)y * W + x;
    P.src_pitch = W;
    P.w = w; P.h = h;
    P.format = format; P.flags = flags;
    P.wide_src = (uintptr_t)P.src % 16 == 0 && W % 4 == 0 && w >= vp::kRun;
    unsigned char* block[3];
    int64_t bytes[3];
    for (int p = 0; p < 3; p++) {
      const int offset = head[13 + p];
      const int64_t pitch = head[10 + p], pw = p && !full ? (w + 1) / 2 : w, ph = p && !full ? (h + 1) / 2 : h, run = (p && !full ? vp::kRun / 2 : vp::kRun) * es;
      if (offset < 0 || offset > 15 || pitch < pw * es) return 2;
      bytes[p] = (ph - 1) * pitch + pw * es;
      block[p] = new unsigned char[(size_t)offset + bytes[p]];
      memset(block[p], 0xEE, (size_t)offset + bytes[p]);
      P.plane[p] = block[p] + offset; P.pitch[p] = pitch;
      P.wide[p] = (uintptr_t)P.plane[p] % (uintptr_t)run == 0 && pitch % run == 0 && pw * es >= run;
      wide[p] += P.wide[p];
    }
    const int32_t* c = fdh::video_export::kCoefficients[vp::ten_bit(format)][matrix][range];
    P.yoff = c[0]; P.coff = c[1];
    for (int k = 0; k < 3; k++) { P.ky[k] = c[2 + k]; P.ku[k] = c[5 + k]; P.kv[k] = c[8 + k]; }
    wide_src += P.wide_src;
    fdh::launch_video_planar_export(nullptr, P);
    for (int p = 0; p < 3; p++) {
      for (int i = 0; i < head[13 + p]; i++)
        if (block[p][i] != 0xEE) { printf("case %ld: plane %d written in front of its pointer\n", cases, p); return 1; }
      fwrite(block[p] + head[13 + p], 1, (size_t)bytes[p], out);
      delete[] block[p];
    }
    delete[] src;
    cases++;
  }
  fclose(in);
  fclose(out);
  printf("cases %ld wide_src %ld wide_y %ld wide_cb %ld wide_cr %ld workgroups %ld lanes %ld\n", cases, wide_src, wide[0], wide[1], wide[2], emu::workgroups, emu::lanes);
  return 0;
}
