// tests/video_alpha_out_emu/emu.cpp -- figdraw_amd/csrc/k_video_alpha_export.hip under the sequential host shim (tests/emu/fdh_device.h);
// the kernel's source and its parameter headers come from csrc, unmodified: tests/test_video_alpha_host.py copies them here.  Built twice:
// emu, and emu_san (the same stand-alone program under AddressSanitizer and UBSan, which also refuses a wide load or store at an address
// that is no multiple of its size).  The parameter block is filled as video_out::read_alpha fills it (fdh_video_out.cpp).
// usage: emu cases.bin out.bin
//   cases.bin: per case eighteen int32 -- W, H of the source, the rectangle x, y, w, h, format, matrix, range, flags, pitch[4], offset[4] --
//              and W * H * 4 bytes: the source's RGBA8 texels, any bytes (a colour byte above its alpha is fine).  The kernel gets the
//              source in a block of its own that ends with its last texel, and each plane the format has (UYVA: planes 0 and 3; pitch and
//              offset of the other two are 0) at an address offset[p] past a 16-byte boundary, in a block of its own that ends with the
//              plane's last row's end (a read or a store past either end is an error under AddressSanitizer), filled with 0xEE bytes
//   out.bin:   per case each plane from its pointer to its last row's end: Y, Cb, Cr, A, or the UYVY plane and A
// It prints, per build b = 2 * kind + straight (kind: A420 0, A420 linear 1, A444 2, A410 3, UYVA 4, UYVA linear 5), its cases and how
// many of them took the wide path for the source and per plane.
#include "fdh_device.h"
#include "k_video_alpha_export.hip"
#include "fdh_video_export.h"
namespace va = fdh::video_alpha;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[18];
  long cases = 0, per_build[12] = {}, wide_src[12] = {}, wide[12][4] = {};
  while (fread(head, 4, 18, in) == 18) {
    const int W = head[0], H = head[1], x = head[2], y = head[3], w = head[4], h = head[5];
    const uint32_t format = (uint32_t)head[6], matrix = (uint32_t)head[7], range = (uint32_t)head[8], flags = (uint32_t)head[9];
    if (W < 1 || H < 1 || W > 4096 || H > 4096 || x < 0 || y < 0 || w < 1 || h < 1 || x + w > W || y + h > H || !va::known(format) || matrix > 2 || range > 1 || (flags & ~3u)) return 2;
    if ((flags & va::kChromaLinear) && va::full_chroma(format)) return 2;
    if ((format == va::kA420 && ((x | y) & 1)) || (va::packed(format) && (x & 1))) return 2;
    uint32_t* src = new uint32_t[(size_t)W * H];
    if (fread(src, 4, (size_t)W * H, in) != (size_t)W * H) return 2;
    const int kind = (format == va::kA420 ? 0 : format == va::kA444 ? 2 : format == va::kA410 ? 3 : 4) + (int)(flags & va::kChromaLinear);
    const int build = 2 * kind + ((flags & va::kStraightAlpha) ? 1 : 0);
    va::OutParams P{};
    P.src = src + (size_t)y * W + x;
    P.src_pitch = W;
    P.w = w; P.h = h;
    P.format = format; P.flags = flags;
    P.wide_src = (uintptr_t)P.src % 16 == 0 && W % 4 == 0 && w >= va::kRun;
    unsigned char* block[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t bytes[4] = {0, 0, 0, 0};
    for (int p = 0; p < 4; p++) {
      const int offset = head[14 + p];
      if (!va::has_plane(format, p)) { if (offset || head[10 + p]) return 2; continue; }
      const int64_t pitch = head[10 + p], row = va::row_bytes(format, p, w), run = va::run_bytes(format, p);
      if (offset < 0 || offset > 15 || pitch < row) return 2;
      bytes[p] = (va::rows(format, p, h) - 1) * pitch + row;
      block[p] = new unsigned char[(size_t)offset + bytes[p]];
      memset(block[p], 0xEE, (size_t)offset + bytes[p]);
      P.plane[p] = block[p] + offset; P.pitch[p] = pitch;
      P.wide[p] = (uintptr_t)P.plane[p] % (uintptr_t)run == 0 && pitch % run == 0 && row >= run;
      wide[build][p] += P.wide[p];
    }
    const int32_t* c = fdh::video_export::kCoefficients[va::ten_bit(format)][matrix][range];
    P.yoff = c[0]; P.coff = c[1];
    for (int k = 0; k < 3; k++) { P.ky[k] = c[2 + k]; P.ku[k] = c[5 + k]; P.kv[k] = c[8 + k]; }
    wide_src[build] += P.wide_src;
    per_build[build]++;
    fdh::launch_video_alpha_export(nullptr, P);
    for (int p = 0; p < 4; p++) {
      if (!block[p]) continue;
      for (int i = 0; i < head[14 + p]; i++)
        if (block[p][i] != 0xEE) { printf("case %ld: plane %d written in front of its pointer\n", cases, p); return 1; }
      fwrite(block[p] + head[14 + p], 1, (size_t)bytes[p], out);
      delete[] block[p];
    }
    delete[] src;
    cases++;
  }
  fclose(in);
  fclose(out);
  printf("cases %ld workgroups %ld lanes %ld", cases, emu::workgroups, emu::lanes);
  for (int b = 0; b < 12; b++)
    printf(" b%d_cases %ld b%d_wide_src %ld b%d_wide_0 %ld b%d_wide_1 %ld b%d_wide_2 %ld b%d_wide_3 %ld", b, per_build[b], b, wide_src[b], b, wide[b][0], b, wide[b][1], b, wide[b][2], b, wide[b][3]);
  printf("\n");
  return 0;
}
