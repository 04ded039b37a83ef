// tests/video_out_emu/emu.cpp -- figdraw_amd/csrc/k_video_export.hip under the sequential host shim (tests/emu/fdh_device.h); the kernel's source and its
// parameter header come from csrc, unmodified: tests/test_video_out_host.py copies them here.  Built twice: emu, and emu_san (the same
// under AddressSanitizer and UBSan, which also refuses a wide load or store at an address that is no multiple of its size).  The
// parameter block is filled as video_out::read fills it (fdh_video_out.cpp).
// usage: emu cases.bin out.bin
//   cases.bin: per case sixteen int32 -- W, H of the source, the rectangle x, y, w, h, format, matrix, range, flags, pitch_y, pitch_c,
//              offset_y, offset_c, 0, 0 -- and W * H * 4 bytes: the source's RGBA8 texels.  The kernel gets the source in a block of its
//              own that ends with its last texel, and each plane at an address offset_* past a 16-byte boundary, in a block of its own
//              that ends with the plane's last element (a read or a store past either end is an error under AddressSanitizer),
//              filled with 0xEE bytes
//   out.bin:   per case each plane from its pointer to its last element's end, luma then chroma
#include "fdh_device.h"
#include "k_video_export.hip"
namespace ve = fdh::video_export;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[16];
  long cases = 0, wide_src = 0, wide_y = 0, wide_c = 0;
  while (fread(head, 4, 16, in) == 16) {
    const int W = head[0], H = head[1], x = head[2], y = head[3], w = head[4], h = head[5];
    const uint32_t format = (uint32_t)head[6], matrix = (uint32_t)head[7], range = (uint32_t)head[8], flags = (uint32_t)head[9];
    if (W < 1 || H < 1 || W > 4096 || H > 4096 || x < 0 || y < 0 || w < 1 || h < 1 || x + w > W || y + h > H || format > ve::kP010 || matrix > 2 || range > 1) return 2;
    if (format != ve::kBgra8 && ((x | y) & 1)) return 2;
    uint32_t* src = new uint32_t[(size_t)W * H];
    if (fread(src, 4, (size_t)W * H, in) != (size_t)W * H) return 2;
    const int64_t es = format == ve::kBgra8 ? 4 : format == ve::kP010 ? 2 : 1;
    const int64_t cw = (w + 1) / 2, ch = (h + 1) / 2;
    const int64_t pitch[2] = {head[10], head[11]};
    const int64_t row[2] = {w * es, format == ve::kBgra8 ? 0 : cw * 2 * es};
    const int64_t bytes[2] = {(h - 1) * pitch[0] + row[0], format == ve::kBgra8 ? 0 : (ch - 1) * pitch[1] + row[1]};
    unsigned char* block[2] = {nullptr, nullptr};
    unsigned char* plane[2] = {nullptr, nullptr};
    for (int p = 0; p < 2; p++) {
      const int offset = head[12 + p];
      if (offset < 0 || offset > 15 || pitch[p] < row[p]) return 2;
      if (!bytes[p]) continue;
      block[p] = new unsigned char[(size_t)offset + bytes[p]];
      memset(block[p], 0xEE, (size_t)offset + bytes[p]);
      plane[p] = block[p] + offset;
    }
    ve::Params P{};
    P.src = src + (size_t)y * W + x;
    P.src_pitch = W;
    P.w = w; P.h = h;
    P.luma = plane[0]; P.chroma = plane[1];
    P.pitch_y = pitch[0]; P.pitch_c = pitch[1];
    P.format = format; P.flags = flags;
    const uintptr_t run = (uintptr_t)(4 * es);
    P.wide_src = (uintptr_t)P.src % 16 == 0 && W % 4 == 0 && w >= 4;
    P.wide_y = (uintptr_t)plane[0] % run == 0 && pitch[0] % (int64_t)run == 0 && w >= 4;
    P.wide_c = format != ve::kBgra8 && (uintptr_t)plane[1] % run == 0 && pitch[1] % (int64_t)run == 0 && cw >= 2;
    if (format != ve::kBgra8) {
      const int32_t* c = ve::kCoefficients[format == ve::kP010][matrix][range];
      P.yoff = c[0]; P.coff = c[1];
      for (int k = 0; k < 3; k++) { P.ky[k] = c[2 + k]; P.ku[k] = c[5 + k]; P.kv[k] = c[8 + k]; }
    }
    wide_src += P.wide_src; wide_y += P.wide_y; wide_c += P.wide_c;
    fdh::launch_video_export(nullptr, P);
    for (int p = 0; p < 2; p++) {
      if (!block[p]) continue;
      for (int i = 0; i < head[12 + p]; i++)
        if (block[p][i] != 0xEE) { printf("case %ld: plane %d written in front of its pointer\n", cases, p); return 1; }
      fwrite(plane[p], 1, (size_t)bytes[p], out);
      delete[] block[p];
    }
    delete[] src;
    cases++;
  }
  fclose(in);
  fclose(out);
  printf("cases %ld wide_src %ld wide_y %ld wide_c %ld workgroups %ld lanes %ld\n", cases, wide_src, wide_y, wide_c, emu::workgroups, emu::lanes);
  return 0;
}
