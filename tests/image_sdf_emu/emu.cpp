// tests/image_sdf_emu/emu.cpp -- figdraw_amd/csrc/k_image_sdf.hip under the sequential host shim (tests/emu/fdh_device.h); the kernel's source comes from csrc,
// unmodified: tests/test_image_sdf_host.py copies it here.  Built three ways: emu, emu_nocull (-DFDH_IMAGE_SDF_NO_CULL=1: no exit from the
// walk, no shortcut) and emu_san (emu under AddressSanitizer and UBSan).
// usage: emu cases.bin fields.bin
//   cases.bin:  per case five int32 (w, h, channel, pad, range) and the w x h RGBA8 texels of the source
//   fields.bin: per case the (w + 2 pad) x (h + 2 pad) RGBA8 texels of the field
// prints the cases, the workgroups and the passes the shim took; exit 1: a texel outside a field was written; exit 4: see fdh_device.h
#include "fdh_device.h"
#include "k_image_sdf.hip"
#include <cstring>
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const int guard = 64;
  int32_t head[5];
  long cases = 0;
  while (fread(head, 4, 5, in) == 5) {
    const int w = head[0], h = head[1], channel = head[2], pad = head[3], range = head[4];
    if (w < 1 || h < 1 || channel < 0 || channel > 3 || pad < 0 || pad > 64 || range < 1 || range > 64) return 2;
    const size_t n_src = (size_t)w * h, n_out = (size_t)(w + 2 * pad) * (h + 2 * pad);
    // exactly-sized source: a read past either end is an error under AddressSanitizer; a write past the field's ends also without it
    uint32_t* src = new uint32_t[n_src];
    if (fread(src, 4, n_src, in) != n_src) return 2;
    std::vector<uint32_t> field(n_out + 2 * guard, 0xEEEEEEEEu);
    fdh::launch_image_sdf_generate(nullptr, src, w, h, w, channel, pad, range, field.data() + guard);
    delete[] src;
    for (int i = 0; i < guard; i++)
      if (field[i] != 0xEEEEEEEEu || field[n_out + guard + i] != 0xEEEEEEEEu) { printf("overrun\n"); return 1; }
    fwrite(field.data() + guard, 4, n_out, out);
    cases++;
  }
  fclose(in);
  fclose(out);
  printf("cases %ld workgroups %ld passes %ld\n", cases, emu::workgroups, emu::passes);
  return 0;
}
