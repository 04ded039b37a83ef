// planar_repack.hip -- what an application does WITHOUT fdh_put_video_planes / fdh_read_video_planes (include_video/figdraw_hip_video_planar.h):
// a pass of its own that turns an I420 / I010 frame into the NV12 / P010 frame fdh_put_video_frame takes, and one that splits what
// fdh_read_video_frame wrote back into three planes.  tools/video_planar_bench.py builds this into build/libplanar_repack.so and times
// it in front of / behind the sibling call: leg (c) of profiles/video_planar.txt.  Not part of the library.  A kernel a careful user
// would write: one launch per frame, a lane per eight chroma samples of either plane (8- or 16-byte loads, 16-byte stores), and for
// 10 bit the same lanes' worth of luma words shifted in the same launch.  Planes are tightly packed and 16-byte aligned, sample counts
// multiples of eight (1920 x 1080 and 3840 x 2160 are).
//   hipcc --offload-arch=gfx950 -O3 -fPIC -shared tools/microbench/planar_repack.hip -o build/libplanar_repack.so
#include <hip/hip_runtime.h>
#include <stdint.h>

// Cb, Cr planes -> Cb,Cr pairs; kTen: and every word << 6, the luma plane too
template <bool kTen>
__global__ __launch_bounds__(256) void k_interleave(const char* y_in, char* y_out, const char* cb, const char* cr, char* pairs, long n_c8, long n_y8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_c8) {
    if (!kTen) {
      const uint2 a = reinterpret_cast<const uint2*>(cb)[i], b = reinterpret_cast<const uint2*>(cr)[i];
      uint4 o;
      o.x = (a.x & 0xFFu) | ((b.x & 0xFFu) << 8) | ((a.x & 0xFF00u) << 8) | ((b.x & 0xFF00u) << 16);
      o.y = ((a.x >> 16) & 0xFFu) | ((b.x >> 8) & 0xFF00u) | ((a.x >> 8) & 0xFF0000u) | (b.x & 0xFF000000u);
      o.z = (a.y & 0xFFu) | ((b.y & 0xFFu) << 8) | ((a.y & 0xFF00u) << 8) | ((b.y & 0xFF00u) << 16);
      o.w = ((a.y >> 16) & 0xFFu) | ((b.y >> 8) & 0xFF00u) | ((a.y >> 8) & 0xFF0000u) | (b.y & 0xFF000000u);
      reinterpret_cast<uint4*>(pairs)[i] = o;
    } else {
      const uint4 a = reinterpret_cast<const uint4*>(cb)[i], b = reinterpret_cast<const uint4*>(cr)[i];
      const uint32_t av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
      uint32_t o[8];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        o[2 * k] = ((av[k] & 0x3FFu) << 6) | ((bv[k] & 0x3FFu) << 22);
        o[2 * k + 1] = (((av[k] >> 16) & 0x3FFu) << 6) | (((bv[k] >> 16) & 0x3FFu) << 22);
      }
      reinterpret_cast<uint4*>(pairs)[2 * i] = uint4{o[0], o[1], o[2], o[3]};
      reinterpret_cast<uint4*>(pairs)[2 * i + 1] = uint4{o[4], o[5], o[6], o[7]};
    }
  } else if (kTen && i < n_c8 + n_y8) {
    const uint4 v = reinterpret_cast<const uint4*>(y_in)[i - n_c8];
    reinterpret_cast<uint4*>(y_out)[i - n_c8] = uint4{(v.x & 0x03FF03FFu) << 6, (v.y & 0x03FF03FFu) << 6, (v.z & 0x03FF03FFu) << 6, (v.w & 0x03FF03FFu) << 6};
  }
}
// Cb,Cr pairs -> Cb, Cr planes; kTen: and every word >> 6, the luma plane too
template <bool kTen>
__global__ __launch_bounds__(256) void k_split(const char* y_in, char* y_out, const char* pairs, char* cb, char* cr, long n_c8, long n_y8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_c8) {
    if (!kTen) {
      const uint4 p = reinterpret_cast<const uint4*>(pairs)[i];
      uint2 a, b;
      a.x = (p.x & 0xFFu) | ((p.x >> 8) & 0xFF00u) | ((p.y & 0xFFu) << 16) | ((p.y & 0xFF0000u) << 8);
      b.x = ((p.x >> 8) & 0xFFu) | ((p.x >> 16) & 0xFF00u) | ((p.y & 0xFF00u) << 8) | (p.y & 0xFF000000u);
      a.y = (p.z & 0xFFu) | ((p.z >> 8) & 0xFF00u) | ((p.w & 0xFFu) << 16) | ((p.w & 0xFF0000u) << 8);
      b.y = ((p.z >> 8) & 0xFFu) | ((p.z >> 16) & 0xFF00u) | ((p.w & 0xFF00u) << 8) | (p.w & 0xFF000000u);
      reinterpret_cast<uint2*>(cb)[i] = a;
      reinterpret_cast<uint2*>(cr)[i] = b;
    } else {
      const uint4 p = reinterpret_cast<const uint4*>(pairs)[2 * i], q = reinterpret_cast<const uint4*>(pairs)[2 * i + 1];
      const uint32_t v[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
      uint32_t a[4], b[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        a[k] = ((v[2 * k] & 0xFFFFu) >> 6) | (((v[2 * k + 1] & 0xFFFFu) >> 6) << 16);
        b[k] = (v[2 * k] >> 22) | ((v[2 * k + 1] >> 22) << 16);
      }
      reinterpret_cast<uint4*>(cb)[i] = uint4{a[0], a[1], a[2], a[3]};
      reinterpret_cast<uint4*>(cr)[i] = uint4{b[0], b[1], b[2], b[3]};
    }
  } else if (kTen && i < n_c8 + n_y8) {
    const uint4 v = reinterpret_cast<const uint4*>(y_in)[i - n_c8];
    reinterpret_cast<uint4*>(y_out)[i - n_c8] = uint4{(v.x >> 6) & 0x03FF03FFu, (v.y >> 6) & 0x03FF03FFu, (v.z >> 6) & 0x03FF03FFu, (v.w >> 6) & 0x03FF03FFu};
  }
}

// n_c, n_y: samples of either chroma plane / of the luma plane, multiples of eight.  ten = 0: the luma plane is not touched (NV12's is I420's)
extern "C" __attribute__((visibility("default"))) int planar_repack_interleave(void* stream, int ten, const void* y_in, void* y_out, const void* cb, const void* cr, void* pairs, long n_c, long n_y) {
  if (n_c % 8 || n_y % 8) return -1;
  const long lanes = n_c / 8 + (ten ? n_y / 8 : 0);
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  if (ten) hipLaunchKernelGGL(k_interleave<true>, grid, block, 0, (hipStream_t)stream, (const char*)y_in, (char*)y_out, (const char*)cb, (const char*)cr, (char*)pairs, n_c / 8, n_y / 8);
  else hipLaunchKernelGGL(k_interleave<false>, grid, block, 0, (hipStream_t)stream, (const char*)y_in, (char*)y_out, (const char*)cb, (const char*)cr, (char*)pairs, n_c / 8, n_y / 8);
  return (int)hipGetLastError();
}
extern "C" __attribute__((visibility("default"))) int planar_repack_split(void* stream, int ten, const void* y_in, void* y_out, const void* pairs, void* cb, void* cr, long n_c, long n_y) {
  if (n_c % 8 || n_y % 8) return -1;
  const long lanes = n_c / 8 + (ten ? n_y / 8 : 0);
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  if (ten) hipLaunchKernelGGL(k_split<true>, grid, block, 0, (hipStream_t)stream, (const char*)y_in, (char*)y_out, (const char*)pairs, (char*)cb, (char*)cr, n_c / 8, n_y / 8);
  else hipLaunchKernelGGL(k_split<false>, grid, block, 0, (hipStream_t)stream, (const char*)y_in, (char*)y_out, (const char*)pairs, (char*)cb, (char*)cr, n_c / 8, n_y / 8);
  return (int)hipGetLastError();
}
