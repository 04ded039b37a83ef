// k_damage_filter.hip -- exact damage readback (include/figdraw_hip_exact.h): the launch in front of k_damage_pack / k_damage_encode that
// drops every pending bin whose pixels are what the application already holds.  The mirror is the frame as of the last read, tile-major
// (fdh_damage_read.h); one launch, the shape of k_damage_pack (k_damage.hip).
#include "fdh_device.h"
#include "fdh_damage.h"

namespace fdh {

// A workgroup per bin; those of bins that are not pending leave after one load.  A tile is 1024 16-byte words, four per thread, as
// tile_walk takes them from the surface; word i of the mirror's slot is word i of the tile, so every mirror access is an aligned word
// whatever W & 3 is.  All eight loads of a thread are issued before the first compare; a tile that differs is stored out of the registers
// that hold it -- no second read, and a thread writes only the words it read, so the compare and the update need no order between them.
constexpr int kFilterThreads = 256;
constexpr int kFilterWords = kBin * kBin / 4 / kFilterThreads;
__global__ __launch_bounds__(kFilterThreads) void k_damage_filter(const DamageFilterParams P) {
  __shared__ uint32_t s_part[kFilterThreads / 64];
  const int nb = P.bins_x * P.bins_y;
  const int bin = (int)blockIdx.x, t = (int)threadIdx.x;
  if (bin >= nb) return;
  if (!P.all && P.stamp[bin] != P.epoch) return;
  const TileBox b = tile_box(bin, P.bins_x, P.W, P.H);
  uint4* __restrict__ mir = reinterpret_cast<uint4*>(P.mirror + (size_t)bin * (kBin * kBin));
  const bool rows_aligned = (P.W & 3) == 0;  // every surface row starts on a 16-byte boundary
  const bool compare = !P.fill;
  uint4 v[kFilterWords], m[kFilterWords];
  if (rows_aligned && b.w == kBin && b.h == kBin) {  // (uniform) a whole tile of an aligned frame: eight plain loads, no branch between them
    tile_walk<kFilterThreads>(P.surf, P.W, b, [&](int i, int, int, bool, const uint32_t* __restrict__ src) {
      const int k = (i - t) / kFilterThreads;
      m[k] = compare ? mir[i] : make_uint4(0u, 0u, 0u, 0u);
      v[k] = *reinterpret_cast<const uint4*>(src);
    });
  } else {  // a clipped tile, or rows that are not 16-byte aligned: a word past the tile's edge is zero on both sides, and neither is read
    tile_walk<kFilterThreads>(P.surf, P.W, b, [&](int i, int, int c, bool inside, const uint32_t* __restrict__ src) {
      const int k = (i - t) / kFilterThreads;
      v[k] = m[k] = make_uint4(0u, 0u, 0u, 0u);
      if (!inside) return;
      if (compare) m[k] = mir[i];
      if (rows_aligned && c + 4 <= b.w) v[k] = *reinterpret_cast<const uint4*>(src);
      else {
        v[k].x = src[0];
        if (c + 1 < b.w) v[k].y = src[1];
        if (c + 2 < b.w) v[k].z = src[2];
        if (c + 3 < b.w) v[k].w = src[3];
      }
    });
  }
  uint32_t differs = 1;
  if (compare) {  // (uniform)
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < kFilterWords; k++) d |= (v[k].x ^ m[k].x) | (v[k].y ^ m[k].y) | (v[k].z ^ m[k].z) | (v[k].w ^ m[k].w);
    differs = workgroup_sum<false>(d ? 1u : 0u, s_part) ? 1u : 0u;
  }
  if (differs) {
#pragma unroll
    for (int k = 0; k < kFilterWords; k++) mir[t + k * kFilterThreads] = v[k];
  }
  if (compare && t == 0) {
    P.stamp[bin] = differs ? P.epoch : P.epoch - 1u;
    // (one 64-bit add: the bins that stay pending in bits 0 .. 31, the arrivals above them; whoever arrives last knows the total)
    const unsigned long long old = atomicAdd(P.arrivals, (unsigned long long)differs | 1ull << 32);
    if ((uint32_t)(old >> 32) + 1u == P.n_pending) P.n_changed[0] = (uint32_t)old + differs;
  }
}

void launch_damage_filter(hipStream_t s, const DamageFilterParams& P) {
  const int nb = P.bins_x * P.bins_y;
  if (nb <= 0) return;
  FDH_LAUNCH(k_damage_filter, dim3(nb), dim3(kFilterThreads), 0, s, P);
}

}  // namespace fdh
