// k_damage.hip -- the launches damage tracking adds to a tracked frame (fdh_set_damage_tracking, fdh_damage.h): k_damage_sign after the
// bin launch (per-bin signatures of the lists and what they index, against the previous frame's), k_damage_resolve (the blur rule, the
// compact list of damaged bins the compositor launches walk) and k_damage_guard (keeps a fused V pass's footprint when its node did not run).
#include "fdh_device.h"
#include "fdh_damage.h"

namespace fdh {

// one step of the signature: a bijection of h for every word w, so two sequences that differ in one word differ in h
__device__ __forceinline__ uint64_t sig_step(uint64_t h, uint32_t w) {
  h ^= w;
  h *= 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 31);
}
__device__ __forceinline__ uint64_t sig_final(uint64_t h) {  // (splitmix64's finaliser: the per-entry values are summed)
  h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 27; h *= 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}

// One wave per bin.  Lane k takes the entries k, k + 64, ... of each phase's list: an entry's value mixes its phase and position in, so
// the per-entry values can be summed (in any order) into an order-DEPENDENT signature of the lists.
__global__ __launch_bounds__(64) void k_damage_sign(const DamageSignParams P) {
  const int nb = P.bins_x * P.bins_y;
  const int bin = (int)blockIdx.x;
  if (bin >= nb) return;
  const int lane = (int)threadIdx.x;
  const int by = bin / P.bins_x, bx = bin - by * P.bins_x;
  uint64_t acc = 0;
  for (int p = 0; p < P.n_phases; p++) {
    if (P.sub_n) {  // a later phase's lists exist for the bins of its sub-grid only (k_bin_draws writes no count elsewhere)
      if (bx < P.sub_x0[p] || bx >= P.sub_x0[p] + P.sub_nx[p] || by < P.sub_y0[p] || by >= P.sub_y0[p] + P.sub_ny[p]) continue;
    }
    const size_t pb = (size_t)p * nb + bin;
    const uint32_t cnt = min(P.counts[pb], (uint32_t)P.stride);
    const uint2* __restrict__ L = P.lists + pb * P.stride;
    for (uint32_t k = lane; k < cnt; k += 64) {
      const uint2 e = L[k];
      uint64_t h = sig_step(sig_step(0x6A09E667F3BCC908ull, (uint32_t)p), k);
      h = sig_step(sig_step(h, e.x), e.y);
      const uint32_t i = e.x & LE_INDEX;
      if (i < (uint32_t)P.n_draws) {
        const uint4* __restrict__ d = reinterpret_cast<const uint4*>(P.draws + i);
        uint32_t op = 0, ext = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const uint4 v = d[q];
          if (q == 0) { op = v.x; ext = v.y; }
          h = sig_step(sig_step(sig_step(sig_step(h, v.x), v.y), v.z), v.w);
        }
        if ((op & F_GENERAL) && ext < (uint32_t)P.n_exts) {
          const uint4* __restrict__ x = reinterpret_cast<const uint4*>(P.exts + ext);
#pragma unroll
          for (int q = 0; q < (int)(sizeof(QuadExt) / 16); q++) {
            const uint4 v = x[q];
            h = sig_step(sig_step(sig_step(sig_step(h, v.x), v.y), v.z), v.w);
          }
        }
      }
      acc += sig_final(h);
    }
  }
  for (int k = lane; k < P.n_nodes; k += 64) {
    const DamageRegion f = P.foot[k];
    if (bx >= f.bx0 && bx < f.bx1 && by >= f.by0 && by < f.by1) acc += sig_final(sig_step(sig_step(0xBB67AE8584CAA73Bull, (uint32_t)k), (uint32_t)P.node_key[k]) ^ (P.node_key[k] >> 32) * 0x9E3779B97F4A7C15ull);
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) acc += __shfl_xor(acc, sh, 64);
  if (lane == 0) {
    const uint64_t old = P.sig[bin];
    P.sig[bin] = acc;
    P.changed[bin] = (P.force || old != acc) ? 1 : 0;
  }
}

// One workgroup: the blur rule over the frame's nodes to its fixed point (damage_close, fdh_damage.h: the code fdh_damage_closure runs on
// the host), then the compact list.  The mask lives in global memory (a grid of any size); the workgroup's barriers order its own stores
// and loads.
constexpr int kResolveThreads = 1024;
struct DamageWorkgroup {
  __device__ int rank() const { return (int)threadIdx.x; }
  __device__ int size() const { return kResolveThreads; }
  __device__ bool any(int v) const { return __syncthreads_or(v) != 0; }
  __device__ void sync() const { __syncthreads(); }
};
__global__ __launch_bounds__(kResolveThreads) void k_damage_resolve(const DamageResolveParams P) {
  __shared__ uint32_t s_n;
  __shared__ uint8_t s_run[kDamageMaxNodes];
  const int nb = P.bins_x * P.bins_y;
  const int t = (int)threadIdx.x;
  for (int b = t; b < nb; b += kResolveThreads) P.mask[b] = P.changed[b];
  if (t < kDamageMaxNodes) s_run[t] = 0;
  if (t == 0) s_n = 0;
  __syncthreads();
  damage_close(P.mask, P.bins_x, P.reg, P.n_nodes, s_run, DamageWorkgroup());
  for (int b = t; b < nb; b += kResolveThreads)
    if (P.mask[b]) P.list[atomicAdd(&s_n, 1u)] = b;
  __syncthreads();
  if (t == 0) P.count[0] = s_n;
  if (t < P.n_nodes) P.run[t] = s_run[t];
}

__global__ __launch_bounds__(256) void k_damage_guard(const uint8_t* __restrict__ run, int node, int restore, uint32_t* __restrict__ surf,
                                                      uint32_t* __restrict__ keep, int pitch, int x0, int y0, int w, int h) {
  if (run[node]) return;
  const size_t n = (size_t)w * h;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int y = y0 + (int)(i / w), x = x0 + (int)(i % w);
    const size_t at = (size_t)y * pitch + x;
    if (restore) surf[at] = keep[at];
    else keep[at] = surf[at];
  }
}

// Damage readback's per-frame launch (one workgroup): the frame's damaged bins become pending -- stamped with the epoch of the read that
// will fetch them -- and the host finds the size of the pending set in *n_pending.
__global__ __launch_bounds__(kResolveThreads) void k_damage_accumulate(const uint8_t* __restrict__ mask, uint32_t* __restrict__ stamp,
                                                                       uint32_t epoch, int nb, uint32_t* __restrict__ n_pending) {
  __shared__ uint32_t s_part[kResolveThreads / 64];
  uint32_t c = 0;
  for (int b = (int)threadIdx.x; b < nb; b += kResolveThreads) {
    const bool hit = mask[b] != 0;
    if (hit) stamp[b] = epoch;
    else if (stamp[b] != epoch) continue;
    c++;
  }
  c = workgroup_sum<false>(c, s_part);
  if (threadIdx.x == 0) n_pending[0] = c;
}

// Damage readback's read: a workgroup per bin; those of bins that are not pending leave at once.  A tile is 64 rows of 256 contiguous
// bytes = 1024 16-byte words, four per thread, in the slot as tile_walk takes them from the surface (fdh_damage_read.h).
constexpr int kPackThreads = 256;
__global__ __launch_bounds__(kPackThreads) void k_damage_pack(const DamagePackParams P) {
  __shared__ uint32_t s_part[kPackThreads / 64];
  const int nb = P.bins_x * P.bins_y;
  const int bin = (int)blockIdx.x, t = (int)threadIdx.x;
  if (bin >= nb) return;
  uint32_t rank;
  if (!pending_slot<kPackThreads, false>(P.stamp, P.epoch, P.all, bin, nb, P.n_tiles, s_part, rank)) return;
  const TileBox b = tile_box(bin, P.bins_x, P.W, P.H);
  if (t == 0) P.tiles[rank] = make_int4(b.x0, b.y0, b.w, b.h);
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(P.pixels + (size_t)rank * (kBin * kBin * 4));
  const bool rows_aligned = (P.W & 3) == 0;  // every surface row starts on a 16-byte boundary
  // (captures by value: by reference the kernel takes 18 registers instead of 14)
  tile_walk<kPackThreads>(P.surf, P.W, b, [=](int i, int, int c, bool inside, const uint32_t* __restrict__ src) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (inside) {
      if (rows_aligned && c + 4 <= b.w) v = *reinterpret_cast<const uint4*>(src);
      else {
        v.x = src[0];
        if (c + 1 < b.w) v.y = src[1];
        if (c + 2 < b.w) v.z = src[2];
        if (c + 3 < b.w) v.w = src[3];
      }
    }
    dst[i] = v;
  });
}

void launch_damage_accumulate(hipStream_t s, const uint8_t* mask, uint32_t* stamp, uint32_t epoch, int bins, uint32_t* n_pending) {
  if (bins <= 0) return;
  FDH_LAUNCH(k_damage_accumulate, dim3(1), dim3(kResolveThreads), 0, s, mask, stamp, epoch, bins, n_pending);
}
void launch_damage_pack(hipStream_t s, const DamagePackParams& P) {
  const int nb = P.bins_x * P.bins_y;
  if (nb <= 0) return;
  FDH_LAUNCH(k_damage_pack, dim3(nb), dim3(kPackThreads), 0, s, P);
}

void launch_damage_sign(hipStream_t s, const DamageSignParams& P) {
  const int nb = P.bins_x * P.bins_y;
  if (nb <= 0) return;
  FDH_LAUNCH(k_damage_sign, dim3(nb), dim3(64), 0, s, P);
}
void launch_damage_resolve(hipStream_t s, const DamageResolveParams& P) {
  if (P.bins_x * P.bins_y <= 0 || P.n_nodes < 0 || P.n_nodes > kDamageMaxNodes) return;  // (DamageTracker::launch clamps n_nodes)
  FDH_LAUNCH(k_damage_resolve, dim3(1), dim3(kResolveThreads), 0, s, P);
}
void launch_damage_guard(hipStream_t s, const uint8_t* run, int node, bool restore, uint32_t* surf, uint32_t* keep, int pitch, int x0, int y0,
                         int x1, int y1) {
  const int w = x1 - x0, h = y1 - y0;
  if (w <= 0 || h <= 0) return;
  const int grid = (int)std::min<size_t>(((size_t)w * h + 255) / 256, 2048);
  FDH_LAUNCH(k_damage_guard, dim3(grid), dim3(256), 0, s, run, node, restore ? 1 : 0, surf, keep, pitch, x0, y0, w, h);
}

}  // namespace fdh
