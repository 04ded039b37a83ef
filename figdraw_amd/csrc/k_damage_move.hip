// k_damage_move.hip -- moved damage readback (include_readback/figdraw_hip_moves.h, which specifies mode COPY and the mover's votes;
// fdh_damage_move.h has the parameter blocks): k_damage_move_match finds the pending tiles that equal a shifted rectangle of the mirror,
// k_damage_encode_moved codes a read in stream version 2, k_damage_move_votes proposes a frame's scroll vectors.  All of them have
// k_damage_pack's shape (k_damage.hip) and read the mirror pixel by pixel: a shifted rectangle spans up to four of its slots and is not
// 16-byte aligned in general, so a wave loads one dword per lane -- 64 consecutive pixels of a row, 256 contiguous bytes of the surface
// and at most two contiguous pieces of the mirror.
#include "fdh_device.h"
#include "fdh_damage.h"

namespace fdh {

static_assert(kBin == 64, "mirror_px and the lane = column walks below are written for 64-pixel bins");
constexpr int kMoveThreads = 256;
constexpr int kMoveWaves = kMoveThreads / 64;

// ------------------------------------------------------------------ k_damage_move_match
// A thread owns column t & 63 of the tile and every fourth row from t >> 6.  A move is first tried on four rows spread over the tile, one
// per wave: a proposal that is wrong for this tile nearly always dies there, after 2 KB instead of 32.  Every branch is workgroup-uniform.
__global__ __launch_bounds__(kMoveThreads) void k_damage_move_match(const DamageMoveMatchParams P) {
  __shared__ uint32_t s_part[kMoveWaves];
  const int nb = P.bins_x * P.bins_y;
  const int bin = (int)blockIdx.x, t = (int)threadIdx.x;
  if (bin >= nb) return;
  if (!P.all && P.stamp[bin] != P.epoch) return;  // (moved[] is read for pending bins only)
  const TileBox b = tile_box(bin, P.bins_x, P.W, P.H);
  const int c = t & 63, r0 = t >> 6;
  const bool in_col = c < b.w;
  const uint32_t* __restrict__ col = P.surf + (size_t)b.y0 * P.W + b.x0 + c;
  uint32_t hit = 0;
  for (int m = 0; m < P.moves.n && !hit; m++) {
    const int sx = b.x0 + P.moves.dx[m], sy = b.y0 + P.moves.dy[m];
    if (sx < 0 || sy < 0 || sx + b.w > P.W || sy + b.h > P.H) continue;  // the source leaves the frame: not a candidate
    const int rp = (r0 * b.h) >> 2;
    uint32_t d = (in_col && col[(size_t)rp * P.W] != mirror_px(P.mirror, P.bins_x, sx + c, sy + rp)) ? 1u : 0u;
    if (workgroup_sum<true>(d, s_part)) continue;
    d = 0;
    if (in_col) {
#pragma unroll 4
      for (int r = r0; r < b.h; r += kMoveWaves) d |= col[(size_t)r * P.W] ^ mirror_px(P.mirror, P.bins_x, sx + c, sy + r);
    }
    if (workgroup_sum<true>(d ? 1u : 0u, s_part)) continue;
    hit = (uint32_t)m + 1u;
  }
  if (t == 0) P.moved[bin] = (uint8_t)hit;
}

void launch_damage_move_match(hipStream_t s, const DamageMoveMatchParams& P) {
  const int nb = P.bins_x * P.bins_y;
  if (nb <= 0) return;
  FDH_LAUNCH(k_damage_move_match, dim3(nb), dim3(kMoveThreads), 0, s, P);
}

// ------------------------------------------------------------------ k_damage_encode_moved
// The per-tile coding is k_damage_encode's (k_damage_codec.hip), written out a second time under other names: calling one shared body
// from both kernels would have changed the existing kernel's code object, which stays as it is.  What differs: step 4a, the COPY entry,
// and step 5's cursor, which also counts the COPY tiles.
constexpr int kMvThreads = 256;
constexpr int kMvPerThread = kBin * kBin / kMvThreads;
constexpr int kMvSlots = 1024;
constexpr int kMvMaxColours = 256;
constexpr uint32_t kMvEmpty = 0xFFFFFFFFu;
constexpr int kMvRunsPerThread = (kBin * kBin * 4 / 6 + kMvThreads - 1) / kMvThreads;
constexpr int kMvCopyShift = 28, kMvArriveShift = 46;  // the cursor's fields (fdh_damage_move.h)

struct MvShared {
  uint32_t buf[kBin * kBin];
  uint32_t key[kMvSlots];
  uint16_t rank[kMvSlots];
  uint32_t list[kMvMaxColours];
  uint16_t slot_of[kMvMaxColours];
  uint32_t part[kMvThreads / 64];
  uint32_t n_colours, has_empty, offset;
};

__device__ __forceinline__ uint32_t mv_hash(uint32_t c) { return (c * 0x9E3779B1u) >> 22; }

__device__ __forceinline__ void mv_insert(MvShared& S, uint32_t c) {
  if (c == kMvEmpty) { S.has_empty = 1u; return; }
  uint32_t slot = mv_hash(c);
  for (;;) {
    if (*(volatile uint32_t*)&S.n_colours > (uint32_t)kMvMaxColours) return;
    const uint32_t old = atomicCAS(&S.key[slot], kMvEmpty, c);
    if (old == c) return;
    if (old == kMvEmpty) {
      const uint32_t k = atomicAdd(&S.n_colours, 1u);
      if (k < (uint32_t)kMvMaxColours) { S.list[k] = c; S.slot_of[k] = (uint16_t)slot; }
      return;
    }
    slot = (slot + 1) & (kMvSlots - 1);
  }
}
__device__ __forceinline__ uint32_t mv_index(const MvShared& S, uint32_t c, uint32_t n) {
  if (c == kMvEmpty) return n - 1;
  uint32_t slot = mv_hash(c);
  while (S.key[slot] != c) slot = (slot + 1) & (kMvSlots - 1);
  return S.rank[slot];
}
template <int B>
__device__ __forceinline__ void mv_pack(const MvShared& S, const uint32_t (&px)[kMvPerThread], int nv, uint32_t starts, uint32_t n_col,
                                        uint32_t (&word)[4]) {
  uint32_t cur = 0;
#pragma unroll
  for (int j = 0; j < kMvPerThread; j++) {
    if (j < nv) {
      if (j == 0 || ((starts >> j) & 1u)) cur = mv_index(S, px[j], n_col);
      word[(j * B) >> 5] |= cur << ((j * B) & 31);
    }
  }
}

__global__ __launch_bounds__(kMvThreads) void k_damage_encode_moved(const DamageEncodeMovedParams Q) {
  __shared__ __attribute__((aligned(16))) MvShared S;
  const DamageEncodeParams& P = Q.enc;
  const int nb = P.bins_x * P.bins_y;
  const int bin = (int)blockIdx.x, t = (int)threadIdx.x;
  if (bin >= nb) return;
  uint32_t slot_dir;
  if (!pending_slot<kMvThreads, true>(P.stamp, P.epoch, P.all, bin, nb, P.n_tiles, S.part, slot_dir)) return;
  const TileBox box = tile_box(bin, P.bins_x, P.W, P.H);
  const int x0 = box.x0, y0 = box.y0, w = box.w, h = box.h;
  const int n_px = w * h;

  // 1. the tile, tight, into LDS
  const bool rows_aligned = (P.W & 3) == 0;
  tile_walk<kMvThreads>(P.surf, P.W, box, [&](int, int r, int c, bool inside, const uint32_t* __restrict__ src) {
    if (!inside) return;
    uint32_t* d = S.buf + r * w + c;
    if (rows_aligned && w == kBin) *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(src);
    else {
      d[0] = src[0];
      if (c + 1 < w) d[1] = src[1];
      if (c + 2 < w) d[2] = src[2];
      if (c + 3 < w) d[3] = src[3];
    }
  });
  if (t == 0) { S.n_colours = 0; S.has_empty = 0; }
  __syncthreads();

  const int base = t * kMvPerThread;
  const int nv = min(max(n_px - base, 0), kMvPerThread);
  uint32_t px[kMvPerThread];
  if (nv == kMvPerThread) {
#pragma unroll
    for (int q = 0; q < kMvPerThread / 4; q++) {
      const uint4 v = reinterpret_cast<const uint4*>(S.buf + base)[q];
      px[4 * q] = v.x; px[4 * q + 1] = v.y; px[4 * q + 2] = v.z; px[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kMvPerThread; j++) px[j] = j < nv ? S.buf[base + j] : 0u;
  }
  const uint32_t before = (t > 0 && nv > 0) ? S.buf[base - 1] : 0u;

  // 2. run starts over the tight order
  uint32_t starts = 0;
#pragma unroll
  for (int j = 0; j < kMvPerThread; j++) {
    const bool st = j < nv && (base + j == 0 || px[j] != (j ? px[j - 1] : before));
    starts |= (st ? 1u : 0u) << j;
  }
  const uint32_t my_runs = (uint32_t)__popc(starts);
  uint32_t incl = my_runs;
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    const uint32_t o = __shfl_up(incl, sh, 64);
    if ((t & 63) >= sh) incl += o;
  }
  if ((t & 63) == 63) S.part[t >> 6] = incl;
#pragma unroll
  for (int k = 0; k < kMvSlots / kMvThreads; k++) S.key[t + k * kMvThreads] = kMvEmpty;
  __syncthreads();
  uint32_t n_runs = 0, first_run = incl - my_runs;
#pragma unroll
  for (int wv = 0; wv < kMvThreads / 64; wv++) {
    const uint32_t p = S.part[wv];
    if (wv < (t >> 6)) first_run += p;
    n_runs += p;
  }

  // 4a. COPY: the tile equals a shifted rectangle of what the receiver holds, and is not one colour (SOLID's empty payload ties with
  // COPY's, and the tie goes to the lower mode).  No payload, no space; still one of the n_pending arrivals.  (uniform)
  const uint32_t mv = Q.moved[bin];
  if (mv != 0 && n_runs > 1) {
    if (t == 0) {
      const unsigned long long old = atomicAdd(P.cursor, 1ull << kMvCopyShift | 1ull << kMvArriveShift);
      if ((uint32_t)(old >> kMvArriveShift) + 1u == P.n_pending) {
        P.payload_bytes[0] = (uint32_t)(old & ((1ull << kMvCopyShift) - 1ull)) * 16u;
        Q.n_copied[0] = (uint32_t)((old >> kMvCopyShift) & ((1ull << (kMvArriveShift - kMvCopyShift)) - 1ull)) + 1u;
      }
      const uint32_t dx = (uint16_t)Q.moves.dx[mv - 1], dy = (uint16_t)Q.moves.dy[mv - 1];
      uint2* e = P.dir + (size_t)slot_dir * 3;
      e[0] = make_uint2((uint32_t)x0 | (uint32_t)y0 << 16, (uint32_t)w | (uint32_t)h << 16);
      e[1] = make_uint2(4u, 0u);
      e[2] = make_uint2(0u, dx | dy << 16);
    }
    return;
  }

  // 3. the distinct colours, when PAL can win at all
  const uint32_t raw_size = 4u * (uint32_t)n_px;
  const uint32_t runs_size = 4u * ((6u * n_runs + 3u) / 4u);
  const bool try_pal = n_runs > 1 && 8u + 4u * (((uint32_t)n_px + 31u) / 32u) <= min(runs_size, raw_size);
  uint32_t n_col = 0, bits = 0, pal_size = 0xFFFFFFFFu;
  if (try_pal) {  // (uniform)
    uint32_t m = starts;
    while (m) {
      const int j = __ffs(m) - 1;
      m &= m - 1;
      uint32_t c = px[0];
#pragma unroll
      for (int q = 1; q < kMvPerThread; q++) c = q == j ? px[q] : c;
      mv_insert(S, c);
    }
    __syncthreads();
    if (S.n_colours <= (uint32_t)kMvMaxColours && S.n_colours + S.has_empty <= (uint32_t)kMvMaxColours) {
      n_col = S.n_colours + S.has_empty;
      bits = n_col <= 2 ? 1u : n_col <= 4 ? 2u : n_col <= 16 ? 4u : 8u;
      pal_size = 4u * n_col + 4u * (((uint32_t)n_px * bits + 31u) / 32u);
    }
  }

  // 4. the mode: the smallest payload, ties to the lower number
  uint32_t mode = 3, size = raw_size;
  if (runs_size <= size) { mode = 2; size = runs_size; }
  if (pal_size <= size) { mode = 1; size = pal_size; }
  if (n_runs == 1) { mode = 0; size = 0; }
  const uint32_t claim = (size + 15u) & ~15u;

  // 5. its space in the blob
  if (t == 0) {
    const unsigned long long old = atomicAdd(P.cursor, (unsigned long long)(claim / 16u) | 1ull << kMvArriveShift);
    const uint32_t at = (uint32_t)(old & ((1ull << kMvCopyShift) - 1ull)) * 16u;
    S.offset = claim ? at : 0u;
    if ((uint32_t)(old >> kMvArriveShift) + 1u == P.n_pending) {
      P.payload_bytes[0] = at + claim;
      Q.n_copied[0] = (uint32_t)((old >> kMvCopyShift) & ((1ull << (kMvArriveShift - kMvCopyShift)) - 1ull));
    }
  }

  // 6. the payload, in S.buf
  if (mode == 1) {
    const uint32_t n_tab = S.n_colours;
    if ((uint32_t)t < n_tab) {
      const uint32_t c = S.list[t];
      uint32_t r = 0;
      for (uint32_t k = 0; k < n_tab; k++) r += S.list[k] < c ? 1u : 0u;
      S.rank[S.slot_of[t]] = (uint16_t)r;
      S.buf[r] = c;
    }
    if (t == 0 && S.has_empty) S.buf[n_col - 1] = kMvEmpty;
    __syncthreads();
    const uint32_t n_words = ((uint32_t)n_px * bits + 31u) / 32u;
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    if (bits == 1) mv_pack<1>(S, px, nv, starts, n_col, word);
    else if (bits == 2) mv_pack<2>(S, px, nv, starts, n_col, word);
    else if (bits == 4) mv_pack<4>(S, px, nv, starts, n_col, word);
    else mv_pack<8>(S, px, nv, starts, n_col, word);
    uint32_t* idx = S.buf + n_col;
    if (bits == 1) {
      if ((uint32_t)t < 2u * n_words) reinterpret_cast<uint16_t*>(idx)[t] = (uint16_t)word[0];
    } else {
      const uint32_t per = bits / 2u;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++)
        if (q < per && (uint32_t)t * per + q < n_words) idx[(uint32_t)t * per + q] = word[q];
    }
  } else if (mode == 2) {
    __syncthreads();
    uint16_t* pos = reinterpret_cast<uint16_t*>(S.buf + n_runs);
    uint32_t m = starts, r = first_run;
    while (m) {
      const int j = __ffs(m) - 1;
      m &= m - 1;
      uint32_t c = px[0];
#pragma unroll
      for (int q = 1; q < kMvPerThread; q++) c = q == j ? px[q] : c;
      S.buf[r] = c;
      pos[r] = (uint16_t)(base + j);
      r++;
    }
    __syncthreads();
    uint16_t len[kMvRunsPerThread];
#pragma unroll
    for (int k = 0; k < kMvRunsPerThread; k++) {
      const uint32_t i = (uint32_t)t + (uint32_t)k * kMvThreads;
      len[k] = i < n_runs ? (uint16_t)((i + 1 < n_runs ? (uint32_t)pos[i + 1] : (uint32_t)n_px) - (uint32_t)pos[i] - 1u) : (uint16_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMvRunsPerThread; k++) {
      const uint32_t i = (uint32_t)t + (uint32_t)k * kMvThreads;
      if (i < n_runs) pos[i] = len[k];
    }
    if (t == 0 && (n_runs & 1u)) pos[n_runs] = 0;
  }
  __syncthreads();
  if ((uint32_t)t < (claim - size) / 4u) S.buf[size / 4u + (uint32_t)t] = 0u;
  __syncthreads();

  // 7. out: payload and entry
  const uint32_t offset = S.offset;
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(P.payload + offset);
  for (uint32_t v = (uint32_t)t; v < claim / 16u; v += kMvThreads) dst[v] = reinterpret_cast<const uint4*>(S.buf)[v];
  if (t == 0) {
    uint2* e = P.dir + (size_t)slot_dir * 3;
    e[0] = make_uint2((uint32_t)x0 | (uint32_t)y0 << 16, (uint32_t)w | (uint32_t)h << 16);
    e[1] = make_uint2(mode | (mode == 1 ? bits : 0u) << 8 | (mode == 1 ? n_col : mode == 2 ? n_runs : 0u) << 16, offset);
    e[2] = make_uint2(size, mode == 0 ? px[0] : 0u);
  }
}

void launch_damage_encode_moved(hipStream_t s, const DamageEncodeMovedParams& P) {
  const int nb = P.enc.bins_x * P.enc.bins_y;
  if (nb <= 0) return;
  FDH_LAUNCH(k_damage_encode_moved, dim3(nb), dim3(kMvThreads), 0, s, P);
}

// ------------------------------------------------------------------ k_damage_move_votes
// Workgroups stride over the bins.  Vertical: a wave per shift, a lane per column -- the mirror's row is 256 contiguous bytes of one slot.
// Horizontal: the columns at every shift are the 64-row strip of the bin's own row of slots; a lane takes a column of a slot and a wave
// 16 of its rows, so each load is again 256 contiguous bytes (no strided column reads, and the strip needs no staging), the four waves'
// verdicts meet in s_ne.  A shift is tallied by one thread of one wave: the LDS counters need no atomics.
constexpr int kVotesGrid = 1024;  // four workgroups a CU
__global__ __launch_bounds__(kMoveThreads) void k_damage_move_votes(const DamageMoveVotesParams P) {
  __shared__ uint32_t s_votes[2 * kDamageVoteSpan];
  __shared__ uint32_t s_probe[2][kBin];
  __shared__ uint32_t s_ne[kBin];
  const int nb = P.bins_x * P.bins_y;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int S = P.max_shift;
  for (int i = t; i < 2 * kDamageVoteSpan; i += kMoveThreads) s_votes[i] = 0;
  if (t < kBin) s_ne[t] = 0;
  for (int bin = (int)blockIdx.x; bin < nb; bin += (int)gridDim.x) {  // (uniform)
    if (!P.all && P.stamp[bin] != P.epoch) continue;
    const TileBox b = tile_box(bin, P.bins_x, P.W, P.H);
    if (b.w != kBin || b.h != kBin) continue;
    __syncthreads();  // the probes of the bin before are read; the counters are zero
    if (wave == 0) s_probe[0][lane] = P.surf[(size_t)(b.y0 + 32) * P.W + b.x0 + lane];
    if (wave == 1) s_probe[1][lane] = P.surf[(size_t)(b.y0 + lane) * P.W + b.x0 + 32];
    __syncthreads();
    const uint32_t pv = s_probe[0][lane];
    if (__ballot(pv != s_probe[0][0]) != 0ull) {  // (the same in every wave)
      for (int i = wave; i <= 2 * S; i += kMoveWaves) {
        const int d = i - S, y = b.y0 + 32 + d;
        if (d == 0 || y < 0 || y >= P.H) continue;
        const bool ne = mirror_px(P.mirror, P.bins_x, b.x0 + lane, y) != pv;
        if (__ballot(ne) == 0ull && lane == 0) s_votes[d + kDamageShiftMax] += 1u;
      }
    }
    if (__ballot(s_probe[1][lane] != s_probe[1][0]) != 0ull) {
      const int xc = b.x0 + 32, by = b.y0 >> 6;
      const int sb0 = max(xc - S, 0) >> 6, sb1 = min(xc + S, P.W - 1) >> 6;
      for (int sb = sb0; sb <= sb1; sb++) {  // (uniform)
        const int x = sb * kBin + lane, d = x - xc;
        const bool live = d != 0 && d >= -S && d <= S && x < P.W;
        const uint32_t* __restrict__ src = P.mirror + ((size_t)(by * P.bins_x + sb) << 12) + lane;
        uint32_t ne = 0;
#pragma unroll 4
        for (int r = wave * (kBin / kMoveWaves); r < (wave + 1) * (kBin / kMoveWaves); r++) ne |= src[r * kBin] ^ s_probe[1][r];
        if (live && ne) s_ne[lane] = 1u;  // (whoever stores, stores 1)
        __syncthreads();
        if (wave == 0) {
          if (live && !s_ne[lane]) s_votes[kDamageVoteSpan + d + kDamageShiftMax] += 1u;
          s_ne[lane] = 0;
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();
  for (int i = t; i < 2 * kDamageVoteSpan; i += kMoveThreads)
    if (const uint32_t v = s_votes[i]) atomicAdd(&P.votes[i], v);
}

void launch_damage_move_votes(hipStream_t s, const DamageMoveVotesParams& P) {
  const int nb = P.bins_x * P.bins_y;
  if (nb <= 0) return;
  FDH_LAUNCH(k_damage_move_votes, dim3(nb < kVotesGrid ? nb : kVotesGrid), dim3(kMoveThreads), 0, s, P);
}

}  // namespace fdh
